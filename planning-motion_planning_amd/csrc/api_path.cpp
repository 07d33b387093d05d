// api_path.cpp -- path extraction: the 2D, obstacle-safe 2D and 3D walkers, their batches, and the batched
// plan (solve + walks) (gdm.hip, gdm_safe.hip; the host API's layout: DESIGN.md §3.19).
#include "api_internal.hpp"

namespace eik_api __attribute__((visibility("hidden"))) {

static long path_steps(double tau) { return (long)std::nearbyint(15000.0 / tau); }  // round(15000/tau), FastMarching.py:173

// the walk's arguments of the two single-path 2D device entries, from theirs
static Gdm2dArgs path2d_args(const void* d_T, int64_t H, int64_t W, const double init[2], const double end[2], double tau,
                             double* d_out, int64_t cap, int64_t* d_n_out, int* d_status, int fused) {
    Gdm2dArgs a;
    a.T = d_T;
    a.H = H;
    a.W = W;
    a.ix = init[0];
    a.iy = init[1];
    a.ex = end[0];
    a.ey = end[1];
    a.tau = tau;
    a.steps = path_steps(tau);
    a.out = d_out;
    a.cap = cap;
    a.n_out = d_n_out;
    a.status = d_status;
    a.fused = fused;
    return a;
}

// The synchronous single-path host entries (dim = 2 or 3) after their own argument checks: the field
// (`cells` values) to c->T2; the device results in c->work, out [cap][dim] | n | info [4] (has_info)
// | status; launch(d_out, d_n, d_st, d_info), an entry's *_dev call on c->stream; then n, status
// and the info words, and the n rows.
template <typename Launch>
static int path_host(eik_ctx* c, int dim, const double* T, int64_t cells, double* out, int64_t cap, int64_t* n_out,
                     int* status, bool has_info, int64_t* info, Launch&& launch) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->T2.ensure(sizeof(double) * cells));
    HIPCHK(c, c->work.ensure(sizeof(double) * dim * cap + (has_info ? 128 : 64)));
    HIPCHK(c, host_to_dev(c, c->T2.p, T, sizeof(double) * cells, c->stream));
    double* d_out = (double*)c->work.p;
    int64_t* d_n = (int64_t*)(d_out + dim * cap);
    int64_t* d_info = has_info ? d_n + 1 : nullptr;
    int* d_st = (int*)(d_n + (has_info ? 5 : 1));
    int rc = launch(d_out, d_n, d_st, d_info);
    if (rc) return rc;
    int64_t h[5] = {0, 0, 0, 0, 0};  // n | info
    int st = 0;
    HIPCHK(c, hipMemcpyAsync(h, d_n, sizeof(int64_t) * (has_info ? 5 : 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t nn = h[0] > cap ? cap : h[0];
    // (as the entries always did: the safe one skips the copy of no rows, the others issue it)
    if (nn > 0 || !has_info) HIPCHK(c, hipMemcpy(out, d_out, sizeof(double) * dim * nn, hipMemcpyDeviceToHost));
    *n_out = nn;
    *status = st;
    if (info)
        for (int k = 0; k < 4; ++k) info[k] = h[1 + k];
    return EIK_OK;
}

// ---- batched paths: P walks in one launch (gdm.hip: gdm2d_kernel / gdm3d_kernel on GdmBatchArgs)
constexpr size_t kDescBlocks = 8;  // descriptor blocks kept per context

// A descriptor block of >= P entries that no earlier call still uses: a block whose event has
// completed (grown if too small), else a new one, else -- kDescBlocks calls in flight -- the oldest,
// after waiting for it.
static int stage_desc(eik_ctx* c, int64_t P, DescBlock** out) {
    DescBlock* b = nullptr;
    for (DescBlock& k : c->desc)
        if (hipEventQuery(k.ev) == hipSuccess && (!b || (b->cap < P && k.cap >= P))) b = &k;
    if (!b && c->desc.size() < kDescBlocks) {
        c->desc.emplace_back();
        b = &c->desc.back();
        HIPCHK(c, hipEventCreateWithFlags(&b->ev, hipEventDisableTiming));
    }
    if (!b) {
        b = &c->desc[c->desc_next++ % c->desc.size()];
        HIPCHK(c, hipEventSynchronize(b->ev));
    }
    if (b->cap < P) {
        if (b->h) (void)hipHostFree(b->h);
        if (b->d) (void)hipFree(b->d);
        b->h = b->d = nullptr;
        b->cap = 0;
        const int64_t cap = std::max<int64_t>(256, P);
        HIPCHK(c, hipHostMalloc((void**)&b->h, sizeof(GdmDesc) * cap));
        HIPCHK(c, hipMalloc((void**)&b->d, sizeof(GdmDesc) * cap));
        b->cap = cap;
    }
    *out = b;
    return EIK_OK;
}

// Host-side checks (batch_check) and staging (batch_stage) shared by the 2D and 3D batch entries
// (dim = 2 or 3): on EIK_OK a.desc holds the P descriptors, on the device in stream order, and *blk
// is to be marked busy (hipEventRecord on st) after the launch.  Nothing is launched on an error.
static int batch_check(eik_ctx* c, int dim, int64_t B, int64_t H, int64_t W, int64_t L, int64_t P,
                       const int32_t* map_of, const double* inits, const double* ends, double tau, int64_t cap) {
    if (!inits || !ends) return set_err(c, EIK_ERR_ARG, "batched path: NULL argument");
    if (B < 1) return set_err(c, EIK_ERR_ARG, "batched path: B = %ld fields (>= 1 needed)", (long)B);
    if (P < 1 || P > 0x7fffffff) return set_err(c, EIK_ERR_ARG, "batched path: P = %ld paths (1 .. 2^31 - 1)", (long)P);
    if (cap < 2) return set_err(c, EIK_ERR_ARG, "batched path: cap = %ld rows per path (>= 2 needed)", (long)cap);
    if (!(tau > 0)) return set_err(c, EIK_ERR_ARG, "batched path: tau = %g (> 0 needed)", tau);
    if (dim == 2 ? (H < 3 || W < 3) : (H < 1 || W < 1 || L < 1))
        return set_err(c, EIK_ERR_ARG, "batched path: field of %ld x %ld x %ld too small", (long)H, (long)W, (long)L);
    if (!map_of && P != B && B != 1)
        return set_err(c, EIK_ERR_ARG, "batched path: map_of is NULL with P = %ld paths on B = %ld fields (P == B or B == 1)",
                       (long)P, (long)B);
    if (map_of)
        for (int64_t p = 0; p < P; ++p)
            if (map_of[p] < 0 || map_of[p] >= B)
                return set_err(c, EIK_ERR_ARG, "batched path: map_of[%ld] = %d outside [0, %ld)", (long)p, map_of[p], (long)B);
    return EIK_OK;
}
static int batch_stage(eik_ctx* c, int dim, const void* d_T, int64_t B, int64_t H, int64_t W, int64_t L, int64_t P,
                       const int32_t* map_of, const double* inits, const double* ends, double tau, double* d_out,
                       int64_t cap, int64_t* d_n_out, int* d_status, hipStream_t st, GdmBatchArgs& a, DescBlock** blk) {
    if (!c) return EIK_ERR_ARG;
    if (!d_T || !d_out || !d_n_out || !d_status) return set_err(c, EIK_ERR_ARG, "batched path: NULL argument");
    int rc = batch_check(c, dim, B, H, W, L, P, map_of, inits, ends, tau, cap);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = stage_desc(c, P, blk);
    if (rc) return rc;
    GdmDesc* h = (*blk)->h;
    for (int64_t p = 0; p < P; ++p) {
        h[p].map = map_of ? map_of[p] : B == 1 ? 0 : (int32_t)p;
        h[p].pad = 0;
        for (int k = 0; k < 3; ++k) {
            h[p].init[k] = k < dim ? inits[dim * p + k] : 0.0;
            h[p].end[k] = k < dim ? ends[dim * p + k] : 0.0;
        }
    }
    HIPCHK(c, hipMemcpyAsync((*blk)->d, h, sizeof(GdmDesc) * P, hipMemcpyHostToDevice, st));
    a.T = d_T;
    a.H = H;
    a.W = W;
    a.L = L;
    a.P = P;
    a.desc = (*blk)->d;
    a.tau = tau;
    a.steps = path_steps(tau);
    a.out = d_out;
    a.cap = cap;
    a.n_out = d_n_out;
    a.status = d_status;
    a.fused = c->path_loop;
    return EIK_OK;
}

// The synchronous host entries' tail: path p's n_out[p] rows into out + p * cap * dim (rows past
// them stay as the caller left them), after the walks on c->stream.
static int batch_fetch(eik_ctx* c, int dim, int64_t P, int64_t cap, const double* d_out, const int64_t* d_n,
                       const int* d_st, double* out, int64_t* n_out, int* status) {
    HIPCHK(c, hipMemcpyAsync(n_out, d_n, sizeof(int64_t) * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, d_st, sizeof(int) * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t p = 0; p < P; ++p) {
        if (n_out[p] > cap) n_out[p] = cap;
        if (n_out[p] > 0)
            HIPCHK(c, hipMemcpyAsync(out + p * cap * dim, d_out + p * cap * dim, sizeof(double) * dim * n_out[p],
                                     hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

// the host entries' device results in c->work: out [P][cap][dim] | info [P][4] (d_info given) | n_out [P]
// | status [P]
static int batch_work(eik_ctx* c, int dim, int64_t P, int64_t cap, double** d_out, int64_t** d_n, int** d_st,
                      int64_t** d_info = nullptr) {
    HIPCHK(c, c->work.ensure(sizeof(double) * dim * cap * P + ((d_info ? 5 : 1) * sizeof(int64_t) + sizeof(int)) * P + 64));
    *d_out = (double*)c->work.p;
    int64_t* const words = (int64_t*)(*d_out + dim * cap * P);
    if (d_info) *d_info = words;
    *d_n = words + (d_info ? 4 * P : 0);
    *d_st = (int*)(*d_n + P);
    return EIK_OK;
}

// The synchronous batched host entries (dim = 2 or 3) after their own argument checks: the B fields
// (`cells` values in all) to c->T2, once; launch(d_out, d_n, d_st, d_info), an entry's *_batch_dev
// call on c->stream; then the info words and batch_fetch.
template <typename Launch>
static int path_batch_host(eik_ctx* c, int dim, const double* T, int64_t cells, int64_t P, double* out, int64_t cap,
                           int64_t* n_out, int* status, bool has_info, int64_t* info, Launch&& launch) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->T2.ensure(sizeof(double) * cells));
    double* d_out;
    int64_t *d_n, *d_info = nullptr;
    int* d_st;
    int rc = batch_work(c, dim, P, cap, &d_out, &d_n, &d_st, has_info ? &d_info : nullptr);
    if (rc) return rc;
    HIPCHK(c, host_to_dev(c, c->T2.p, T, sizeof(double) * cells, c->stream));
    rc = launch(d_out, d_n, d_st, d_info);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);  // the upload still reads T
        return rc;
    }
    if (info) HIPCHK(c, hipMemcpyAsync(info, d_info, sizeof(int64_t) * 4 * P, hipMemcpyDeviceToHost, c->stream));
    return batch_fetch(c, dim, P, cap, d_out, d_n, d_st, out, n_out, status);
}

// ---- the obstacle-safe 2D walker (gdm_safe.hip): the entries above with tau <= 1 and the info words
static long safe_stall(double tau) { return std::max(16L, (long)std::ceil(8.0 / tau)); }  // S of the stall rule

}  // namespace eik_api

extern "C" {

int eik_selftest_walker_math(eik_ctx* c, int64_t n, uint64_t seed, int64_t mismatches[6]) {
    if (!c || !mismatches || n < 1) return EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->misc.ensure(64));
    unsigned long long* d = (unsigned long long*)c->misc.p;
    HIPCHK(c, hipMemsetAsync(d, 0, 6 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, walker_math_selftest((long long)n, (unsigned long long)seed, d, c->stream));
    unsigned long long h[6];
    HIPCHK(c, hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 6; ++k) mismatches[k] = (int64_t)h[k];
    return EIK_OK;
}

int eik_path2d_dev(eik_ctx* c, const void* d_T, int dtype, int64_t H, int64_t W, const double init[2],
                   const double end[2], double tau, double* d_out, int64_t cap, int64_t* d_n_out, int* d_status,
                   void* stream) {
    if (!c || !d_T || !init || !end || !d_out || !d_n_out || !d_status || cap < 2 || H < 3 || W < 3 || !(tau > 0))
        return c ? set_err(c, EIK_ERR_ARG, "bad path arguments") : EIK_ERR_ARG;
    const Gdm2dArgs a = path2d_args(d_T, H, W, init, end, tau, d_out, cap, d_n_out, d_status, c->path_loop);
    HIPCHK(c, gdm2d(a, dtype == EIK_F64, (hipStream_t)stream));
    return EIK_OK;
}

int eik_path2d_f64(eik_ctx* c, const double* T, int64_t H, int64_t W, const double init[2], const double end[2],
                   double tau, double* out, int64_t cap, int64_t* n_out, int* status) {
    if (!c || !T || !out || !n_out || !status) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    return path_host(c, 2, T, H * W, out, cap, n_out, status, false, nullptr,
                     [&](double* d_out, int64_t* d_n, int* d_st, int64_t*) {
                         return eik_path2d_dev(c, c->T2.p, EIK_F64, H, W, init, end, tau, d_out, cap, d_n, d_st, c->stream);
                     });
}

int eik_path2d_batch_dev(eik_ctx* c, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, int64_t P,
                         const int32_t* map_of, const double* inits, const double* ends, double tau, double* d_out,
                         int64_t cap, int64_t* d_n_out, int* d_status, void* stream) {
    GdmBatchArgs a{};
    DescBlock* blk = nullptr;
    int rc = batch_stage(c, 2, d_T, B, H, W, 1, P, map_of, inits, ends, tau, d_out, cap, d_n_out, d_status,
                         (hipStream_t)stream, a, &blk);
    if (rc) return rc;
    HIPCHK(c, gdm2d_batch(a, dtype == EIK_F64, (hipStream_t)stream));
    HIPCHK(c, hipEventRecord(blk->ev, (hipStream_t)stream));
    return EIK_OK;
}

int eik_path2d_batch_f64(eik_ctx* c, const double* T, int64_t B, int64_t H, int64_t W, int64_t P, const int32_t* map_of,
                         const double* inits, const double* ends, double tau, double* out, int64_t cap, int64_t* n_out,
                         int* status) {
    if (!c || !T || !out || !n_out || !status) return c ? set_err(c, EIK_ERR_ARG, "batched path: NULL argument") : EIK_ERR_ARG;
    int rc = batch_check(c, 2, B, H, W, 1, P, map_of, inits, ends, tau, cap);
    if (rc) return rc;
    return path_batch_host(c, 2, T, B * H * W, P, out, cap, n_out, status, false, nullptr,
                           [&](double* d_out, int64_t* d_n, int* d_st, int64_t*) {
                               return eik_path2d_batch_dev(c, c->T2.p, EIK_F64, B, H, W, P, map_of, inits, ends, tau, d_out,
                                                           cap, d_n, d_st, c->stream);
                           });
}

int eik_path2d_safe_dev(eik_ctx* c, const void* d_T, int dtype, int64_t H, int64_t W, const double init[2],
                        const double end[2], double tau, double* d_out, int64_t cap, int64_t* d_n_out, int* d_status,
                        int64_t* d_info, void* stream) {
    if (!c || !d_T || !init || !end || !d_out || !d_n_out || !d_status || cap < 2 || H < 3 || W < 3 || !(tau > 0))
        return c ? set_err(c, EIK_ERR_ARG, "bad path arguments") : EIK_ERR_ARG;
    if (tau > 1) return set_err(c, EIK_ERR_ARG, "safe path: tau = %g (0 < tau <= 1 needed)", tau);
    GdmSafeArgs s;
    s.a = path2d_args(d_T, H, W, init, end, tau, d_out, cap, d_n_out, d_status, 0);
    s.stall = safe_stall(tau);
    s.info = d_info;
    HIPCHK(c, gdm2d_safe(s, dtype == EIK_F64, (hipStream_t)stream));
    return EIK_OK;
}

int eik_path2d_safe_f64(eik_ctx* c, const double* T, int64_t H, int64_t W, const double init[2], const double end[2],
                        double tau, double* out, int64_t cap, int64_t* n_out, int* status, int64_t info[4]) {
    if (!c || !T || !out || !n_out || !status) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    if (!init || !end || cap < 2 || H < 3 || W < 3 || !(tau > 0)) return set_err(c, EIK_ERR_ARG, "bad path arguments");
    if (tau > 1) return set_err(c, EIK_ERR_ARG, "safe path: tau = %g (0 < tau <= 1 needed)", tau);
    return path_host(c, 2, T, H * W, out, cap, n_out, status, true, info,
                     [&](double* d_out, int64_t* d_n, int* d_st, int64_t* d_info) {
                         return eik_path2d_safe_dev(c, c->T2.p, EIK_F64, H, W, init, end, tau, d_out, cap, d_n, d_st, d_info,
                                                    c->stream);
                     });
}

int eik_path2d_safe_batch_dev(eik_ctx* c, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, int64_t P,
                              const int32_t* map_of, const double* inits, const double* ends, double tau,
                              double* d_out, int64_t cap, int64_t* d_n_out, int* d_status, int64_t* d_info,
                              void* stream) {
    if (c && tau > 1) return set_err(c, EIK_ERR_ARG, "safe path: tau = %g (0 < tau <= 1 needed)", tau);
    GdmSafeBatchArgs s{};
    DescBlock* blk = nullptr;
    int rc = batch_stage(c, 2, d_T, B, H, W, 1, P, map_of, inits, ends, tau, d_out, cap, d_n_out, d_status,
                         (hipStream_t)stream, s.b, &blk);
    if (rc) return rc;
    s.stall = safe_stall(tau);
    s.info = d_info;
    HIPCHK(c, gdm2d_safe_batch(s, dtype == EIK_F64, (hipStream_t)stream));
    HIPCHK(c, hipEventRecord(blk->ev, (hipStream_t)stream));
    return EIK_OK;
}

int eik_path2d_safe_batch_f64(eik_ctx* c, const double* T, int64_t B, int64_t H, int64_t W, int64_t P,
                              const int32_t* map_of, const double* inits, const double* ends, double tau, double* out,
                              int64_t cap, int64_t* n_out, int* status, int64_t* info) {
    if (!c || !T || !out || !n_out || !status) return c ? set_err(c, EIK_ERR_ARG, "batched path: NULL argument") : EIK_ERR_ARG;
    int rc = batch_check(c, 2, B, H, W, 1, P, map_of, inits, ends, tau, cap);
    if (rc) return rc;
    if (tau > 1) return set_err(c, EIK_ERR_ARG, "safe path: tau = %g (0 < tau <= 1 needed)", tau);
    return path_batch_host(c, 2, T, B * H * W, P, out, cap, n_out, status, true, info,
                           [&](double* d_out, int64_t* d_n, int* d_st, int64_t* d_info) {
                               return eik_path2d_safe_batch_dev(c, c->T2.p, EIK_F64, B, H, W, P, map_of, inits, ends, tau,
                                                                d_out, cap, d_n, d_st, d_info, c->stream);
                           });
}

int eik_plan2d_batch_f32(eik_ctx* c, const float* cost, int64_t B, int64_t H, int64_t W, const int64_t* goals,
                         const double* starts, double tau, double* paths, int64_t cap, int64_t* n_out, int* status,
                         float* T_out) {
    if (!c || !cost || !goals || !starts || !paths || !n_out || !status)
        return c ? set_err(c, EIK_ERR_ARG, "batched plan: NULL argument") : EIK_ERR_ARG;
    if (B < 1 || H < 3 || W < 3 || cap < 2 || !(tau > 0))
        return set_err(c, EIK_ERR_ARG, "batched plan: B = %ld, field %ld x %ld, cap = %ld, tau = %g", (long)B, (long)H,
                       (long)W, (long)cap, tau);
    for (int64_t b = 0; b < B; ++b)
        if (goals[2 * b] < 0 || goals[2 * b + 1] < 0 || goals[2 * b] >= W || goals[2 * b + 1] >= H)
            return set_err(c, EIK_ERR_ARG, "goal (%ld, %ld) of map %ld outside %ldx%ld", (long)goals[2 * b],
                           (long)goals[2 * b + 1], (long)b, (long)H, (long)W);
    const int64_t n = B * H * W;
    HIPCHK(c, hipSetDevice(c->device));
    eik_fim2d* f = nullptr;
    int rc = get_solver(c, B, H, W, EIK_F32, &f);
    if (rc) return rc;
    HIPCHK(c, c->cost.ensure(sizeof(float) * n));
    HIPCHK(c, c->T.ensure(sizeof(float) * n));
    double* d_out;
    int64_t* d_n;
    int* d_st;
    rc = batch_work(c, 2, B, cap, &d_out, &d_n, &d_st);
    if (rc) return rc;
    HIPCHK(c, host_to_dev(c, c->cost.p, cost, sizeof(float) * n, c->stream));
    rc = check_cost(c, cost, c->cost.p, n, c->stream);
    if (rc) return rc;
    rc = eik_fim2d_solve(f, c->cost.p, c->T.p, goals, c->stream);  // the B fields stay on the device
    if (rc) return rc;
    std::vector<double> ends(2 * B);
    for (int64_t k = 0; k < 2 * B; ++k) ends[k] = (double)goals[k];
    rc = eik_path2d_batch_dev(c, c->T.p, EIK_F32, B, H, W, B, nullptr, starts, ends.data(), tau, d_out, cap, d_n, d_st,
                              c->stream);
    if (rc) return rc;
    rc = batch_fetch(c, 2, B, cap, d_out, d_n, d_st, paths, n_out, status);
    if (rc) return rc;
    if (T_out) {
        HIPCHK(c, dev_to_host(c, T_out, c->T.p, sizeof(float) * n, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return EIK_OK;
}

int eik_path3d_dev(eik_ctx* c, const void* d_T, int dtype, int64_t H, int64_t W, int64_t L, const double init[3],
                   const double end[3], double tau, double* d_out, int64_t cap, int64_t* d_n_out, int* d_status,
                   void* stream) {
    if (!c || !d_T || !init || !end || !d_out || !d_n_out || !d_status || cap < 2 || !(tau > 0) || H < 1 || W < 1 ||
        L < 1)
        return c ? set_err(c, EIK_ERR_ARG, "bad 3D path arguments") : EIK_ERR_ARG;
    Gdm3dArgs a;
    a.T = d_T;
    a.H = H;
    a.W = W;
    a.L = L;
    for (int i = 0; i < 3; ++i) {
        a.init[i] = init[i];
        a.end[i] = end[i];
    }
    a.tau = tau;
    a.steps = path_steps(tau);  // int(round(15000/tau)), FastMarching3D.py:207
    a.out = d_out;
    a.cap = cap;
    a.n_out = d_n_out;
    a.status = d_status;
    HIPCHK(c, gdm3d(a, dtype == EIK_F64, (hipStream_t)stream));
    return EIK_OK;
}

int eik_path3d_f64(eik_ctx* c, const double* T, int64_t H, int64_t W, int64_t L, const double init[3],
                   const double end[3], double tau, double* out, int64_t cap, int64_t* n_out, int* status) {
    if (!c || !T || !out || !n_out || !status) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    return path_host(c, 3, T, H * W * L, out, cap, n_out, status, false, nullptr,
                     [&](double* d_out, int64_t* d_n, int* d_st, int64_t*) {
                         return eik_path3d_dev(c, c->T2.p, EIK_F64, H, W, L, init, end, tau, d_out, cap, d_n, d_st, c->stream);
                     });
}

int eik_path3d_batch_dev(eik_ctx* c, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, int64_t L, int64_t P,
                         const int32_t* map_of, const double* inits, const double* ends, double tau, double* d_out,
                         int64_t cap, int64_t* d_n_out, int* d_status, void* stream) {
    GdmBatchArgs a{};
    DescBlock* blk = nullptr;
    int rc = batch_stage(c, 3, d_T, B, H, W, L, P, map_of, inits, ends, tau, d_out, cap, d_n_out, d_status,
                         (hipStream_t)stream, a, &blk);
    if (rc) return rc;
    HIPCHK(c, gdm3d_batch(a, dtype == EIK_F64, (hipStream_t)stream));
    HIPCHK(c, hipEventRecord(blk->ev, (hipStream_t)stream));
    return EIK_OK;
}

int eik_path3d_batch_f64(eik_ctx* c, const double* T, int64_t B, int64_t H, int64_t W, int64_t L, int64_t P,
                         const int32_t* map_of, const double* inits, const double* ends, double tau, double* out,
                         int64_t cap, int64_t* n_out, int* status) {
    if (!c || !T || !out || !n_out || !status) return c ? set_err(c, EIK_ERR_ARG, "batched 3D path: NULL argument") : EIK_ERR_ARG;
    int rc = batch_check(c, 3, B, H, W, L, P, map_of, inits, ends, tau, cap);
    if (rc) return rc;
    return path_batch_host(c, 3, T, B * H * W * L, P, out, cap, n_out, status, false, nullptr,
                           [&](double* d_out, int64_t* d_n, int* d_st, int64_t*) {
                               return eik_path3d_batch_dev(c, c->T2.p, EIK_F64, B, H, W, L, P, map_of, inits, ends, tau,
                                                           d_out, cap, d_n, d_st, c->stream);
                           });
}

}  // extern "C"
