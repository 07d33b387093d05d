// eikonal_api.cpp -- C ABI (include/eikonal.h) over the HIP kernels: contexts, device buffers,
// the outer FIM iteration driver and the synchronous host-buffer drop-ins.
//
// Every entry point fails loudly (status + eik_last_error) -- there is no CPU fallback: a
// missing device is EIK_ERR_NODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "api_internal.hpp"

using namespace eik;

namespace eik_api __attribute__((visibility("hidden"))) {

static thread_local std::string g_create_err;

// Host memcpy split over a few worker threads and the caller (the pinned-staging copies below).
// ONE pool per process, shared by every context (8 DD ranks sharing a node each started
// their own threads), created on the first large copy; concurrent callers take turns.
class CopyPool {
  public:
    static CopyPool* shared() {
        static CopyPool* p = new CopyPool((int)std::max(1u, std::min(3u, std::thread::hardware_concurrency() / 2)));
        return p;  // (never destroyed: workers outlive the contexts, the process ends them)
    }
    explicit CopyPool(int workers) {
        for (int i = 0; i < workers; ++i) th_.emplace_back([this] { loop(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void copy(void* dst, const void* src, size_t len) {
        std::lock_guard<std::mutex> turn(caller_);  // one copy at a time (contexts of other threads wait)
        const int parts = (int)th_.size() + 1;
        {
            std::lock_guard<std::mutex> g(m_);
            dst_ = static_cast<char*>(dst);
            src_ = static_cast<const char*>(src);
            len_ = len;
            parts_ = parts;
            next_ = 1;  // part 0 is the caller's
            left_ = parts - 1;
            ++gen_;
        }
        cv_.notify_all();
        part(0, parts);
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return left_ == 0; });
    }

  private:
    std::mutex caller_;
    void part(int k, int parts) {
        const size_t a = len_ * k / parts, e = len_ * (k + 1) / parts;
        std::memcpy(dst_ + a, src_ + a, e - a);
    }
    void loop() {
        for (;;) {
            int k, parts;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return quit_ || next_ < parts_; });
                if (quit_) return;
                k = next_++;
                parts = parts_;
            }
            part(k, parts);
            {
                std::lock_guard<std::mutex> g(m_);
                if (--left_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    char* dst_ = nullptr;
    const char* src_ = nullptr;
    size_t len_ = 0;
    int parts_ = 0, next_ = 0, left_ = 0;
    unsigned long long gen_ = 0;
    bool quit_ = false;
};

// The fp32 2D persistent kernel's form: the 4-waves-per-SIMD one on one large raster (a batch of
// small maps: no gain), or as EIK_OPT_WIDE says.  fp64 has the one form.
static bool wide_form(const eik_fim2d* f) {
    if (f->f64) return false;
    return f->ctx->wide >= 0 ? f->ctx->wide != 0 : f->a.tiles_per_map >= kWideTiles;
}

// ... and its co-resident workgroups, kept per solver and form
static int persist_resident(eik_fim2d* f, bool wide) {
    if (f->persist_grid == 0 || f->persist_wide != wide) {
        f->persist_grid = fim2d_persist_resident(f->f64, f->ctx->cu_count, wide);
        f->persist_wide = wide;
    }
    return f->persist_grid;
}

int set_err(eik_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c)
        c->err = buf;
    else
        g_create_err = buf;
    return code;
}

static int bytes_per_visit(bool f64) { return (f64 ? 8 : 4) * (3 * kTile * kTile + 4 * kTile); }
// in-place pass of a busy tile (persistent mode): T write-back + halo ring re-read
static int bytes_per_pass(bool f64) { return (f64 ? 8 : 4) * (kTile * kTile + 4 * kTile); }

// Large host <-> device copies through a pinned ring of two 8 MiB chunks, host memcpy by a few
// threads overlapped with the DMA of the other chunk.  A pageable hipMemcpyAsync of a FRESH host
// buffer (every numpy array the drop-in receives or returns) ran at ~8 GB/s: 16 ms per 128 MiB,
// 3 ms only once the runtime had seen the buffer; staged: ~4 ms either way (tools/h2d_probe.cpp).
// Staged (pageable) buffers: host_to_dev returns once the source has been read (the DMA of the last
// chunk may still run on st); dev_to_host returns with the data in dst (it waits for st's earlier
// work).  A buffer wholly inside a pinned block (eik_host_alloc) goes as ONE hipMemcpyAsync on st
// and both return at once: the source must stay unchanged, and dst is valid, only after st is
// synchronised -- every caller synchronises st before it returns to its own caller.
// pinned host blocks handed out by eik_host_alloc: a copy wholly inside one goes as one DMA
static std::mutex g_pin_mu;
static std::vector<std::pair<uintptr_t, size_t>> g_pinned;
static bool is_pinned(const void* p, size_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (const auto& b : g_pinned)
        if (a >= b.first && a + bytes <= b.first + b.second) return true;
    return false;
}
static hipError_t stage_init(eik_ctx* c) {
    for (int b = 0; b < 2; ++b) {
        if (!c->stage[b]) {
            hipError_t e = hipHostMalloc((void**)&c->stage[b], kStageChunk);
            if (e != hipSuccess) return e;
        }
        if (!c->stage_ev[b]) {
            hipError_t e = hipEventCreateWithFlags(&c->stage_ev[b], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
    }
    if (!c->pool) c->pool = CopyPool::shared();
    return hipSuccess;
}
hipError_t host_to_dev(eik_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (bytes < 2 * kStageChunk || is_pinned(src, bytes)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    hipError_t e = stage_init(c);
    if (e != hipSuccess) return e;
    int k = 0;
    for (size_t off = 0; off < bytes; off += kStageChunk, ++k) {
        const int b = k & 1;
        const size_t len = std::min(kStageChunk, bytes - off);
        if ((e = hipEventSynchronize(c->stage_ev[b])) != hipSuccess) return e;  // its last DMA is done
        c->pool->copy(c->stage[b], static_cast<const char*>(src) + off, len);
        if ((e = hipMemcpyAsync(static_cast<char*>(dst) + off, c->stage[b], len, hipMemcpyHostToDevice, st)) != hipSuccess)
            return e;
        if ((e = hipEventRecord(c->stage_ev[b], st)) != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t dev_to_host(eik_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (bytes < 2 * kStageChunk || is_pinned(dst, bytes)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    hipError_t e = stage_init(c);
    if (e != hipSuccess) return e;
    const size_t nch = (bytes + kStageChunk - 1) / kStageChunk;
    // a host_to_dev on another stream may still be reading the staging buffers
    for (int b = 0; b < 2; ++b)
        if ((e = hipStreamWaitEvent(st, c->stage_ev[b], 0)) != hipSuccess) return e;
    auto issue = [&](size_t k) -> hipError_t {
        const int b = (int)(k & 1);
        const size_t off = k * kStageChunk, len = std::min(kStageChunk, bytes - off);
        hipError_t r = hipMemcpyAsync(c->stage[b], static_cast<const char*>(src) + off, len, hipMemcpyDeviceToHost, st);
        return r == hipSuccess ? hipEventRecord(c->stage_ev[b], st) : r;
    };
    if ((e = issue(0)) != hipSuccess) return e;
    for (size_t k = 0; k < nch; ++k) {
        // the next chunk's DMA lands in the buffer chunk k - 1 used, already copied out
        if (k + 1 < nch && (e = issue(k + 1)) != hipSuccess) return e;
        const int b = (int)(k & 1);
        if ((e = hipEventSynchronize(c->stage_ev[b])) != hipSuccess) return e;
        const size_t off = k * kStageChunk;
        c->pool->copy(static_cast<char*>(dst) + off, c->stage[b], std::min(kStageChunk, bytes - off));
    }
    return hipSuccess;
}

// the checked seeds (or root entries) into the block's pinned half and on to the device in stream order
template <typename D>
static int seeds_upload(eik_ctx* c, Stage<D>& s, const std::vector<D>& v, hipStream_t st) {
    const int64_t K = (int64_t)v.size();
    if (!s.ev) HIPCHK(c, hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(s.ev));  // the block's last upload (a never-recorded event is complete)
    if (s.cap < K) {
        if (s.h) (void)hipHostFree(s.h);
        if (s.d) (void)hipFree(s.d);
        s.h = s.d = nullptr;
        s.cap = 0;
        const int64_t cap = std::max<int64_t>(1024, K);
        HIPCHK(c, hipHostMalloc((void**)&s.h, sizeof(D) * cap));
        HIPCHK(c, hipMalloc((void**)&s.d, sizeof(D) * cap));
        s.cap = cap;
    }
    memcpy(s.h, v.data(), sizeof(D) * (size_t)K);
    HIPCHK(c, hipMemcpyAsync(s.d, s.h, sizeof(D) * (size_t)K, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(s.ev, st));
    return EIK_OK;
}

}  // namespace eik_api

extern "C" {

const char* eik_version(void) { return "eikonal-mi355x 0.1 (gfx950 block-FIM, 64x64 tiles)"; }

int eik_create(int device, eik_ctx** out) {
    if (!out) return set_err(nullptr, EIK_ERR_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_err(nullptr, EIK_ERR_NODEVICE, "no HIP device visible (the Eikonal solver has no CPU path)");
    if (device < 0 || device >= n) return set_err(nullptr, EIK_ERR_ARG, "device %d out of range [0,%d)", device, n);
    if (hipSetDevice(device) != hipSuccess) return set_err(nullptr, EIK_ERR_HIP, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return set_err(nullptr, EIK_ERR_HIP, "hipGetDeviceProperties failed");
    auto* c = new eik_ctx();
    c->device = device;
    c->cu_count = prop.multiProcessorCount;
    c->grid = 4 * c->cu_count;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return set_err(nullptr, EIK_ERR_HIP, "hipStreamCreate failed");
    }
    *out = c;
    return EIK_OK;
}

void eik_destroy(eik_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->cached) eik_fim2d_destroy(c->cached);
    if (c->cached_l) eik_fim2d_destroy(c->cached_l);
    if (c->cached_l64) eik_fim2d_destroy(c->cached_l64);
    if (c->cached_fronts) eik_fim2d_destroy(c->cached_fronts);
    if (c->h3) (void)hipHostFree(c->h3);
    if (c->h_q3) (void)hipHostFree(c->h_q3);
    for (hipEvent_t e : c->e3)
        if (e) (void)hipEventDestroy(e);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    for (int b = 0; b < 2; ++b) {
        if (c->stage[b]) (void)hipHostFree(c->stage[b]);
        if (c->stage_ev[b]) (void)hipEventDestroy(c->stage_ev[b]);
    }
    for (DescBlock& b : c->desc) {
        if (b.ev) {
            (void)hipEventSynchronize(b.ev);
            (void)hipEventDestroy(b.ev);
        }
        if (b.h) (void)hipHostFree(b.h);
        if (b.d) (void)hipFree(b.d);
    }
    if (c->h_diff) (void)hipHostFree(c->h_diff);
    for (hipEvent_t e : c->ev_diff)
        if (e) (void)hipEventDestroy(e);
    if (c->lab_seeds.ev) (void)hipEventSynchronize(c->lab_seeds.ev);
    c->lab_seeds.release();
    for (Seed3Stage* s : {&c->seeds3, &c->lab_seeds3}) {
        if (s->ev) (void)hipEventSynchronize(s->ev);
        s->release();
    }
    c->pool = nullptr;  // (the process-wide pool stays)
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* eik_last_error(const eik_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int eik_set_option(eik_ctx* c, int opt, double v) {
    if (!c) return EIK_ERR_ARG;
    switch (opt) {
        case EIK_OPT_MAX_ROUNDS: c->max_rounds = std::max(1, (int)v); break;
        case EIK_OPT_SYNC_EVERY: c->sync_every = std::max(1, (int)v); break;
        case EIK_OPT_TIMING: c->timing = v != 0; break;
        case EIK_OPT_GRID: c->grid = v > 0 ? (int)v : 4 * c->cu_count; break;
        case EIK_OPT_TOL: c->tol = v > 0 ? v : 0.0; break;
        case EIK_OPT_DELTA: c->delta = v > 0 ? v : 0.0; break;
        case EIK_OPT_MODE:
            if (v != EIK_MODE_LIST && v != EIK_MODE_PERSISTENT) return set_err(c, EIK_ERR_ARG, "bad mode %g", v);
            c->mode = (int)v;
            break;
        case EIK_OPT_QTIMEOUT: c->qtimeout_s = v > 0 ? v : 30.0; break;
        case EIK_OPT_MAX_VISITS: c->max_visits = v > 0 ? (unsigned long long)v : 0ull; break;
        case EIK_OPT_PASSES: c->passes = std::max(0, std::min(64, (int)v)); break;
        case EIK_OPT_FRESH_FIRST: c->fresh_first = v != 0; break;
        case EIK_OPT_SCHED: c->sched = std::max(0, std::min(3, (int)v)); break;
        case EIK_OPT_LIVE_PACK: c->live_pack = v != 0; break;
        case EIK_OPT_PRIO: c->prio = v; break;
        case EIK_OPT_PRIO_RING: c->prio_ring = v < 0 ? 0 : (int)std::min(v, 1073741824.0); break;
        case EIK_OPT_PRIO_DISPATCH: c->prio_dispatch = v < 0 ? 0 : (int)std::min(v, 128.0); break;
        case EIK_OPT_LAYER_PLANAR: c->layer_planar = v != 0; break;
        case EIK_OPT_SEEDS_LAYERED: c->seeds_layered = v != 0; break;
        case EIK_OPT_PATH_LOOP: c->path_loop = std::max(0, std::min(4, (int)v)); break;
        case EIK_OPT_EXACT_BAND: c->exact_band = v != 0; break;
        case EIK_OPT_WIDE: c->wide = v < 0 ? -1 : v != 0 ? 1 : 0; break;
        case EIK_OPT_DIFF_LOADS: c->diff_nt = v != 0; break;
        case EIK_OPT_DIFF_SHARE: c->diff_share = v < 0 ? -1.0 : v; break;
        case EIK_OPT_FRONTS_CAP: c->fronts_cap = v <= 0 ? 0.0 : v == 1 ? kFrontsMargin : std::max(1.0, v); break;
        default: return set_err(c, EIK_ERR_ARG, "unknown option %d", opt);
    }
    return EIK_OK;
}

int eik_get_stats(const eik_ctx* c, eik_stats* out) {
    if (!c || !out) return EIK_ERR_ARG;
    *out = c->last;
    return EIK_OK;
}

// ------------------------------------------------------------------------------ fim2d
// th: tile rows (64; the fp64 layered solver's tiles have fim2dl_rows(true) = 40)
// The default priority-band width (EIK_OPT_PRIO < 0; fp64 2D solves and the layered solver): 0.25 on
// a 4096^2 raster, growing with the raster's side -- the front's T range grows with it, and bands too
// narrow for it leave the queue to the open-ended last band.  Band-width A/B, 0.25 / 0.5 / 1:
//   C2 4096^2 fp64 2.14-2.16 / 2.15-2.19 / 2.17-2.20 ms; C4 16384^2 fp64 3.9-4.0 / 9.0-9.1 / 16.3-16.7
//   Gcells/s (profiles/r05ad_prio_width_ab.log, r05ae_c4_width_ab.log);
//   layered (C5's volume, tools/layered_scale_probe.py) fp64 4096^2 3.79 / 3.75 / 3.61, 8192^2 4.16 /
//   4.33 / 4.19, 16384^2 1.65 / 3.95 / 4.30; fp32 6.80 / 6.83 / 6.79, 7.78 / 8.02 / 7.86, 4.84 / 8.13 /
//   8.50 Gcells/s (the FIFO: fp64 2.89, 1.77, 1.29; fp32 6.63, 4.62, 3.11; profiles/r05af_*, r05ah_*).
// Below a side of min_side the FIFO is the default: the bands' dispatch latency outweighs the order on
// small rasters.  fp64 2D FIFO vs bands (0.25), ms: 1024^2 0.48 / 0.57, 2048^2 0.79 / 0.92, 2560^2 1.06 /
// 1.20, 3072^2 1.22 / 1.37, 3584^2 1.43 / 1.58, the C4 DEM at 4096^2 1.79 / 1.85 but C2's raster 2.35 /
// 2.15 (profiles/r05an_prio_size_2d.log, r05ao_prio_crossover.log, r05ap_c2_prio_vs_fifo_ab.log): 2D
// min_side 4096.  Layered (C5's volume) fp64 / fp32 FIFO vs bands, ms: 1024^2 2.34 / 2.55, 1.55 / 1.70;
// 2048^2 4.37 / 4.46, 2.61 / 2.86; 3072^2 8.49 / 7.75, 4.29 / 4.35: layered min_side 3072.
static double default_prio(int64_t H, int64_t W, double min_side) {
    const double side = std::sqrt((double)H * (double)W);
    if (side < min_side) return 0.0;
    return 0.25 * std::max(1.0, side / 4096.0);
}

// Priority bands' buffers for a solve of `tiles` tiles (fim_engine.hpp): kBands rings of a power of
// two >= 2 x the tiles (EIK_OPT_PRIO_RING: any power of two, tests), the per-tile band-membership
// words (at most one entry per (tile, band): a ring of >= tiles slots cannot lap) and the head /
// tail words, all cleared on the stream.  Fills a.bslot / bmask / bmem / bctl.  (The band-tagged
// FIFO entries hold tile + 1 in kBandTagShift bits: bands need tiles < 2^25 - 1.)
static hipError_t setup_bands(eik_ctx* c, DevBuf& bslot, DevBuf& bctl, int64_t tiles, Fim2dArgs& a, hipStream_t st) {
    uint64_t bc = 1024;
    while (bc < 2 * (uint64_t)tiles) bc <<= 1;
    if (c->prio_ring > 0) {  // (tests: a ring below the tile count can lap -> qerror bit 4 -> FIFO re-solve)
        bc = 1;
        while (bc < (uint64_t)c->prio_ring) bc <<= 1;
    }
    const size_t ring_bytes = sizeof(unsigned) * kBands * bc;
    const size_t mem_off = (ring_bytes + 255) & ~(size_t)255;
    const size_t bytes = mem_off + sizeof(unsigned long long) * (size_t)tiles;
    hipError_t e = bslot.ensure(bytes);
    if (e == hipSuccess) e = bctl.ensure(128 * kBands + 128);  // + the band width's word
    if (e == hipSuccess) e = hipMemsetAsync(bslot.p, 0, bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(bctl.p, 0, 128 * kBands, st);
    if (e != hipSuccess) return e;
    a.bslot = (unsigned*)bslot.p;
    a.bmask = (unsigned)(bc - 1);
    a.bmem = (unsigned long long*)((char*)bslot.p + mem_off);
    a.bctl = (unsigned long long*)bctl.p;
    return hipSuccess;
}

static int fim2d_create_rows(eik_ctx* c, int64_t B, int64_t H, int64_t W, int dtype, int th, eik_fim2d** out) {
    if (!c || !out) return EIK_ERR_ARG;
    *out = nullptr;
    if (B < 1 || H < 1 || W < 1) return set_err(c, EIK_ERR_ARG, "bad shape B=%ld H=%ld W=%ld", (long)B, (long)H, (long)W);
    if (dtype != EIK_F32 && dtype != EIK_F64) return set_err(c, EIK_ERR_ARG, "bad dtype %d", dtype);
    const int64_t ntx = (W + kTile - 1) / kTile, nty = (H + th - 1) / th;
    const int64_t tiles = B * ntx * nty;
    if (tiles >= (1ll << 31) - 8) return set_err(c, EIK_ERR_ARG, "too many tiles");
    HIPCHK(c, hipSetDevice(c->device));
    auto* f = new eik_fim2d();
    f->ctx = c;
    f->B = B;
    f->H = H;
    f->W = W;
    f->f64 = dtype == EIK_F64;
    f->stream = c->stream;
    Fim2dArgs& a = f->a;
    a.H = H;
    a.W = W;
    a.ntx = (int)ntx;
    a.nty = (int)nty;
    a.tiles_per_map = (int)(ntx * nty);
    a.capacity = (int)tiles;
    for (auto& g : a.ghost) g = nullptr;
    a.ls = 1;
    a.z0 = 0;
    a.lzs = 1;
    // FIFO slots: a power of two with ample headroom over the tiles (each tile holds at most one
    // filled slot; the margin keeps a slow poller's slot from being lapped by the tail)
    uint64_t q = 4096;
    while (q < 8 * (uint64_t)tiles) q <<= 1;
    hipError_t e = hipSuccess;
    if ((e = f->lists.ensure(sizeof(int) * 3 * tiles)) != hipSuccess ||
        (e = f->qctl.ensure(kQueueCtlBytes)) != hipSuccess || (e = f->qslot.ensure(sizeof(unsigned) * q)) != hipSuccess ||
        (e = f->qstate.ensure(sizeof(unsigned) * tiles)) != hipSuccess ||
        (e = hipHostMalloc((void**)&f->h_q, kQueueCtlBytes)) != hipSuccess ||
        (e = f->counts.ensure(sizeof(int) * 64)) != hipSuccess || (e = f->mark.ensure(sizeof(unsigned) * tiles)) != hipSuccess ||
        (e = f->key.ensure(sizeof(unsigned) * tiles)) != hipSuccess ||
        (e = f->edge.ensure(sizeof(unsigned) * 4)) != hipSuccess || (e = f->goals.ensure(sizeof(int64_t) * 2 * B)) != hipSuccess ||
        (e = f->ecol.ensure((dtype == EIK_F64 ? 8 : 4) * 2 * kTile * (size_t)tiles)) != hipSuccess ||
        (e = hipHostMalloc((void**)&f->h_counts, sizeof(int) * 64)) != hipSuccess ||
        (e = hipHostMalloc((void**)&f->h_visits, 3 * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipHostMalloc((void**)&f->h_goals, sizeof(int64_t) * 2 * B)) != hipSuccess ||
        (e = hipEventCreate(&f->ev_start)) != hipSuccess || (e = hipEventCreate(&f->ev_stop)) != hipSuccess) {
        eik_fim2d_destroy(f);
        return set_err(c, EIK_ERR_NOMEM, "fim2d allocation: %s", hipGetErrorString(e));
    }
    a.lists = (int*)f->lists.p;
    a.ecol = f->ecol.p;
    a.counts = (int*)f->counts.p;
    a.mark = (unsigned*)f->mark.p;
    a.key = (unsigned*)f->key.p;
    a.minkey = (unsigned*)f->counts.p + 16;
    // the visit counters sit in the queue words' block (own 128-B line): one read-back after a
    // persistent launch brings both
    a.visits = (unsigned long long*)((char*)f->qctl.p + kVisitsOff);
    a.edge_dirty = nullptr;
    a.qhead = (unsigned long long*)f->qctl.p;
    a.qtail = (unsigned long long*)((char*)f->qctl.p + 64);
    a.qactive = (int*)((char*)f->qctl.p + 128);
    a.qerror = (unsigned*)((char*)f->qctl.p + 192);
    a.qslot = (unsigned*)f->qslot.p;
    a.qmask = (unsigned)(q - 1);
    a.qstate = (unsigned*)f->qstate.p;
    // safety cap: a monotone solve visits each tile a bounded number of times; negative costs
    // (invalid input on a device buffer) would otherwise iterate forever.
    f->max_iters = 64 * (ntx + nty) + 8 * tiles / B + 4096;
    *out = f;
    return EIK_OK;
}

// The solver cached in `slot`, reused when it is one of B maps of H x W cells of this dtype, else remade in
// tiles of th rows.  Every slot compares what the host entries' slot always did: the layered slots are per
// dtype and the coarse fronts' solver is always B = 2 fp64, so for them only H and W ever differ.  Destroy,
// clear the slot, then create: a failed create leaves the slot empty.
static int cached_solver(eik_ctx* c, eik_fim2d*& slot, int64_t B, int64_t H, int64_t W, int dtype, int th, eik_fim2d** out) {
    eik_fim2d* f = slot;
    if (f && f->B == B && f->H == H && f->W == W && (int)f->f64 == (dtype == EIK_F64)) {
        *out = f;
        return EIK_OK;
    }
    if (f) eik_fim2d_destroy(f);
    slot = nullptr;
    int rc = fim2d_create_rows(c, B, H, W, dtype, th, &f);
    if (rc) return rc;
    slot = f;
    *out = f;
    return EIK_OK;
}

int eik_fim2d_create(eik_ctx* c, int64_t B, int64_t H, int64_t W, int dtype, eik_fim2d** out) {
    return fim2d_create_rows(c, B, H, W, dtype, kTile, out);
}

void eik_fim2d_destroy(eik_fim2d* f) {
    if (!f) return;
    if (f->h_counts) (void)hipHostFree(f->h_counts);
    if (f->h_visits) (void)hipHostFree(f->h_visits);
    if (f->h_goals) (void)hipHostFree(f->h_goals);
    if (f->h_q) (void)hipHostFree(f->h_q);
    if (f->ev_start) (void)hipEventDestroy(f->ev_start);
    if (f->ev_stop) (void)hipEventDestroy(f->ev_stop);
    if (f->box) (void)hipHostFree(f->box);
    if (f->h_rects) (void)hipHostFree(f->h_rects);
    if (f->h_info) (void)hipHostFree(f->h_info);
    f->sd.release();
    f->roots.release();
    for (hipEvent_t ev : f->ev_rp)
        if (ev) (void)hipEventDestroy(ev);
    for (auto ev : f->ev_pool) (void)hipEventDestroy(ev);
    delete f;
}

// the queue counters of the last persistent launch (EIK_QDEBUG builds; zeros otherwise)
int eik_fim2d_qcount(const eik_fim2d* f, uint64_t out[8]) {
    if (!f || !out) return EIK_ERR_ARG;
    memcpy(out, (const char*)f->h_q + kVisitsOff + 24, 8 * sizeof(uint64_t));
    return EIK_OK;
}

int eik_fim2d_set_ghosts(eik_fim2d* f, void* n, void* s, void* w, void* e) {
    if (!f) return EIK_ERR_ARG;
    if (f->B != 1) return set_err(f->ctx, EIK_ERR_ARG, "ghost strips need B == 1");
    f->a.ghost[0] = n;
    f->a.ghost[1] = s;
    f->a.ghost[2] = w;
    f->a.ghost[3] = e;
    f->a.edge_dirty = (n || s || w || e) ? (unsigned*)f->edge.p : nullptr;
    return EIK_OK;
}

// Bind the buffers and the stream and set a solve's options, budgets and priority bands: everything of
// eik_fim2d_start but the goals' upload and the init / seed kernels (eik_fim2d_update and
// eik_fim2d_adopt restart a solve without wiping T).
static int fim2d_configure(eik_fim2d* f, const void* d_cost, void* d_T, void* stream) {
    eik_ctx* c = f->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    f->stream = (hipStream_t)stream;  // as given: NULL is the default (null) stream
    f->a.cost = d_cost;
    f->a.T = d_T;
    f->a.iter = 0;
    f->a.max_rounds = c->max_rounds;
    f->a.keep = (float)(1.0 - c->tol);
    f->a.delta = c->delta > 0 ? (float)c->delta : __builtin_inff();
    // persistent mode needs 32-bit byte offsets per map (buffer resources) and no ordering window
    const bool fits = f->H * f->W * (f->f64 ? 8 : 4) < (int64_t)UINT32_MAX;
    f->a.mode = (c->mode == kModePersistent && fits && !(c->delta > 0)) ? kModePersistent : kModeList;
    f->a.qtimeout = (unsigned long long)(c->qtimeout_s * 1e8);  // s_memrealtime: 100 MHz
    // in-place passes: a single map's solve is front-latency-bound (long in-place refinement of
    // the front tiles pays), a batch is throughput-bound (hand the workgroup to tiles with fresher
    // halos early): C2 2.07-2.09 ms at 8-16 vs 2.23 at 2; C3 6.86 ms at 2 vs 8.0 at 8.  Single map
    // 24 (profiles/r01g_passes_8_16_24.log): C2 2.03-2.04 ms vs 2.05-2.08 at 16 (within noise),
    // C4 at one GPU 16.4-16.6 vs 16.3-16.4 at 16 (within noise); 8 is clearly slower on both.
    // A single map large enough for the 4-waves-per-SIMD kernel (>= kWideTiles tiles, 16384^2) is
    // throughput-bound: 16 passes, 17.1-17.3 -> 18.3-18.9 Gcells/s (profiles/r02w_passes_wide.log).
    // A few large maps (biComputeTmap's two fronts: B = 2 of 4096^2) are latency-bound like one map.
    const bool batch = f->B > 4 || (f->B > 1 && f->a.tiles_per_map < 1024);
    // One map (round 3, profiles/r03v_passes_f64_c2_ab.log): 40 -- C2 fp64 2.461-2.468 ms at 24,
    // 2.394-2.420 at 40; fp32 1.733-1.748 at 24, 1.723-1.726 at 40.
    f->a.max_passes = c->passes > 0 ? c->passes
                      : batch                                             ? 2
                      : (!f->f64 && f->a.tiles_per_map >= kWideTiles)     ? 16
                                                                          : 40;
    // The default visit budget, 1024 per tile (in-place passes count), x the raster's elongation: a
    // tile is re-visited as corrections travel down the chain of tiles behind it, and that chain is
    // ntx + nty long -- 2 sqrt(tiles) on a square raster (factor 1), but the whole raster on a strip.
    // Measured on valid 3-cell-wide U(1, 10) strips, visits + passes per tile: 1024 tiles 830 (fp32) /
    // 980 (fp64), 16384 tiles 2350 / 1590 -- the flat 1024 per tile reported the latter as not converging.
    const double elong = std::max(1.0, (f->a.ntx + f->a.nty) / (2.0 * std::sqrt((double)f->a.tiles_per_map)));
    f->a.qbudget = c->max_visits ? c->max_visits
                                 : (unsigned long long)(1024.0 * elong * (double)(f->B * f->a.tiles_per_map)) + (1ull << 20);
    f->iterations = 0;
    f->host_syncs = 0;
    f->sweep_ms = 0.0;
    f->solve_ms = 0.0;
    f->ev_used = 0;
    HIPCHK(c, hipEventRecord(f->ev_start, f->stream));
    // priority bands (persistent mode): kBands rings of twice the tiles each (a pending tile has at
    // most one live entry per band it was pushed to plus stale ones, dropped when taken), cleared
    // with the queue before the seed kernel pushes the goal's tile
    f->a.bctl = nullptr;
    // (one map or a few: a batch of independent maps keeps the FIFO -- their keys do not compare)
    // (a domain-decomposition block -- ghost strips bound -- keeps the bands at any size, at width >= 1:
    // they order the ghosts' arrivals, whose T spans the whole raster's range, not the block's.  The
    // 16384^2 4 x 2 rehearsal: FIFO 3.7x the single domain's visits, width 1 0.96x (22 ms), the
    // block-sized 0.35 2.96x (61 ms), profiles/r05d_c4_rehearsal_n8_*.json, r05h_c4_rehearsal_n8.log)
    const bool dd_block = f->a.ghost[0] || f->a.ghost[1] || f->a.ghost[2] || f->a.ghost[3];
    // fp32 keeps the FIFO below kWideTiles tiles (its passes are twice as fast and the one dispatcher held
    // it back: C2 fp32 1.6 -> 1.9 ms with bands, round 5); one map of >= kWideTiles tiles takes the bands
    // since the 128-entry dispatches (round 6: C4 at one GPU fp32 18.4 -> 19.5 Gcells/s mean of 5 same-box
    // alternations, 145 k -> 108 k visits, profiles/r06s7/r06s7_c4f32_prio_ab{,2}.log)
    const bool f32_wide = !f->f64 && f->B == 1 && f->a.tiles_per_map >= kWideTiles && !dd_block;
    // (the tile count is fp32's gate, as include/eikonal.h states it: a thin raster of >= kWideTiles
    // tiles can have fewer than 4096^2 cells, and took 16 passes and the wide form but no bands)
    const double prio = c->prio >= 0 ? c->prio
                        : f32_wide ? default_prio(f->H, f->W, 0.0)
                        : !f->f64  ? 0.0
                        : dd_block ? std::max(1.0, default_prio(f->H, f->W, 0.0))
                                   : default_prio(f->H, f->W, 4096.0);
    if (prio > 0 && f->a.mode == kModePersistent && f->B <= 2 && !f->no_bands && f->a.capacity < (1 << kBandTagShift) - 1) {
        // (a decomposition block's launch lives through many halo rounds: the band-membership bits
        // bound every band to one entry per tile however many pending episodes its tiles go through;
        // round 5 gave blocks 16 x the tiles per ring instead, which only moved the threshold)
        HIPCHK(c, setup_bands(c, f->bslot, f->bctl, f->a.capacity, f->a, f->stream));
        float* pd = (float*)((char*)f->bctl.p + 128 * kBands);
        HIPCHK(c, fim2d_prio_delta(d_cost, f->f64, f->H * f->W, (float)prio, pd, f->stream));
        f->a.pdelta = pd;
        f->a.disp = c->prio_dispatch > 0 ? (unsigned)c->prio_dispatch
                                         : f->a.tiles_per_map >= kWideTiles ? 128u : 16u;  // (fim_engine.hpp band_dispatch)
    }
    // eik_last_form (the launch fills in the kernel's form)
    c->last_form[0] = 0;
    c->last_form[1] = f->a.bctl != nullptr;
    c->last_form[2] = f->a.max_passes;
    c->last_form[3] = f->a.bctl ? (int64_t)f->a.disp : 0;
    f->last_active = -1;  // unknown until a launch's queue words are read back
    return EIK_OK;
}

static int upload_goals(eik_fim2d* f, const int64_t* goals) {
    // (the previous solve on this solver synchronised before returning: h_goals is free)
    memcpy(f->h_goals, goals, sizeof(int64_t) * 2 * f->B);
    HIPCHK(f->ctx, hipMemcpyAsync(f->goals.p, f->h_goals, sizeof(int64_t) * 2 * f->B, hipMemcpyHostToDevice, f->stream));
    return EIK_OK;
}

int eik_fim2d_start(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* goals, void* stream) {
    if (!f || !d_cost || !d_T || !goals) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    int rc = fim2d_configure(f, d_cost, d_T, stream);
    if (!rc) rc = upload_goals(f, goals);
    if (rc) return rc;
    HIPCHK(c, fim2d_init(f->a, f->f64, (int)f->B, (const int64_t*)f->goals.p, (unsigned*)f->edge.p, f->stream));
    f->started = true;
    f->seeded = false;
    f->need_rewind = false;  // the init cleared the queue words
    return EIK_OK;
}

// ---- multi-source solves (seeds.hip)
// Seed k's start value as the 2D and the 3D solvers take it (seeds_check, seeds3_check): finite and >= 0,
// rounded to the dtype without reaching +inf, -0 as +0.
static int seed_t0(eik_ctx* c, const char* who, const double* t0, int64_t k, bool f64, double* out) {
    double v = t0 ? t0[k] : 0.0;
    if (!(v >= 0.0) || std::isinf(v))
        return set_err(c, EIK_ERR_ARG, "%s: t0[%ld] = %g (finite and >= 0 needed)", who, (long)k, v);
    if (!f64) {
        v = (double)(float)v;
        if (std::isinf(v)) return set_err(c, EIK_ERR_ARG, "%s: t0[%ld] = %g rounds to +inf in fp32", who, (long)k, t0[k]);
    }
    *out = v + 0.0;  // (+ 0.0: -0 -> +0, values order like their bits)
    return EIK_OK;
}

// The host checks shared by the seeded start and the labels: on EIK_OK out holds the K descriptors,
// t0 rounded to the dtype.  Every failure is EIK_ERR_ARG with the offending index; nothing is launched.
static int seeds_check(eik_ctx* c, const char* who, int64_t B, int64_t H, int64_t W, bool f64, const int64_t* seeds,
                       const double* t0, const int32_t* map_of, int64_t K, std::vector<SeedDesc>& out) {
    if (K < 1 || K > kMaxSeeds) return set_err(c, EIK_ERR_ARG, "%s: K = %ld seeds (1 .. 2^24)", who, (long)K);
    if (!seeds) return set_err(c, EIK_ERR_ARG, "%s: seeds is NULL", who);
    if (!map_of && B != 1)
        return set_err(c, EIK_ERR_ARG, "%s: map_of is NULL with B = %ld maps (B == 1 needed)", who, (long)B);
    out.resize((size_t)K);
    for (int64_t k = 0; k < K; ++k) {
        const int64_t x = seeds[2 * k], y = seeds[2 * k + 1];
        if (x < 0 || y < 0 || x >= W || y >= H)
            return set_err(c, EIK_ERR_ARG, "%s: seed %ld (%ld, %ld) outside %ldx%ld", who, (long)k, (long)x, (long)y, (long)H,
                           (long)W);
        const int32_t m = map_of ? map_of[k] : 0;
        if (m < 0 || m >= B) return set_err(c, EIK_ERR_ARG, "%s: map_of[%ld] = %d outside [0, %ld)", who, (long)k, m, (long)B);
        double v = 0.0;
        const int rc = seed_t0(c, who, t0, k, f64, &v);
        if (rc) return rc;
        out[k] = SeedDesc{(int32_t)x, (int32_t)y, m, 0, v};
    }
    return EIK_OK;
}

// eik_fim2d_start_seeds' own checks: what it refuses, then the seeds into v
static int start_seeds_check(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* seeds, const double* t0,
                             const int32_t* map_of, int64_t K, std::vector<SeedDesc>& v) {
    if (!f) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    const char* who = "eik_fim2d_start_seeds";
    if (!d_cost || !d_T) return set_err(c, EIK_ERR_ARG, "%s: %s is NULL", who, !d_cost ? "d_cost" : "d_T");
    if (f->lnl) return set_err(c, EIK_ERR_ARG, "%s: not for a layered block", who);
    if (f->a.ghost[0] || f->a.ghost[1] || f->a.ghost[2] || f->a.ghost[3])
        return set_err(c, EIK_ERR_ARG, "%s: not for a domain-decomposition block (ghost strips are bound)", who);
    return seeds_check(c, who, f->B, f->H, f->W, f->f64, seeds, t0, map_of, K, v);
}

// The seeded start from checked descriptors.  v by value: it becomes the bound list, and a caller that starts
// again from the bound list (solve_bound) passes f->bound itself.
static int start_seeds_desc(eik_fim2d* f, const void* d_cost, void* d_T, std::vector<SeedDesc> v, void* stream) {
    eik_ctx* c = f->ctx;
    int rc = fim2d_configure(f, d_cost, d_T, stream);
    if (rc) return rc;
    // the ordinary init with no goal on any map (a goal outside the map seeds nothing), then the seeds
    std::vector<int64_t> none(2 * (size_t)f->B, -1);
    rc = upload_goals(f, none.data());
    if (!rc) rc = seeds_upload(c, f->sd, v, f->stream);
    if (rc) return rc;
    HIPCHK(c, fim2d_init(f->a, f->f64, (int)f->B, (const int64_t*)f->goals.p, (unsigned*)f->edge.p, f->stream));
    HIPCHK(c, fim2d_start_seeds(f->a, f->f64, f->sd.d, (int64_t)v.size(), f->stream));
    f->started = true;
    f->seeded = true;
    f->bound = std::move(v);
    f->need_rewind = false;  // the init cleared the queue words
    return EIK_OK;
}

int eik_fim2d_start_seeds(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* seeds, const double* t0,
                          const int32_t* map_of, int64_t K, void* stream) {
    std::vector<SeedDesc> v;
    const int rc = start_seeds_check(f, d_cost, d_T, seeds, t0, map_of, K, v);
    return rc ? rc : start_seeds_desc(f, d_cost, d_T, std::move(v), stream);
}

// the persistent launch's queue words (h_q, read back after it): errors and the active count
static int persist_result(eik_fim2d* f, int64_t* active) {
    eik_ctx* c = f->ctx;
    const unsigned err = f->h_q[kQErrorWord];
    f->band_overflow = (err & 4u) != 0u;
    if (f->band_overflow)
        return set_err(c, EIK_ERR_HIP, "persistent solver: a priority band's ring is full (EIK_OPT_PRIO=0 "
                                       "uses the FIFO; eik_fim2d_solve falls back by itself)");
    if (err & 1u)
        return set_err(c, EIK_ERR_HIP, "persistent solver: a queue wait exceeded %.1f s (EIK_OPT_QTIMEOUT)",
                       c->qtimeout_s);
    if (err & 2u)
        return set_err(c, EIK_ERR_NOCONVERGE, "no convergence within %llu tile visits (negative costs?)",
                       (unsigned long long)f->a.qbudget);
    f->last_active = f->h_q[kQActiveWord];
    if (active) *active = f->h_q[kQActiveWord];
    return EIK_OK;
}

static int drain_timing(eik_fim2d* f) {
    // events were recorded in (start, stop) pairs; the stream has been synchronised
    for (size_t i = 0; i + 1 < f->ev_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, f->ev_pool[i], f->ev_pool[i + 1]) == hipSuccess) f->sweep_ms += ms;
    }
    f->ev_used = 0;
    return EIK_OK;
}

// A persistent launch's idle waiters take tickets past the tail; eik_fim2d_solve skips the rewind
// kernel after its launch, so before anything appends to the same queue again (merge_ghost, the
// next iterate) the ticket counter is restarted at the tail.
static hipError_t rewind_if_needed(eik_fim2d* f) {
    if (!f->need_rewind) return hipSuccess;
    f->need_rewind = false;
    return fim2d_qrewind(f->a, f->stream);
}

// ---- a layered volume's block in a domain decomposition (split in x-y, the
// layers stay together): the layered solver (fim2dl.hip) with ghost strips of nl values per edge
// cell, driven by the relaunch schedule (eikonal/dd.py solve: iterate to local convergence, pack,
// exchange, merge)
int eik_fim3dl_create(eik_ctx* c, int64_t H, int64_t W, int64_t L, int z0, int nl, int dtype, eik_fim2d** out) {
    if (!c || !out) return EIK_ERR_ARG;
    const int kmax = dtype == EIK_F64 ? 3 : 4;
    if (nl < 1 || nl > kmax || z0 < 0 || z0 + nl > L)
        return set_err(c, EIK_ERR_ARG, "layered block: nl=%d z0=%d L=%ld (nl <= %d)", nl, z0, (long)L, kmax);
    // the layered kernel addresses T through one buffer resource per tile row band and layer: 32-bit
    // byte offsets over (rows + 2) raster rows of W cells of L values (fim3d_solve_one's gate)
    const int64_t esz = dtype == EIK_F64 ? 8 : 4;
    if (W < 1 || L < 1 || (fim2dl_rows(dtype == EIK_F64) + 2) * W * L * esz >= (int64_t)UINT32_MAX)
        return set_err(c, EIK_ERR_ARG, "layered block: a tile row band of W=%ld x L=%ld exceeds 4 GiB", (long)W, (long)L);
    const int rc = fim2d_create_rows(c, 1, H, W, dtype, fim2dl_rows(dtype == EIK_F64), out);
    if (rc) return rc;
    (*out)->lnl = nl;
    (*out)->lz0 = z0;
    (*out)->lL = L;
    return EIK_OK;
}

int eik_fim3dl_start(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t goal[3], void* stream) {
    if (!f || !f->lnl || !d_cost || !d_T || !goal) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    f->stream = (hipStream_t)stream;
    Fim2dArgs& a = f->a;
    a.cost = d_cost;
    a.T = d_T;
    a.ls = f->lL;
    a.z0 = f->lz0;
    a.lzs = 1;
    a.mode = kModePersistent;
    a.max_rounds = 1;
    a.keep = (float)(1.0 - c->tol);
    a.delta = __builtin_inff();
    a.edge_dirty = nullptr;
    a.bctl = nullptr;
    a.qhold = nullptr;
    a.live = nullptr;
    a.qtimeout = (unsigned long long)(c->qtimeout_s * 1e8);
    a.max_passes = c->passes > 0 ? c->passes : 24;  // the layered solver's (solve_layered)
    a.qbudget = c->max_visits ? c->max_visits : 1024ull * (unsigned long long)a.tiles_per_map + (1ull << 20);
    a.fresh_first = c->fresh_first;
    f->iterations = 0;
    f->host_syncs = 0;
    f->sweep_ms = f->solve_ms = 0.0;
    HIPCHK(c, hipMemsetAsync((void*)a.visits, 0, 3 * sizeof(unsigned long long), f->stream));
    // (the FIFO: priority bands on these blocks were measured slower -- 2048^2 x 3 in 2 x 2 blocks, fp64
    // 99 -> 108 ms, fp32 40 -> 44 ms, the same visits; the relaunch schedule has no work inflation for
    // them to remove, profiles/r05as_dd_layered_prio_probe.log)
    const bool in = goal[0] >= 0 && goal[1] >= 0 && goal[0] < f->W && goal[1] < f->H;
    if (in && (goal[2] < f->lz0 || goal[2] >= f->lz0 + f->lnl))
        return set_err(c, EIK_ERR_ARG, "goal layer %ld outside the solved layers", (long)goal[2]);
    // (a block without the goal: no seed -- its first launch ends at once, its ghosts bring the front)
    HIPCHK(c, fim2dl_init(a, f->f64, in ? goal[0] : -1, goal[1], goal[2] - f->lz0, f->H * f->W * f->lL, f->stream));
    f->started = true;
    f->need_rewind = false;
    return EIK_OK;
}

int eik_fim2d_iterate(eik_fim2d* f, int64_t max_iters, int64_t* active) {
    if (!f || !f->started) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (f->lnl) {  // a layered block: one persistent launch to local convergence (fim2dl.hip)
        if (max_iters < 1) {
            if (active) *active = -1;
            return EIK_OK;
        }
        int& res = c->resident_l[f->f64 ? 1 : 0][f->lnl];
        if (res == 0) res = fim2dl_persist_resident(f->lnl, f->f64, c->cu_count);
        const int g = std::min(c->grid > 0 ? c->grid : 4 * c->cu_count, res);
        HIPCHK(c, hipEventRecord(f->ev_start, f->stream));
        HIPCHK(c, fim2dl_persist(f->a, f->lnl, f->f64, g, f->stream));  // (+ the queue rewind)
        HIPCHK(c, hipEventRecord(f->ev_stop, f->stream));
        ++f->iterations;
        HIPCHK(c, hipMemcpyAsync(f->h_q, f->qctl.p, kQueueCtlBytes, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(c, hipStreamSynchronize(f->stream));
        ++f->host_syncs;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, f->ev_start, f->ev_stop) == hipSuccess) f->solve_ms += ms;
        memcpy(f->h_visits, (const char*)f->h_q + kVisitsOff, 3 * sizeof(unsigned long long));
        return persist_result(f, active);
    }
    int64_t done = 0;
    int h = 1;
    const int grid = c->grid > 0 ? c->grid : 4 * c->cu_count;
    if (f->a.mode == kModePersistent) {  // one launch runs the local solve to its fixed point
        if (max_iters < 1) {
            if (active) *active = -1;
            return EIK_OK;
        }
        if (c->timing) {
            while (f->ev_pool.size() < f->ev_used + 2) {
                hipEvent_t ev;
                HIPCHK(c, hipEventCreate(&ev));
                f->ev_pool.push_back(ev);
            }
            HIPCHK(c, hipEventRecord(f->ev_pool[f->ev_used++], f->stream));
        }
        const bool wide = wide_form(f);
        const int g = std::min(grid, persist_resident(f, wide));
        c->last_form[0] = wide;
        f->a.fresh_first = c->fresh_first;
        f->a.sched = c->sched;
        f->a.live_pack = c->live_pack;
        // eik_fim2d_solve launches without the queue rewind (the next solve's init clears the
        // queue); a later merge_ghost / iterate on the same solve issues it first (need_rewind)
        HIPCHK(c, rewind_if_needed(f));
        HIPCHK(c, fim2d_persist(f->a, f->f64, g, f->stream, wide, !f->defer_sync));
        f->need_rewind = f->defer_sync;
        if (c->timing) HIPCHK(c, hipEventRecord(f->ev_pool[f->ev_used++], f->stream));
        ++f->iterations;
        HIPCHK(c, hipMemcpyAsync(f->h_q, f->qctl.p, kQueueCtlBytes, hipMemcpyDeviceToHost, f->stream));
        if (f->defer_sync) return EIK_OK;  // eik_fim2d_solve: one synchronisation for the whole solve
        HIPCHK(c, hipStreamSynchronize(f->stream));
        ++f->host_syncs;
        if (c->timing) drain_timing(f);
        return persist_result(f, active);
    }
    while (done < max_iters) {
        const int64_t K = std::min<int64_t>(c->sync_every, max_iters - done);
        for (int64_t k = 0; k < K; ++k) {
            f->a.iter = (unsigned)f->iterations;
            if (c->timing) {
                while (f->ev_pool.size() < f->ev_used + 2) {
                    hipEvent_t ev;
                    HIPCHK(c, hipEventCreate(&ev));
                    f->ev_pool.push_back(ev);
                }
                HIPCHK(c, hipEventRecord(f->ev_pool[f->ev_used++], f->stream));
            }
            HIPCHK(c, fim2d_sweep(f->a, f->f64, grid, f->stream));
            if (c->timing) HIPCHK(c, hipEventRecord(f->ev_pool[f->ev_used++], f->stream));
            ++f->iterations;
        }
        done += K;
        HIPCHK(c, hipMemcpyAsync(f->h_counts, (int*)f->counts.p + (f->iterations % 3), sizeof(int),
                                 hipMemcpyDeviceToHost, f->stream));
        HIPCHK(c, hipStreamSynchronize(f->stream));
        ++f->host_syncs;
        if (c->timing) drain_timing(f);
        h = f->h_counts[0];
        if (h == 0) break;
    }
    if (active) *active = h;
    return EIK_OK;
}

int eik_fim2d_active(eik_fim2d* f, int64_t* active) {
    if (!f || !active) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    if (f->a.mode == kModePersistent) {
        HIPCHK(c, hipMemcpyAsync(f->h_q, f->qctl.p, kQueueCtlBytes, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(c, hipStreamSynchronize(f->stream));
        *active = f->h_q[kQActiveWord];
        return EIK_OK;
    }
    HIPCHK(c, hipMemcpyAsync(f->h_counts, (int*)f->counts.p + (f->iterations % 3), sizeof(int), hipMemcpyDeviceToHost,
                             f->stream));
    HIPCHK(c, hipStreamSynchronize(f->stream));
    *active = f->h_counts[0];
    return EIK_OK;
}

static void fill_stats(const eik_fim2d* f, eik_stats* out);

// Wait for a solve's stream: poll first (a blocking wait's wake-up cost ~20 us per solve on the
// C2 raster, ~1 % of it), then block for long solves.
static hipError_t wait_stream(hipStream_t st) {
    static const int spin_on = [] {
        const char* v = getenv("EIK_WAIT_SPIN");
        return v ? atoi(v) : 1;
    }();
    if (!spin_on) return hipStreamSynchronize(st);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if ((spin & 63u) == 63u &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.02)
            return hipStreamSynchronize(st);
        __builtin_ia32_pause();
    }
}

// the stop event and the visit counters after the solve's launches, then ONE synchronisation
// (the persistent launch's queue words were queued for read-back behind it)
static int finish_solve(eik_fim2d* f, int64_t* active) {
    eik_ctx* c = f->ctx;
    HIPCHK(c, hipEventRecord(f->ev_stop, f->stream));
    const bool persist = f->a.mode == kModePersistent;  // h_q (queued after the launch) holds the counters
    if (!persist)
        HIPCHK(c, hipMemcpyAsync(f->h_visits, (void*)f->a.visits, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                 f->stream));
    HIPCHK(c, wait_stream(f->stream));
    ++f->host_syncs;
    if (persist) memcpy(f->h_visits, (const char*)f->h_q + kVisitsOff, 3 * sizeof(unsigned long long));
    if (c->timing) drain_timing(f);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, f->ev_start, f->ev_stop);
    f->solve_ms = ms;
    fill_stats(f, &c->last);
    return f->a.mode == kModePersistent ? persist_result(f, active) : EIK_OK;
}

// One solve to convergence: start() binds the buffers and seeds the field (from goals or from a seed list;
// it checks its own arguments, f among them), the iteration runs with the synchronisation deferred to the
// finish.
extern "C++" {
template <typename Start>
static int solve_loop(eik_fim2d* f, Start start) {
    int64_t active = 0;
    int rc = EIK_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        rc = start();
        if (rc) return rc;
        f->defer_sync = f->a.mode == kModePersistent;
        rc = eik_fim2d_iterate(f, f->max_iters, &active);
        f->defer_sync = false;
        if (!rc) rc = finish_solve(f, &active);  // (the persistent launch's error word is read here)
        if (!(rc && f->band_overflow)) break;
        // a priority band's ring was full: solve again from the same start with the FIFO (this solver
        // keeps it); finish_solve waited for the stream
        f->band_overflow = false;
        f->no_bands = true;
    }
    if (rc) return rc;
    if (active != 0)
        return set_err(f->ctx, EIK_ERR_NOCONVERGE, "no convergence after %ld iterations (negative costs?)",
                       (long)f->iterations);
    return EIK_OK;
}
}  // extern "C++"

int eik_fim2d_solve(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* goals, void* stream) {
    return solve_loop(f, [&] { return eik_fim2d_start(f, d_cost, d_T, goals, stream); });
}

static int solve_seeds_desc(eik_fim2d* f, const void* d_cost, void* d_T, const std::vector<SeedDesc>& v, void* stream) {
    return solve_loop(f, [&] { return start_seeds_desc(f, d_cost, d_T, v, stream); });
}

int eik_fim2d_solve_seeds(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* seeds, const double* t0,
                          const int32_t* map_of, int64_t K, void* stream) {
    std::vector<SeedDesc> v;
    const int rc = start_seeds_check(f, d_cost, d_T, seeds, t0, map_of, K, v);
    return rc ? rc : solve_seeds_desc(f, d_cost, d_T, v, stream);
}

// A solve from scratch from what the solver is bound to (one map: replan_gate passed): the goal of the last
// start / adopt, or the bound seed list.
static int solve_bound(eik_fim2d* f, const void* d_cost, void* d_T, void* stream) {
    if (f->seeded) return solve_seeds_desc(f, d_cost, d_T, f->bound, stream);
    const int64_t g[2] = {f->h_goals[0], f->h_goals[1]};  // (a copy: the start writes h_goals)
    return eik_fim2d_solve(f, d_cost, d_T, g, stream);
}

// the labels from checked descriptors (fewer than 2^31 cells in all)
static int labels2d_desc(eik_ctx* c, const void* d_T, bool f64, int64_t B, int64_t H, int64_t W, const std::vector<SeedDesc>& v,
                         int32_t* d_label, hipStream_t st) {
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = B * H * W;
    HIPCHK(c, c->lab_work.ensure(sizeof(int) * (size_t)n + sizeof(unsigned) * kLabelPasses));
    const int rc = seeds_upload(c, c->lab_seeds, v, st);
    if (rc) return rc;
    LabelArgs l{};
    l.T = d_T;
    l.H = H;
    l.W = W;
    l.n = n;
    l.seeds = c->lab_seeds.d;
    l.K = (int)v.size();
    l.par = (int*)c->lab_work.p;
    l.label = d_label;
    l.flags = (unsigned*)(l.par + n);
    HIPCHK(c, labels2d(l, f64, st));
    return EIK_OK;
}

// Nearest-seed labels of a converged field (seeds.hip): asynchronous on `stream`, no read-back.
int eik_labels2d_dev(eik_ctx* c, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, const int64_t* seeds,
                     const double* t0, const int32_t* map_of, int64_t K, int32_t* d_label, void* stream) {
    if (!c) return EIK_ERR_ARG;
    const char* who = "eik_labels2d_dev";
    if (!d_T || !d_label) return set_err(c, EIK_ERR_ARG, "%s: %s is NULL", who, !d_T ? "d_T" : "d_label");
    if (dtype != EIK_F32 && dtype != EIK_F64) return set_err(c, EIK_ERR_ARG, "%s: bad dtype %d", who, dtype);
    if (B < 1 || H < 1 || W < 1 || B * H * W >= (1ll << 31))
        return set_err(c, EIK_ERR_ARG, "%s: B = %ld maps of %ld x %ld (1 .. 2^31 - 1 cells in all)", who, (long)B, (long)H,
                       (long)W);
    std::vector<SeedDesc> v;
    const int rc = seeds_check(c, who, B, H, W, dtype == EIK_F64, seeds, t0, map_of, K, v);
    return rc ? rc : labels2d_desc(c, d_T, dtype == EIK_F64, B, H, W, v, d_label, (hipStream_t)stream);
}

// ---- incremental re-solve after local cost changes (replan.hip)
// What the update, its restart and adopt apply to: one map, no ghost strips, not a layered block, no
// live launch, the persistent mode on a raster within its 32-bit offsets.
static int replan_gate(eik_fim2d* f, const char* who) {
    eik_ctx* c = f->ctx;
    if (f->B != 1) return set_err(c, EIK_ERR_ARG, "%s needs one map (B = %ld)", who, (long)f->B);
    if (f->lnl) return set_err(c, EIK_ERR_ARG, "%s: not for a layered block", who);
    if (f->a.ghost[0] || f->a.ghost[1] || f->a.ghost[2] || f->a.ghost[3])
        return set_err(c, EIK_ERR_ARG, "%s: not for a domain-decomposition block (ghost strips are bound)", who);
    if (f->live_on) return set_err(c, EIK_ERR_ARG, "%s: a live launch is still running (eik_fim2d_release)", who);
    if (c->mode != kModePersistent || c->delta > 0)
        return set_err(c, EIK_ERR_ARG, "%s needs the persistent mode (EIK_OPT_MODE, no EIK_OPT_DELTA)", who);
    if (f->H * f->W * (f->f64 ? 8 : 4) >= (int64_t)UINT32_MAX)
        return set_err(c, EIK_ERR_ARG, "%s: the raster is past the persistent mode's 32-bit offsets", who);
    return EIK_OK;
}

static int replan_buffers(eik_fim2d* f, ReplanArgs* r) {
    eik_ctx* c = f->ctx;
    const size_t tiles = (size_t)f->a.capacity;
    HIPCHK(c, f->rp_rects.ensure(sizeof(ReplanRect) * kMaxRects));
    HIPCHK(c, f->rp_list.ensure(sizeof(int) * tiles));
    HIPCHK(c, f->rp_flag.ensure(sizeof(unsigned) * tiles));
    HIPCHK(c, f->rp_info.ensure(64));
    if (!f->h_rects) HIPCHK(c, hipHostMalloc((void**)&f->h_rects, sizeof(ReplanRect) * kMaxRects));
    if (!f->h_info) {
        HIPCHK(c, hipHostMalloc((void**)&f->h_info, 64));
        memset(f->h_info, 0, 64);
    }
    for (hipEvent_t& ev : f->ev_rp)
        if (!ev) HIPCHK(c, hipEventCreate(&ev));
    r->rects = (const ReplanRect*)f->rp_rects.p;
    r->K = 0;
    r->gx = f->h_goals[0];  // (the goals of the last start / adopt)
    r->gy = f->h_goals[1];
    r->rlist = (int*)f->rp_list.p;
    r->rflag = (unsigned*)f->rp_flag.p;
    r->info = (unsigned long long*)f->rp_info.p;
    return EIK_OK;
}

// The rectangles of an update, checked and clipped (eik_fim2d_update, eik_fim2d_update_seeds): every
// failure is EIK_ERR_ARG with the offending index.  *any: an EIK_CHANGE_ANY rectangle is among them.
static int replan_rects_check(eik_fim2d* f, const char* who, const int64_t* rects, const int* kinds, int64_t K,
                              std::vector<ReplanRect>& v, bool* any) {
    eik_ctx* c = f->ctx;
    if (K < 0 || K > kMaxRects) return set_err(c, EIK_ERR_ARG, "%s: K = %ld outside [0, %d]", who, (long)K, kMaxRects);
    if (K > 0 && !rects) return set_err(c, EIK_ERR_ARG, "%s: rects is NULL", who);
    v.resize((size_t)K);
    *any = false;
    for (int64_t k = 0; k < K; ++k) {
        const int64_t x0 = rects[4 * k], y0 = rects[4 * k + 1], x1 = rects[4 * k + 2], y1 = rects[4 * k + 3];
        const int kind = kinds ? kinds[k] : kChangeAny;
        if (kind != kChangeAny && kind != kChangeLowered)
            return set_err(c, EIK_ERR_ARG, "%s: rectangle %ld has kind %d (0 or 1)", who, (long)k, kind);
        if (x1 <= x0 || y1 <= y0)
            return set_err(c, EIK_ERR_ARG, "%s: rectangle %ld (%ld, %ld, %ld, %ld) is empty", who, (long)k, (long)x0, (long)y0,
                           (long)x1, (long)y1);
        const int64_t cx0 = std::max<int64_t>(x0, 0), cy0 = std::max<int64_t>(y0, 0);
        const int64_t cx1 = std::min<int64_t>(x1, f->W), cy1 = std::min<int64_t>(y1, f->H);
        if (cx1 <= cx0 || cy1 <= cy0)
            return set_err(c, EIK_ERR_ARG, "%s: rectangle %ld (%ld, %ld, %ld, %ld) lies outside %ldx%ld", who, (long)k, (long)x0,
                           (long)y0, (long)x1, (long)y1, (long)f->H, (long)f->W);
        v[k] = ReplanRect{(int32_t)cx0, (int32_t)cy0, (int32_t)cx1, (int32_t)cy1, kind, 0};
        *any |= kind == kChangeAny;
    }
    return EIK_OK;
}

// The state an update needs, after replan_gate: started or adopted, a binding the caller can re-solve
// (wrong_binding: why it cannot, or NULL), the persistent mode, converged.
static int replan_state(eik_fim2d* f, const char* who, const char* wrong_binding) {
    eik_ctx* c = f->ctx;
    if (!f->started || !f->a.cost || !f->a.T) return set_err(c, EIK_ERR_ARG, "%s: the solver was never started or adopted", who);
    if (wrong_binding) return set_err(c, EIK_ERR_ARG, "%s: %s", who, wrong_binding);
    if (f->a.mode != kModePersistent) return set_err(c, EIK_ERR_ARG, "%s: the bound solve did not run in the persistent mode", who);
    if (f->last_active != 0) return set_err(c, EIK_ERR_ARG, "%s: the last solve did not end converged (0 active tiles)", who);
    return EIK_OK;
}

// an update's checked rectangles on the device (the last update's copy has completed: a solve synchronised since)
static int replan_stage_rects(eik_fim2d* f, const std::vector<ReplanRect>& v) {
    if (v.empty()) return EIK_OK;
    memcpy(f->h_rects, v.data(), sizeof(ReplanRect) * v.size());
    HIPCHK(f->ctx, hipMemcpyAsync(f->rp_rects.p, f->h_rects, sizeof(ReplanRect) * v.size(), hipMemcpyHostToDevice, f->stream));
    return EIK_OK;
}

// the flood runs on the plain FIFO of the solver's queue
static Fim2dArgs fifo_args(const eik_fim2d* f) {
    Fim2dArgs fa = f->a;
    fa.bctl = nullptr;
    fa.fresh_first = 0;
    fa.qhold = nullptr;
    fa.live = nullptr;
    fa.edge_dirty = nullptr;
    return fa;
}

// ... on the flood kernel's co-resident workgroups at most
static int flood_grid(eik_fim2d* f) {
    eik_ctx* c = f->ctx;
    if (f->flood_grid == 0) f->flood_grid = replan_flood_resident(f->f64, c->cu_count);
    return std::max(1, std::min(c->grid > 0 ? c->grid : 4 * c->cu_count, f->flood_grid));
}

// after an update's last kernel: its stop event and the counters' read-back
static int replan_update_done(eik_fim2d* f) {
    eik_ctx* c = f->ctx;
    HIPCHK(c, hipEventRecord(f->ev_rp[1], f->stream));
    HIPCHK(c, hipMemcpyAsync(f->h_info, f->rp_info.p, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
    f->rp_timed = true;
    f->rp_fallback = false;
    f->need_rewind = false;  // the prep cleared the queue words
    return EIK_OK;
}

int eik_fim2d_update(eik_fim2d* f, const int64_t* rects, const int* kinds, int64_t K, void* stream) {
    if (!f) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    const char* who = "eik_fim2d_update";
    // (the invalidation spares one goal, r.gx / r.gy: the other seeds would be reset)
    const char* seed_set = "the bound solve has a seed set (eik_fim2d_start_seeds); start or adopt a single-goal solve first";
    int rc = replan_gate(f, who);
    if (!rc) rc = replan_state(f, who, f->seeded ? seed_set : nullptr);
    if (rc) return rc;
    std::vector<ReplanRect> v;
    bool any = false;
    rc = replan_rects_check(f, who, rects, kinds, K, v, &any);
    if (rc) return rc;
    ReplanArgs r{};
    rc = replan_buffers(f, &r);
    // options, budgets and the priority bands (their width from the NEW cost) as eik_fim2d_start sets them
    if (!rc) rc = fim2d_configure(f, f->a.cost, f->a.T, stream);
    if (!rc) rc = replan_stage_rects(f, v);
    if (rc) return rc;
    r.K = (int)K;
    const Fim2dArgs fa = fifo_args(f);
    HIPCHK(c, hipEventRecord(f->ev_rp[0], f->stream));
    HIPCHK(c, replan_prep(fa, r, 0, f->stream));
    if (any) {
        const int g = flood_grid(f);
        HIPCHK(c, replan_seed(fa, r, f->f64, f->stream));
        HIPCHK(c, replan_flood(fa, r, f->f64, g, f->stream));
    }
    HIPCHK(c, replan_prep(f->a, r, 1, f->stream));
    if (K > 0) HIPCHK(c, replan_reset(f->a, r, f->f64, f->stream));
    rc = replan_update_done(f);
    if (rc) return rc;
    if (K == 0) f->last_active = 0;  // nothing queued: still converged
    return EIK_OK;
}

// One re-solve: update() queues the tiles to re-solve (it checks its own arguments, f among them), the
// iteration runs with the synchronisation deferred to the finish.
extern "C++" {
template <typename Update>
static int resolve_loop(eik_fim2d* f, void* stream, Update update) {
    int rc = update();
    if (rc) return rc;
    int64_t active = 0;
    f->defer_sync = true;
    rc = eik_fim2d_iterate(f, f->max_iters, &active);
    f->defer_sync = false;
    if (!rc) rc = finish_solve(f, &active);
    if (rc && f->band_overflow) {  // a priority band's ring was full: a full solve on the FIFO (a seed set: the new list)
        f->band_overflow = false;
        f->no_bands = true;
        rc = solve_bound(f, f->a.cost, f->a.T, stream);
        f->rp_fallback = true;
        return rc;
    }
    if (rc) return rc;
    if (active != 0)
        return set_err(f->ctx, EIK_ERR_NOCONVERGE, "no convergence of the re-solve (%ld tiles left; negative costs?)", (long)active);
    return EIK_OK;
}
}  // extern "C++"

int eik_fim2d_resolve(eik_fim2d* f, const int64_t* rects, const int* kinds, int64_t K, void* stream) {
    return resolve_loop(f, stream, [&] { return eik_fim2d_update(f, rects, kinds, K, stream); });
}

// Adopt's launches, after its checks and the goals' upload: the field's marks and the queue as after a
// converged solve.  (What the field is bound to is the caller's to set.)
static int adopt_bound(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* goals, void* stream) {
    eik_ctx* c = f->ctx;
    ReplanArgs r{};
    int rc = replan_buffers(f, &r);
    if (!rc) rc = fim2d_configure(f, d_cost, d_T, stream);
    if (!rc) rc = upload_goals(f, goals);
    if (rc) return rc;
    HIPCHK(c, replan_adopt(f->a, f->f64, f->stream));
    HIPCHK(c, replan_prep(f->a, r, 0, f->stream));  // the queue as after a converged solve
    HIPCHK(c, hipMemcpyAsync(f->h_info, f->rp_info.p, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
    f->rp_timed = false;
    f->rp_fallback = false;
    f->started = true;
    f->need_rewind = false;
    f->last_active = 0;
    return EIK_OK;
}

int eik_fim2d_adopt(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* goals, void* stream) {
    if (!f) return EIK_ERR_ARG;
    if (!d_cost || !d_T || !goals) return set_err(f->ctx, EIK_ERR_ARG, "eik_fim2d_adopt: NULL argument");
    int rc = replan_gate(f, "eik_fim2d_adopt");
    if (!rc) rc = adopt_bound(f, d_cost, d_T, goals, stream);
    if (rc) return rc;
    f->seeded = false;
    return EIK_OK;
}

// ---- the re-solve of a seeded field: cost and seed-list changes (replan.hip)
// adopt from a checked list (replan_gate passed)
static int adopt_seeds_desc(eik_fim2d* f, const void* d_cost, void* d_T, std::vector<SeedDesc> v, void* stream) {
    const int64_t none[2] = {-1, -1};  // no goal, as after eik_fim2d_start_seeds
    const int rc = adopt_bound(f, d_cost, d_T, none, stream);
    if (rc) return rc;
    f->seeded = true;
    f->bound = std::move(v);
    return EIK_OK;
}

int eik_fim2d_adopt_seeds(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t* seeds, const double* t0, int64_t Ks,
                          void* stream) {
    if (!f) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    const char* who = "eik_fim2d_adopt_seeds";
    if (!d_cost || !d_T) return set_err(c, EIK_ERR_ARG, "%s: %s is NULL", who, !d_cost ? "d_cost" : "d_T");
    int rc = replan_gate(f, who);
    if (rc) return rc;
    std::vector<SeedDesc> v;
    rc = seeds_check(c, who, 1, f->H, f->W, f->f64, seeds, t0, nullptr, Ks, v);
    return rc ? rc : adopt_seeds_desc(f, d_cost, d_T, std::move(v), stream);
}

static const char* const kUpdateSeeds = "eik_fim2d_update_seeds";

// eik_fim2d_update_seeds' checks before the new list's: what it refuses, then the rectangles into v
static int update_seeds_check(eik_fim2d* f, const int64_t* rects, const int* kinds, int64_t K, std::vector<ReplanRect>& v,
                              bool* any) {
    if (!f) return EIK_ERR_ARG;
    const char* single = "the bound solve has a single goal: eik_fim2d_update, or eik_fim2d_adopt_seeds first";
    int rc = replan_gate(f, kUpdateSeeds);
    if (!rc) rc = replan_state(f, kUpdateSeeds, !f->seeded || f->bound.empty() ? single : nullptr);
    return rc ? rc : replan_rects_check(f, kUpdateSeeds, rects, kinds, K, v, any);
}

// The seeded update from checked rectangles and a checked new list (nw by value: it becomes the bound list,
// and a caller whose list stays passes f->bound itself): the diff of nw against the bound list, then the launches.
static int update_seeds_desc(eik_fim2d* f, const std::vector<ReplanRect>& v, bool any, std::vector<SeedDesc> nw, void* stream) {
    eik_ctx* c = f->ctx;
    const int64_t K = (int64_t)v.size();
    std::vector<SeedCell> co(f->bound.size()), cn(nw.size());
    for (size_t k = 0; k < co.size(); ++k) co[k] = SeedCell{f->bound[k].x, f->bound[k].y, f->bound[k].t0};
    for (size_t k = 0; k < cn.size(); ++k) cn[k] = SeedCell{nw[k].x, nw[k].y, nw[k].t0};
    std::vector<RootDesc> roots;
    const SeedDiff diff = seed_diff(co.data(), (int64_t)co.size(), cn.data(), (int64_t)cn.size(), roots);
    const bool flood = any || diff.released > 0;  // there is a cone to find: the roots take part
    ReplanArgs r{};
    int rc = replan_buffers(f, &r);
    // options, budgets and the priority bands (their width from the NEW cost) as eik_fim2d_start sets them
    if (!rc) rc = fim2d_configure(f, f->a.cost, f->a.T, stream);
    if (!rc) rc = replan_stage_rects(f, v);
    if (!rc && flood) rc = seeds_upload(c, f->roots, roots, f->stream);
    if (!rc) rc = seeds_upload(c, f->sd, nw, f->stream);
    if (rc) return rc;
    r.K = (int)K;
    const Fim2dArgs fa = fifo_args(f);
    const int64_t nroots = (int64_t)roots.size();
    HIPCHK(c, hipEventRecord(f->ev_rp[0], f->stream));
    HIPCHK(c, replan_prep(fa, r, 0, f->stream));
    if (flood) {
        const int g = flood_grid(f);
        HIPCHK(c, replan_roots(fa, r, f->f64, f->roots.d, nroots, f->stream));
        HIPCHK(c, replan_seed(fa, r, f->f64, f->stream));
        HIPCHK(c, replan_flood(fa, r, f->f64, g, f->stream));
        HIPCHK(c, replan_unlift(fa, f->f64, f->roots.d, nroots, f->stream));
    }
    HIPCHK(c, replan_prep(f->a, r, 1, f->stream));
    if (K > 0 || diff.released > 0) HIPCHK(c, replan_reset(f->a, r, f->f64, f->stream));
    // (always: a dominated seed of an unchanged list may lie in the cone, and is put back at its t0)
    HIPCHK(c, replan_reseed(f->a, r, f->f64, f->sd.d, (int64_t)nw.size(), f->stream));
    rc = replan_update_done(f);
    if (rc) return rc;
    f->bound = std::move(nw);
    if (K == 0 && diff.same) f->last_active = 0;  // nothing queued: still converged
    return EIK_OK;
}

int eik_fim2d_update_seeds(eik_fim2d* f, const int64_t* rects, const int* kinds, int64_t K, const int64_t* seeds,
                           const double* t0, int64_t Ks, void* stream) {
    std::vector<ReplanRect> v;
    bool any = false;
    int rc = update_seeds_check(f, rects, kinds, K, v, &any);
    if (rc) return rc;
    if (!seeds && Ks == 0) return update_seeds_desc(f, v, any, f->bound, stream);  // the bound list stays
    std::vector<SeedDesc> nw;
    rc = seeds_check(f->ctx, kUpdateSeeds, 1, f->H, f->W, f->f64, seeds, t0, nullptr, Ks, nw);
    return rc ? rc : update_seeds_desc(f, v, any, std::move(nw), stream);
}

int eik_fim2d_resolve_seeds(eik_fim2d* f, const int64_t* rects, const int* kinds, int64_t K, const int64_t* seeds,
                            const double* t0, int64_t Ks, void* stream) {
    return resolve_loop(f, stream, [&] { return eik_fim2d_update_seeds(f, rects, kinds, K, seeds, t0, Ks, stream); });
}

// ... with a checked new list (nw == NULL: the bound list stays)
static int resolve_seeds_desc(eik_fim2d* f, const int64_t* rects, const int* kinds, int64_t K, const std::vector<SeedDesc>* nw,
                              void* stream) {
    return resolve_loop(f, stream, [&] {
        std::vector<ReplanRect> v;
        bool any = false;
        const int rc = update_seeds_check(f, rects, kinds, K, v, &any);
        return rc ? rc : update_seeds_desc(f, v, any, nw ? *nw : f->bound, stream);
    });
}

int eik_fim2d_update_info(eik_fim2d* f, int64_t out[6]) {
    if (!f || !out) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (!f->h_info) return EIK_OK;  // no update yet
    HIPCHK(c, hipStreamSynchronize(f->stream));
    for (int i = 0; i < 4; ++i) out[i] = (int64_t)f->h_info[i];
    float ms = 0.f;
    if (f->rp_timed && hipEventElapsedTime(&ms, f->ev_rp[0], f->ev_rp[1]) == hipSuccess) out[4] = (int64_t)(ms * 1000.0f + 0.5f);
    out[5] = f->rp_fallback ? 1 : 0;
    return EIK_OK;
}

// ---- rectangle-free replanning: the device cost diff feeding the re-solve (cost_diff.hip)
// eik_fim2d_resolve_cost solves from scratch when more than this share of the raster's tiles changed: the
// largest measured share at which the update still beat the full solve by more than the full solve's own
// run-to-run spread (the share table; profiles/cost_diff_ab.log).
constexpr double kDiffFullShare = 1.0 / 64.0;
// ... and more than this many tiles: on a raster of a few tiles one changed tile is already above any share,
// and the table's smallest raster has 4096 tiles (one 4 x 4 block of tiles, a 256^2 raster, always updates)
constexpr int64_t kDiffMinTiles = 16;

// Both kernels on st, the totals and the first kMaxRects list entries back in one pinned copy, then one
// synchronisation: *hdr = the totals, c->h_diff[1 ..] the list's head, *us the kernels' device time.
static int diff_run(eik_ctx* c, const void* d_old, const void* d_new, bool f64, int64_t H, int64_t W, hipStream_t st,
                    DiffHeader* hdr, int64_t* us) {
    const int64_t ntx = (W + kTile - 1) / kTile, nty = (H + kTile - 1) / kTile, tiles = ntx * nty;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->diff_rec.ensure(sizeof(DiffRecord) * (size_t)tiles));
    HIPCHK(c, c->diff_out.ensure(sizeof(DiffRecord) * (size_t)(1 + tiles)));
    const int64_t want = 1 + std::max<int64_t>(kMaxRects, tiles);
    if (c->h_diff_cap < want) {
        if (c->h_diff) (void)hipHostFree(c->h_diff);
        c->h_diff = nullptr;
        c->h_diff_cap = 0;
        HIPCHK(c, hipHostMalloc((void**)&c->h_diff, sizeof(DiffRecord) * (size_t)want));
        c->h_diff_cap = want;
    }
    for (hipEvent_t& ev : c->ev_diff)
        if (!ev) HIPCHK(c, hipEventCreate(&ev));
    HIPCHK(c, hipEventRecord(c->ev_diff[0], st));
    HIPCHK(c, cost_diff_tiles(d_old, d_new, f64, H, W, (int)ntx, (int)nty, (DiffRecord*)c->diff_rec.p, c->diff_nt, st));
    HIPCHK(c, cost_diff_compact((const DiffRecord*)c->diff_rec.p, (int)tiles, (DiffRecord*)c->diff_out.p, st));
    HIPCHK(c, hipEventRecord(c->ev_diff[1], st));
    // (entries past the changed tiles are stale words of an earlier call: only hdr->tiles of them are read)
    const int64_t head = 1 + std::min<int64_t>(kMaxRects, tiles);
    HIPCHK(c, hipMemcpyAsync(c->h_diff, c->diff_out.p, sizeof(DiffRecord) * (size_t)head, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(hdr, c->h_diff, sizeof *hdr);
    float ms = 0.f;
    *us = hipEventElapsedTime(&ms, c->ev_diff[0], c->ev_diff[1]) == hipSuccess ? (int64_t)(ms * 1000.0f + 0.5f) : 0;
    return EIK_OK;
}

// the whole list of n changed tiles in c->h_diff[1 ..]: a second read-back only past the first kMaxRects
static int diff_list(eik_ctx* c, int64_t n, hipStream_t st, const DiffRecord** list) {
    if (n > kMaxRects) {
        HIPCHK(c, hipMemcpyAsync(c->h_diff + 1 + kMaxRects, (const DiffRecord*)c->diff_out.p + 1 + kMaxRects,
                                 sizeof(DiffRecord) * (size_t)(n - kMaxRects), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    *list = c->h_diff + 1;
    return EIK_OK;
}

int eik_cost_diff_dev(eik_ctx* c, const void* d_old, const void* d_new, int dtype, int64_t H, int64_t W, int64_t* rects,
                      int* kinds, int64_t cap, int64_t* K, int64_t info[6], void* stream) {
    if (!c) return EIK_ERR_ARG;
    const char* who = "eik_cost_diff_dev";
    if (!d_old || !d_new || !rects || !kinds || !K || !info) return set_err(c, EIK_ERR_ARG, "%s: NULL argument", who);
    if (dtype != EIK_F32 && dtype != EIK_F64) return set_err(c, EIK_ERR_ARG, "%s: bad dtype %d", who, dtype);
    if (H < 1 || W < 1 || H >= (1ll << 31) - kTile || W >= (1ll << 31) - kTile ||
        ((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile) >= (1ll << 31) - 8)
        return set_err(c, EIK_ERR_ARG, "%s: bad shape %ld x %ld", who, (long)H, (long)W);
    if (cap < 1 || cap > kMaxRects) return set_err(c, EIK_ERR_ARG, "%s: cap = %ld outside [1, %d]", who, (long)cap, kMaxRects);
    *K = 0;
    DiffHeader h{};
    int64_t us = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = diff_run(c, d_old, d_new, dtype == EIK_F64, H, W, st, &h, &us);
    if (rc) return rc;
    int side = 0;
    if (h.tiles > 0) {
        const DiffRecord* list = nullptr;
        rc = diff_list(c, (int64_t)h.tiles, st, &list);
        if (rc) return rc;
        std::vector<DiffRect> out;
        side = diff_rects(list, (int64_t)h.tiles, (int)((W + kTile - 1) / kTile), cap, out);
        for (size_t k = 0; k < out.size(); ++k) {
            rects[4 * k] = out[k].x0;
            rects[4 * k + 1] = out[k].y0;
            rects[4 * k + 2] = out[k].x1;
            rects[4 * k + 3] = out[k].y1;
            kinds[k] = out[k].kind;
        }
        *K = (int64_t)out.size();
    }
    info[0] = (int64_t)h.changed;
    info[1] = (int64_t)h.raised;
    info[2] = (int64_t)h.invalid;
    info[3] = (int64_t)h.tiles;
    info[4] = side;
    info[5] = us;
    return EIK_OK;
}

// the error of an invalid new cost: its count and the first such cell (row-major) of the lowest changed
// tile holding one, read back from that tile alone
static int diff_invalid_error(eik_fim2d* f, const void* d_new, const DiffHeader& h, hipStream_t st) {
    eik_ctx* c = f->ctx;
    const char* who = "eik_fim2d_resolve_cost";
    const DiffRecord* list = nullptr;
    int rc = diff_list(c, (int64_t)h.tiles, st, &list);
    if (rc) return rc;
    for (uint64_t i = 0; i < h.tiles; ++i) {
        if (!list[i].invalid) continue;
        const int64_t x0 = (int64_t)(list[i].tile % f->a.ntx) * kTile, y0 = (int64_t)(list[i].tile / f->a.ntx) * kTile;
        const int64_t w = std::min<int64_t>(kTile, f->W - x0), hh = std::min<int64_t>(kTile, f->H - y0);
        const size_t cell = f->f64 ? 8 : 4;
        std::vector<char> buf(cell * (size_t)(w * hh));
        HIPCHK(c, hipMemcpy2DAsync(buf.data(), cell * w, (const char*)d_new + cell * (size_t)(y0 * f->W + x0), cell * f->W,
                                   cell * w, (size_t)hh, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (int64_t k = 0; k < w * hh; ++k) {
            const double v = f->f64 ? ((const double*)buf.data())[k] : (double)((const float*)buf.data())[k];
            if (!(v >= 0.0))
                return set_err(c, EIK_ERR_ARG, "%s: %llu cells of the new cost are NaN or negative, cost[%ld][%ld] = %g among "
                                               "them: costs must be >= 0 or +inf; nothing was rebound",
                               who, (unsigned long long)h.invalid, (long)(y0 + k / w), (long)(x0 + k % w), v);
        }
    }
    return set_err(c, EIK_ERR_ARG, "%s: %llu cells of the new cost are NaN or negative: costs must be >= 0 or +inf; nothing was "
                                   "rebound", who, (unsigned long long)h.invalid);
}

int eik_fim2d_resolve_cost(eik_fim2d* f, const void* d_cost_new, void* stream) {
    if (!f) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    const char* who = "eik_fim2d_resolve_cost";
    if (!d_cost_new) return set_err(c, EIK_ERR_ARG, "%s: d_cost_new is NULL", who);
    // what eik_fim2d_update / eik_fim2d_update_seeds refuse, before anything is launched or rebound
    int rc = replan_gate(f, who);
    if (!rc) rc = replan_state(f, who, f->seeded && f->bound.empty() ? "the bound seed list is empty" : nullptr);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DiffHeader h{};
    int64_t us = 0;
    rc = diff_run(c, f->a.cost, d_cost_new, f->f64, f->H, f->W, st, &h, &us);
    if (rc) return rc;
    int64_t* di = f->diff_info;
    di[0] = (int64_t)h.changed;
    di[1] = (int64_t)h.raised;
    di[2] = (int64_t)h.invalid;
    di[3] = (int64_t)h.tiles;
    di[4] = 0;
    di[5] = us;
    di[6] = di[7] = 0;
    if (h.invalid > 0) return diff_invalid_error(f, d_cost_new, h, st);
    const double share = c->diff_share >= 0 ? c->diff_share : kDiffFullShare;
    if ((int64_t)h.tiles > kDiffMinTiles && (double)h.tiles > share * (double)f->a.capacity) {
        // the share rule: most of the raster changed, the solve from scratch is the faster one (no list is built)
        di[6] = 1;
        return solve_bound(f, d_cost_new, f->a.T, stream);
    }
    std::vector<int64_t> rects;
    std::vector<int> kinds;
    if (h.tiles > 0) {
        const DiffRecord* list = nullptr;
        rc = diff_list(c, (int64_t)h.tiles, st, &list);
        if (rc) return rc;
        std::vector<DiffRect> out;
        di[4] = diff_rects(list, (int64_t)h.tiles, f->a.ntx, kMaxRects, out);
        rects.resize(4 * out.size());
        kinds.resize(out.size());
        for (size_t k = 0; k < out.size(); ++k) {
            rects[4 * k] = out[k].x0;
            rects[4 * k + 1] = out[k].y0;
            rects[4 * k + 2] = out[k].x1;
            rects[4 * k + 3] = out[k].y1;
            kinds[k] = out[k].kind;
        }
    }
    const int64_t K = (int64_t)kinds.size();
    di[7] = K;
    // the rebind: the update path reads the cost through f->a.cost (K == 0, equal rasters: its no-op contract)
    f->a.cost = d_cost_new;
    if (f->seeded) return eik_fim2d_resolve_seeds(f, K ? rects.data() : nullptr, K ? kinds.data() : nullptr, K, nullptr, nullptr, 0, stream);
    return eik_fim2d_resolve(f, K ? rects.data() : nullptr, K ? kinds.data() : nullptr, K, stream);
}

int eik_fim2d_diff_info(eik_fim2d* f, int64_t out[8]) {
    if (!f || !out) return EIK_ERR_ARG;
    memcpy(out, f->diff_info, sizeof f->diff_info);
    return EIK_OK;
}

int eik_fim2d_pack_edges(eik_fim2d* f, void* n, void* s, void* w, void* e) {
    if (!f || !f->started) return EIK_ERR_ARG;
    if (f->lnl)  // a layered block: nl values per edge cell
        HIPCHK(f->ctx, fim2dl_pack_edges(f->a, f->lnl, f->f64, n, s, w, e, f->stream));
    else
        HIPCHK(f->ctx, fim2d_pack_edges(f->a, f->f64, n, s, w, e, f->stream));
    return EIK_OK;
}

int eik_fim2d_merge_ghost(eik_fim2d* f, int side, const void* recv) {
    if (!f || !f->started || side < 0 || side > 3 || !recv || !f->a.ghost[side]) return EIK_ERR_ARG;
    if (f->lnl) {  // a layered block (its launches rewind their queue themselves)
        HIPCHK(f->ctx, fim2dl_merge_ghost(f->a, f->lnl, f->f64, side, recv, f->stream));
        return EIK_OK;
    }
    f->a.iter = (unsigned)f->iterations;  // enqueue for the next sweep launch
    HIPCHK(f->ctx, rewind_if_needed(f));
    HIPCHK(f->ctx, fim2d_merge_ghost(f->a, f->f64, side, recv, side < 2 ? f->W : f->H, f->stream));
    return EIK_OK;
}

// ------------------------------------------------------------- live domain decomposition
static int live_box(eik_fim2d* f) {
    if (f->box) return EIK_OK;
    const hipError_t e = hipHostMalloc((void**)&f->box, sizeof(LiveBox), hipHostMallocCoherent);
    if (e != hipSuccess) {
        f->box = nullptr;
        return set_err(f->ctx, EIK_ERR_NOMEM, "live mailbox: %s", hipGetErrorString(e));
    }
    memset(f->box, 0, sizeof(LiveBox));
    return EIK_OK;
}

int eik_fim2d_live_bind(eik_fim2d* f, void* const send[8], void* const recv[8]) {
    if (!f || !send || !recv) return EIK_ERR_ARG;
    if (f->live_on) return set_err(f->ctx, EIK_ERR_ARG, "cannot rebind strips during a live launch");
    int rc = live_box(f);
    if (rc) return rc;
    for (int p = 0; p < 2; ++p)
        for (int s = 0; s < 4; ++s) {
            f->box->send[p][s] = send[p * 4 + s];
            f->box->recv[p][s] = recv[p * 4 + s];
        }
    return EIK_OK;
}

// a live launch's queue error bits (the halo agent's copy in the mailbox, the queue's own word after the release)
static int live_queue_error(eik_fim2d* f, unsigned err) {
    eik_ctx* c = f->ctx;
    if (err & 4u)
        return set_err(c, EIK_ERR_HIP, "live solve: a priority band's ring is full (EIK_OPT_PRIO=0 or a larger "
                                       "EIK_OPT_PRIO_RING)");
    if (err & 1u)
        return set_err(c, EIK_ERR_HIP, "live solve: a queue wait exceeded %.1f s (EIK_OPT_QTIMEOUT)", c->qtimeout_s);
    if (err & 2u)
        return set_err(c, EIK_ERR_NOCONVERGE, "no convergence within %llu tile visits (negative costs?)",
                       (unsigned long long)f->a.qbudget);
    return EIK_OK;
}

// post one command to the halo agent and wait for it (bounded by the queue timeout)
static int live_cmd(eik_fim2d* f, unsigned op, unsigned par) {
    eik_ctx* c = f->ctx;
    LiveBox* b = f->box;
    const unsigned seq = __atomic_load_n(&b->seq, __ATOMIC_RELAXED) + 1u;
    __atomic_store_n(&b->cmd, op | (par & 1u) << 8, __ATOMIC_RELAXED);
    __atomic_store_n(&b->seq, seq, __ATOMIC_RELEASE);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0; __atomic_load_n(&b->done, __ATOMIC_ACQUIRE) != seq; ++spin) {
        if ((spin & 1023u) == 1023u) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (el > c->qtimeout_s + 1.0)
                return set_err(c, EIK_ERR_HIP, "live solve: the halo agent did not answer within %.1f s", el);
            if (__atomic_load_n(&b->error, __ATOMIC_RELAXED) & 1u) break;
            // the launch ended early (fault, or every workgroup left): nothing will answer
            if (hipStreamQuery(f->stream) == hipSuccess) {
                // the queue's words (error bits: 1 a wait timed out, 2 the visit budget, 4 a priority
                // band's ring lapped), the visit counters and the fullest band (tail - head)
                unsigned q[kQueueCtlBytes / 4] = {};
                (void)hipMemcpy(q, f->qctl.p, kQueueCtlBytes, hipMemcpyDeviceToHost);
                unsigned long long vis[2] = {};
                memcpy(vis, (const char*)q + kVisitsOff, sizeof vis);
                long long band_max = -1;
                if (f->a.bctl) {
                    std::vector<unsigned long long> bw(16 * kBands);
                    if (hipMemcpy(bw.data(), f->a.bctl, 128 * kBands, hipMemcpyDeviceToHost) == hipSuccess)
                        for (int b = 0; b < kBands; ++b)
                            band_max = std::max(band_max, (long long)(bw[16 * b + 8] - bw[16 * b]));
                }
                unsigned long long qh = 0, qt = 0;
                memcpy(&qh, q, 8);
                memcpy(&qt, (const char*)q + 64, 8);
                return set_err(c, EIK_ERR_HIP,
                               "live solve: the persistent launch is no longer running (queue error %u, active %d, "
                               "visits %llu, passes %llu, fifo head-tail %lld, fullest band %lld of %u slots)",
                               q[kQErrorWord], (int)q[kQActiveWord], vis[0], vis[1], (long long)(qh - qt), band_max,
                               f->a.bctl ? f->a.bmask + 1u : 0u);
            }
        }
        __builtin_ia32_pause();
    }
    return live_queue_error(f, __atomic_load_n(&b->error, __ATOMIC_RELAXED));
}

int eik_fim2d_launch(eik_fim2d* f, int live) {
    if (!f || !f->started) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    if (f->live_on) return set_err(c, EIK_ERR_ARG, "a live launch is still running (eik_fim2d_release)");
    if (f->a.mode != kModePersistent)
        return set_err(c, EIK_ERR_ARG, "eik_fim2d_launch needs the persistent mode (EIK_OPT_MODE)");
    HIPCHK(c, hipSetDevice(c->device));
    const int grid = c->grid > 0 ? c->grid : 4 * c->cu_count;
    const bool wide = !f->lnl && wide_form(f);
    if (f->lnl) {  // a layered block (eik_fim3dl_create): the layered kernel's co-resident count
        int& res = c->resident_l[f->f64 ? 1 : 0][f->lnl];
        if (res == 0) res = fim2dl_persist_resident(f->lnl, f->f64, c->cu_count);
        f->persist_grid = res;
    } else {
        (void)persist_resident(f, wide);
        c->last_form[0] = wide;
    }
    Fim2dArgs a = f->a;
    if (live) {
        int rc = live_box(f);
        if (rc) return rc;
        hipError_t e = f->hold.ensure(64);
        if (e != hipSuccess) return set_err(c, EIK_ERR_NOMEM, "live hold word: %s", hipGetErrorString(e));
        HIPCHK(c, hipMemsetAsync(f->hold.p, 0, 64, f->stream));
        f->box->seq = f->box->done = 0;
        f->box->error = 0;
        a.qhold = (unsigned*)f->hold.p;
        a.live = f->box;
    }
    if (c->timing) {
        while (f->ev_pool.size() < f->ev_used + 2) {
            hipEvent_t ev;
            HIPCHK(c, hipEventCreate(&ev));
            f->ev_pool.push_back(ev);
        }
        HIPCHK(c, hipEventRecord(f->ev_pool[f->ev_used++], f->stream));
    }
    // live: workgroup 0 is the halo agent (dispatched first); the others should be co-resident (grid <= resident)
    const int g = std::max(live ? 2 : 1, std::min(grid, f->persist_grid));
    a.fresh_first = c->fresh_first;
    a.sched = c->sched;
    if (f->lnl) {  // (its launches rewind their queue themselves)
        // a live layered block orders its waiting tiles on the priority bands at width >= 1, as the 2D
        // blocks do (§3.2): on the FIFO the blocks re-solved their interiors as the ghosts' corrections
        // arrived (C5 split 4 x 2: 4.5 x the single domain's visits, profiles/r06i_c4_rehearsal_n8.log).
        // (The relaunch schedule keeps the FIFO: its launches run to local convergence either way.)
        const double prio = c->prio >= 0 ? c->prio : std::max(1.0, default_prio(f->H, f->W, 0.0));
        a.bctl = nullptr;
        if (live && prio > 0 && a.capacity < (1 << kBandTagShift) - 1) {
            HIPCHK(c, setup_bands(c, f->bslot, f->bctl, a.capacity, a, f->stream));
            HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)a.key, 0x7f800000u, (size_t)a.capacity, f->stream));  // keys: +inf
            float* pd = (float*)((char*)f->bctl.p + 128 * kBands);
            HIPCHK(c, fim2d_prio_delta(a.cost, f->f64, f->H * f->W * f->lL, (float)prio, pd, f->stream));
            a.pdelta = pd;
            a.disp = c->prio_dispatch > 0 ? (unsigned)c->prio_dispatch : 32u;
        }
        HIPCHK(c, fim2dl_persist(a, f->lnl, f->f64, g, f->stream));
    } else {
        HIPCHK(c, rewind_if_needed(f));
        HIPCHK(c, fim2d_persist(a, f->f64, g, f->stream, wide));
    }
    if (c->timing) HIPCHK(c, hipEventRecord(f->ev_pool[f->ev_used++], f->stream));
    f->live_on = live != 0;
    ++f->iterations;
    return EIK_OK;
}

int eik_fim2d_live_pack(eik_fim2d* f, int par) {
    if (!f || !f->live_on) return EIK_ERR_ARG;
    return live_cmd(f, kLivePack, (unsigned)par);
}

int eik_fim2d_live_merge(eik_fim2d* f, int par, int64_t* active, int64_t* changed) {
    if (!f || !f->live_on) return EIK_ERR_ARG;
    int rc = live_cmd(f, kLiveMerge, (unsigned)par);
    if (rc) return rc;
    ++f->host_syncs;
    if (active) *active = __atomic_load_n(&f->box->active, __ATOMIC_RELAXED);
    if (changed) *changed = __atomic_load_n(&f->box->changed, __ATOMIC_RELAXED);
    return EIK_OK;
}

int eik_fim2d_release(eik_fim2d* f, int64_t* active) {
    if (!f || !f->live_on) return EIK_ERR_ARG;
    eik_ctx* c = f->ctx;
    f->live_on = false;
    const int rc_cmd = live_cmd(f, kLiveRelease, 0);
    HIPCHK(c, hipMemcpyAsync(f->h_q, f->qctl.p, kQueueCtlBytes, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(c, hipStreamSynchronize(f->stream));
    ++f->host_syncs;
    if (c->timing) drain_timing(f);
    if (rc_cmd) return rc_cmd;
    const int rc = live_queue_error(f, f->h_q[kQErrorWord]);
    if (rc) return rc;
    if (active) *active = f->h_q[kQActiveWord];
    return EIK_OK;
}

// ---------------------------------------------------------------- inter-process buffers
int eik_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes <= 0) return EIK_ERR_ARG;
    *out = nullptr;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault);
    if (e != hipSuccess) return set_err(nullptr, EIK_ERR_NOMEM, "pinned host allocation of %lld bytes: %s",
                                        (long long)bytes, hipGetErrorString(e));
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pinned.emplace_back(reinterpret_cast<uintptr_t>(p), (size_t)bytes);
    *out = p;
    return EIK_OK;
}

int eik_host_free(void* p) {
    if (!p) return EIK_OK;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = std::find_if(g_pinned.begin(), g_pinned.end(),
                               [&](const std::pair<uintptr_t, size_t>& b) { return b.first == reinterpret_cast<uintptr_t>(p); });
        if (it == g_pinned.end()) return EIK_ERR_ARG;
        g_pinned.erase(it);
    }
    return hipHostFree(p) == hipSuccess ? EIK_OK : EIK_ERR_HIP;
}

int eik_ipc_alloc(eik_ctx* c, int64_t bytes, void** d_ptr, unsigned char handle[64]) {
    if (!c || !d_ptr || !handle || bytes <= 0) return EIK_ERR_ARG;
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "IPC handle size");
    HIPCHK(c, hipSetDevice(c->device));
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, (size_t)bytes));
    hipIpcMemHandle_t h;
    const hipError_t e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return set_err(c, EIK_ERR_HIP, "hipIpcGetMemHandle: %s", hipGetErrorString(e));
    }
    memset(handle, 0, 64);
    memcpy(handle, &h, sizeof h);
    *d_ptr = p;
    return EIK_OK;
}

int eik_ipc_free(eik_ctx* c, void* d_ptr) {
    if (!c) return EIK_ERR_ARG;
    if (d_ptr) HIPCHK(c, hipFree(d_ptr));
    return EIK_OK;
}

int eik_ipc_open(eik_ctx* c, const unsigned char handle[64], void** d_ptr) {
    if (!c || !handle || !d_ptr) return EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof h);
    HIPCHK(c, hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return EIK_OK;
}

int eik_ipc_close(eik_ctx* c, void* d_ptr) {
    if (!c) return EIK_ERR_ARG;
    if (d_ptr) HIPCHK(c, hipIpcCloseMemHandle(d_ptr));
    return EIK_OK;
}

int eik_fim2d_stats(eik_fim2d* f, eik_stats* out) {
    if (!f || !out) return EIK_ERR_ARG;
    if (f->started) {
        eik_ctx* c = f->ctx;
        HIPCHK(c, hipMemcpyAsync(f->h_visits, (void*)f->a.visits, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                 f->stream));
        HIPCHK(c, hipStreamSynchronize(f->stream));
    }
    fill_stats(f, out);
    return EIK_OK;
}

static void fill_stats(const eik_fim2d* f, eik_stats* out) {
    out->iterations = f->iterations;
    out->tile_visits = (int64_t)f->h_visits[0];
    out->inplace_passes = (int64_t)f->h_visits[1];
    out->host_syncs = f->host_syncs;
    out->solve_ms = f->solve_ms;
    out->sweep_ms = f->sweep_ms;
    out->fresh_visits = (int64_t)f->h_visits[2];
    out->bytes_alg = (double)out->tile_visits * bytes_per_visit(f->f64) -
                     (double)out->fresh_visits * kTile * kTile * (f->f64 ? 8 : 4) +
                     (double)out->inplace_passes * bytes_per_pass(f->f64) +
                     (double)f->B * f->H * f->W * (f->f64 ? 8 : 4);
}

}  // extern "C"

namespace eik_api __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------- host-buffer drop-ins
int get_solver(eik_ctx* c, int64_t B, int64_t H, int64_t W, int dtype, eik_fim2d** out) {
    return cached_solver(c, c->cached, B, H, W, dtype, kTile, out);
}

// The host entries' inputs of n cells on the device, in stream order: cost_old (optional) in c->cost2, cost in
// c->cost, T_in (optional: a field to re-solve) in c->T, which is made in any case; labels: c->lab_out too.
template <typename R>
static int stage_inputs(eik_ctx* c, int64_t n, const R* cost, bool labels = false, const R* T_in = nullptr,
                        const R* cost_old = nullptr) {
    const size_t bytes = sizeof(R) * n;
    HIPCHK(c, c->cost.ensure(bytes));
    if (cost_old) HIPCHK(c, c->cost2.ensure(bytes));
    HIPCHK(c, c->T.ensure(bytes));
    if (labels) HIPCHK(c, c->lab_out.ensure(sizeof(int32_t) * n));
    if (cost_old) HIPCHK(c, host_to_dev(c, c->cost2.p, cost_old, bytes, c->stream));
    HIPCHK(c, host_to_dev(c, c->cost.p, cost, bytes, c->stream));
    if (T_in) HIPCHK(c, host_to_dev(c, c->T.p, T_in, bytes, c->stream));
    return EIK_OK;
}

// ... and their results back: the field of n cells at d_T, the labels (optional) of c->lab_out, then the
// stream synchronised
template <typename R>
static int fetch_results(eik_ctx* c, int64_t n, R* T, const void* d_T, int32_t* labels = nullptr) {
    HIPCHK(c, dev_to_host(c, T, d_T, sizeof(R) * n, c->stream));
    if (labels) HIPCHK(c, dev_to_host(c, labels, c->lab_out.p, sizeof(int32_t) * n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

template <typename R>
static int tmap_host(eik_ctx* c, const R* cost, int64_t B, int64_t H, int64_t W, const int64_t* goals, R* T) {
    if (!c || !cost || !T || !goals || B < 1 || H < 1 || W < 1) return c ? set_err(c, EIK_ERR_ARG, "bad arguments") : EIK_ERR_ARG;
    for (int64_t b = 0; b < B; ++b)
        if (goals[2 * b] < 0 || goals[2 * b + 1] < 0 || goals[2 * b] >= W || goals[2 * b + 1] >= H)
            return set_err(c, EIK_ERR_ARG, "goal (%ld, %ld) of map %ld outside %ldx%ld", (long)goals[2 * b],
                           (long)goals[2 * b + 1], (long)b, (long)H, (long)W);
    const int64_t n = B * H * W;
    HIPCHK(c, hipSetDevice(c->device));
    eik_fim2d* f = nullptr;
    int rc = get_solver(c, B, H, W, sizeof(R) == 8 ? EIK_F64 : EIK_F32, &f);
    if (!rc) rc = stage_inputs(c, n, cost);
    if (!rc) rc = check_cost(c, cost, c->cost.p, n, c->stream);
    if (!rc) rc = eik_fim2d_solve(f, c->cost.p, c->T.p, goals, c->stream);
    return rc ? rc : fetch_results(c, n, T, c->T.p);
}

// cost_new and the converged field of the earlier cost go up; adopt + resolve on the cached solver
template <typename R>
static int tmap_update_host(eik_ctx* c, const R* cost, R* T, int64_t H, int64_t W, int64_t gx, int64_t gy,
                            const int64_t* rects, const int* kinds, int64_t K) {
    if (!c || !cost || !T || H < 1 || W < 1) return c ? set_err(c, EIK_ERR_ARG, "bad arguments") : EIK_ERR_ARG;
    if (gx < 0 || gy < 0 || gx >= W || gy >= H)
        return set_err(c, EIK_ERR_ARG, "goal (%ld, %ld) outside %ldx%ld", (long)gx, (long)gy, (long)H, (long)W);
    const int64_t n = H * W;
    HIPCHK(c, hipSetDevice(c->device));
    eik_fim2d* f = nullptr;
    int rc = get_solver(c, 1, H, W, sizeof(R) == 8 ? EIK_F64 : EIK_F32, &f);
    if (!rc) rc = replan_gate(f, "eik_tmap2d_update");
    if (rc) return rc;
    if (f->seeded)  // (T is most likely that solve's field, which one goal does not describe)
        return set_err(c, EIK_ERR_ARG, "eik_tmap2d_update: the bound solve has a seed set (eik_tmap2d_seeds); run a "
                                       "single-goal solve first");
    rc = stage_inputs(c, n, cost, false, T);
    if (!rc) rc = check_cost(c, cost, c->cost.p, n, c->stream);
    const int64_t g[2] = {gx, gy};
    if (!rc) rc = eik_fim2d_adopt(f, c->cost.p, c->T.p, g, c->stream);
    if (!rc) rc = eik_fim2d_resolve(f, rects, kinds, K, c->stream);
    return rc ? rc : fetch_results(c, n, T, c->T.p);
}

// both costs and the converged field of cost_old go up; adopt on cost_old, then the diff names what changed
template <typename R>
static int tmap_update_cost_host(eik_ctx* c, const R* cost_old, const R* cost_new, R* T, int64_t H, int64_t W, int64_t gx,
                                 int64_t gy) {
    if (!c) return EIK_ERR_ARG;
    const char* who = "eik_tmap2d_update_cost";
    if (!cost_old || !cost_new || !T)
        return set_err(c, EIK_ERR_ARG, "%s: %s is NULL", who, !cost_old ? "cost_old" : !cost_new ? "cost_new" : "T_inout");
    if (H < 1 || W < 1) return set_err(c, EIK_ERR_ARG, "%s: bad shape %ld x %ld", who, (long)H, (long)W);
    if (gx < 0 || gy < 0 || gx >= W || gy >= H)
        return set_err(c, EIK_ERR_ARG, "%s: goal (%ld, %ld) outside %ldx%ld", who, (long)gx, (long)gy, (long)H, (long)W);
    const int64_t n = H * W;
    HIPCHK(c, hipSetDevice(c->device));
    eik_fim2d* f = nullptr;
    int rc = get_solver(c, 1, H, W, sizeof(R) == 8 ? EIK_F64 : EIK_F32, &f);
    if (!rc) rc = replan_gate(f, who);
    if (rc) return rc;
    rc = stage_inputs(c, n, cost_new, false, T, cost_old);
    const int64_t g[2] = {gx, gy};
    if (!rc) rc = eik_fim2d_adopt(f, c->cost2.p, c->T.p, g, c->stream);
    if (!rc) rc = eik_fim2d_resolve_cost(f, c->cost.p, c->stream);  // (it checks cost_new: NaN or negative is EIK_ERR_ARG)
    return rc ? rc : fetch_results(c, n, T, c->T.p);
}

// one map from a seed set on the cached solver; labels (optional) from the field while it is on the device
template <typename R>
static int tmap_seeds_host(eik_ctx* c, const R* cost, int64_t H, int64_t W, const int64_t* seeds, const double* t0,
                           int64_t K, R* T, int32_t* labels) {
    if (!c) return EIK_ERR_ARG;
    if (!cost || !T) return set_err(c, EIK_ERR_ARG, "eik_tmap2d_seeds: %s is NULL", !cost ? "cost" : "T");
    if (H < 1 || W < 1) return set_err(c, EIK_ERR_ARG, "eik_tmap2d_seeds: bad shape %ld x %ld", (long)H, (long)W);
    constexpr int dtype = sizeof(R) == 8 ? EIK_F64 : EIK_F32;
    std::vector<SeedDesc> v;  // (checked once, before anything is uploaded: the solve and the labels take the descriptors)
    int rc = seeds_check(c, "eik_tmap2d_seeds", 1, H, W, sizeof(R) == 8, seeds, t0, nullptr, K, v);
    if (rc) return rc;
    if (labels && H * W >= (1ll << 31)) return set_err(c, EIK_ERR_ARG, "eik_tmap2d_seeds: labels need fewer than 2^31 cells");
    const int64_t n = H * W;
    HIPCHK(c, hipSetDevice(c->device));
    eik_fim2d* f = nullptr;
    rc = get_solver(c, 1, H, W, dtype, &f);
    if (!rc) rc = stage_inputs(c, n, cost, labels != nullptr);
    if (!rc) rc = check_cost(c, cost, c->cost.p, n, c->stream);
    if (!rc) rc = solve_seeds_desc(f, c->cost.p, c->T.p, v, c->stream);
    if (!rc && labels) rc = labels2d_desc(c, c->T.p, sizeof(R) == 8, 1, H, W, v, (int32_t*)c->lab_out.p, c->stream);
    return rc ? rc : fetch_results(c, n, T, c->T.p, labels);
}

// cost_new and the converged field of the earlier cost and the old list go up; adopt_seeds + resolve_seeds
// on the cached solver; labels (optional) of the new list from the field while it is on the device
template <typename R>
static int tmap_update_seeds_host(eik_ctx* c, const R* cost, R* T, int64_t H, int64_t W, const int64_t* seeds_old,
                                  const double* t0_old, int64_t K_old, const int64_t* seeds_new, const double* t0_new,
                                  int64_t K_new, const int64_t* rects, const int* kinds, int64_t K, int32_t* labels) {
    if (!c) return EIK_ERR_ARG;
    const char* who = "eik_tmap2d_update_seeds";
    if (!cost || !T) return set_err(c, EIK_ERR_ARG, "%s: %s is NULL", who, !cost ? "cost_new" : "T_inout");
    if (H < 1 || W < 1) return set_err(c, EIK_ERR_ARG, "%s: bad shape %ld x %ld", who, (long)H, (long)W);
    constexpr int dtype = sizeof(R) == 8 ? EIK_F64 : EIK_F32;
    std::vector<SeedDesc> old, nw;  // (checked once, before anything is uploaded: adopt, resolve and the labels take the descriptors)
    int rc = seeds_check(c, who, 1, H, W, sizeof(R) == 8, seeds_old, t0_old, nullptr, K_old, old);
    const bool keep = !seeds_new && K_new == 0;  // the list is unchanged
    if (!rc && !keep) rc = seeds_check(c, who, 1, H, W, sizeof(R) == 8, seeds_new, t0_new, nullptr, K_new, nw);
    if (rc) return rc;
    if (labels && H * W >= (1ll << 31)) return set_err(c, EIK_ERR_ARG, "%s: labels need fewer than 2^31 cells", who);
    const int64_t n = H * W;
    HIPCHK(c, hipSetDevice(c->device));
    eik_fim2d* f = nullptr;
    rc = get_solver(c, 1, H, W, dtype, &f);
    if (!rc) rc = replan_gate(f, who);
    if (!rc) rc = stage_inputs(c, n, cost, labels != nullptr, T);
    if (!rc) rc = check_cost(c, cost, c->cost.p, n, c->stream);
    if (!rc) rc = adopt_seeds_desc(f, c->cost.p, c->T.p, old, c->stream);
    if (!rc) rc = resolve_seeds_desc(f, rects, kinds, K, keep ? nullptr : &nw, c->stream);
    if (!rc && labels) rc = labels2d_desc(c, c->T.p, sizeof(R) == 8, 1, H, W, keep ? old : nw, (int32_t*)c->lab_out.p, c->stream);
    return rc ? rc : fetch_results(c, n, T, c->T.p, labels);
}

// nodeJoin + partial fields from the two device-resident full fields dT[0:n] (goal front) and
// dT[n:2n] (start front), in place; *best = the packed join (~0: the fronts never meet).  d_cost
// (the fronts' raster): band cells by the band relaxation (bidir.hip), else at their full-field
// values; d_chk: the capped fronts' check.  Ends with the stream synchronised on *best.
// src (with d_cost): the goal's and the start's linear index, for EIK_OPT_EXACT_BAND's replay.
static int join_and_partial(eik_ctx* c, double* dT, int64_t n, int64_t H, int64_t W, unsigned long long* best,
                            int64_t members[2], const double* d_cost = nullptr, FrontsCheck* d_chk = nullptr,
                            FrontsCheck* h_chk = nullptr, const int64_t* src = nullptr) {
    hipStream_t st = c->stream;
    HIPCHK(c, c->work.ensure(bidir_join_work_bytes(n)));
    HIPCHK(c, c->misc.ensure(64));
    HIPCHK(c, bidir_join(dT, dT + n, n, c->work.p, c->work.bytes, (unsigned long long*)c->misc.p, st, members));
    if (d_cost && src && c->exact_band && members[0] > 0 && members[1] > 0) {
        // the reference's own band values, LIFO ties and nodeJoin, replayed from the join's ranks
        const unsigned *rg = nullptr, *rs = nullptr;
        bidir_join_ranks(c->work.p, n, &rg, &rs);
        HIPCHK(c, c->exact.ensure(bidir_exact_work_bytes(n, members[0], members[1])));
        EventPair ev;  // (destroyed on every return path)
        hipEvent_t &e0 = ev.e0, &e1 = ev.e1;
        HIPCHK(c, hipEventCreate(&e0));
        HIPCHK(c, hipEventCreate(&e1));
        HIPCHK(c, hipEventRecord(e0, st));
        unsigned long long info[4] = {0, 0, 0, 0};
        const hipError_t e = bidir_exact(dT, dT + n, d_cost, H, W, src[0], src[1], rg, rs, members, c->exact.p,
                                         c->exact.bytes, (unsigned long long*)c->misc.p, st, info);
        if (e == hipErrorNotReady || e == hipErrorNotSupported || e == hipErrorIllegalState)
            return set_err(c, EIK_ERR_NOCONVERGE,
                           e == hipErrorNotReady      ? "biComputeTmap: the exact band replay did not settle"
                           : e == hipErrorNotSupported ? "biComputeTmap: the exact band replay met a run of more than "
                                                         "4096 cells of exactly equal T (a zero-cost region)"
                                                       : "biComputeTmap: the exact meeting is not clear of the ranked "
                                                         "cells' bound");
        HIPCHK(c, e);
        HIPCHK(c, hipEventRecord(e1, st));
        HIPCHK(c, hipMemcpyAsync(best, c->misc.p, sizeof *best, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        for (int q = 0; q < 4; ++q) c->exact_info[q] = info[q];
        c->exact_info[4] = (unsigned long long)(ms * 1000.0f);
        for (int q = 0; q < 4; ++q) c->fronts_info[6 + q] = 0;
        if (d_chk) {
            HIPCHK(c, hipMemcpyAsync(h_chk, d_chk, sizeof *h_chk, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            h_chk->viol = 0;  // band values come from the replay's events, not from the capped field
        }
        return EIK_OK;
    }
    {
        const hipError_t e = bidir_partial(dT, dT + n, H, W, c->work.p, (const unsigned long long*)c->misc.p, st, d_cost,
                                           d_chk ? &d_chk->viol : nullptr);
        if (e == hipErrorNotReady)
            return set_err(c, EIK_ERR_NOCONVERGE, "biComputeTmap: the band relaxation of the partial fields did not settle");
        HIPCHK(c, e);
    }
    if (d_cost) {
        unsigned bs[4] = {0, 0, 0, 0};
        HIPCHK(c, bidir_band_stats(c->work.p, n, bs, st));
        for (int q = 0; q < 4; ++q) c->fronts_info[6 + q] = bs[q];
    }
    HIPCHK(c, hipMemcpyAsync(best, c->misc.p, sizeof *best, hipMemcpyDeviceToHost, st));
    if (d_chk) HIPCHK(c, hipMemcpyAsync(h_chk, d_chk, sizeof *h_chk, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return EIK_OK;
}

// Capped fronts: rasters of at least kFrontsCapCells cells, F x F coarse blocks with F =
// max(4, ceil(max(H, W) / 512)), cap = F x (coarse T at the join bound's rank K0, bidir.hip
// fronts_estimate) x margin (kFrontsMargin, EIK_OPT_FRONTS_CAP) + the largest finite cost
constexpr int64_t kFrontsCapCells = 1 << 20;

// biComputeTmap's two fronts (FastMarching.py:114-162) as one B = 2 batch -- map 0 from the goal
// (g[0], g[1]), map 1 from the start (g[2], g[3]) -- over the device cost dcost (both maps), into
// dT, then nodeJoin (*best) and the partial fields.  The fronts only matter up to their meeting,
// so by default (EIK_OPT_FRONTS_CAP) each is solved only up to a cap on T estimated from a coarse
// copy of the raster (bidir.hip "capped fronts"); a capped result that cannot be shown equal to
// the full one (meeting rank at or above a front's kept cells, a band cell cut off, no meeting)
// is replaced by the uncapped solve.
int solve_fronts(eik_ctx* c, eik_fim2d* f, double* dcost, double* dT, const int64_t g[4], int64_t H, int64_t W,
                 unsigned long long* best) {
    hipStream_t st = c->stream;
    const int64_t n = H * W;
    const int64_t src[2] = {g[1] * W + g[0], g[3] * W + g[2]};
    for (int64_t& v : c->fronts_info) v = 0;  // (join_and_partial fills the band entries)
    for (auto& v : c->exact_info) v = 0;
    // exact band: the fronts in the reference's arithmetic, so the replay mostly confirms their values
    struct RefArith {
        eik_fim2d* f;
        RefArith(eik_fim2d* f_, bool on) : f(f_) { f->a.ref_arith = on ? 1 : 0; }
        ~RefArith() { f->a.ref_arith = 0; }
    } ref_guard(f, c->exact_band);
    HIPCHK(c, c->work.ensure(bidir_join_work_bytes(n)));
    const bool capped = c->fronts_cap > 0 && n >= kFrontsCapCells && std::min(H, W) >= 256;
    if (capped) {
        // coarse side 512 (EIK_FRONTS_COARSE, diagnostics): 256 / 1024 were slower at 4096^2
        // (profiles/r04t_fronts_coarse_side.log: looser caps / a longer coarse chain)
        static const int64_t cside = getenv("EIK_FRONTS_COARSE") ? std::max(64, atoi(getenv("EIK_FRONTS_COARSE"))) : 512;
        const int64_t F = std::max<int64_t>(4, (std::max(H, W) + cside - 1) / cside);
        const int64_t Hc = (H + F - 1) / F, Wc = (W + F - 1) / F, nc = Hc * Wc;
        const size_t cb = sizeof(double) * 2 * nc;
        HIPCHK(c, c->fronts.ensure(2 * cb + 256));
        double* ccost = (double*)c->fronts.p;
        double* cT = ccost + 2 * nc;
        FrontsCheck* chk = (FrontsCheck*)((char*)c->fronts.p + 2 * cb);
        HIPCHK(c, fronts_coarse_cost(dcost, H, W, (int)F, ccost, Hc, Wc, chk, st));
        HIPCHK(c, hipMemcpyAsync(ccost + nc, ccost, sizeof(double) * nc, hipMemcpyDeviceToDevice, st));
        eik_fim2d* fc = nullptr;
        int rc = cached_solver(c, c->cached_fronts, 2, Hc, Wc, EIK_F64, kTile, &fc);
        if (rc) return rc;
        const int64_t gc[4] = {g[0] / F, g[1] / F, g[2] / F, g[3] / F};
        const eik_stats keep = c->last;  // the coarse estimate's solve is not the caller's
        int64_t keep_form[4];
        memcpy(keep_form, c->last_form, sizeof keep_form);
        rc = eik_fim2d_solve(fc, ccost, cT, gc, st);
        c->last = keep;
        memcpy(c->last_form, keep_form, sizeof keep_form);
        if (rc) return rc;
        HIPCHK(c, fronts_estimate(cT, cT + nc, nc, c->work.p, (double)F, c->fronts_cap, chk, st));
        f->a.tcap = chk->caps;
        rc = eik_fim2d_solve(f, dcost, dT, g, st);
        f->a.tcap = nullptr;
        if (rc) return rc;
        HIPCHK(c, fronts_clean(dT, n, chk, st));
        FrontsCheck h{};
        int64_t mem[2] = {0, 0};
        rc = join_and_partial(c, dT, n, H, W, best, mem, dcost, chk, &h, src);
        if (rc) return rc;
        const unsigned long long k = *best >> 30;
        const bool ok = *best != ~0ull && h.viol == 0 && k < h.kept[0] && k < h.kept[1];
        c->fronts_info[0] = std::isfinite(h.caps[0]) || std::isfinite(h.caps[1]);
        c->fronts_info[2] = h.kept[0];
        c->fronts_info[3] = h.kept[1];
        c->fronts_info[4] = mem[0];
        c->fronts_info[5] = mem[1];
        if (ok || !c->fronts_info[0]) return EIK_OK;  // (no finite cap: that was the full solve)
        c->fronts_info[1] = 1;  // the capped fronts did not settle the join: solve them in full
    }
    int rc = eik_fim2d_solve(f, dcost, dT, g, st);
    if (rc) return rc;
    int64_t mem[2] = {0, 0};
    rc = join_and_partial(c, dT, n, H, W, best, mem, dcost, nullptr, nullptr, src);
    if (!capped) {
        c->fronts_info[4] = mem[0];
        c->fronts_info[5] = mem[1];
    }
    return rc;
}

}  // namespace eik_api

extern "C" {

int eik_tmap2d_update_seeds_f32(eik_ctx* c, const float* cost_new, float* T, int64_t H, int64_t W, const int64_t* seeds_old,
                                const double* t0_old, int64_t K_old, const int64_t* seeds_new, const double* t0_new,
                                int64_t K_new, const int64_t* rects, const int* kinds, int64_t K, int32_t* labels) {
    return tmap_update_seeds_host<float>(c, cost_new, T, H, W, seeds_old, t0_old, K_old, seeds_new, t0_new, K_new, rects, kinds,
                                         K, labels);
}

int eik_tmap2d_update_seeds_f64(eik_ctx* c, const double* cost_new, double* T, int64_t H, int64_t W, const int64_t* seeds_old,
                                const double* t0_old, int64_t K_old, const int64_t* seeds_new, const double* t0_new,
                                int64_t K_new, const int64_t* rects, const int* kinds, int64_t K, int32_t* labels) {
    return tmap_update_seeds_host<double>(c, cost_new, T, H, W, seeds_old, t0_old, K_old, seeds_new, t0_new, K_new, rects, kinds,
                                          K, labels);
}

int eik_tmap2d_seeds_f32(eik_ctx* c, const float* cost, int64_t H, int64_t W, const int64_t* seeds, const double* t0,
                         int64_t K, float* T, int32_t* labels) {
    return tmap_seeds_host<float>(c, cost, H, W, seeds, t0, K, T, labels);
}

int eik_tmap2d_seeds_f64(eik_ctx* c, const double* cost, int64_t H, int64_t W, const int64_t* seeds, const double* t0,
                         int64_t K, double* T, int32_t* labels) {
    return tmap_seeds_host<double>(c, cost, H, W, seeds, t0, K, T, labels);
}

int eik_tmap2d_update_f32(eik_ctx* c, const float* cost_new, float* T, int64_t H, int64_t W, int64_t gx, int64_t gy,
                          const int64_t* rects, const int* kinds, int64_t K) {
    return tmap_update_host<float>(c, cost_new, T, H, W, gx, gy, rects, kinds, K);
}

int eik_tmap2d_update_f64(eik_ctx* c, const double* cost_new, double* T, int64_t H, int64_t W, int64_t gx, int64_t gy,
                          const int64_t* rects, const int* kinds, int64_t K) {
    return tmap_update_host<double>(c, cost_new, T, H, W, gx, gy, rects, kinds, K);
}

int eik_tmap2d_update_cost_f32(eik_ctx* c, const float* cost_old, const float* cost_new, float* T, int64_t H, int64_t W,
                               int64_t gx, int64_t gy) {
    return tmap_update_cost_host<float>(c, cost_old, cost_new, T, H, W, gx, gy);
}

int eik_tmap2d_update_cost_f64(eik_ctx* c, const double* cost_old, const double* cost_new, double* T, int64_t H, int64_t W,
                               int64_t gx, int64_t gy) {
    return tmap_update_cost_host<double>(c, cost_old, cost_new, T, H, W, gx, gy);
}

int eik_tmap2d_f32(eik_ctx* c, const float* cost, int64_t H, int64_t W, int64_t gx, int64_t gy, float* T) {
    const int64_t g[2] = {gx, gy};
    return tmap_host<float>(c, cost, 1, H, W, g, T);
}

int eik_tmap2d_f64(eik_ctx* c, const double* cost, int64_t H, int64_t W, int64_t gx, int64_t gy, double* T) {
    const int64_t g[2] = {gx, gy};
    return tmap_host<double>(c, cost, 1, H, W, g, T);
}

int eik_tmap2d_batch_f32(eik_ctx* c, const float* cost, int64_t B, int64_t H, int64_t W, const int64_t* goals,
                         float* T) {
    return tmap_host<float>(c, cost, B, H, W, goals, T);
}

int eik_exact_info(const eik_ctx* c, int64_t out[5]) {
    if (!c || !out) return EIK_ERR_ARG;
    for (int i = 0; i < 5; ++i) out[i] = (int64_t)c->exact_info[i];
    return EIK_OK;
}

int eik_last_form(const eik_ctx* c, int64_t out[4]) {
    if (!c || !out) return EIK_ERR_ARG;
    for (int i = 0; i < 4; ++i) out[i] = c->last_form[i];
    return EIK_OK;
}

int eik_fronts_info(const eik_ctx* c, int64_t out[10]) {
    if (!c || !out) return EIK_ERR_ARG;
    for (int i = 0; i < 10; ++i) out[i] = c->fronts_info[i];
    return EIK_OK;
}

int eik_tmap2d_bidir_f64(eik_ctx* c, const double* cost, int64_t H, int64_t W, int64_t gx, int64_t gy, int64_t sx,
                         int64_t sy, double* TG, double* TS, uint32_t join[2]) {
    if (!c || !cost || !TG || !TS || !join) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    const int64_t n = H * W;
    if (n >= (1ll << 29)) return set_err(c, EIK_ERR_ARG, "bidirectional join supports < 2^29 cells");
    // both fronts as one 2-map batch: map 0 from the goal, map 1 from the start.  The raster goes up
    // once and is duplicated on the device; the fields come back straight into TG / TS (no host
    // staging copies: the drop-in's biComputeTmap spent ~200 ms in them for a 4096^2 raster)
    const int64_t goals[4] = {gx, gy, sx, sy};
    for (int b = 0; b < 2; ++b)
        if (goals[2 * b] < 0 || goals[2 * b + 1] < 0 || goals[2 * b] >= W || goals[2 * b + 1] >= H)
            return set_err(c, EIK_ERR_ARG, "node (%ld, %ld) outside %ldx%ld", (long)goals[2 * b], (long)goals[2 * b + 1],
                           (long)H, (long)W);
    HIPCHK(c, hipSetDevice(c->device));
    eik_fim2d* f = nullptr;
    int rc = get_solver(c, 2, H, W, EIK_F64, &f);
    if (rc) return rc;
    HIPCHK(c, c->cost.ensure(sizeof(double) * 2 * n));
    HIPCHK(c, c->T.ensure(sizeof(double) * 2 * n));
    double* dcost = (double*)c->cost.p;
    HIPCHK(c, host_to_dev(c, dcost, cost, sizeof(double) * n, c->stream));
    rc = check_cost(c, cost, dcost, n, c->stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(dcost + n, dcost, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    // the fronts (c->T holds both maps back to back), nodeJoin and the partial fields at the
    // meeting iteration (FastMarching.py:141-162)
    unsigned long long best = 0;
    rc = solve_fronts(c, f, dcost, (double*)c->T.p, goals, H, W, &best);
    if (rc) return rc;
    HIPCHK(c, dev_to_host(c, TG, c->T.p, sizeof(double) * n, c->stream));
    HIPCHK(c, dev_to_host(c, TS, (double*)c->T.p + n, sizeof(double) * n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (best == ~0ull) return set_err(c, EIK_ERR_UNREACHABLE, "goal and start are not connected");
    const int64_t node = (int64_t)(best & ((1ull << 29) - 1));
    join[0] = (uint32_t)(node % W);
    join[1] = (uint32_t)(node / W);
    return EIK_OK;
}

int eik_bidir_join_f64(eik_ctx* c, const double* TG, const double* TS, int64_t H, int64_t W, double* TGp,
                       double* TSp, uint32_t join[2], int64_t members[2]) {
    if (!c || !TG || !TS || !TGp || !TSp || !join) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    if (H < 1 || W < 1) return set_err(c, EIK_ERR_ARG, "empty field");
    const int64_t n = H * W;
    if (n >= (1ll << 29)) return set_err(c, EIK_ERR_ARG, "bidirectional join supports < 2^29 cells");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->T.ensure(sizeof(double) * 2 * n));
    double* dT = (double*)c->T.p;
    HIPCHK(c, host_to_dev(c, dT, TG, sizeof(double) * n, c->stream));
    HIPCHK(c, host_to_dev(c, dT + n, TS, sizeof(double) * n, c->stream));
    unsigned long long best = 0;
    int64_t mem[2] = {0, 0};
    int rc = join_and_partial(c, dT, n, H, W, &best, mem);
    if (rc) return rc;
    if (members) {
        members[0] = mem[0];
        members[1] = mem[1];
    }
    if (best == ~0ull) return set_err(c, EIK_ERR_UNREACHABLE, "the fields share no finite cell");
    HIPCHK(c, dev_to_host(c, TGp, dT, sizeof(double) * n, c->stream));
    HIPCHK(c, dev_to_host(c, TSp, dT + n, sizeof(double) * n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t node = (int64_t)(best & ((1ull << 29) - 1));
    join[0] = (uint32_t)(node % W);
    join[1] = (uint32_t)(node / W);
    return EIK_OK;
}

// ------------------------------------------------------------------------------ 3D
// How one persistent launch of a 3D driver ended, after its synchronisation: the queue error word's refusal
// (who names the solver, budget_who prefixes the visit budget's text), else c->last's fields that both
// drivers fill alike -- inplace_passes, fresh_visits and bytes_alg are the caller's.
static int persist3_outcome(eik_ctx* c, unsigned err, const char* who, const char* budget_who, unsigned long long qbudget,
                            hipEvent_t e0, hipEvent_t e1, unsigned long long visits) {
    if (err & 1u) return set_err(c, EIK_ERR_HIP, "%s: a queue wait exceeded %.1f s (EIK_OPT_QTIMEOUT)", who, c->qtimeout_s);
    if (err & 2u)
        return set_err(c, EIK_ERR_NOCONVERGE, "%sno convergence within %llu tile visits (negative costs?)", budget_who, qbudget);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    c->last = eik_stats{};
    c->last.iterations = 1;
    c->last.host_syncs = 1;
    c->last.tile_visits = (int64_t)visits;
    c->last.solve_ms = ms;
    return EIK_OK;
}

// Few-layer fp32 volumes (the rover's (x, y, mode) costmaps) on the layered 2D-tile solver:
// layers z0 .. z0+nl-1 of a [H][W][L] volume, one persistent launch.
// d_seeds: a seed set in place of the goal (fim2dl_init_seeds; every seed's z in [z0, z0 + nl), goal unused).
// The bands' keys are then the seeds' t0, and a retry on the FIFO seeds again from the same list.
static int solve_layered(eik_ctx* c, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int z0, int nl,
                         const int64_t goal[3], int dtype, hipStream_t st, const Seed3Desc* d_seeds = nullptr,
                         int64_t K = 0) {
    const bool f64 = dtype == EIK_F64;
    const int th = fim2dl_rows(f64);
    eik_fim2d* f = nullptr;
    {
        const int rc = cached_solver(c, f64 ? c->cached_l64 : c->cached_l, 1, H, W, dtype, th, &f);
        if (rc) return rc;
    }
    Fim2dArgs a = f->a;
    a.cost = d_cost;
    a.T = d_T;
    a.ls = L;
    a.z0 = z0;
    a.lzs = 1;
    int64_t nT = H * W * L;  // T's elements (the init's +inf)
    const bool planar = c->layer_planar != 0;
    const size_t esz = f64 ? 8 : 4;
    if (planar) {  // the solve on layer-planar copies (fim2dl.hip layer_planar_in_kernel)
        HIPCHK(c, c->lp_cost.ensure(esz * nl * H * W));
        HIPCHK(c, c->lp_T.ensure(esz * nl * H * W));
        a.cost = c->lp_cost.p;
        a.T = c->lp_T.p;
        a.ls = 1;
        a.z0 = 0;
        a.lzs = H * W;
        nT = (int64_t)nl * H * W;
    }
    a.mode = kModePersistent;
    a.max_rounds = 1;
    a.keep = (float)(1.0 - c->tol);
    a.delta = __builtin_inff();
    a.edge_dirty = nullptr;
    for (auto& g : a.ghost) g = nullptr;
    a.qtimeout = (unsigned long long)(c->qtimeout_s * 1e8);
    // C5 A/B (profiles/r02a_c5_passes.log): 8 / 16 / 24 passes 15.5-16.3 / 13.9 / 12.9 ms
    a.max_passes = c->passes > 0 ? c->passes : 24;
    a.qbudget = c->max_visits ? c->max_visits : 1024ull * (unsigned long long)a.tiles_per_map + (1ull << 20);
    int& res = c->resident_l[f64 ? 1 : 0][nl];
    if (res == 0) res = fim2dl_persist_resident(nl, f64, c->cu_count);
    const int grid = std::min(c->grid > 0 ? c->grid : 4 * c->cu_count, res);
    a.fresh_first = c->fresh_first;
    unsigned err = 0;
    // attempt 1 without bands when attempt 0's band ring overflowed (qerror bit 4, as eik_fim2d_solve)
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIPCHK(c, hipEventRecord(f->ev_start, st));
        HIPCHK(c, hipMemsetAsync((void*)f->a.visits, 0, 3 * sizeof(unsigned long long), st));
        if (planar) HIPCHK(c, layer_planar(d_cost, c->lp_cost.p, f64, H * W, L, z0, nl, true, st));
        // priority bands (fim_engine.hpp), as eik_fim2d_start sets them up: on an explicit EIK_OPT_PRIO
        a.bctl = nullptr;
        const double prio = c->prio < 0 ? default_prio(H, W, 3072.0) : c->prio;
        if (prio > 0 && attempt == 0 && a.capacity < (1 << kBandTagShift) - 1) {
            HIPCHK(c, setup_bands(c, f->bslot, f->bctl, a.capacity, a, st));
            HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)a.key, 0x7f800000u, (size_t)a.capacity, st));  // keys: +inf
            float* pd = (float*)((char*)f->bctl.p + 128 * kBands);
            HIPCHK(c, fim2d_prio_delta(a.cost, f64, planar ? (int64_t)nl * H * W : H * W * L, (float)prio, pd, st));
            a.pdelta = pd;
            // the dispatch batch: 32 below kWideTiles tiles (C5 16 / 32 / 48 / 64: fp64 3.61 / 3.67-3.69 / 3.65 /
            // 3.58, fp32 6.30-6.33 / 6.37-6.38 / 6.27 / 6.08-6.12 Gcells/s, profiles/r05ak_layered_dispatch_ab.log)
            a.disp = c->prio_dispatch > 0 ? (unsigned)c->prio_dispatch : a.tiles_per_map >= kWideTiles ? 64u : 32u;
        }
        if (d_seeds) {
            HIPCHK(c, fim2dl_init_seeds(a, f64, d_seeds, K, z0, nT, st));
        } else {
            HIPCHK(c, fim2dl_init(a, f64, goal[0], goal[1], goal[2] - z0, nT, st));
        }
        HIPCHK(c, fim2dl_persist(a, nl, f64, grid, st));
        if (planar) HIPCHK(c, layer_planar(c->lp_T.p, d_T, f64, H * W, L, z0, nl, false, st));
        HIPCHK(c, hipEventRecord(f->ev_stop, st));
        HIPCHK(c, hipMemcpyAsync(f->h_q, f->qctl.p, kQueueCtlBytes, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(f->h_visits, (void*)f->a.visits, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        err = f->h_q[kQErrorWord];
        if (!(err & 4u) || (err & 3u)) break;
    }
    c->last_solver3[0] = 1;  // eik_fim3d_last_solver
    c->last_solver3[1] = z0;
    c->last_solver3[2] = nl;
    c->last_solver3[3] = a.bctl != nullptr;  // (of the attempt that stands)
    const int rc = persist3_outcome(c, err, "layered solver", "", a.qbudget, f->ev_start, f->ev_stop, f->h_visits[0]);
    if (rc) return rc;
    c->last.inplace_passes = (int64_t)f->h_visits[1];
    c->last.fresh_visits = (int64_t)f->h_visits[2];
    // per visit: cost + T read and T write of the tile's nl layers plus the halo ring (a first
    // visit reads no T); per in-place pass: T write + halo
    // (esz: the element size above)
    // (+ the init's T store; planar: + the copies, cost in (L read, nl written) and field out (nl
    // read, L written) per cell, instead of the init's L)
    c->last.bytes_alg = (double)esz * nl *
                            ((double)c->last.tile_visits * (3.0 * kTile * th + 2.0 * (kTile + th)) -
                             (double)c->last.fresh_visits * kTile * th +
                             (double)c->last.inplace_passes * (1.0 * kTile * th + 2.0 * (kTile + th))) +
                        (double)esz * H * W * (planar ? 2.0 * (L + nl) + nl : (double)L);
    return EIK_OK;
}

// Layers [z0, z0 + nl) of a volume the layered solver can take, or nl = 0: L <= kmax layers (fp32 4,
// fp64 3), or L <= kmax + 2 whose first and last layers are entirely +inf (the reference's z padding).
static int layered_plan(eik_ctx* c, const void* d_cost, int64_t H, int64_t W, int64_t L, int dtype, hipStream_t st,
                        int* z0, int* nl) {
    const bool f64 = dtype == EIK_F64;
    const int kmax = f64 ? 3 : 4;
    *z0 = 0;
    *nl = 0;
    if (L <= kmax) {
        *nl = (int)L;
        return EIK_OK;
    }
    if (L > kmax + 2) return EIK_OK;
    HIPCHK(c, c->misc.ensure(64));
    int* d_flag = (int*)c->misc.p;
    int h_flag = 0;
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(int), st));
    HIPCHK(c, layer_finite(d_cost, f64, H * W, L, 0, d_flag, st));
    HIPCHK(c, layer_finite(d_cost, f64, H * W, L, L - 1, d_flag, st));
    HIPCHK(c, hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (h_flag == 0) {
        *z0 = 1;
        *nl = (int)L - 2;
    }
    return EIK_OK;
}

// May this solve go to the layered solver: few-layer volumes (the rover's (x, y, mode) costmaps, C5), fp32
// and fp64, in the persistent mode, whose sources' layers zlo .. zhi (the goal's z; a seed set's lowest and
// highest) all lie among the solved ones -- a source in an all-+inf padding layer feeds its z neighbour in
// the specification, and the layered solver never reads the padding.
// *nl > 0: layers [*z0, *z0 + *nl) go there; *nl = 0: the general solver.
static int layered_route(eik_ctx* c, const void* d_cost, int64_t H, int64_t W, int64_t L, int dtype, hipStream_t st,
                         int64_t zlo, int64_t zhi, int* z0, int* nl) {
    *z0 = 0;
    *nl = 0;
    const int64_t esz = dtype == EIK_F64 ? 8 : 4;
    // (the layered kernel addresses T per tile and layer: (rows + 2) x W x L elements under 4 GiB)
    if (c->mode != kModePersistent || c->max_rounds != 1 ||
        (fim2dl_rows(dtype == EIK_F64) + 2) * W * L * esz >= (int64_t)UINT32_MAX)
        return EIK_OK;
    const int rc = layered_plan(c, d_cost, H, W, L, dtype, st, z0, nl);
    if (rc) return rc;
    if (zlo < *z0 || zhi >= *z0 + *nl) *nl = 0;
    return EIK_OK;
}

// Persistent driver of the 3D solver (fim3d_persist_kernel): one launch per solve, the tiles of
// all B volumes share one device FIFO (fim_engine.hpp), a visit's face activations queue the
// neighbours into the running launch -- no per-iteration launches or host syncs (the list driver
// took 16-32 launches of ~41 us on the planner's 60 x 60 x 41 end-effector volume).
// d_seeds (B = 1): a seed set in place of the goals (fim3d_persist_init_seeds)
static int fim3d_solve_persist(eik_ctx* c, Fim3dArgs a, int64_t B, int dtype, const int64_t* goals, hipStream_t st,
                               const Seed3Desc* d_seeds = nullptr, int64_t K = 0) {
    const int64_t tiles = a.capacity;
    uint64_t nq = 4096;
    while (nq < 8 * (uint64_t)tiles) nq <<= 1;
    HIPCHK(c, c->q3ctl.ensure(kQueueCtlBytes));
    HIPCHK(c, c->q3slot.ensure(sizeof(unsigned) * nq));
    HIPCHK(c, c->q3state.ensure(sizeof(unsigned) * tiles));
    HIPCHK(c, c->q3vis.ensure(3 * sizeof(unsigned long long)));  // visits, (unused) in-place, relaxation passes
    if (!c->h_q3) HIPCHK(c, hipHostMalloc((void**)&c->h_q3, kQueueCtlBytes + 3 * sizeof(unsigned long long)));
    for (hipEvent_t& e : c->e3)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    Fim2dArgs q{};
    q.mode = kModePersistent;
    q.qhead = (unsigned long long*)c->q3ctl.p;
    q.qtail = (unsigned long long*)((char*)c->q3ctl.p + 64);
    q.qactive = (int*)((char*)c->q3ctl.p + 128);
    q.qerror = (unsigned*)((char*)c->q3ctl.p + 192);
    q.qslot = (unsigned*)c->q3slot.p;
    q.qmask = (unsigned)(nq - 1);
    q.qstate = (unsigned*)c->q3state.p;
    q.visits = (unsigned long long*)c->q3vis.p;
    q.qtimeout = (unsigned long long)(c->qtimeout_s * 1e8);
    q.qbudget = c->max_visits ? c->max_visits : 1024ull * (unsigned long long)tiles + (1ull << 20);
    q.fresh_first = 0;
    q.qhold = nullptr;
    a.visits = (unsigned long long*)c->q3vis.p + 2;
    const bool f64 = dtype == EIK_F64;
    int& res = c->resident3[f64 ? 1 : 0];
    if (res == 0) res = fim3d_persist_resident(f64, c->cu_count);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(c->grid > 0 ? c->grid : res, res), tiles));
    hipEvent_t e0 = c->e3[0], e1 = c->e3[1];
    HIPCHK(c, hipEventRecord(e0, st));
    HIPCHK(c, hipMemsetAsync(c->q3vis.p, 0, 3 * sizeof(unsigned long long), st));
    if (d_seeds) {
        HIPCHK(c, fim3d_persist_init_seeds(a, q, f64, d_seeds, K, st));
    } else {
        HIPCHK(c, c->goals.ensure(sizeof(int64_t) * 3 * B));
        HIPCHK(c, hipMemcpyAsync(c->goals.p, goals, sizeof(int64_t) * 3 * B, hipMemcpyHostToDevice, st));
        HIPCHK(c, fim3d_persist_init(a, q, f64, (const int64_t*)c->goals.p, (int)B, st));
    }
    HIPCHK(c, fim3d_persist(a, q, f64, grid, st));
    HIPCHK(c, hipEventRecord(e1, st));
    unsigned* hq = c->h_q3;
    unsigned long long* hv = (unsigned long long*)((char*)hq + kQueueCtlBytes);
    HIPCHK(c, hipMemcpyAsync(hq, c->q3ctl.p, kQueueCtlBytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hv, c->q3vis.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int rc = persist3_outcome(c, hq[kQErrorWord], "3D solver", "3D solve: ", q.qbudget, e0, e1, hv[0]);
    if (rc) return rc;
    c->last.inplace_passes = (int64_t)hv[2];  // 3D: relaxation passes summed over the visits
    c->last.bytes_alg = (double)hv[0] * (f64 ? 8 : 4) * 3.0 * a.tx * a.ty * a.tz;
    return EIK_OK;
}

// B independent volumes of one shape (list mode; the tiles of all volumes share the lists).
// goals: B x (x, y, z), host memory.
// stop_off >= 0 (B = 1): FastMarching3D.computeTmap's early exit at that cell follows, so cells are
// only lowered to values the early-exit field keeps (Fim3dArgs::stop_off)
// d_seeds (B = 1, goals unused): the volume is seeded from the K device descriptors instead of a goal
static int fim3d_solve_batch(eik_ctx* c, const void* d_cost, void* d_T, int64_t B, int64_t H, int64_t W, int64_t L,
                             int dtype, const int64_t* goals, hipStream_t st, int64_t stop_off = -1,
                             const Seed3Desc* d_seeds = nullptr, int64_t K = 0) {
    Fim3dArgs a{};
    a.cost = d_cost;
    a.T = d_T;
    a.H = H;
    a.W = W;
    a.L = L;
    a.stop_off = -1;
    for (auto& v : c->last_solver3) v = 0;  // eik_fim3d_last_solver: the general solver
    if (stop_off >= 0 && B == 1) {
        HIPCHK(c, c->misc.ensure(64));
        HIPCHK(c, max_finite(d_cost, H * W * L, dtype == EIK_F64, (char*)c->misc.p + 32, st));
        a.stop_off = stop_off;
        a.stop_slack = (char*)c->misc.p + 32;
    }
    fim3d_tile_shape(L, &a.tx, &a.ty, &a.tz);
    a.ntx = (int)((W + a.tx - 1) / a.tx);
    a.nty = (int)((H + a.ty - 1) / a.ty);
    a.ntz = (int)((L + a.tz - 1) / a.tz);
    const int64_t tpv = (int64_t)a.ntx * a.nty * a.ntz;
    const int64_t tiles = B * tpv;
    if (tiles >= (1ll << 31) - 8) return set_err(c, EIK_ERR_ARG, "too many 3D tiles");
    a.tpv = (int)tpv;
    a.capacity = (int)tiles;
    a.max_passes = c->passes > 0 ? c->passes : c->max_passes3;
    if (c->mode == kModePersistent && H * W * L * (dtype == EIK_F64 ? 8 : 4) < (int64_t)UINT32_MAX)
        return fim3d_solve_persist(c, a, B, dtype, goals, st, d_seeds, K);
    HIPCHK(c, c->l3.ensure(sizeof(int) * 3 * tiles));
    HIPCHK(c, c->c3.ensure(sizeof(int) * 64));
    HIPCHK(c, c->m3.ensure(sizeof(unsigned) * tiles));
    HIPCHK(c, c->v3.ensure(sizeof(unsigned long long)));
    a.lists = (int*)c->l3.p;
    a.counts = (int*)c->c3.p;
    a.mark = (unsigned*)c->m3.p;
    a.visits = (unsigned long long*)c->v3.p;
    // pinned words and events live in the context: a solve of a small volume (the planner's
    // end-effector volumes) is ~1 ms, so per-call hipHostMalloc / event creation would show
    if (!c->h3) HIPCHK(c, hipHostMalloc((void**)&c->h3, sizeof(int) * 2 + sizeof(unsigned long long)));
    for (hipEvent_t& e : c->e3)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipEvent_t e0 = c->e3[0], e1 = c->e3[1];
    HIPCHK(c, hipEventRecord(e0, st));
    HIPCHK(c, hipMemsetAsync(c->v3.p, 0, sizeof(unsigned long long), st));
    if (d_seeds) {
        HIPCHK(c, fim3d_init_seeds(a, dtype == EIK_F64, d_seeds, K, st));
    } else {
        HIPCHK(c, c->goals.ensure(sizeof(int64_t) * 3 * B));
        HIPCHK(c, hipMemcpyAsync(c->goals.p, goals, sizeof(int64_t) * 3 * B, hipMemcpyHostToDevice, st));
        HIPCHK(c, fim3d_init(a, dtype == EIK_F64, (const int64_t*)c->goals.p, (int)B, st));
    }
    int* h = c->h3;
    const int grid = c->grid > 0 ? c->grid : 4 * c->cu_count;
    const int64_t max_iters = 64 * ((int64_t)a.ntx + a.nty + a.ntz) + 8 * tiles + 4096;
    int64_t it = 0;
    int rc = EIK_OK;
    for (;;) {
        for (int k = 0; k < c->sync_every; ++k, ++it) {
            a.iter = (unsigned)it;
            hipError_t e = fim3d_sweep(a, dtype == EIK_F64, grid, st);
            if (e != hipSuccess) { rc = set_err(c, EIK_ERR_HIP, "fim3d_sweep: %s", hipGetErrorString(e)); break; }
        }
        if (rc) break;
        hipError_t e = hipMemcpyAsync(h, (int*)c->c3.p + (it % 3), sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { rc = set_err(c, EIK_ERR_HIP, "fim3d sync: %s", hipGetErrorString(e)); break; }
        if (h[0] == 0) break;
        if (it >= max_iters) { rc = set_err(c, EIK_ERR_NOCONVERGE, "3D solve did not converge"); break; }
    }
    if (rc == EIK_OK) {
        unsigned long long* hv = (unsigned long long*)(h + 2);
        (void)hipEventRecord(e1, st);
        (void)hipMemcpyAsync(hv, c->v3.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        c->last = eik_stats{};
        c->last.iterations = it;
        c->last.tile_visits = (int64_t)*hv;
        c->last.solve_ms = ms;
        c->last.bytes_alg = (double)*hv * (dtype == EIK_F64 ? 8 : 4) * 3.0 * a.tx * a.ty * a.tz;
    }
    return rc;
}

int eik_fim3d_solve(eik_ctx* c, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int dtype,
                    const int64_t goal[3], void* stream) {
    return fim3d_solve_one(c, d_cost, d_T, H, W, L, dtype, goal, (hipStream_t)stream, -1);
}

// ---- goal sets for 3D solves (fim3d.hip seeding, seeds.hip labels3d)
// The host checks shared by the seeded solve and the labels: on EIK_OK out holds the K descriptors, t0
// rounded to the dtype.  Every failure is EIK_ERR_ARG with the offending index; nothing is launched.
static int seeds3_check(eik_ctx* c, const char* who, int64_t H, int64_t W, int64_t L, int dtype, const int64_t* seeds,
                        const double* t0, int64_t K, std::vector<Seed3Desc>& out) {
    if (dtype != EIK_F32 && dtype != EIK_F64) return set_err(c, EIK_ERR_ARG, "%s: bad dtype %d", who, dtype);
    if (H < 1 || W < 1 || L < 1)
        return set_err(c, EIK_ERR_ARG, "%s: bad shape %ld x %ld x %ld", who, (long)H, (long)W, (long)L);
    if (K < 1 || K > kMaxSeeds) return set_err(c, EIK_ERR_ARG, "%s: K = %ld seeds (1 .. 2^24)", who, (long)K);
    if (!seeds) return set_err(c, EIK_ERR_ARG, "%s: seeds is NULL", who);
    out.resize((size_t)K);
    for (int64_t k = 0; k < K; ++k) {
        const int64_t x = seeds[3 * k], y = seeds[3 * k + 1], z = seeds[3 * k + 2];
        if (x < 0 || y < 0 || z < 0 || x >= W || y >= H || z >= L)
            return set_err(c, EIK_ERR_ARG, "%s: seed %ld (%ld, %ld, %ld) outside %ldx%ldx%ld", who, (long)k, (long)x, (long)y,
                           (long)z, (long)H, (long)W, (long)L);
        double v = 0.0;
        const int rc = seed_t0(c, who, t0, k, dtype == EIK_F64, &v);
        if (rc) return rc;
        out[k] = Seed3Desc{x, y, z, v};
    }
    return EIK_OK;
}

// The seeded 3D solve from checked descriptors.  By default the general solver (fim3d_solve_batch: the
// persistent driver under 4 GiB in persistent mode, else the list driver).  With EIK_OPT_SEEDS_LAYERED the
// few-layer volumes that fim3d_solve_one gives to the layered solver go there too (layered_route).
static int fim3d_solve_seeds_desc(eik_ctx* c, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int dtype,
                                  const std::vector<Seed3Desc>& v, hipStream_t st) {
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t K = (int64_t)v.size();
    int rc = seeds_upload(c, c->seeds3, v, st);
    if (rc) return rc;
    int z0 = 0, nl = 0;
    if (c->seeds_layered) {
        int64_t zlo = v[0].z, zhi = v[0].z;
        for (const Seed3Desc& s : v) {
            zlo = std::min<int64_t>(zlo, s.z);
            zhi = std::max<int64_t>(zhi, s.z);
        }
        rc = layered_route(c, d_cost, H, W, L, dtype, st, zlo, zhi, &z0, &nl);
        if (rc) return rc;
    }
    if (nl > 0) return solve_layered(c, d_cost, d_T, H, W, L, z0, nl, nullptr, dtype, st, c->seeds3.d, K);
    return fim3d_solve_batch(c, d_cost, d_T, 1, H, W, L, dtype, nullptr, st, -1, c->seeds3.d, K);
}

int eik_fim3d_solve_seeds(eik_ctx* c, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int dtype,
                          const int64_t* seeds, const double* t0, int64_t K, void* stream) {
    if (!c) return EIK_ERR_ARG;
    const char* who = "eik_fim3d_solve_seeds";
    if (!d_cost || !d_T) return set_err(c, EIK_ERR_ARG, "%s: %s is NULL", who, !d_cost ? "d_cost" : "d_T");
    std::vector<Seed3Desc> v;
    const int rc = seeds3_check(c, who, H, W, L, dtype, seeds, t0, K, v);
    return rc ? rc : fim3d_solve_seeds_desc(c, d_cost, d_T, H, W, L, dtype, v, (hipStream_t)stream);
}

int eik_fim3d_last_solver(const eik_ctx* c, int64_t out[4]) {
    if (!c || !out) return EIK_ERR_ARG;
    for (int i = 0; i < 4; ++i) out[i] = c->last_solver3[i];
    return EIK_OK;
}

// the labels' cell indices are 32-bit: fewer than 2^31 cells
// (each of H, W, L checked first: the product of three values below 2^31 / of any two cannot wrap)
static bool labels3d_fit(int64_t H, int64_t W, int64_t L) {
    return H < (1ll << 31) && W < (1ll << 31) && L < (1ll << 31) && H * W < (1ll << 31) && H * W * L < (1ll << 31);
}

// the labels from checked descriptors (labels3d_fit holds)
static int labels3d_desc(eik_ctx* c, const void* d_T, int dtype, int64_t H, int64_t W, int64_t L, const std::vector<Seed3Desc>& v,
                         int32_t* d_label, hipStream_t st) {
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = H * W * L;
    HIPCHK(c, c->lab_work.ensure(sizeof(int) * (size_t)n + sizeof(unsigned) * kLabelPasses));
    const int rc = seeds_upload(c, c->lab_seeds3, v, st);
    if (rc) return rc;
    Label3Args l{};
    l.T = d_T;
    l.H = H;
    l.W = W;
    l.L = L;
    l.n = n;
    l.seeds = c->lab_seeds3.d;
    l.K = (int)v.size();
    l.par = (int*)c->lab_work.p;
    l.label = d_label;
    l.flags = (unsigned*)(l.par + n);
    HIPCHK(c, labels3d(l, dtype == EIK_F64, st));
    return EIK_OK;
}

// Nearest-goal labels of a converged volume (seeds.hip labels3d): asynchronous on `stream`, no read-back.
int eik_labels3d_dev(eik_ctx* c, const void* d_T, int dtype, int64_t H, int64_t W, int64_t L, const int64_t* seeds,
                     const double* t0, int64_t K, int32_t* d_label, void* stream) {
    if (!c) return EIK_ERR_ARG;
    const char* who = "eik_labels3d_dev";
    if (!d_T || !d_label) return set_err(c, EIK_ERR_ARG, "%s: %s is NULL", who, !d_T ? "d_T" : "d_label");
    std::vector<Seed3Desc> v;
    const int rc = seeds3_check(c, who, H, W, L, dtype, seeds, t0, K, v);
    if (rc) return rc;
    if (!labels3d_fit(H, W, L))
        return set_err(c, EIK_ERR_ARG, "%s: %ld x %ld x %ld cells (fewer than 2^31 needed)", who, (long)H, (long)W, (long)L);
    return labels3d_desc(c, d_T, dtype, H, W, L, v, d_label, (hipStream_t)stream);
}

}  // extern "C"

namespace eik_api __attribute__((visibility("hidden"))) {

// one volume; stop_off >= 0: the caller applies the early exit at that cell afterwards
int fim3d_solve_one(eik_ctx* c, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int dtype,
                    const int64_t goal[3], hipStream_t st, int64_t stop_off) {
    if (!c || !d_cost || !d_T || !goal || H < 1 || W < 1 || L < 1)
        return c ? set_err(c, EIK_ERR_ARG, "bad 3D arguments") : EIK_ERR_ARG;
    if (goal[0] < 0 || goal[1] < 0 || goal[2] < 0 || goal[0] >= W || goal[1] >= H || goal[2] >= L)
        return set_err(c, EIK_ERR_ARG, "goal (%ld,%ld,%ld) outside %ldx%ldx%ld", (long)goal[0], (long)goal[1],
                       (long)goal[2], (long)H, (long)W, (long)L);
    HIPCHK(c, hipSetDevice(c->device));
    // (an fp64 early-exit solve stays on fim3d.hip: its solve3_ref keeps the reference's exact ties,
    // which decide FM3D's closed set)
    int z0 = 0, nl = 0;
    if (!(stop_off >= 0 && dtype == EIK_F64)) {
        const int rc = layered_route(c, d_cost, H, W, L, dtype, st, goal[2], goal[2], &z0, &nl);
        if (rc) return rc;
    }
    if (nl > 0) return solve_layered(c, d_cost, d_T, H, W, L, z0, nl, goal, dtype, st);
    return fim3d_solve_batch(c, d_cost, d_T, 1, H, W, L, dtype, goal, st, stop_off);
}

// Linear index of `start` for the early exit of FastMarching3D.computeTmap (:141), or -1 when the
// reference never pops it: start == goal (the goal is closed without a pop, :132-134) or outside
// the volume.  A start on +inf cost is never popped either; the kernel sees T[start] = +inf then.
int64_t early_offset(const int64_t goal[3], const int64_t start[3], int64_t H, int64_t W, int64_t L) {
    if (!start) return -1;
    if (start[0] < 0 || start[1] < 0 || start[2] < 0 || start[0] >= W || start[1] >= H || start[2] >= L) return -1;
    if (start[0] == goal[0] && start[1] == goal[1] && start[2] == goal[2]) return -1;
    return (start[1] * W + start[0]) * L + start[2];
}

template <typename R>
static int tmap3d_host(eik_ctx* c, const R* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3],
                       const int64_t* start, R* T) {
    if (!c || !cost || !T || !goal) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    const int64_t n = H * W * L;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = stage_inputs(c, n, cost);
    if (!rc) rc = check_cost(c, cost, c->cost.p, n, c->stream);
    if (rc) return rc;
    const int dt = sizeof(R) == 8 ? EIK_F64 : EIK_F32;
    rc = fim3d_solve_one(c, c->cost.p, c->T.p, H, W, L, dt, goal, c->stream, early_offset(goal, start, H, W, L));
    if (rc) return rc;
    const void* src = c->T.p;
    if (start) {
        HIPCHK(c, c->T2.ensure(sizeof(R) * n));
        rc = eik_fim3d_early_exit(c, c->cost.p, c->T.p, c->T2.p, H, W, L, dt, goal, start, c->stream);
        if (rc) return rc;
        src = c->T2.p;
    }
    return fetch_results(c, n, T, src);
}

// one volume from a seed set; labels (optional) from the field while it is on the device
template <typename R>
static int tmap3d_seeds_host(eik_ctx* c, const R* cost, int64_t H, int64_t W, int64_t L, const int64_t* seeds,
                             const double* t0, int64_t K, R* T, int32_t* labels) {
    if (!c) return EIK_ERR_ARG;
    if (!cost || !T) return set_err(c, EIK_ERR_ARG, "eik_tmap3d_seeds: %s is NULL", !cost ? "cost" : "T");
    constexpr int dtype = sizeof(R) == 8 ? EIK_F64 : EIK_F32;
    std::vector<Seed3Desc> v;  // (checked once, before anything is uploaded: the solve and the labels take the descriptors)
    int rc = seeds3_check(c, "eik_tmap3d_seeds", H, W, L, dtype, seeds, t0, K, v);
    if (rc) return rc;
    if (labels && !labels3d_fit(H, W, L)) return set_err(c, EIK_ERR_ARG, "eik_tmap3d_seeds: labels need fewer than 2^31 cells");
    const int64_t n = H * W * L;
    HIPCHK(c, hipSetDevice(c->device));
    rc = stage_inputs(c, n, cost, labels != nullptr);
    if (!rc) rc = check_cost(c, cost, c->cost.p, n, c->stream);
    if (!rc) rc = fim3d_solve_seeds_desc(c, c->cost.p, c->T.p, H, W, L, dtype, v, c->stream);
    if (!rc && labels) rc = labels3d_desc(c, c->T.p, dtype, H, W, L, v, (int32_t*)c->lab_out.p, c->stream);
    return rc ? rc : fetch_results(c, n, T, c->T.p, labels);
}

}  // namespace eik_api

extern "C" {

int eik_tmap3d_seeds_f32(eik_ctx* c, const float* cost, int64_t H, int64_t W, int64_t L, const int64_t* seeds,
                         const double* t0, int64_t K, float* T, int32_t* labels) {
    return tmap3d_seeds_host<float>(c, cost, H, W, L, seeds, t0, K, T, labels);
}

int eik_tmap3d_seeds_f64(eik_ctx* c, const double* cost, int64_t H, int64_t W, int64_t L, const int64_t* seeds,
                         const double* t0, int64_t K, double* T, int32_t* labels) {
    return tmap3d_seeds_host<double>(c, cost, H, W, L, seeds, t0, K, T, labels);
}

int eik_fim3d_early_exit(eik_ctx* c, const void* d_cost, const void* d_T, void* d_Te, int64_t H, int64_t W, int64_t L,
                         int dtype, const int64_t goal[3], const int64_t start[3], void* stream) {
    if (!c || !d_cost || !d_T || !d_Te || !goal || !start || H < 1 || W < 1 || L < 1 || d_T == d_Te)
        return c ? set_err(c, EIK_ERR_ARG, "bad early-exit arguments") : EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t ts_off = early_offset(goal, start, H, W, L);
    for (auto& v : c->exact_info) v = 0;
    if (c->exact_band && dtype == EIK_F64 && ts_off >= 0) {
        // the reference's own band values and LIFO ties (bidir_exact.hip fm3d_exact)
        const int64_t n = H * W * L;
        if (n >= (1ll << 29)) return set_err(c, EIK_ERR_ARG, "exact band replay: volumes of < 2^29 cells");
        HIPCHK(c, c->exact.ensure(fm3d_exact_work_bytes(n)));
        hipStream_t st = (hipStream_t)stream;
        EventPair ev;  // (destroyed on every return path)
        hipEvent_t &e0 = ev.e0, &e1 = ev.e1;
        HIPCHK(c, hipEventCreate(&e0));
        HIPCHK(c, hipEventCreate(&e1));
        HIPCHK(c, hipEventRecord(e0, st));
        unsigned long long info[4] = {0, 0, 0, 0};
        const int64_t goal_off = (goal[1] * W + goal[0]) * L + goal[2];
        const hipError_t e = fm3d_exact(static_cast<const double*>(d_cost), static_cast<const double*>(d_T),
                                        static_cast<double*>(d_Te), H, W, L, goal_off, ts_off, c->exact.p,
                                        c->exact.bytes, st, info);
        if (e == hipErrorNotReady || e == hipErrorNotSupported)
            return set_err(c, EIK_ERR_NOCONVERGE, e == hipErrorNotReady
                                                      ? "FM3D early exit: the exact band replay did not settle"
                                                      : "FM3D early exit: the exact band replay met a run of more "
                                                        "than 4096 cells of exactly equal T (a zero-cost region)");
        HIPCHK(c, e);
        HIPCHK(c, hipEventRecord(e1, st));
        HIPCHK(c, hipEventSynchronize(e1));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        for (int q = 0; q < 4; ++q) c->exact_info[q] = info[q];
        c->exact_info[4] = (unsigned long long)(ms * 1000.0f);
        return EIK_OK;
    }
    HIPCHK(c, fim3d_early(d_cost, d_T, d_Te, H, W, L, ts_off, dtype == EIK_F64, (hipStream_t)stream));
    return EIK_OK;
}

int eik_tmap3d_f32(eik_ctx* c, const float* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3], float* T) {
    return tmap3d_host<float>(c, cost, H, W, L, goal, nullptr, T);
}

int eik_tmap3d_f64(eik_ctx* c, const double* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3],
                   double* T) {
    return tmap3d_host<double>(c, cost, H, W, L, goal, nullptr, T);
}

int eik_tmap3d_early_f32(eik_ctx* c, const float* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3],
                         const int64_t start[3], float* T) {
    if (!start) return c ? set_err(c, EIK_ERR_ARG, "NULL start") : EIK_ERR_ARG;
    return tmap3d_host<float>(c, cost, H, W, L, goal, start, T);
}

int eik_tmap3d_early_f64(eik_ctx* c, const double* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3],
                         const int64_t start[3], double* T) {
    if (!start) return c ? set_err(c, EIK_ERR_ARG, "NULL start") : EIK_ERR_ARG;
    return tmap3d_host<double>(c, cost, H, W, L, goal, start, T);
}

int eik_tmap3d_batch_f64(eik_ctx* c, const double* cost, int64_t B, int64_t H, int64_t W, int64_t L,
                         const int64_t* goals, double* T) {
    if (!c || !cost || !T || !goals || B < 1 || H < 1 || W < 1 || L < 1)
        return c ? set_err(c, EIK_ERR_ARG, "bad 3D batch arguments") : EIK_ERR_ARG;
    for (int64_t b = 0; b < B; ++b)
        if (goals[3 * b] < 0 || goals[3 * b + 1] < 0 || goals[3 * b + 2] < 0 || goals[3 * b] >= W ||
            goals[3 * b + 1] >= H || goals[3 * b + 2] >= L)
            return set_err(c, EIK_ERR_ARG, "goal of volume %ld outside %ldx%ldx%ld", (long)b, (long)H, (long)W, (long)L);
    const int64_t n = B * H * W * L;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->cost.ensure(sizeof(double) * n));
    HIPCHK(c, c->T.ensure(sizeof(double) * n));
    HIPCHK(c, host_to_dev(c, c->cost.p, cost, sizeof(double) * n, c->stream));
    int rc = check_cost(c, cost, c->cost.p, n, c->stream);
    if (rc) return rc;
    rc = fim3d_solve_batch(c, c->cost.p, c->T.p, B, H, W, L, EIK_F64, goals, c->stream);
    if (rc) return rc;
    HIPCHK(c, dev_to_host(c, T, c->T.p, sizeof(double) * n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

}  // extern "C"
