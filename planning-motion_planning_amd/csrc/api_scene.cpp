// api_scene.cpp -- the planner's scene pipeline: the gradient, the cost-raster builder, the rover path and
// the end-effector volume (costmap.hip, rover.cpp, arm.hip; the host API's layout: DESIGN.md §3.19).
#include <chrono>
#include <cstdlib>

#include "api_internal.hpp"

namespace eik_api __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------ cost-raster builder
// image_filling (:82-94) of the device mask m in place: the pixels equal to m[0] that the
// 4-connected flood fill from (0, 0) reaches, by connected components (cm_fill_ccl, union-find).
static int cm_fill(eik_ctx* c, unsigned char* m, int64_t H, int64_t W, float* fcost, float* fT, hipStream_t st) {
    // the two f32 scratch planes serve as the int32 lroot / parent arrays
    HIPCHK(c, cm_fill_ccl(m, H, W, reinterpret_cast<int*>(fcost), reinterpret_cast<int*>(fT), st));
    return EIK_OK;
}

// The builder's scratch: 3 masks, 3 int planes (column distances, squared EDT, envelope apexes),
// 2 f32 (fill cost, fill T), 2 f64 planes, reduction words.  obst = the caller's device mask if given.
struct cm_scratch {
    unsigned char *obst, *tmp, *dil;
    int *g, *D, *vbuf;
    float *fcost, *fT;
    double *work, *tmpd;
    unsigned long long* red;
};

static int cm_scratch_get(eik_ctx* c, int64_t n, uint8_t* d_obst, cm_scratch* s) {
    HIPCHK(c, c->cm_u8.ensure(3 * n + 64));
    HIPCHK(c, c->cm_i32.ensure(sizeof(int) * 3 * n));
    HIPCHK(c, c->cm_f32.ensure(sizeof(float) * 2 * n));
    HIPCHK(c, c->cm_f64.ensure(sizeof(double) * 2 * n + 64));
    s->obst = d_obst ? d_obst : (unsigned char*)c->cm_u8.p;
    s->tmp = (unsigned char*)c->cm_u8.p + n;
    s->dil = (unsigned char*)c->cm_u8.p + 2 * n;
    s->g = (int*)c->cm_i32.p;
    s->D = s->g + n;
    s->vbuf = s->g + 2 * n;
    s->fcost = (float*)c->cm_f32.p;
    s->fT = s->fcost + n;
    s->work = (double*)c->cm_f64.p;
    s->tmpd = s->work + n;
    s->red = (unsigned long long*)(s->tmpd + n);
    return EIK_OK;
}

static const eik_costmap_params kCmDefaults = {0.20, 0.9, 1.0, 10.0, 300.0};

// The cost tail (:1180-1216) on the device mask s.obst as it stands after :1177: obstacle border,
// expansion dilation, distance ramp, cost, blur.  s.obst ends as the final obstacle map.
static int cm_tail(eik_ctx* c, const cm_scratch& s, int64_t H, int64_t W, double res, const eik_costmap_params& p,
                   double* d_cost, hipStream_t st) {
    const int r3 = (int)std::nearbyint(p.expansion / res);                      // :1190-1191
    HIPCHK(c, cm_border(s.obst, H, W, 1, st));                                  // :1180-1184
    HIPCHK(c, cm_morph(s.obst, H, W, r3, false, s.dil, s.g, s.D, s.vbuf, st));  // :1192
    HIPCHK(c, cm_edt_ramp(s.obst, H, W, r3, s.g, s.D, s.vbuf, st));  // :1194 (distance to obstacles, as :1196 uses it)
    HIPCHK(c, cm_cost(s.obst, s.dil, s.D, H, W, res, p.high, p.gradient, s.work, s.tmpd, d_cost, s.red, st));  // :1187-1216
    return EIK_OK;
}

// ------------------------------------------- end-effector cost volume (planner step 3, :1462-1593)
namespace {

// The host side of arm.hip: the tables TunnelCost forms in Python floats (:515-519, :527-546,
// :571-590, :621-631, :655-668, :683-703), in the reference's evaluation order.
struct ArmTables {
    std::vector<double> buf;  // toaA | toaB | toaC | I | K | norm | valA | ct | st | cs | ss | ks | valC
    size_t oA = 0, oB = 0, oC = 0, oI = 0, oK = 0, oN = 0, oV = 0, oct = 0, ost = 0, ocs = 0, oss = 0, oks = 0, ovc = 0;
    int nX = 0, nZ = 0, nK = 0;
    double rad = 0;
};

void np_linspace(double a, double b, int64_t n, double* out) {
#pragma clang fp contract(off)
    if (n == 1) {
        out[0] = a;
        return;
    }
    const double div = (double)(n - 1), delta = b - a, step = delta / div;
    for (int64_t i = 0; i < n; ++i) out[i] = step == 0 ? ((double)i / div) * delta + a : (double)i * step + a;
    out[n - 1] = b;
}

void arm_toa(const double* h, const double* p, double yaw_off, double* t) {
#pragma clang fp contract(off)
    const double alpha = h[2] - yaw_off, beta = h[1], gamma = h[0];
    const double ca = std::cos(alpha), cb = std::cos(beta), cg = std::cos(gamma);
    const double sa = std::sin(alpha), sb = std::sin(beta), sg = std::sin(gamma);
    const double r[12] = {ca * cb, ca * sb * sg - sa * cg, ca * sb * cg + sa * sg, p[0],
                          sa * cb, sa * sb * sg + ca * cg, sa * sb * cg - ca * sg, p[1],
                          -sb,     cb * sg,                cb * cg,                p[2]};
    for (int i = 0; i < 12; ++i) t[i] = r[i];
}

void arm_tables(const double* gamma2D, const double* heading, int64_t npts, const eik_arm_volume& v, ArmTables& T) {
#pragma clang fp contract(off)
    const double gradient = 15.0;                                              // :512
    const double tunnelRad = v.rlim + 2 * v.resX;                              // :515
    T.nX = (int)(std::nearbyint(2 * tunnelRad / v.resX) + 1);                  // :516
    T.nZ = (int)(std::nearbyint(2 * tunnelRad / v.resZ) + 1);                  // :517
    T.nK = (int)std::nearbyint(T.nZ / 2.0) + 1;                                // :671
    T.rad = v.rlim + 2 * v.resZ;                                               // :688-690
    const size_t nik = (size_t)T.nX * T.nZ;
    size_t o = 0;
    T.oA = o; o += 12 * (size_t)npts;
    T.oB = o; o += 12;
    T.oC = o; o += 12;
    T.oI = o; o += T.nX;
    T.oK = o; o += T.nZ;
    T.oN = o; o += nik;
    T.oV = o; o += nik;
    T.oct = o; o += 100;
    T.ost = o; o += 100;
    T.ocs = o; o += 90;
    T.oss = o; o += 90;
    T.oks = o; o += T.nK;
    T.ovc = o; o += T.nK;
    T.buf.assign(o, 0.0);
    double* b = T.buf.data();
    const double half_pi = 3.141592653589793 / 2;  // math.pi / 2
    for (int64_t j = 0; j < npts; ++j) arm_toa(heading + 3 * j, gamma2D + 3 * j, half_pi, b + T.oA + 12 * j);
    arm_toa(heading, gamma2D, half_pi, b + T.oB);                                          // :617-631
    arm_toa(heading + 3 * (npts - 1), gamma2D + 3 * (npts - 1), 0.0, b + T.oC);            // :655-668
    np_linspace(-tunnelRad, tunnelRad, T.nX, b + T.oI);                                     // :563
    np_linspace(-tunnelRad, tunnelRad, T.nZ, b + T.oK);                                     // :564
    const double c = (v.rO + v.rm) / 2;
    for (int i = 0; i < T.nX; ++i)
        for (int k = 0; k < T.nZ; ++k) {
            const double I = b[T.oI + i], K = b[T.oK + k];
            const double i2 = I * I, k2 = K * K;
            const double norm = std::sqrt(i2 + k2);                                         // :578
            const double d = norm - c;
            const double t1 = gradient * (d * d) + 2;
            const double u = ((I + v.rlim) + 2 * v.resZ);
            b[T.oN + (size_t)i * T.nZ + k] = norm;
            b[T.oV + (size_t)i * T.nZ + k] = t1 + 4 * u;                                   // :590
        }
    for (int ti = 0; ti < 100; ++ti) {                                                      // :674-676
        const double theta = 3.141592653589793 * (-100 + 2 * ti) / 180;
        b[T.oct + ti] = std::cos(theta);
        b[T.ost + ti] = std::sin(theta);
    }
    for (int si = 0; si < 90; ++si) {                                                       // :679-681
        const double sigma = 3.141592653589793 * (-90 + 2 * si) / 180;
        b[T.ocs + si] = std::cos(sigma);
        b[T.oss + si] = std::sin(sigma);
    }
    np_linspace(0.0, tunnelRad, T.nK, b + T.oks);                                           // :684
    for (int k = 0; k < T.nK; ++k) {
        const double d = b[T.oks + k] - c;
        b[T.ovc + k] = gradient * (d * d) + 2;                                              // :703
    }
}

}  // namespace

// arm_obst_columns' flag: bit 1 a NaN / inf height (:334 raises), bit 0 an index below -sZ (:341 / :346)
static int arm_obst_bad(eik_ctx* c, unsigned bad) {
    if (bad & 2u) return set_err(c, EIK_ERR_ARG, "GetObstMap: a height is NaN or infinite (the reference raises)");
    return set_err(c, EIK_ERR_ARG, "GetObstMap: a surface index below -sZ (the reference raises IndexError)");
}

// Build the volume on the device into d_cost (fmap * tunnel) and/or return the pieces.  d_fmap:
// GetObstMap's finalMap (computed here when d_Z != nullptr); d_tunnel: TunnelCost's map.
static int arm_volume_dev(eik_ctx* c, const double* d_Z, const double* d_obst, int64_t m, int64_t n,
                          const double* gamma2D, const double* heading, int64_t npts, const eik_arm_volume* v,
                          double* d_fmap, double* d_omap, double* d_gmap, double* d_tunnel, double* d_cost,
                          hipStream_t st) {
    const int64_t nc = v->sX * v->sY * v->sZ;
    // int(round(.)) of a NaN / inf raises in the reference (:558-560 and their repeats), and so does
    // math.cos of an inf (:531-536).  Every event converts its node, so one such input fails the call;
    // nothing is launched for it.  (A finite input whose node overflows to inf is left to the kernel.)
    for (int64_t k = 0; k < 3 * npts; ++k)
        if (!std::isfinite(gamma2D[k]) || !std::isfinite(heading[k]))
            return set_err(c, EIK_ERR_ARG, "TunnelCost: base point or heading %ld is NaN or infinite (the reference raises)",
                           (long)(k / 3));
    HIPCHK(c, c->misc.ensure(64));
    HIPCHK(c, hipMemsetAsync(c->misc.p, 0, 2 * sizeof(unsigned), st));  // [0] GetObstMap, [1] TunnelCost
    if (d_Z) {
        HIPCHK(c, arm_obst_map(d_Z, d_obst, m, n, v->resX, v->resY, v->resZ, v->sX, v->sY, v->sZ, v->xm, v->ym, d_fmap,
                               d_omap, d_gmap, (unsigned*)c->misc.p, st));
    }
    if (!d_tunnel) return EIK_OK;
    ArmTables T;
    arm_tables(gamma2D, heading, npts, *v, T);
    ArmArgs a{};
    a.sX = v->sX;
    a.sY = v->sY;
    a.sZ = v->sZ;
    a.resX = v->resX;
    a.resY = v->resY;
    a.resZ = v->resZ;
    a.rlim = v->rlim;
    a.rad = T.rad;
    a.nX = T.nX;
    a.nZ = T.nZ;
    a.nK = T.nK;
    a.nA = 2ull * (unsigned long long)npts * T.nX * T.nZ;
    a.nB = (unsigned long long)T.nX * T.nZ;
    a.nC = 100ull * 90ull * (unsigned long long)(T.nK + 1);
    if (a.nA + a.nB + a.nC >= 0xffffffffull) return set_err(c, EIK_ERR_ARG, "too many tunnel events");
    for (int k = 0; k < 3; ++k) {
        a.fw[k] = v->final_wp[k];
        a.iw[k] = v->initial_wp[k];
    }
    // scratch: tables | first (u32) | closed (u8)
    const size_t tb = sizeof(double) * T.buf.size();
    const size_t need = tb + sizeof(unsigned) * nc + nc + 256;
    HIPCHK(c, c->arm.ensure(need));
    char* p = (char*)c->arm.p;
    HIPCHK(c, hipMemcpyAsync(p, T.buf.data(), tb, hipMemcpyHostToDevice, st));
    const double* d = (const double*)p;
    a.toaA = d + T.oA;
    a.toaB = d + T.oB;
    a.toaC = d + T.oC;
    a.tabI = d + T.oI;
    a.tabK = d + T.oK;
    a.norm = d + T.oN;
    a.valA = d + T.oV;
    a.ct = d + T.oct;
    a.st = d + T.ost;
    a.cs = d + T.ocs;
    a.ss = d + T.oss;
    a.ks = d + T.oks;
    a.valC = d + T.ovc;
    a.first = (unsigned*)(p + ((tb + 255) & ~(size_t)255));
    a.closed = (unsigned char*)(a.first + nc);
    a.tunnel = d_tunnel;
    a.fmap = d_fmap;
    a.out = d_cost;
    a.bad = (unsigned*)c->misc.p + 1;
    HIPCHK(c, arm_tunnel(a, st));
    // the tables must outlive the kernels: T.buf is host memory copied above; wait before return
    HIPCHK(c, hipStreamSynchronize(st));
    unsigned bad[2] = {0, 0};
    HIPCHK(c, hipMemcpy(bad, c->misc.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0]) return arm_obst_bad(c, bad[0]);
    if (bad[1]) return set_err(c, EIK_ERR_ARG, "TunnelCost: a node index is infinite (the reference raises OverflowError)");
    return EIK_OK;
}

static int arm_check(eik_ctx* c, const eik_arm_volume* v) {
    if (!v || v->sX < 1 || v->sY < 1 || v->sZ < 1 || !(v->resX > 0) || !(v->resY > 0) || !(v->resZ > 0))
        return set_err(c, EIK_ERR_ARG, "bad arm volume");
    if (v->sX != v->sY) return set_err(c, EIK_ERR_ARG, "arm volume must be square in x, y (sX %ld != sY %ld)",
                                       (long)v->sX, (long)v->sY);
    return EIK_OK;
}

}  // namespace eik_api

extern "C" {

int eik_gradient2d_f64(eik_ctx* c, const double* T, int64_t H, int64_t W, double* gnx, double* gny) {
    if (!c || !T || !gnx || !gny || H < 2 || W < 2) return c ? set_err(c, EIK_ERR_ARG, "bad arguments") : EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = H * W;
    HIPCHK(c, c->T2.ensure(sizeof(double) * n));
    HIPCHK(c, c->work.ensure(sizeof(double) * 2 * n));
    HIPCHK(c, host_to_dev(c, c->T2.p, T, sizeof(double) * n, c->stream));
    double* gx = (double*)c->work.p;
    HIPCHK(c, gradient2d((const double*)c->T2.p, H, W, gx, gx + n, c->stream));
    HIPCHK(c, dev_to_host(c, gnx, gx, sizeof(double) * n, c->stream));
    HIPCHK(c, dev_to_host(c, gny, gx + n, sizeof(double) * n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

int eik_costmap_dev(eik_ctx* c, const double* d_Z, int64_t H, int64_t W, double res, double size,
                    const eik_costmap_params* params, double* d_cost, uint8_t* d_obst, void* stream) {
    if (!c || !d_Z || !d_cost || H < 3 || W < 3 || !(res > 0) || !(size > 0))
        return c ? set_err(c, EIK_ERR_ARG, "bad cost-map arguments") : EIK_ERR_ARG;
    const eik_costmap_params p = params ? *params : kCmDefaults;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    cm_scratch s;
    int rc = cm_scratch_get(c, H * W, d_obst, &s);
    if (rc) return rc;
    const int r1 = 10;                                              // :1167
    const int r2 = (int)std::nearbyint((p.diagonal / 2) / res);     // :1172-1173
    HIPCHK(c, cm_normals(d_Z, H, W, size, s.red, p.slope_max, s.obst, nullptr, nullptr, nullptr, st));  // :1104-1160
    // min(Z)'s key (red is reused below) for the rover path's z lookup (:1101, :1246): misc word 5
    HIPCHK(c, c->misc.ensure(64));
    HIPCHK(c, hipMemcpyAsync((unsigned long long*)c->misc.p + 5, s.red, sizeof(unsigned long long),
                             hipMemcpyDeviceToDevice, st));
    rc = cm_fill(c, s.obst, H, W, s.fcost, s.fT, st);                         // :1163-1164
    if (rc) return rc;
    HIPCHK(c, cm_morph(s.obst, H, W, r1, true, s.tmp, s.g, s.D, s.vbuf, st));  // :1168
    HIPCHK(c, cm_morph(s.tmp, H, W, r1, false, s.obst, s.g, s.D, s.vbuf, st)); // :1169
    HIPCHK(c, cm_morph(s.obst, H, W, r2, false, s.tmp, s.g, s.D, s.vbuf, st)); // :1175
    rc = cm_fill(c, s.tmp, H, W, s.fcost, s.fT, st);                          // :1176
    if (rc) return rc;
    HIPCHK(c, cm_morph(s.tmp, H, W, r2, true, s.obst, s.g, s.D, s.vbuf, st));  // :1177
    return cm_tail(c, s, H, W, res, p, d_cost, st);                           // :1180-1216
}

int eik_costmap_f64(eik_ctx* c, const double* Z, int64_t H, int64_t W, double res, double size,
                    const eik_costmap_params* params, double* cost_out, uint8_t* obst_out) {
    if (!c || !Z || !cost_out) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = H * W;
    HIPCHK(c, c->T2.ensure(sizeof(double) * 2 * n + n));
    double* dZ = (double*)c->T2.p;
    double* dC = dZ + n;
    uint8_t* dO = (uint8_t*)(dC + n);
    HIPCHK(c, host_to_dev(c, dZ, Z, sizeof(double) * n, c->stream));
    int rc = eik_costmap_dev(c, dZ, H, W, res, size, params, dC, dO, c->stream);
    if (rc) return rc;
    HIPCHK(c, dev_to_host(c, cost_out, dC, sizeof(double) * n, c->stream));
    if (obst_out) HIPCHK(c, dev_to_host(c, obst_out, dO, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

int eik_cost_tail_u8(eik_ctx* c, const uint8_t* obst, int64_t H, int64_t W, double res,
                     const eik_costmap_params* params, double* cost_out, uint8_t* obst_out) {
    if (!c || !obst || !cost_out || H < 3 || W < 3 || !(res > 0))
        return c ? set_err(c, EIK_ERR_ARG, "bad cost-tail arguments") : EIK_ERR_ARG;
    const eik_costmap_params p = params ? *params : kCmDefaults;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = H * W;
    cm_scratch s;
    int rc = cm_scratch_get(c, n, nullptr, &s);
    if (rc) return rc;
    HIPCHK(c, c->T2.ensure(sizeof(double) * n));
    double* dC = (double*)c->T2.p;
    HIPCHK(c, host_to_dev(c, s.obst, obst, n, c->stream));
    rc = cm_tail(c, s, H, W, res, p, dC, c->stream);
    if (rc) return rc;
    HIPCHK(c, dev_to_host(c, cost_out, dC, sizeof(double) * n, c->stream));
    if (obst_out) HIPCHK(c, dev_to_host(c, obst_out, s.obst, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

int eik_surface_normal_f64(eik_ctx* c, const double* Z, int64_t H, int64_t W, double size, double* Nx, double* Ny,
                           double* Nz) {
    if (!c || !Z || !Nx || !Ny || !Nz || H < 3 || W < 3 || !(size > 0))
        return c ? set_err(c, EIK_ERR_ARG, "bad surface_normal arguments") : EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = H * W;
    HIPCHK(c, c->T2.ensure(sizeof(double) * 4 * n + 64));
    double* dZ = (double*)c->T2.p;
    unsigned long long* red = (unsigned long long*)(dZ + 4 * n);
    HIPCHK(c, host_to_dev(c, dZ, Z, sizeof(double) * n, c->stream));
    HIPCHK(c, cm_normals(dZ, H, W, size, red, 0.0, nullptr, dZ + n, dZ + 2 * n, dZ + 3 * n, c->stream));
    HIPCHK(c, dev_to_host(c, Nx, dZ + n, sizeof(double) * n, c->stream));
    HIPCHK(c, dev_to_host(c, Ny, dZ + 2 * n, sizeof(double) * n, c->stream));
    HIPCHK(c, dev_to_host(c, Nz, dZ + 3 * n, sizeof(double) * n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

int eik_image_fill_u8(eik_ctx* c, const uint8_t* im, int64_t H, int64_t W, uint8_t* out) {
    if (!c || !im || !out || H < 1 || W < 1) return c ? set_err(c, EIK_ERR_ARG, "bad image_filling arguments") : EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = H * W;
    HIPCHK(c, c->cm_u8.ensure(3 * n + 64));
    HIPCHK(c, c->cm_f32.ensure(sizeof(float) * 2 * n));
    unsigned char* m = (unsigned char*)c->cm_u8.p;
    HIPCHK(c, host_to_dev(c, m, im, n, c->stream));
    float* fcost = (float*)c->cm_f32.p;
    int rc = cm_fill(c, m, H, W, fcost, fcost + n, c->stream);
    if (rc) return rc;
    HIPCHK(c, dev_to_host(c, out, m, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

int eik_disk_morph_u8(eik_ctx* c, const uint8_t* im, int64_t H, int64_t W, int radius, int erode, uint8_t* out) {
    if (!c || !im || !out || H < 1 || W < 1 || radius < 0)
        return c ? set_err(c, EIK_ERR_ARG, "bad disk morphology arguments") : EIK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = H * W;
    HIPCHK(c, c->cm_u8.ensure(3 * n + 64));
    HIPCHK(c, c->cm_i32.ensure(sizeof(int) * 3 * n));
    unsigned char* a = (unsigned char*)c->cm_u8.p;
    unsigned char* o = a + n;
    int* g = (int*)c->cm_i32.p;
    HIPCHK(c, host_to_dev(c, a, im, n, c->stream));
    HIPCHK(c, cm_morph(a, H, W, radius, erode != 0, o, g, g + n, g + 2 * n, c->stream));
    HIPCHK(c, dev_to_host(c, out, o, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

// ------------------------------------------------------- rover path (planner step 1, :1097-1258)
int eik_rover_path_f64(eik_ctx* c, const double* Z, int64_t H, int64_t W, const eik_rover_query* q,
                       const eik_costmap_params* params, double* path_xyz, double* heading, int64_t cap,
                       int64_t* n_out, uint32_t join[2], double* cost_out) {
    if (!c || !Z || !q || !path_xyz || !heading || !n_out || H < 3 || W < 3 || !(q->resolution > 0) ||
        !(q->size > 0) || !(q->tau > 0))
        return c ? set_err(c, EIK_ERR_ARG, "bad rover-path arguments") : EIK_ERR_ARG;
    const int64_t n = H * W;
    if (n >= (1ll << 29)) return set_err(c, EIK_ERR_ARG, "bidirectional join supports < 2^29 cells");
    // nodes: int(round(v / res - 1)), Python's round = half to even   :1107-1117
    const double res = q->resolution;
    const int64_t g[4] = {(int64_t)std::nearbyint(q->xm / res - 1), (int64_t)std::nearbyint(q->ym / res - 1),
                          (int64_t)std::nearbyint(q->xr / res - 1), (int64_t)std::nearbyint(q->yr / res - 1)};
    for (int k = 0; k < 2; ++k)
        if (g[2 * k] < 0 || g[2 * k + 1] < 0 || g[2 * k] >= W || g[2 * k + 1] >= H)
            return set_err(c, EIK_ERR_ARG, "%s node (%ld, %ld) outside the %ldx%ld DEM", k ? "rover" : "sample",
                           (long)g[2 * k], (long)g[2 * k + 1], (long)H, (long)W);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t steps = (int64_t)std::nearbyint(15000.0 / q->tau);  // FastMarching.py:173
    const int64_t pcap = steps + 4;
    const size_t pbytes = sizeof(double) * 2 * 2 * pcap + 64;
    HIPCHK(c, c->T2.ensure(std::max(sizeof(double) * n, pbytes)));  // Z, then (Z consumed) the paths
    HIPCHK(c, c->cost.ensure(sizeof(double) * 2 * n));
    HIPCHK(c, c->T.ensure(sizeof(double) * 2 * n));
    double* dZ = (double*)c->T2.p;
    double* dcost = (double*)c->cost.p;
    double* dT = (double*)c->T.p;
    // EIK_ROVER_PHASES=1 (diagnostics): synchronise after each phase and print its wall time
    static const bool phases = getenv("EIK_ROVER_PHASES") != nullptr;
    auto tp = std::chrono::steady_clock::now();
    auto phase = [&](const char* name) {
        if (!phases) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[rover] %-10s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(now - tp).count());
        tp = now;
    };
    phase("setup");
    HIPCHK(c, host_to_dev(c, dZ, Z, sizeof(double) * n, st));
    phase("dem_h2d");
    int rc = eik_costmap_dev(c, dZ, H, W, res, q->size, params, dcost, nullptr, st);  // :1101-1216
    if (rc) return rc;
    phase("costmap");
    // biComputeTmap(cMap.T, goal = sample node, start = rover node)   :1222; both fronts, one batch
    HIPCHK(c, hipMemcpyAsync(dcost + n, dcost, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    if (cost_out) HIPCHK(c, dev_to_host(c, cost_out, dcost, sizeof(double) * n, st));
    eik_fim2d* f = nullptr;
    rc = get_solver(c, 2, H, W, EIK_F64, &f);
    if (rc) return rc;
    unsigned long long best = 0;
    rc = solve_fronts(c, f, dcost, dT, g, H, W, &best);  // :114-162
    if (rc) return rc;
    phase("fronts");
    if (best == ~0ull) return set_err(c, EIK_ERR_UNREACHABLE, "the rover cannot reach the sample");
    const int64_t node = (int64_t)(best & ((1ull << 29) - 1));
    const double jn[2] = {(double)(node % W), (double)(node / W)};
    if (join) {
        join[0] = (uint32_t)(node % W);
        join[1] = (uint32_t)(node / W);
    }
    // pathG = getPathGDM(TmapG, nodeJoin, goal, tau), pathS = getPathGDM(TmapS, nodeJoin, start, tau)   :1225-1226
    double* dP = (double*)c->T2.p;  // [pathG | pathS], then n_out[2], status[2]
    int64_t* dn = (int64_t*)(dP + 2 * 2 * pcap);
    int* dst = (int*)(dn + 2);
    const double eg[2] = {(double)g[0], (double)g[1]}, es[2] = {(double)g[2], (double)g[3]};
    // the two walks are independent one-workgroup kernels: pathS runs on a second stream beside
    // pathG (each walk is one dependent chain of steps, ~0.4 us each)
    if (!c->stream2) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    if (!c->ev_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_fork, st));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    rc = eik_path2d_dev(c, dT, EIK_F64, H, W, jn, eg, q->tau, dP, pcap, dn, dst, st);
    if (rc) return rc;
    rc = eik_path2d_dev(c, dT + n, EIK_F64, H, W, jn, es, q->tau, dP + 2 * pcap, pcap, dn + 1, dst + 1, c->stream2);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
    phase("walks");
    int64_t hn[2];
    int hs[2];
    unsigned long long zkey = 0;
    HIPCHK(c, hipMemcpyAsync(hn, dn, sizeof hn, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hs, dst, sizeof hs, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&zkey, (unsigned long long*)c->misc.p + 5, sizeof zkey, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (hs[0] == EIK_PATH_ERROR || hs[1] == EIK_PATH_ERROR)
        return set_err(c, EIK_ERR_ARG, "getPathGDM failed (the reference raises): NaN point or out of range");
    std::vector<double> pg((size_t)(2 * hn[0])), ps((size_t)(2 * hn[1]));
    HIPCHK(c, hipMemcpyAsync(pg.data(), dP, sizeof(double) * 2 * hn[0], hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(ps.data(), dP + 2 * pcap, sizeof(double) * 2 * hn[1], hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    phase("paths_d2h");
    // the cost builder's min(Z), from its order-preserving key (costmap.hip dkey)
    const unsigned long long zb = (zkey >> 63) ? (zkey & ~(1ull << 63)) : ~zkey;
    double zmin;
    memcpy(&zmin, &zb, sizeof zmin);
    rc = rover_assemble(ps.data(), hn[1], pg.data(), hn[0], Z, H, W, q, path_xyz, heading, cap, n_out, zmin);
    phase("assemble");
    if (rc) return set_err(c, rc, *n_out > cap ? "path buffer too small (%ld rows needed)" : "waypoint outside the DEM",
                           (long)*n_out);
    return EIK_OK;
}

int eik_arm_obst_map_f64(eik_ctx* c, const double* Z, const double* obst, int64_t m, int64_t n,
                         const eik_arm_volume* v, double* fmap, double* omap, double* gmap) {
    if (!c || !Z || !obst || !fmap || m < 1 || n < 1) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    int rc = arm_check(c, v);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t nc = v->sX * v->sY * v->sZ, nz = m * n;
    HIPCHK(c, c->T2.ensure(sizeof(double) * (2 * nz + 3 * nc)));
    double* dZ = (double*)c->T2.p;
    double* dO = dZ + nz;
    double* dF = dO + nz;
    double* dOm = omap ? dF + nc : nullptr;
    double* dGm = gmap ? dF + 2 * nc : nullptr;
    HIPCHK(c, host_to_dev(c, dZ, Z, sizeof(double) * nz, st));
    HIPCHK(c, host_to_dev(c, dO, obst, sizeof(double) * nz, st));
    rc = arm_volume_dev(c, dZ, dO, m, n, nullptr, nullptr, 0, v, dF, dOm, dGm, nullptr, nullptr, st);
    if (rc) return rc;
    unsigned bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, c->misc.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(c, dev_to_host(c, fmap, dF, sizeof(double) * nc, st));
    if (omap) HIPCHK(c, dev_to_host(c, omap, dOm, sizeof(double) * nc, st));
    if (gmap) HIPCHK(c, dev_to_host(c, gmap, dGm, sizeof(double) * nc, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (bad) return arm_obst_bad(c, bad);
    return EIK_OK;
}

int eik_arm_tunnel_cost_f64(eik_ctx* c, const double* gamma2D, const double* heading, int64_t npts,
                            const eik_arm_volume* v, double* Cmap) {
    if (!c || !gamma2D || !heading || !Cmap || npts < 1) return c ? set_err(c, EIK_ERR_ARG, "NULL argument") : EIK_ERR_ARG;
    int rc = arm_check(c, v);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t nc = v->sX * v->sY * v->sZ;
    HIPCHK(c, c->T2.ensure(sizeof(double) * nc));
    double* dT = (double*)c->T2.p;
    rc = arm_volume_dev(c, nullptr, nullptr, 0, 0, gamma2D, heading, npts, v, nullptr, nullptr, nullptr, dT, nullptr,
                        c->stream);
    if (rc) return rc;
    HIPCHK(c, dev_to_host(c, Cmap, dT, sizeof(double) * nc, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EIK_OK;
}

int eik_arm_path_f64(eik_ctx* c, const double* Z, const double* obst, int64_t m, int64_t n, const double* gamma2D,
                     const double* heading, int64_t npts, const eik_arm_volume* v, double tau, double* path,
                     int64_t cap, int64_t* n_out, int* status, double* cost_out, double* T_out) {
    if (!c || !Z || !obst || !gamma2D || !heading || !path || !n_out || !status || npts < 1 || m < 1 || n < 1 ||
        !(tau > 0) || cap < 2)
        return c ? set_err(c, EIK_ERR_ARG, "bad arm-path arguments") : EIK_ERR_ARG;
    int rc = arm_check(c, v);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) {
        const int64_t lim = k == 0 ? v->sX : k == 1 ? v->sY : v->sZ;
        if ((int64_t)v->final_wp[k] >= lim || (int64_t)v->initial_wp[k] >= lim)
            return set_err(c, EIK_ERR_ARG, "waypoint outside the %ldx%ldx%ld volume", (long)v->sX, (long)v->sY,
                           (long)v->sZ);
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t nc = v->sX * v->sY * v->sZ, nz = m * n;
    const int64_t steps = (int64_t)std::nearbyint(15000.0 / tau);
    const int64_t pcap = std::min<int64_t>(cap, steps + 4);
    // Z | obst | fmap | tunnel | cost | T (full) | T (early exit) | path | n_out | status
    HIPCHK(c, c->T2.ensure(sizeof(double) * (2 * nz + 5 * nc + 3 * pcap) + 64));
    double* dZ = (double*)c->T2.p;
    double* dO = dZ + nz;
    double* dF = dO + nz;
    double* dTun = dF + nc;
    double* dC = dTun + nc;
    double* dTf = dC + nc;
    double* dT = dTf + nc;
    double* dP = dT + nc;
    int64_t* dn = (int64_t*)(dP + 3 * pcap);
    int* dst = (int*)(dn + 1);
    HIPCHK(c, host_to_dev(c, dZ, Z, sizeof(double) * nz, st));
    HIPCHK(c, host_to_dev(c, dO, obst, sizeof(double) * nz, st));
    rc = arm_volume_dev(c, dZ, dO, m, n, gamma2D, heading, npts, v, dF, nullptr, nullptr, dTun, dC, st);
    if (rc) return rc;
    // FM3D.computeTmap(Cmap, finalWayPointArm, initialWayPointArm) :1585; H = sY rows, W = sX columns
    // with its early exit once initialWayPointArm is popped (FastMarching3D.py:141)
    const int64_t goal[3] = {v->final_wp[0], v->final_wp[1], v->final_wp[2]};
    const int64_t start[3] = {v->initial_wp[0], v->initial_wp[1], v->initial_wp[2]};
    rc = fim3d_solve_one(c, dC, dTf, v->sY, v->sX, v->sZ, EIK_F64, goal, st,
                         early_offset(goal, start, v->sY, v->sX, v->sZ));
    if (rc) return rc;
    rc = eik_fim3d_early_exit(c, dC, dTf, dT, v->sY, v->sX, v->sZ, EIK_F64, goal, start, st);
    if (rc) return rc;
    // FM3D.getPathGDM(Tmap3D, initialWayPointArm, finalWayPointArm, 0.5) :1588
    const double init[3] = {(double)v->initial_wp[0], (double)v->initial_wp[1], (double)v->initial_wp[2]};
    const double end[3] = {(double)v->final_wp[0], (double)v->final_wp[1], (double)v->final_wp[2]};
    rc = eik_path3d_dev(c, dT, EIK_F64, v->sY, v->sX, v->sZ, init, end, tau, dP, pcap, dn, dst, st);
    if (rc) return rc;
    int64_t hn = 0;
    HIPCHK(c, hipMemcpyAsync(&hn, dn, sizeof hn, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(status, dst, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *n_out = hn;
    HIPCHK(c, hipMemcpyAsync(path, dP, sizeof(double) * 3 * hn, hipMemcpyDeviceToHost, st));
    if (cost_out) HIPCHK(c, dev_to_host(c, cost_out, dC, sizeof(double) * nc, st));
    if (T_out) HIPCHK(c, dev_to_host(c, T_out, dT, sizeof(double) * nc, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return EIK_OK;
}

}  // extern "C"
