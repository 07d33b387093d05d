// gdm_walk.hpp -- what the 2D path kernels share (gdm.hip: the reference-faithful walker, all loop
// forms; gdm_safe.hip: the obstacle-safe walker): the gradient and interpolation helpers, the
// range-free f64 square root / division of the fast step, the step's arithmetic in its three forms
// (walk_step_*), and the window machinery (LDS windows of the normalised gradient, builder waves and
// their polling loop -- the 3D walker's too --, the walker's window state Walk2Win).  Include it after
// `#pragma clang fp contract(off)`: every function here is IEEE fp64 without contraction.
#pragma once
#include "eik_common.hpp"
#include "eik_kernels.hpp"

namespace eik {

template <typename R>
__device__ __forceinline__ double tv(const R* __restrict__ T, int64_t W, int64_t j, int64_t i) {
    return (double)T[j * W + i];
}

// computeGradient body at one (j, i), FastMarching.py:262-297
template <typename R>
__device__ void grad_at(const R* __restrict__ T, int64_t m, int64_t n, int64_t j, int64_t i, double& gnx, double& gny) {
    double gy, gx;
    if (j == 0)
        gy = tv(T, n, 1, i) - tv(T, n, 0, i);
    else if (j == m - 1)
        gy = tv(T, n, j, i) - tv(T, n, j - 1, i);
    else if (__builtin_isinf(tv(T, n, j + 1, i)))
        gy = __builtin_isinf(tv(T, n, j - 1, i)) ? 0.0 : tv(T, n, j, i) - tv(T, n, j - 1, i);
    else
        gy = __builtin_isinf(tv(T, n, j - 1, i)) ? tv(T, n, j + 1, i) - tv(T, n, j, i)
                                                 : (tv(T, n, j + 1, i) - tv(T, n, j - 1, i)) / 2;
    if (i == 0)
        gx = tv(T, n, j, 1) - tv(T, n, j, 0);
    else if (i == n - 1)
        gx = tv(T, n, j, i) - tv(T, n, j, i - 1);
    else if (__builtin_isinf(tv(T, n, j, i + 1)))
        gx = __builtin_isinf(tv(T, n, j, i - 1)) ? 0.0 : tv(T, n, j, i) - tv(T, n, j, i - 1);
    else
        gx = __builtin_isinf(tv(T, n, j, i - 1)) ? tv(T, n, j, i + 1) - tv(T, n, j, i)
                                                 : (tv(T, n, j, i + 1) - tv(T, n, j, i - 1)) / 2;
    const double den = __builtin_sqrt(gx * gx + gy * gy);
    gnx = gx / den;
    gny = gy / den;
}

// interpolatePoint FastMarching.py:305-338 on a 2x2 patch g[jj][ii]
__device__ __forceinline__ double interp2_patch(double a, double b, const double (&g)[2][2]) {
    const double a00 = g[0][0];
    const double a10 = g[0][1] - g[0][0];
    const double a01 = g[1][0] - g[0][0];
    const double a11 = g[1][1] + g[0][0] - g[0][1] - g[1][0];
    if (a == 0) return b == 0 ? a00 : a00 + a01 * b;
    return b == 0 ? a00 + a10 * a : a00 + a10 * a + a01 * b + a11 * a * b;
}

// interp2_patch with the four cases of :327-336 evaluated and selected (no divergent branches on
// the walker's critical path; same operations in the same order as each case)
__device__ __forceinline__ double interp2_sel(double a, double b, double g00, double g01, double g10, double g11) {
    const double a00 = g00;
    const double a10 = g01 - g00;
    const double a01 = g10 - g00;
    const double a11 = g11 + g00 - g01 - g10;
    const double ra = a00 + a10 * a;            // b == 0
    const double rb = a00 + a01 * b;            // a == 0
    const double rf = ra + a01 * b + a11 * a * b;
    // bitwise selects: the compiler turns the ?: form into branches on the walker's chain
    const long long za = -(long long)(a == 0), zb = -(long long)(b == 0);
    const long long r0 = (__double_as_longlong(rb) & ~zb) | (__double_as_longlong(a00) & zb);   // a == 0
    const long long r1 = (__double_as_longlong(rf) & ~zb) | (__double_as_longlong(ra) & zb);    // a != 0
    return __longlong_as_double((r1 & ~za) | (r0 & za));
}

__device__ __forceinline__ double norm2(double a, double b) { return __builtin_sqrt(a * a + b * b); }

// Correctly rounded f64 square root and division exactly as the compiler lowers them for gfx950,
// minus the range handling: the same operations in the same order, so the same bits wherever
// that handling is the identity.  sqrt: the input scaling (x < 2^-767) and its undo are
// identities for x >= 2^-767 (and the compiler's final select, which keeps +-0 and +inf, is one
// for finite x > 0, so it is left out: the walker never takes x = 0 or +inf here).  n / d: v_div_scale_f64 leaves
// both operands as they are and v_div_fmas_f64 is a plain fma when d is normal in
// [2^-900, 2^100], n is 0 or normal with |n| >= 2^-900 and |n| <= |d|; v_div_fixup_f64 then only
// forces the sign of the quotient to sign(n) ^ sign(d), which it already has -- except a zero
// quotient of n = -0, which comes out +0 here (only ever squared or subtracted later: same path
// bits).  The walker takes these on its fast path and leaves it for the exact forms outside
// that domain (walk_odd).
__device__ __forceinline__ double sqrt_core(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
// sqrt_core that also hands out its refined half reciprocal hh ~ 1 / (2 sqrt(x)) (one
// Goldschmidt update of v_rsq_f64's estimate: ~2^-44 relative or better).  Same bits as sqrt_core.
__device__ __forceinline__ double sqrt_core_h(double x, double& hh) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    hh = h;
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
// sqrt_core_h with ONE residual correction after the Goldschmidt update instead of two: g is
// within ~2^-43 of sqrt(x) there, so g + (x - g^2) h is within ~2^-86 and the final fma rounds it
// as the correctly rounded root unless sqrt(x) lies that close to a rounding midpoint (~2^-33 of
// roots; an exact midpoint is impossible).  Checked bit for bit against sqrt by
// walker_math_selftest_kernel (counts[5]) on the walker's domain x in [2^-767, 2^200].  Two
// dependent operations shorter: the lane-pair walker's chain (LOOP 4) holds two of them per step.
__device__ __forceinline__ double sqrt_c1_h(double x, double& hh) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    hh = h;
    const double d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
// n / d for d = sqrt_core_h(x, h), from the reciprocal 2h the square root already holds: q0 =
// n * 2h is formed while the root is still being refined, and ONE residual correction (e = n -
// d q0 by fma, q0 + e 2h by fma) leaves two dependent operations after d instead of div_core's
// eight.  The exact sum q0 + e 2h is within ~2^-86 (relative) of n / d, so the final fma rounds it
// as the correctly rounded quotient unless n / d lies that close to a rounding midpoint (~2^-33
// of quotients): checked bit for bit against n / d by walker_math_selftest_kernel (counts[4]) on
// the walker's domain (d = sqrt(x), x in [2^-767, 2^200], |n| <= d, n = 0 or |n| >= 2^-900).
__device__ __forceinline__ double div_rs(double n, double d, double h) {
    const double r = h + h;  // exact
    const double q0 = n * r;
    const double e = __builtin_fma(-d, q0, n);
    return __builtin_fma(e, r, q0);
}
__device__ __forceinline__ double div_core(double n, double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    const double q = n * r;
    e = __builtin_fma(-d, q, n);
    return __builtin_fma(e, r, q);
}
// interpolatePoint's general case (:336) for every (a, b): where a == 0 or b == 0 it equals the
// special cases of :327-334 bit for bit (the skipped terms are exact zeros added to a nonzero
// sum; only the sign of a zero result can differ) as long as the four corners are finite; a NaN
// corner makes |g|^2 NaN, and walk_odd sends the step to the exact form.
__device__ __forceinline__ double interp2_general(double a, double b, double g00, double g01, double g10, double g11) {
    const double a10 = g01 - g00, a01 = g10 - g00, a11 = g11 + g00 - g01 - g10;
    return g00 + a10 * a + a01 * b + a11 * a * b;
}
// The step's operands leave the domain of sqrt_core / div_core: |g|^2 outside [2^-767, 2^200]
// or not finite, or an interpolated component that is nonzero but below 2^-900 in magnitude.
// (With |g|^2 >= 2^-767 every divisor is >= 2^-383; with |g|^2 <= 2^200 both divisors, |g| and
// sqrt(dx_n^2 + dy^2) <= |g| + 1, stay <= 2^100, the range div_core's argument and the self-test
// cover; in the |g| >= 0.01 branch dx_n^2 + dy^2 >= 5e-5.)
__device__ __forceinline__ bool walk_odd(double dx, double dy, double s1) {
    const double lo = 0x1p-767, big = 0x1p200, tiny = 0x1p-900;
    return !(s1 >= lo && s1 <= big) | ((dx != 0.0) & (__builtin_fabs(dx) < tiny)) |
           ((dy != 0.0) & (__builtin_fabs(dy) < tiny));
}

// One step's arithmetic from the four corners (g00, g01, g10, g11) of the point's cell and the
// fractions (fa, fb) of (px, py) in it: :175-176 interpolation, :220-229 normalisation, :230 step.
// The one copy both 2D walkers take their steps from.
struct WalkStep {
    double dx, dy, sx, sy;
};
// the exact form: interpolation with the a == 0 / b == 0 cases, the compiler's sqrt and division
__device__ __forceinline__ WalkStep walk_step_exact(const double2& g00, const double2& g01, const double2& g10,
                                                    const double2& g11, double fa, double fb, double px, double py,
                                                    double tau) {
    WalkStep o;
    o.dx = interp2_sel(fa, fb, g00.x, g01.x, g10.x, g11.x);  // :175
    o.dy = interp2_sel(fa, fb, g00.y, g01.y, g10.y, g11.y);  // :176
    // |(dx, dy)| is the same value in the test (:220) and both normalisations (:221-227)
    const double nrm = __builtin_sqrt(o.dx * o.dx + o.dy * o.dy);
    const double dxn = o.dx / nrm;  // both branches
    // :220-224 (|g| < 0.01: unit step) or :225-229 (dy normalised with the normalised dx)
    const double dyn = nrm < 0.01 ? o.dy / nrm : o.dy / __builtin_sqrt(dxn * dxn + o.dy * o.dy);
    o.sx = px - tau * dxn;
    o.sy = py - tau * dyn;
    return o;
}
// walk_step_exact with interp2_general, sqrt_core and div_core (same bits where walk_odd is false,
// set in `odd`)
__device__ __forceinline__ WalkStep walk_step_core(const double2& g00, const double2& g01, const double2& g10,
                                                   const double2& g11, double fa, double fb, double px, double py,
                                                   double tau, bool& odd) {
    WalkStep o;
    o.dx = interp2_general(fa, fb, g00.x, g01.x, g10.x, g11.x);
    o.dy = interp2_general(fa, fb, g00.y, g01.y, g10.y, g11.y);
    const double s1 = o.dx * o.dx + o.dy * o.dy;
    const double nrm = sqrt_core(s1);
    const double dxn = div_core(o.dx, nrm);
    // both divisors computed, selected bitwise (a ?: here becomes a branch on the chain)
    const double r2 = sqrt_core(dxn * dxn + o.dy * o.dy);
    const long long small = -(long long)(nrm < 0.01);
    const double den = __longlong_as_double((__double_as_longlong(nrm) & small) | (__double_as_longlong(r2) & ~small));
    const double dyn = div_core(o.dy, den);
    o.sx = px - tau * dxn;
    o.sy = py - tau * dyn;
    odd = walk_odd(o.dx, o.dy, s1);
    return o;
}
// walk_step_core with the divisions taken from the square roots' reciprocals (div_rs): the step's
// dependent f64 chain 45 -> 33 operations (loop form 3 and the obstacle-safe walker's run loop).  The
// same bits wherever `odd` comes back false, which eik_selftest_walker_math vouches for (counts[2],
// counts[4]).
__device__ __forceinline__ WalkStep walk_step_rs(const double2& g00, const double2& g01, const double2& g10,
                                                 const double2& g11, double fa, double fb, double px, double py,
                                                 double tau, bool& odd) {
    WalkStep o;
    o.dx = interp2_general(fa, fb, g00.x, g01.x, g10.x, g11.x);
    o.dy = interp2_general(fa, fb, g00.y, g01.y, g10.y, g11.y);
    const double s1 = o.dx * o.dx + o.dy * o.dy;
    double h1, h2;
    const double nrm = sqrt_core_h(s1, h1);
    const double dxn = div_rs(o.dx, nrm, h1);
    const double r2 = sqrt_core_h(dxn * dxn + o.dy * o.dy, h2);
    const long long small = -(long long)(nrm < 0.01);
    const double den = __longlong_as_double((__double_as_longlong(nrm) & small) | (__double_as_longlong(r2) & ~small));
    const double hd = __longlong_as_double((__double_as_longlong(h1) & small) | (__double_as_longlong(h2) & ~small));
    const double dyn = div_rs(o.dy, den, hd);
    o.sx = px - tau * dxn;
    o.sy = py - tau * dyn;
    odd = walk_odd(o.dx, o.dy, s1);
    return o;
}

// DPP quad_perm moves of a double, the 2D walker's lane-pair form: Q = 0xB1 [1, 0, 3, 2] the
// partner lane's value (lane ^ 1), 0xA0 [0, 0, 2, 2] the even lane's, 0xF5 [1, 1, 3, 3] the odd one's
template <int Q>
__device__ __forceinline__ double quad_perm_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)b, Q, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(unsigned)(b >> 32), Q, 0xf, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double pair_swap(double v) { return quad_perm_f64<0xB1>(v); }

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

enum { kGdmDone = 0, kGdmFallback = 1, kGdmError = 2, kGdmStuck = 3 };  // eik_path_status

// Path kernel layout: ONE workgroup of 16 waves.  Wave 0 is the walker: it runs the reference
// loop (:173-232) step by step, reading the inf-aware normalised gradient (Gnx, Gny) of the four
// bilinear corners from an LDS window of 64 x 64 nodes.  Waves 1..15 are builders: they compute
// the gradient of a window (computeGradient's body, :262-297, at every node of the window) from
// T in HBM into one of two LDS buffers.  When the walker comes within kPrefetch nodes of an
// inner window edge it requests the window centred on itself into the idle buffer and keeps
// walking; when it leaves the current window it switches (waiting only if the build is still
// running, or if it turned away from the prefetched window).  The gradient at a node depends on
// T only, so precomputing it is exactly the reference's per-step computeGradient evaluated
// earlier: the path is bit-identical to the single-lane form.
constexpr int kPW = 64;                          // window side (nodes), one builder lane per column
constexpr int kPathThreads = 1024;               // 16 waves: walker + 15 builders
// (Round 4, measured and removed: EIK_PATH_SIMD0_FREE -- the waves sharing the walker's SIMD (4, 8,
// 12) did not build, so builds never took the walker's issue slots.  Walk 2.512-2.532 ms against
// 2.513-2.527 ms, 0.406-0.410 us/step both (profiles/r04g_walker_simd0_ab.log): the walker's step
// is its own dependent f64 chain, not issue-bound.)
constexpr int kBuilders = kPathThreads / 64 - 1;
constexpr int kRowsPerBuilder = (kPW + kBuilders - 1) / kBuilders;
constexpr int kPrefetch = 16;                    // nodes from an inner edge that trigger a prefetch
constexpr unsigned long long kPathSpin = 200000000ull;  // 2 s of s_memrealtime (100 MHz): never hang

struct PathLds {
    double2 g[2][kPW][kPW];  // (Gnx, Gny) per node, 2 x 64 KiB
    long long req_x0, req_y0;
    int req_seq;             // walker -> builders: request number (-1: quit)
    int req_b;               // target buffer of the request
    int done;                // builders -> walker: finished builds x kBuilders
};

// Builder wave `w` fills rows w, w + kBuilders, ... of window buffer b (origin x0, y0).  Every T
// load of a wave is issued before any is used (5 neighbours x kRowsPerBuilder rows per lane), so
// a build costs about one HBM/L2 round trip plus the arithmetic.  BLOCK (the obstacle-safe walker):
// the gradient of a node whose own T is +inf is NaN, so every interpolation that uses such a corner
// is NaN -- the value is already in the builder's registers, the walker's step pays nothing for it.
template <typename R, bool BLOCK = false>
__device__ void build_window(PathLds& s, const R* __restrict__ T, int64_t H, int64_t W, int b, int64_t x0,
                             int64_t y0, int w) {
    const int lane = threadIdx.x & 63;
    const int64_t i = x0 + lane;
    const bool col_ok = i < W;
    const int64_t ic = col_ok ? i : W - 1;
    const int64_t iw = ic > 0 ? ic - 1 : 0, ie = ic + 1 < W ? ic + 1 : W - 1;
    double c[kRowsPerBuilder], nn[kRowsPerBuilder], ss[kRowsPerBuilder], ww[kRowsPerBuilder], ee[kRowsPerBuilder];
#pragma unroll
    for (int k = 0; k < kRowsPerBuilder; ++k) {
        const int r = w + k * kBuilders;
        int64_t j = y0 + r;
        j = (r < kPW && j < H) ? j : H - 1;
        const int64_t jn = j > 0 ? j - 1 : 0, js = j + 1 < H ? j + 1 : H - 1;
        c[k] = (double)T[j * W + ic];
        nn[k] = (double)T[jn * W + ic];
        ss[k] = (double)T[js * W + ic];
        ww[k] = (double)T[j * W + iw];
        ee[k] = (double)T[j * W + ie];
    }
#pragma unroll
    for (int k = 0; k < kRowsPerBuilder; ++k) {
        const int r = w + k * kBuilders;
        const int64_t j = y0 + r;
        if (r >= kPW || j >= H || !col_ok) continue;
        double gy, gx;  // FastMarching.py:262-294 with the five loaded values
        if (j == 0)
            gy = ss[k] - c[k];
        else if (j == H - 1)
            gy = c[k] - nn[k];
        else if (__builtin_isinf(ss[k]))
            gy = __builtin_isinf(nn[k]) ? 0.0 : c[k] - nn[k];
        else
            gy = __builtin_isinf(nn[k]) ? ss[k] - c[k] : (ss[k] - nn[k]) / 2;
        if (i == 0)
            gx = ee[k] - c[k];
        else if (i == W - 1)
            gx = c[k] - ww[k];
        else if (__builtin_isinf(ee[k]))
            gx = __builtin_isinf(ww[k]) ? 0.0 : c[k] - ww[k];
        else
            gx = __builtin_isinf(ww[k]) ? ee[k] - c[k] : (ee[k] - ww[k]) / 2;
        const double den = __builtin_sqrt(gx * gx + gy * gy);  // :296-297
        if constexpr (BLOCK) {
            const double nan = __builtin_nan("");
            const bool blocked = __builtin_isinf(c[k]);
            s.g[b][r][lane] = make_double2(blocked ? nan : gx / den, blocked ? nan : gy / den);
        } else {
            s.g[b][r][lane] = make_double2(gx / den, gy / den);
        }
    }
}

// A builder wave's life, the 2D and the 3D walkers' (LDS = PathLds or gdm.hip's Path3Lds): poll
// req_seq, run build(w) -- w the builder's index, wave - 1 -- for each new request, publish it in
// `done`; leave on the walker's quit (-1), or when no request came for kPathSpin.
template <typename LDS, typename F>
__device__ __forceinline__ void builder_loop(LDS& s, F&& build) {
    const int w = (int)(threadIdx.x >> 6) - 1;
    int seen = 0;
    unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        const int q = __hip_atomic_load(&s.req_seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q < 0) return;
        if (q == seen) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > kPathSpin) return;  // walker gone: give up
            __builtin_amdgcn_s_sleep(1);
            continue;
        }
        seen = q;
        build(w);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&s.done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        t0 = __builtin_amdgcn_s_memrealtime();
    }
}

template <typename R, bool BLOCK = false>
__device__ void path_builder(PathLds& s, const R* __restrict__ T, int64_t H, int64_t W) {
    builder_loop(s, [&](int w) { build_window<R, BLOCK>(s, T, H, W, s.req_b, s.req_x0, s.req_y0, w); });
}

// The walker's window state, the 2D counterpart of gdm.hip's Win3: which buffer holds which
// window, the request in flight and the fast bounds of the step.
struct Walk2Win {
    PathLds& s;
    const int64_t H, W;
    // window origins of the two buffers (scalars, not an indexed array: no private->LDS promotion)
    int64_t wx0 = -((int64_t)1 << 40), wx1 = wx0, wy0 = wx0, wy1 = wx0;
    int cur = 0, seq = 0;
    bool pending = false;
    const int64_t xmax, ymax;
    // Fast path: while lo_x <= i <= hi_x and lo_y <= j <= hi_y nothing has to happen this step
    // (the corners lie in the current window and, unless a build is pending, not within
    // kPrefetch of an inner edge) -- four int32 compares on the step's dependency chain instead
    // of the window bookkeeping, which runs only when the bounds are crossed.
    int lo_x = 1, hi_x = 0, lo_y = 1, hi_y = 0;  // empty: the first step takes the slow path
    int cx0i = 0, cy0i = 0;                     // current window origin
    __device__ __forceinline__ Walk2Win(PathLds& lds, int64_t h, int64_t w)
        : s(lds), H(h), W(w), xmax(w > kPW ? w - kPW : 0), ymax(h > kPW ? h - kPW : 0) {}
    __device__ __forceinline__ void issue(int b, int64_t i, int64_t j) {  // build the window centred on (i, j) into b
        int64_t x0 = i - kPW / 2, y0 = j - kPW / 2;
        x0 = x0 > xmax ? xmax : x0 < 0 ? 0 : x0;
        y0 = y0 > ymax ? ymax : y0 < 0 ? 0 : y0;
        if (b) { wx1 = x0; wy1 = y0; } else { wx0 = x0; wy0 = y0; }
        s.req_x0 = x0;
        s.req_y0 = y0;
        s.req_b = b;
        __hip_atomic_store(&s.req_seq, ++seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ bool wait_built() {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(&s.done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < seq * kBuilders) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > kPathSpin) return false;
            __builtin_amdgcn_s_sleep(1);
        }
        return true;
    }
    __device__ __forceinline__ bool inside(int b, int64_t i, int64_t j) const {
        const int64_t x0 = b ? wx1 : wx0, y0 = b ? wy1 : wy0;
        return i >= x0 && j >= y0 && i + 1 < x0 + kPW && j + 1 < y0 + kPW;
    }
    __device__ __forceinline__ void set_bounds() {
        const int64_t x0 = cur ? wx1 : wx0, y0 = cur ? wy1 : wy0;
        cx0i = (int)x0;
        cy0i = (int)y0;
        lo_x = cx0i + (!pending && x0 > 0 ? kPrefetch : 0);
        hi_x = cx0i + kPW - 2 - (!pending && x0 < xmax ? kPrefetch : 0);
        lo_y = cy0i + (!pending && y0 > 0 ? kPrefetch : 0);
        hi_y = cy0i + kPW - 2 - (!pending && y0 < ymax ? kPrefetch : 0);
        hi_x = hi_x < (int)W - 2 ? hi_x : (int)W - 2;  // inside the bounds implies i + 1 < W, j + 1 < H
        hi_y = hi_y < (int)H - 2 ? hi_y : (int)H - 2;
    }
    // The cell (i, j) of a point in the raster (i + 1 < W, j + 1 < H) left the fast bounds: switch
    // to the window that holds its corners (waiting only if the build is still running, or the
    // walk turned away from the prefetched window), prefetch when it is within kPrefetch of an
    // inner edge, set the bounds anew.  false: a build never finished.
    __device__ __forceinline__ bool cross(int64_t i, int64_t j) {
        if (!inside(cur, i, j)) {  // the 2 x 2 interpolation corners left the window
            const int nb = seq == 0 ? 0 : 1 - cur;
            bool have = false;
            if (pending) {
                pending = false;
                if (!wait_built()) return false;
                have = inside(nb, i, j);
            }
            if (!have) {
                issue(nb, i, j);
                if (!wait_built()) return false;
            }
            cur = nb;
        }
        const int64_t cx0 = cur ? wx1 : wx0, cy0 = cur ? wy1 : wy0;
        if (!pending && ((i - cx0 < kPrefetch && cx0 > 0) || (cx0 + kPW - 2 - i < kPrefetch && cx0 < xmax) ||
                         (j - cy0 < kPrefetch && cy0 > 0) || (cy0 + kPW - 2 - j < kPrefetch && cy0 < ymax))) {
            issue(1 - cur, i, j);
            pending = true;
        }
        set_bounds();
        return true;
    }
};

// One path's walk by one workgroup.  ONE kernel template for the single-path launch (A = Gdm2dArgs,
// one workgroup) and the grid form (A = GdmBatchArgs: workgroup p takes descriptor p -- its map,
// init, end --, walks its own map T + map * H * W and writes its own slab out + p * cap * 2, n_out[p],
// status[p]): path_args turns either into the walk's Gdm2dArgs and everything below is shared, so
// a batch walk is the single walk's arithmetic by construction.  Nothing below reads blockIdx or
// a global word other than its own `a`'s: workgroups are independent.  The 128 KiB of windows take a
// whole CU's LDS, so one workgroup runs per CU and those past the co-resident ones start as CUs
// free up.
template <typename R>
__device__ __forceinline__ Gdm2dArgs path_args(const Gdm2dArgs& a) { return a; }
template <typename R>
__device__ __forceinline__ Gdm2dArgs path_args(const GdmBatchArgs& b) {
    const int64_t p = blockIdx.x;
    const GdmDesc* __restrict__ d = b.desc + p;
    Gdm2dArgs a;
    a.T = static_cast<const R*>(b.T) + (int64_t)d->map * b.H * b.W;
    a.H = b.H;
    a.W = b.W;
    a.ix = d->init[0];
    a.iy = d->init[1];
    a.ex = d->end[0];
    a.ey = d->end[1];
    a.tau = b.tau;
    a.steps = b.steps;
    a.out = b.out + p * b.cap * 2;
    a.cap = b.cap;
    a.n_out = b.n_out + p;
    a.status = b.status + p;
    a.fused = b.fused;
    return a;
}

}  // namespace eik
