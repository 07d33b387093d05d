// gdm.hip -- gradient-descent path extraction (getPathGDM, FastMarching.py:164-236) and the
// inf-aware normalised gradient (computeGradient, FastMarching.py:242-300) on gfx950.
//
// The path is inherently sequential (<= round(15000/tau) dependent steps), so it runs as ONE
// small kernel: a single wave whose lane 0 walks the field.  Per step the reference builds the
// normalised gradient in a 6x6 window (allocating four full-size arrays, :255-258) but only ever
// reads it at the four bilinear corners; the kernel evaluates the gradient at exactly those
// four corners (bit-identical control flow, see oracle/eikonal_oracle.c grad_at/orc_gdm2d).
//
// Arithmetic is IEEE fp64 with contraction disabled.  The one deliberate difference: the
// reference squares numpy scalars with `x**2`, which goes through glibc pow() and is not
// always correctly rounded; the device uses the exact product x*x (<= 1 ulp per square,
// tolerance stated in tests/test_gpu_path.py).
#include "eik_common.hpp"
#include "eik_kernels.hpp"

#pragma clang fp contract(off)

// the helpers, the step's arithmetic (walk_step_*, its range-free square root / division), the window
// machinery (LDS windows, the builder waves' loop, the walker's window state Walk2Win): the one copy
// this walker and the obstacle-safe one (gdm_safe.hip) both run
#include "gdm_walk.hpp"

namespace eik {

#ifndef EIK_P3PROBE
#define EIK_P3PROBE(k) ((void)0)  // 3D walker phase timing hooks (tools/path3_prof.hip)
#define EIK_P3DECL ((void)0)
#define EIK_P3FLUSH ((void)0)
#endif
#ifndef EIK_P3RUN
#define EIK_P3RUN 1  // the 3D walker's integer-descent run loop (gdm3d_kernel)
#endif
#ifndef EIK_P2PROBE
#define EIK_P2PROBE(k) ((void)0)  // 2D walker phase timing hooks (tools/path2_prof.hip)
#define EIK_P2DECL ((void)0)
#define EIK_P2FLUSH ((void)0)
#endif


// (uint32_t)trunc(x) as ONE defined conversion: the hardware truncates and CLAMPS to the type's range
// (x <= -1, NaN and -inf -> 0; x >= 2^32 and +inf -> 2^32 - 1), where a C++ cast of such a value is
// undefined.  The result is the reference's np.uint32(np.fix(p)) only for p in (-1, 2^31); both
// walkers decide every other coordinate themselves.
__device__ __forceinline__ uint32_t cvt_u32(double x) {
    uint32_t r;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
// the 2D walker's: every lane holds the same point, so the cell index is wave-uniform -- read into a
// scalar register, the branches on it stay scalar branches
__device__ __forceinline__ uint32_t cell_u32(double x) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)cvt_u32(x));
}

template <typename R, int LOOP, typename A = Gdm2dArgs>
__global__ __launch_bounds__(kPathThreads) void gdm2d_kernel(A arg) {
    const Gdm2dArgs a = path_args<R>(arg);
    __shared__ PathLds s;
    const R* __restrict__ T = static_cast<const R*>(a.T);
    const int64_t H = a.H, W = a.W;
    if (threadIdx.x == 0) {
        s.req_seq = 0;
        s.done = 0;
    }
    __syncthreads();
    if (threadIdx.x >= 64) {
        path_builder<R>(s, T, H, W);
        return;
    }
    // ---- walker (wave 0; every lane runs the same uniform loop, lane 0 stores)
    EIK_P2DECL;
    const bool lead = threadIdx.x == 0;
    double* out = a.out;
    int status = kGdmDone;
    double px = a.ix, py = a.iy;  // gamma[-1], kept in registers
    if (lead) {
        out[0] = px;
        out[1] = py;
    }
    int64_t n = 1;
    const double tau = a.tau;
    Walk2Win win(s, H, W);
    // Window bookkeeping of a step whose cell (i, j) = cell_u32 of (px, py) left the fast bounds -- and
    // the coordinate-to-index rule of DESIGN 3.4b, which every point outside the fast bounds passes
    // here before anything is indexed with (i, j): the clamped conversions are the reference's
    // np.uint32(np.fix(p)) only for p in (-1, 2^31).  A NaN or infinite coordinate raises at
    // computeGradient's int(point) (:250), p <= -1 (numpy: index 2^32 - |fix(p)|), W - 1 <= p and
    // p >= 2^31 (not wrapped modulo 2^32) are the IndexError of :323: status ERROR, false.  The
    // range test is in 64 bits (i + 1 of i = 2^32 - 1 does not wrap).  A point in (-1, 0) has cell 0
    // and a negative fraction and walks on.  false as well when a build never finished; else the
    // corners are in window `win.cur` afterwards.
    auto slow_step = [&](uint32_t i, uint32_t j) -> bool {
        if (!(__builtin_isfinite(px) && __builtin_isfinite(py))) { status = kGdmError; return false; }
        if (px <= -1.0 || py <= -1.0 || ((i | j) >> 31) != 0u || (int64_t)i + 1 >= W || (int64_t)j + 1 >= H) {
            status = kGdmError;
            return false;
        }
        if (!win.cross((int64_t)i, (int64_t)j)) { status = kGdmError; return false; }
        return true;
    };
    // forms 0-3: the fast bounds as integer tests on the conversions' results.  Cell 0 of either
    // axis is never inside them -- p <= -1, NaN and -inf convert to 0 as a point of cell 0 does --
    // and +inf and p >= 2^31 convert to a negative int: all of them take slow_step.
    auto fast_cell = [&](uint32_t i, uint32_t j) -> bool {
        const int lx = win.lo_x > 1 ? win.lo_x : 1, ly = win.lo_y > 1 ? win.lo_y : 1;
        return (int)i >= lx && (int)i <= win.hi_x && (int)j >= ly && (int)j <= win.hi_y;
    };
    // NaN fallback (:178-218) as the reference behaves under numpy 2: the neighbour probe
    // `np.uint32(nearN + [0,-1])` raises OverflowError, caught at :217.  Lane 0 edits the path.
    auto nan_fallback = [&]() {
        if (lead) {
            int64_t nx = (int64_t)__builtin_rint(px), ny = (int64_t)__builtin_rint(py);
            bool empty = false, oob = false;
            for (;;) {
                const int64_t qx = nx < 0 ? nx + W : nx, qy = ny < 0 ? ny + H : ny;
                if (qx < 0 || qy < 0 || qx >= W || qy >= H) { oob = true; break; }
                if (!__builtin_isinf(tv(T, W, qy, qx))) break;
                --n;
                if (n == 0) { empty = true; break; }
                nx = (int64_t)__builtin_rint(out[2 * (n - 1)]);
                ny = (int64_t)__builtin_rint(out[2 * (n - 1) + 1]);
            }
            if (!empty && !oob) {
                while (n > 0 && norm2(out[2 * (n - 1)] - (double)nx, out[2 * (n - 1) + 1] - (double)ny) < 1) --n;
                if (n < a.cap) {
                    out[2 * n] = (double)nx;
                    out[2 * n + 1] = (double)ny;
                    ++n;
                }
            }
        }
        status = kGdmFallback;
    };
    // the point budget folded into the step count: point n = k + 1 is stored at step k (:173)
    const long kmax = a.steps < a.cap - 1 ? a.steps : a.cap - 1;
    long k = 0;
    if constexpr (LOOP >= 1) {
        // One exit per step: the step is computed before its special cases are known (window
        // bookkeeping due, NaN gradient, stop radius, point budget), and a single uniform branch
        // leaves the tight loop when any of them holds; the handler below then takes the same
        // decisions as the reference-structured loop (the `else` branch) for that step.  The
        // many uniform branches of that loop, each behind a VALU compare, cost more per step than
        // the arithmetic they skip.  The LDS address of a step whose cell is outside the fast
        // bounds is clamped into the window buffers (its values are discarded).
        constexpr unsigned kWinBytes = sizeof(s.g[0]);
        // LOOP 4, the lane-pair form: even lanes carry the x component of every per-component
        // quantity (coordinate, fraction, interpolated gradient, quotient), odd lanes the y one,
        // so each f64 instruction of the step does the work of both components; the few sums and
        // hand-overs across the pair are DPP moves (pair_swap).  Every lane computes the same
        // operations on the same operands as form 3 does for its component -- sums of the two
        // components (dx dx + dy dy, ex ex + ey ey) are commutative, so both lanes of a pair hold
        // the same bits -- and the exit conditions are wave-uniform votes.
        const bool yl = (threadIdx.x & 1) != 0;
        const double dmax = __builtin_fabs(tau) * 1.4142135623730951 * (1.0 + 0x1p-20) + 0x1p-20;
        double* const outl = out + (threadIdx.x & 1);
        for (; k < kmax;) {
            uint32_t i, j;
            bool in, odd = false;
            WalkStep o;
            double fa, fb;
            if constexpr (LOOP == 4) {
                double p = yl ? py : px, d = 0.0, pn = 0.0;
                // this lane's fast bounds (x or y) as a half-open f64 range: lo <= p < hi + 1 (NaN
                // fails it; p in (-1, 0) goes to the handler, which is exact anyway)
                const double loc = yl ? win.lo_y : win.lo_x, hic = (yl ? win.hi_y : win.hi_x) + 1;
                // Steps this loop may take without the stop test: none of them can come within 1.5
                // of the goal (:231) -- a step moves each coordinate by at most |tau| (|dxn|, |dyn|
                // <= 1), so k steps move at most k |tau| sqrt(2) (with slack for rounding) -- and
                // within the point budget.  The step after them leaves to the handler, which tests.
                const double ex0 = px - a.ex, ey0 = py - a.ey;
                const double room = (__builtin_sqrt(ex0 * ex0 + ey0 * ey0) * (1.0 - 0x1p-30) - 1.5) / dmax;
                long kl = kmax - 1 - k;
                const long safe = room >= 1.0 ? (room < 2e9 ? (long)room : 2000000000L) : 0L;  // NaN: 0
                kl = kl < safe ? kl : safe;
                const int left = (int)kl;
                // the corners' LDS address in vector registers: each lane scales its own cell
                // index (x: 16 B per column, y: kPW x 16 B per row) and adds its partner's (DPP)
                const unsigned sc = yl ? kPW * (unsigned)sizeof(double2) : (unsigned)sizeof(double2);
                const unsigned c0 = (unsigned)(yl ? win.cy0i : win.cx0i) * sc;
                const char* const base = reinterpret_cast<const char*>(s.g[win.cur]) + (yl ? sizeof(double) : 0);
                int kk = 0;
                // One conditional branch per step: the state is advanced before the exit test and the
                // exit undoes the advance.  Each pass stores the point it starts from, row n - 1 (the
                // first pass rewrites the row with the bits it holds): the point of a step that
                // leaves -- computed from corners outside the window, or of a step that ends in an
                // error or the NaN fallback -- is never stored, so nothing is written past the
                // rows returned.
                double pp = p;
                bool leave;
                do {
                    outl[2 * (n - 1)] = p;  // every lane: its component's address
                    // (one v_cvt_u32_f64 on p, the corner as (double)u beside it: no difference,
                    // profiles/r05k_walker_ab.log P4_CVT=1)
                    const double t = __builtin_trunc(p);
                    const uint32_t u = (uint32_t)t;
                    in = __builtin_amdgcn_ballot_w64(!(p >= loc && p < hic)) == 0ull;
                    const unsigned own = u * sc - c0;
                    unsigned off = own + (unsigned)__builtin_amdgcn_mov_dpp((int)own, 0xB1, 0xf, 0xf, false);
                    off = off < kWinBytes - (kPW + 2) * (unsigned)sizeof(double2) ? off : kWinBytes - (kPW + 2) * (unsigned)sizeof(double2);
                    const char* gq = base + off;
                    const double g00 = *reinterpret_cast<const double*>(gq);
                    const double g01 = *reinterpret_cast<const double*>(gq + sizeof(double2));
                    const double g10 = *reinterpret_cast<const double*>(gq + kPW * sizeof(double2));
                    const double g11 = *reinterpret_cast<const double*>(gq + (kPW + 1) * sizeof(double2));
                    const double f = p - t;  // fa (even) / fb (odd); in bounds t = i or j
                    fa = quad_perm_f64<0xA0>(f);
                    fb = quad_perm_f64<0xF5>(f);
                    d = interp2_general(fa, fb, g00, g01, g10, g11);  // dx (even) / dy (odd)
                    const double sq = d * d;
                    const double s1 = sq + pair_swap(sq);            // dx dx + dy dy in both lanes
                    double h1, h2;
                    const double nrm = sqrt_c1_h(s1, h1);
                    const double q1 = div_rs(d, nrm, h1);            // dxn (even) / dy / nrm (odd)
                    const double dxn = pair_swap(q1);                // odd lanes: dxn
                    const double r2 = sqrt_c1_h(dxn * dxn + sq, h2);
                    const double q2 = div_rs(d, r2, h2);             // odd lanes: dy / r2
                    const double dn = (yl && !(nrm < 0.01)) ? q2 : q1;
                    pn = p - tau * dn;                               // sx (even) / sy (odd)
                    // (a NaN d makes s1 NaN: odd)
                    const bool oddl = !(s1 >= 0x1p-767 && s1 <= 0x1p200) | ((d != 0.0) & (__builtin_fabs(d) < 0x1p-900));
                    const bool bad = __builtin_amdgcn_ballot_w64(oddl) != 0ull;
                    leave = (int)!in | (int)bad | (int)(kk >= left);
                    ++n;
                    pp = p;
                    p = pn;
                    ++kk;
                } while (!leave);
                --n;  // the exit step is the handler's
                --kk;
                p = pp;
                k += kk;
                // the scalar state of the exit step for the handler below: lanes 0 (x) and 1 (y)
                // read into scalar registers, so the handler stays wave-uniform code
                px = readlane_f64(p, 0);
                py = readlane_f64(p, 1);
                i = cell_u32(px);  // (the handler uses them after `in` or slow_step vouched for them)
                j = cell_u32(py);
                o.dx = readlane_f64(d, 0);
                o.dy = readlane_f64(d, 1);
                o.sx = readlane_f64(pn, 0);
                o.sy = readlane_f64(pn, 1);
                odd = walk_odd(o.dx, o.dy, o.dx * o.dx + o.dy * o.dy);  // the loop's test, on lanes 0 / 1
                fa = px - i;
                fb = py - j;
            } else
            for (;;) {
                EIK_P2PROBE(0);
                i = cell_u32(px);
                j = cell_u32(py);
                in = fast_cell(i, j);
                unsigned off = (unsigned)(((int)j - win.cy0i) * kPW + ((int)i - win.cx0i)) * (unsigned)sizeof(double2);
                off = off <= kWinBytes - (kPW + 2) * sizeof(double2) ? off : 0u;  // unsigned: negatives too
                const double2* g = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(s.g[win.cur]) + off);
                EIK_P2PROBE(1);
                fa = px - i;
                fb = py - j;
                if constexpr (LOOP == 3)
                    o = walk_step_rs(g[0], g[1], g[kPW], g[kPW + 1], fa, fb, px, py, tau, odd);
                else if constexpr (LOOP == 2)
                    o = walk_step_core(g[0], g[1], g[kPW], g[kPW + 1], fa, fb, px, py, tau, odd);
                else
                    o = walk_step_exact(g[0], g[1], g[kPW], g[kPW + 1], fa, fb, px, py, tau);
                EIK_P2PROBE(2);
                const double ex = o.sx - a.ex, ey = o.sy - a.ey;
                const bool stop = ex * ex + ey * ey < 2.25;  // :231-232, as in the loop below
                EIK_P2PROBE(3);
                // one branch: the conditions combined bitwise (a || chain becomes one branch each)
                const bool leave = (int)!in | (int)odd | (int)__builtin_isnan(o.dx + o.dy) | (int)stop |
                                   (int)(k + 1 >= kmax);
                if (leave) break;
                *reinterpret_cast<double2*>(out + 2 * n) = make_double2(o.sx, o.sy);
                ++n;
                px = o.sx;
                py = o.sy;
                ++k;
            }
            if (!in || odd) {  // window bookkeeping (or an error), then this step again -- exactly
                if (!in && !slow_step(i, j)) break;
                const int li = (int)i - win.cx0i, lj = (int)j - win.cy0i;
                const auto& g = s.g[win.cur];
                o = walk_step_exact(g[lj][li], g[lj][li + 1], g[lj + 1][li], g[lj + 1][li + 1], fa, fb, px, py, tau);
            }
            // the reference-structured loop's end of step
            const double ex = o.sx - a.ex, ey = o.sy - a.ey;
            const bool stop = ex * ex + ey * ey < 2.25;
            if (__builtin_isnan(o.dx) || __builtin_isnan(o.dy)) {
                nan_fallback();
                break;
            }
            *reinterpret_cast<double2*>(out + 2 * n) = make_double2(o.sx, o.sy);
            ++n;
            px = o.sx;
            py = o.sy;
            if (stop) break;  // k counts completed non-final steps, as the for loop's ++k
            if (++k >= kmax) break;
        }
    } else {
        for (; k < kmax; ++k) {
            EIK_P2PROBE(0);
            const uint32_t i = cell_u32(px), j = cell_u32(py);
            // one test on the chain: a coordinate the conversion clamped, out of range, cell 0, or
            // window bookkeeping due
            if (!fast_cell(i, j)) {
                if (!slow_step(i, j)) break;
            }
            EIK_P2PROBE(1);
            const int li = (int)i - win.cx0i, lj = (int)j - win.cy0i;
            const double fa = px - i, fb = py - j;
            const auto& g = s.g[win.cur];
            const WalkStep o = walk_step_exact(g[lj][li], g[lj][li + 1], g[lj + 1][li], g[lj + 1][li + 1], fa, fb, px, py, tau);
            EIK_P2PROBE(2);
            // :231-232  sqrt(e) < 1.5  <=>  e < 2.25 for a correctly rounded sqrt (2.25 = 1.5^2 exactly)
            const double ex = o.sx - a.ex, ey = o.sy - a.ey;
            const bool stop = ex * ex + ey * ey < 2.25;
            EIK_P2PROBE(3);
            // one test after the step: a NaN gradient (the fallback: nothing of this step is kept)
            // or the stop radius; NaN in dx + dy also catches inf - inf, re-tested precisely
            if (__builtin_isnan(o.dx + o.dy) || stop) {
                if (__builtin_isnan(o.dx) || __builtin_isnan(o.dy)) {
                    nan_fallback();
                    break;
                }
            }
            *reinterpret_cast<double2*>(out + 2 * n) = make_double2(o.sx, o.sy);  // every lane: same address and value
            ++n;
            px = o.sx;
            py = o.sy;
            if (stop) break;
        }
    }
    // Out of point budget: the loop ended (step count, point budget or stop radius) with no row left
    // for `end` -- n = cap, also when the stop radius was reached by the step that wrote row cap - 1.
    if (status == kGdmDone && n >= a.cap) status = kGdmError;
    __hip_atomic_store(&s.req_seq, -1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);  // builders exit
    EIK_P2FLUSH;
    if (lead) {
        if (status == kGdmDone && n < a.cap) {  // :234
            out[2 * n] = a.ex;
            out[2 * n + 1] = a.ey;
            ++n;
        }
        *a.n_out = n;
        *a.status = status;
    }
}

// Self-test of the 2D walker's fast-path arithmetic against the exact forms it stands in for,
// on n pseudo-random inputs per function drawn from the walker's fast-path domain (walk_odd
// false): sqrt_core(x) vs sqrt(x) for x in [2^-767, 2^1000]; div_core(n, d) vs n / d for d in
// [2^-900, 2^100], |n| <= d, n = 0 or |n| >= 2^-900 (a zero quotient may differ in sign only);
// interp2_general vs interp2_sel for corners in [-1, 1] and fractions in [0, 1) that are exactly
// 0 a quarter of the time; div_rs(n, sqrt_core_h(x, h), h) vs n / sqrt(x) for x in [2^-767, 2^200],
// |n| <= sqrt(x), n = 0 or |n| >= 2^-900.  counts[0..2]: mismatches of the first three;
// counts[3]: samples evaluated; counts[4]: mismatches of div_rs; counts[5]: sqrt_c1_h(x) vs sqrt(x)
// on the same x.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {  // splitmix64
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double dbl_exp(unsigned long long r, int e_lo, int e_hi) {  // 2^e * (1 + m)
    const int e = e_lo + (int)((r >> 52) % (unsigned long long)(e_hi - e_lo + 1));
    return __longlong_as_double((long long)(((unsigned long long)(e + 1023) << 52) | (r & 0xfffffffffffffull)));
}
__device__ __forceinline__ double unit_f(unsigned long long r) { return (double)(r >> 11) * 0x1p-53; }  // [0, 1)
__global__ void walker_math_selftest_kernel(long long n, unsigned long long seed, unsigned long long* counts) {
    unsigned long long bad[5] = {0, 0, 0, 0, 0}, done = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        ++done;
        const unsigned long long r0 = mix64(seed ^ (4 * t)), r1 = mix64(seed ^ (4 * t + 1)), r2 = mix64(seed ^ (4 * t + 2)),
                                 r3 = mix64(seed ^ (4 * t + 3));
        const double x = t == 0 ? 0x1p-767 : dbl_exp(r0, -767, 999);
        if (__double_as_longlong(sqrt_core(x)) != __double_as_longlong(__builtin_sqrt(x))) ++bad[0];
        const double d = dbl_exp(r1, -900, 99);
        double q = d * (2.0 * unit_f(r2) - 1.0);
        if (__builtin_fabs(q) < 0x1p-900 || (r2 & 15) == 0) q = (r2 & 16) ? -0.0 : 0.0;
        const double e1 = div_core(q, d), e0 = q / d;
        if (e0 == 0.0 ? e1 != 0.0 : __double_as_longlong(e1) != __double_as_longlong(e0)) ++bad[1];
        const double fa = (r3 & 3) == 0 ? 0.0 : unit_f(mix64(r3)), fb = (r3 & 12) == 0 ? 0.0 : unit_f(mix64(r3 + 1));
        double g[4];
        for (int c = 0; c < 4; ++c) g[c] = 2.0 * unit_f(mix64(r3 + 2 + c)) - 1.0;
        const double i1 = interp2_general(fa, fb, g[0], g[1], g[2], g[3]), i0 = interp2_sel(fa, fb, g[0], g[1], g[2], g[3]);
        if (i0 == 0.0 ? i1 != 0.0 : __double_as_longlong(i1) != __double_as_longlong(i0)) ++bad[2];
        const unsigned long long r4 = mix64(seed ^ ~(4 * t)), r5 = mix64(r4);
        const double xs = dbl_exp(r4, -767, 199);
        double hs;
        const double ds = sqrt_core_h(xs, hs);
        double ns = ds * (2.0 * unit_f(r5) - 1.0);
        if (__builtin_fabs(ns) < 0x1p-900 || (r5 & 15) == 0) ns = (r5 & 16) ? -0.0 : 0.0;
        if ((r5 & 0x300) == 0) ns = (r5 & 32) ? -ds : ds;  // |n| = d exactly (a unit component)
        const double f1 = div_rs(ns, ds, hs), f0 = ns / __builtin_sqrt(xs);
        if (f0 == 0.0 ? f1 != 0.0 : __double_as_longlong(f1) != __double_as_longlong(f0)) ++bad[3];
        double hc;
        if (__double_as_longlong(sqrt_c1_h(xs, hc)) != __double_as_longlong(__builtin_sqrt(xs))) ++bad[4];
    }
    for (int k = 0; k < 3; ++k)
        if (bad[k]) atomicAdd(&counts[k], bad[k]);
    if (bad[3]) atomicAdd(&counts[4], bad[3]);
    if (bad[4]) atomicAdd(&counts[5], bad[4]);
    if (done) atomicAdd(&counts[3], done);
}
hipError_t walker_math_selftest(long long n, unsigned long long seed, unsigned long long* d_counts, hipStream_t st) {
    hipLaunchKernelGGL(walker_math_selftest_kernel, dim3(1024), dim3(256), 0, st, n, seed, d_counts);
    return hipGetLastError();
}

// The runtime (f64, fused) as gdm2d_kernel<R, LOOP, A>, A = Gdm2dArgs or GdmBatchArgs; a `fused`
// outside 1..4 is form 0.
template <typename R, typename A>
static void gdm2d_launch_form(const A& a, dim3 g, hipStream_t st) {
    const dim3 b(kPathThreads);
    switch (a.fused) {
    case 4: hipLaunchKernelGGL((gdm2d_kernel<R, 4, A>), g, b, 0, st, a); break;
    case 3: hipLaunchKernelGGL((gdm2d_kernel<R, 3, A>), g, b, 0, st, a); break;
    case 2: hipLaunchKernelGGL((gdm2d_kernel<R, 2, A>), g, b, 0, st, a); break;
    case 1: hipLaunchKernelGGL((gdm2d_kernel<R, 1, A>), g, b, 0, st, a); break;
    default: hipLaunchKernelGGL((gdm2d_kernel<R, 0, A>), g, b, 0, st, a); break;
    }
}
template <typename A>
static hipError_t gdm2d_launch(const A& a, unsigned blocks, bool f64, hipStream_t st) {
    if (f64)
        gdm2d_launch_form<double>(a, dim3(blocks), st);
    else
        gdm2d_launch_form<float>(a, dim3(blocks), st);
    return hipGetLastError();
}

hipError_t gdm2d(const Gdm2dArgs& a, bool f64, hipStream_t st) { return gdm2d_launch(a, 1u, f64, st); }

hipError_t gdm2d_batch(const GdmBatchArgs& a, bool f64, hipStream_t st) {
    return gdm2d_launch(a, (unsigned)a.P, f64, st);
}

// ---------------------------------------------------------------- 3D path (FM3D)
// np.gradient(T) along `axis` (0 y, 1 x, 2 z) at (j, i, k): central differences / 2 inside,
// one-sided at the ends (numpy's edge_order=1), no inf awareness (FastMarching3D.py:200).
// The 3D walk is one wave (wave 0) with every lane running the same scalar step (LDS reads are
// broadcasts, so no lane divergence).  T is read from an LDS window [WY][WX][WZ] (z fastest, the
// volume's own order), double-buffered: waves 1..7 build windows, as the 2D kernel's builders do.
// When the step's 4x4x4 cube (trilinear corners +-1 for np.gradient) comes within kPre3 cells of
// an inner window edge, the walker requests the window centred on itself into the idle buffer and
// keeps walking; it waits only if the cube leaves the current window before that build is done
// (or the prefetched window does not hold it).  The integer-descent fallback reads outside the
// window from global memory.  The last kRing path points are mirrored in LDS, so the
// back-tracking of :231-249 does not wait on its own global stores.  The arithmetic, its order
// and every branch are FastMarching3D.py's (bit-identical to the oracle's restatement).
constexpr int kWin3Bytes = 48 * 1024;  // per buffer
constexpr int kRing = 256;
constexpr int kP3Threads = 512;        // walker + 7 builder waves
constexpr int kB3 = kP3Threads / 64 - 1;
constexpr int kPre3 = 14;              // cells from an inner window edge that trigger a prefetch

struct Path3Lds {
    __attribute__((aligned(16))) char wbuf[2][kWin3Bytes];
    double ring[kRing][3];
    double gsh[3][8], nsh[7];  // per-step lane exchange of the walker
    int nbad[7];
    long long req_y0, req_x0, req_z0;
    int req_seq;  // walker -> builders: request number (-1: quit)
    int req_b;    // target buffer
    int done;     // builders -> walker: finished builds x kB3
};

// window dimensions (walker and builders compute the same)
template <typename R>
__device__ __forceinline__ void win3_dims(int64_t H, int64_t W, int64_t L, int& WY, int& WX, int& WZ) {
    constexpr int cells = kWin3Bytes / (int)sizeof(R);
    WZ = (int)(L < 16 ? L : 16);
    int s = 1;
    while ((s + 1) * (s + 1) * WZ <= cells && s < 128) ++s;
    WY = (int)(H < s ? H : s);
    WX = (int)(W < s ? W : s);
}

// Builder wave w (0..kB3-1): cells w * 64 + lane + k * 64 kB3 of the window at (y0, x0, z0) into
// buffer b -- (yy, xx, zz) advanced by carries, 32 loads in flight per lane before their stores.
template <typename R>
__device__ void build3(Path3Lds& s, const R* __restrict__ T, int64_t H, int64_t W, int64_t L, int b, int64_t y0,
                       int64_t x0, int64_t z0, int w) {
    int WY, WX, WZ;
    win3_dims<R>(H, W, L, WY, WX, WZ);
    R* const wl = reinterpret_cast<R*>(s.wbuf[b]);
    const int lane = threadIdx.x & 63;
    const int nc = WY * WX * WZ;
    constexpr int S = 64 * kB3;
    const int sz = S % WZ, sx = (S / WZ) % WX, sy = (S / WZ) / WX;
    const int c00 = w * 64 + lane;
    int zz = c00 % WZ, xx = (c00 / WZ) % WX, yy = (c00 / WZ) / WX;
    constexpr int kB = 32;
    for (int c0 = c00; c0 < nc; c0 += S * kB) {
        R val[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            if (c0 + S * u < nc) val[u] = T[((y0 + yy) * W + x0 + xx) * L + z0 + zz];
            zz += sz;
            if (zz >= WZ) { zz -= WZ; ++xx; }
            xx += sx;
            if (xx >= WX) { xx -= WX; ++yy; }
            yy += sy;
        }
#pragma unroll
        for (int u = 0; u < kB; ++u)
            if (c0 + S * u < nc) wl[c0 + S * u] = val[u];
    }
}

template <typename R>
__device__ __forceinline__ void path3_builder(Path3Lds& s, const R* __restrict__ T, int64_t H, int64_t W, int64_t L) {
    builder_loop(s, [&](int w) { build3<R>(s, T, H, W, L, s.req_b, s.req_y0, s.req_x0, s.req_z0, w); });
}

template <typename R>
struct Win3 {
    const R* __restrict__ T;
    int64_t H, W, L;
    const R* w;           // LDS window
    int64_t y0, x0, z0;   // window origin
    int WY, WX, WZ;
    __device__ __forceinline__ bool inside(int64_t y, int64_t x, int64_t z) const {
        return (uint64_t)(y - y0) < (uint64_t)WY && (uint64_t)(x - x0) < (uint64_t)WX && (uint64_t)(z - z0) < (uint64_t)WZ;
    }
    // T[y, x, z] (in range), from the window when it holds the cell
    __device__ __forceinline__ double at(int64_t y, int64_t x, int64_t z) const {
        if (inside(y, x, z)) return (double)w[((y - y0) * WX + (x - x0)) * WZ + (z - z0)];
        return (double)T[(y * W + x) * L + z];
    }
    // window-only read (the step's cube is always inside the window)
    __device__ __forceinline__ double atw(int64_t y, int64_t x, int64_t z) const {
        return (double)w[((int)(y - y0) * WX + (int)(x - x0)) * WZ + (int)(z - z0)];
    }
};

// FastMarching3D.interpolatePoint :275-314, interior branch (a7 coefficient as written, :290), on
// the eight corner values m[4 dj + 2 di + dk] = m{dj}{di}{dk}
__device__ __forceinline__ double tri3(const double* m, double a, double b, double c) {
    const double m000 = m[0], m001 = m[1], m010 = m[2], m011 = m[3];
    const double m100 = m[4], m101 = m[5], m110 = m[6], m111 = m[7];
    const double a0 = m000;
    const double a1 = m010 - m000;
    const double a2 = m100 - m000;
    const double a3 = m001 - m000;
    const double a4 = m110 + m000 - m010 - m100;
    const double a5 = m011 + m000 - m010 - m001;
    const double a6 = m101 + m000 - m100 - m001;
    const double a7 = m111 + m000 - m100 - m001 - m010;
    return a0 + a1 * a + a2 * b + a3 * c + a4 * a * b + a5 * a * c + a6 * b * c + a7 * a * b * c;
}

// sqrt(a*a + b*b + c*c) < t  <=>  a*a + b*b + c*c < t*t for t = 1 and 1.5 (t*t exact, sqrt correctly
// rounded and monotone; the largest double below t*t has a root that rounds below t): the
// distance tests of :238-240 and :266-267 without the square root on the walker's chain
__device__ __forceinline__ double sq3(double a, double b, double c) { return a * a + b * b + c * c; }

// The walk is ONE wave: its LDS accesses complete in issue order, so lanes exchange values through
// LDS with only a compiler fence (and an LDS-count wait) -- a workgroup barrier would also wait
// for the path's global stores.
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// (uint32_t)trunc(x) and rint(x) as int: one conversion each.  The hardware truncates and CLAMPS to
// the type's range (negative -> 0 for the unsigned form, NaN -> 0), which is not what the
// reference's np.uint32(np.fix(p)) does: numpy on x86-64 gives index 0 for NaN and +-inf and
// 2^32 - |fix(p)| for p <= -1, which raises IndexError at mapI[j,i,k] (FastMarching3D.py:283).  So
// the general step uses a conversion's result as an index only for a coordinate in (-1, 2^31)
// (where clamping is truncation: (-1, 0) -> 0, as numpy) and decides every other coordinate itself
// (DESIGN 3.4b); a finite coordinate's clamped rint, INT_MIN / INT_MAX, fails the same range tests
// as the exact value.  No index is formed from a clamped or wrapped conversion.
// (cvt_u32: above gdm2d_kernel)
__device__ __forceinline__ int rint_i32(double x) {
    int r;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(__builtin_rint(x)));
    return r;
}

// v from lane - SH of the same 16-lane row (DPP row_shr); lanes with no source keep their own
template <int SH>
__device__ __forceinline__ double row_shr_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)b, (int)(unsigned)b, 0x110 + SH, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(b >> 32), (int)(unsigned)(b >> 32), 0x110 + SH, 0xf, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// window origin along one axis: the needed span [lo, hi] (clipped to the volume) centred in a
// window of n cells that stays inside [0, len)
__device__ __forceinline__ int64_t win_origin(int64_t lo, int64_t hi, int n, int64_t len) {
    int64_t o = (lo + hi + 1) / 2 - n / 2;
    if (o + n > len) o = len - n;
    return o < 0 ? 0 : o;
}

// as the 2D kernel: one template for the single launch (A = Gdm3dArgs) and the grid form (A =
// GdmBatchArgs: workgroup p walks path p of volume desc[p].map into out + p * cap * 3)
template <typename R>
__device__ __forceinline__ Gdm3dArgs path3_args(const Gdm3dArgs& a) { return a; }
template <typename R>
__device__ __forceinline__ Gdm3dArgs path3_args(const GdmBatchArgs& b) {
    const int64_t p = blockIdx.x;
    const GdmDesc* __restrict__ d = b.desc + p;
    Gdm3dArgs a;
    a.T = static_cast<const R*>(b.T) + (int64_t)d->map * b.H * b.W * b.L;
    a.H = b.H;
    a.W = b.W;
    a.L = b.L;
    for (int i = 0; i < 3; ++i) {
        a.init[i] = d->init[i];
        a.end[i] = d->end[i];
    }
    a.tau = b.tau;
    a.steps = b.steps;
    a.out = b.out + p * b.cap * 3;
    a.cap = b.cap;
    a.n_out = b.n_out + p;
    a.status = b.status + p;
    return a;
}

template <typename R, typename A = Gdm3dArgs>
__global__ __launch_bounds__(kP3Threads) void gdm3d_kernel(A arg) {
    const Gdm3dArgs a = path3_args<R>(arg);
    __shared__ Path3Lds sl;
    if (threadIdx.x == 0) {
        sl.req_seq = 0;
        sl.done = 0;
    }
    __syncthreads();
    if (threadIdx.x >= 64) {
        path3_builder<R>(sl, static_cast<const R*>(a.T), a.H, a.W, a.L);
        return;
    }
    auto& ring = sl.ring;
    auto& gsh = sl.gsh;
    auto& nsh = sl.nsh;
    auto& nbad = sl.nbad;
    const int lane = threadIdx.x;
    const bool lead = lane == 0;
    Win3<R> v;
    v.T = static_cast<const R*>(a.T);
    v.H = a.H; v.W = a.W; v.L = a.L;
    const int64_t H = a.H, W = a.W, L = a.L;
    win3_dims<R>(a.H, a.W, a.L, v.WY, v.WX, v.WZ);
    // lane constants of the interior gather (see the step): lanes 0..23 sample np.gradient along
    // axis g_ax at corner (cj, ci, ck) of the cube -- window offset g_off from the cube's origin,
    // g_str the axis stride, g_c the corner's coordinate along its axis; lanes 24..30 read the
    // rint node (-1) and its six neighbours (0..5: y-1, y+1, x-1, x+1, z-1, z+1) at g_off from it
    const int sy = v.WX * v.WZ, sx = v.WZ;
    int g_ax = 0, g_c = 0, g_off = 0, g_str = 0;
    if (lane < 24) {
        g_ax = lane >> 3;
        const int cj = (lane >> 2) & 1, ci = (lane >> 1) & 1, ck = lane & 1;
        g_c = g_ax == 0 ? cj : g_ax == 1 ? ci : ck;
        g_off = cj * sy + ci * sx + ck;
        g_str = g_ax == 0 ? sy : g_ax == 1 ? sx : 1;
    } else if (lane < 31) {
        const int q = lane - 25;
        const int st = q < 0 ? 0 : (q >> 1) == 0 ? sy : (q >> 1) == 1 ? sx : 1;
        g_off = q < 0 ? 0 : (q & 1) ? st : -st;
    }
    v.w = reinterpret_cast<const R*>(sl.wbuf[0]);
    v.y0 = v.x0 = v.z0 = -((int64_t)1 << 40);  // empty: the first step requests a window
    // the two buffers' origins (scalars: no private array), the current one mirrored in v
    int64_t oy[2] = {v.y0, v.y0}, ox[2] = {v.x0, v.x0}, oz[2] = {v.z0, v.z0};
    int cur = 0, seq = 0;
    bool pending = false;
    auto issue = [&](int b, int64_t y0, int64_t x0, int64_t z0) {
        oy[b] = y0; ox[b] = x0; oz[b] = z0;
        sl.req_y0 = y0;
        sl.req_x0 = x0;
        sl.req_z0 = z0;
        sl.req_b = b;
        __hip_atomic_store(&sl.req_seq, ++seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto wait_built = [&]() -> bool {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(&sl.done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < seq * kB3) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > kPathSpin) return false;
            __builtin_amdgcn_s_sleep(1);
        }
        return true;
    };
    int bj_lo = 1, bj_hi = 0, bi_lo = 1, bi_hi = 0, bk_lo = 1, bk_hi = 0;  // empty: the first step decides
    // step bounds of the fast path (sufficient conditions for "holds and no prefetch trigger")
    auto set_bounds = [&]() {
        const int m = pending ? 0 : kPre3;
        auto lo = [&](int64_t o) { return o == 0 ? 0 : (int)(o + 1 + m); };
        auto hi = [&](int64_t o, int n, int64_t len) { return o + n >= len ? (int)(len - 1) : (int)(o + n - 3 - m); };
        bj_lo = lo(v.y0); bj_hi = hi(v.y0, v.WY, H);
        bi_lo = lo(v.x0); bi_hi = hi(v.x0, v.WX, W);
        bk_lo = lo(v.z0); bk_hi = hi(v.z0, v.WZ, L);
    };
    auto holds = [&](int b, int64_t ylo, int64_t xlo, int64_t zlo, int64_t yhi, int64_t xhi, int64_t zhi) {
        return ylo >= oy[b] && xlo >= ox[b] && zlo >= oz[b] && yhi < oy[b] + v.WY && xhi < ox[b] + v.WX &&
               zhi < oz[b] + v.WZ;
    };
    double* out = a.out;
    // path point q: the LDS ring while it holds it (the last kRing points), else global memory
    auto pt = [&](int64_t q, int c) -> double { return ring[(int)q & (kRing - 1)][c]; };  // q >= 0
    auto put = [&](int64_t q, double x, double y, double z) {
        out[3 * q] = x;  // every lane: same address and value (each lane reads back its own
        out[3 * q + 1] = y;  // stores when back-tracking below the ring)
        out[3 * q + 2] = z;
        ring[(int)q & (kRing - 1)][0] = x;
        ring[(int)q & (kRing - 1)][1] = y;
        ring[(int)q & (kRing - 1)][2] = z;
    };
    int64_t n = 0, lo = 0;  // ring holds points [lo, n); below lo: global
    auto point = [&](int64_t q, int c) -> double { return q >= lo ? pt(q, c) : out[3 * q + c]; };
    put(0, a.init[0], a.init[1], a.init[2]);
    n = 1;
    int status = kGdmDone;
    const double tau = a.tau;
    const int off[6][3] = {{0, -1, 0}, {0, 1, 0}, {-1, 0, 0}, {1, 0, 0}, {0, 0, -1}, {0, 0, 1}};
    double gx = a.init[0], gy = a.init[1], gz = a.init[2];  // the last point, out[n - 1]
    double ustep[6][3];  // (-off) / tau of the integer-descent moves (:244-252), divided once
#pragma unroll
    for (int q = 0; q < 6; ++q)
        for (int c = 0; c < 3; ++c) ustep[q][c] = (double)(-off[q][c]) / tau;
    // what the step's tail (:255-264) subtracts from the node after the descent move q: its
    // |(dx, dy, dz)| is the one nonzero |ustep| (sqrt(u*u) == |u| for a correctly rounded root), so
    // the branch and the products are known per move
    double mstep[6][3];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double u = ustep[q][q >> 1 == 0 ? 1 : q >> 1 == 1 ? 0 : 2];
        const double nrm = __builtin_fabs(u);
        for (int c = 0; c < 3; ++c) mstep[q][c] = nrm < 0.01 ? tau * (ustep[q][c] / nrm) : tau * ustep[q][c];
    }
    double p2x = 0.0, p2y = 0.0, p2z = 0.0;  // path point n - 2 (point n - 1 is (gx, gy, gz))
    // the descent's moves are exact unit steps (tau * (-off / tau) == -off, e.g. tau = 0.5): after
    // an integer-node step the walk stays on nodes, and the run loop below takes the next ones
    bool int_moves = EIK_P3RUN != 0;
#pragma unroll
    for (int q = 0; q < 6; ++q)
        for (int c = 0; c < 3; ++c) int_moves &= mstep[q][c] == (double)(-off[q][c]);
    bool run = false;  // the previous step was an integer-node step and int_moves holds
    EIK_P3DECL;
    for (long k = 0; k < a.steps; ++k) {
        // Integer-descent run (the C5 regime).  After an integer-node step from node M to its
        // neighbour N the step at N, as the general body below takes it, is: the point test of
        // :238-240 pops N itself (distance 0) but not M (distance exactly 1), puts N back where
        // it was (the same value in the same slot), and -- when the fallback is taken (a T sample
        // of the gradient not finite, T[N] finite, every neighbour in range: an interior node) and
        // some neighbour is lower -- appends N + off[best] (the tail's N - mstep[best], exact).
        // The run loop does exactly that on scalar node coordinates; any other case (window
        // bookkeeping due, a face node, no lower neighbour, the point budget) leaves it for the
        // general body of the same step.
        if (run) {
            // every value the loop branches on is wave-uniform and held in scalar registers (the
            // window bounds come from the general body's VALU conversions: read them once)
            auto rfl = [](int q) { return __builtin_amdgcn_readfirstlane(q); };
            auto rfl64 = [](int64_t q) {
                return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)q >> 32)) << 32) |
                                 (uint32_t)__builtin_amdgcn_readfirstlane((int)q));
            };
            int x = rfl((int)gx), y = rfl((int)gy), z = rfl((int)gz);
            const int wy0 = rfl((int)v.y0), wx0 = rfl((int)v.x0), wz0 = rfl((int)v.z0);
            // the fast window bounds and the interior test in one range per axis
            const int ylo = rfl(bj_lo > 1 ? bj_lo : 1), yhi = rfl(bj_hi < (int)H - 2 ? bj_hi : (int)H - 2);
            const int xlo = rfl(bi_lo > 1 ? bi_lo : 1), xhi = rfl(bi_hi < (int)W - 2 ? bi_hi : (int)W - 2);
            const int zlo = rfl(bk_lo > 1 ? bk_lo : 1), zhi = rfl(bk_hi < (int)L - 2 ? bk_hi : (int)L - 2);
            const int len = g_ax == 0 ? (int)H : g_ax == 1 ? (int)W : (int)L;  // lanes 0..23: the sample axis
            const int lane_xyz = g_ax;  // which coordinate a gradient lane's corner runs along
            const bool node_lane = lane >= 24 && lane < 31;
            const R* w = v.w;
            int64_t nn = rfl64(n), ll = rfl64(lo), kq = rfl64((int64_t)k);
            const int64_t cap = a.cap, steps = a.steps;
            bool fin = false, moved = false;
            int xp = 0, yp = 0, zp = 0;
            for (;;) {
                if (y < ylo || y > yhi || x < xlo || x > xhi || z < zlo || z > zhi) break;
                const int base = ((y - wy0) * v.WX + (x - wx0)) * v.WZ + (z - wz0);
                const int pc = (lane_xyz == 0 ? y : lane_xyz == 1 ? x : z) + g_c;  // >= 1: never the first
                const int idx = base + g_off;
                const R r_hi = w[idx + (pc == len - 1 ? 0 : g_str)];
                const R r_lo = w[idx - g_str];
                const double t_hi = (double)r_hi;
                const unsigned long long nonfin =
                    __ballot(lane < 24 && !(__builtin_isfinite(r_hi) && __builtin_isfinite(r_lo)));
                const double tnode = readlane_f64(t_hi, 24);
                // T[N] +inf (the general body's fallback test) or NaN (its ordered scan below never
                // moves; the minimum below would skip the NaN): the general body
                if (nonfin == 0ull || !(tnode < __builtin_inf())) break;
                // The reference's ordered scan (curT = T[N]; `if T[nb] < curT` over the six
                // neighbours) picks the FIRST neighbour attaining the minimum, if that minimum is
                // below T[N].  As a lane minimum over lanes 24..30 (the node first: a tie with it
                // keeps the node) and the lowest lane holding it; NaN neighbours are never taken by
                // either (v_min_f64 returns the other operand, NaN == m is false).
                double mv = node_lane ? t_hi : __builtin_inf();
                mv = __builtin_fmin(mv, row_shr_f64<1>(mv));
                mv = __builtin_fmin(mv, row_shr_f64<2>(mv));
                mv = __builtin_fmin(mv, row_shr_f64<4>(mv));
                const double m = readlane_f64(mv, 30);  // row_shr 1, 2, 4: lanes 23..30, lane 23 +inf
                const unsigned long long eq = __ballot(node_lane && t_hi == m);
                const int best = rfl(__builtin_ctzll(eq) - 25);  // -1: the node itself
                if (best < 0 || nn >= cap) break;
                const int nx = x + (best == 2 ? -1 : best == 3 ? 1 : 0);
                const int ny = y + (best == 0 ? -1 : best == 1 ? 1 : 0);
                const int nz = z + (best == 4 ? -1 : best == 5 ? 1 : 0);
                put(nn, (double)nx, (double)ny, (double)nz);
                ++nn;
                if (nn - ll > kRing) ll = nn - kRing;
                moved = true;
                xp = x;
                yp = y;
                zp = z;
                x = nx;
                y = ny;
                z = nz;
                if (sq3((double)nx - a.end[0], (double)ny - a.end[1], (double)nz - a.end[2]) < 2.25) {
                    fin = true;  // :266-267
                    break;
                }
                if (++kq >= steps) {
                    fin = true;
                    break;
                }
            }
            n = nn;
            lo = ll;
            k = (long)kq;
            if (moved) {  // the last two points: the current node and the node before it
                p2x = (double)xp;
                p2y = (double)yp;
                p2z = (double)zp;
                gx = (double)x;
                gy = (double)y;
                gz = (double)z;
            }
            if (fin) break;
        }
        EIK_P3PROBE(3);
        // np.uint32(np.fix(p)) of :276-278 and the rint node of :213-215.  The hardware conversions
        // clamp, so they are numpy's only for a coordinate in (-1, 2^31).  Every other coordinate
        // shows in the integer results -- p <= -1, NaN and -inf convert to 0, p >= 2^31 and +inf to
        // 2^31 or more, which fails the range test -- so the step pays three integer tests and
        // decides those rare cases (and a point in a cell of a low face) in the block below: a
        // finite coordinate <= -1 or past the last cell is the reference's IndexError, a non-finite
        // one takes index 0 with its own fraction, as numpy's cast gives it, and has no rint node
        // (-1: nothing is gathered for it; the NaN branch raises at its int(round())).
        uint32_t i = cvt_u32(gx), j = cvt_u32(gy), kk = cvt_u32(gz);
        int64_t rx = rint_i32(gx), ry = rint_i32(gy), rz = rint_i32(gz);
        bool gfin = true;  // all three coordinates finite
        if ((int64_t)i + 1 >= W || (int64_t)j + 1 >= H || (int64_t)kk + 1 >= L || i == 0u || j == 0u || kk == 0u) {
            const bool fx = __builtin_isfinite(gx), fy = __builtin_isfinite(gy), fz = __builtin_isfinite(gz);
            auto raises = [](double p, uint32_t u, int64_t len, bool fin) {
                return fin ? p <= -1.0 || (int64_t)u + 1 >= len : len < 2;
            };
            if (raises(gx, i, W, fx) || raises(gy, j, H, fy) || raises(gz, kk, L, fz)) { status = kGdmError; break; }
            if (!(fx && fy && fz)) {
                gfin = false;
                i = fx ? i : 0u;  // index 0 as such, not a clamped conversion's result
                j = fy ? j : 0u;
                kk = fz ? kk : 0u;
                rx = ry = rz = -1;
            }
        }
        // fast path: while bj_lo <= j <= bj_hi (and for i, kk) the cube is in the current window and
        // not within kPre3 of an inner edge (or a build is pending): nothing to do this step
        if ((int)j < bj_lo || (int)j > bj_hi || (int)i < bi_lo || (int)i > bi_hi || (int)kk < bk_lo || (int)kk > bk_hi) {
            const int64_t ylo = j > 0 ? j - 1 : 0, yhi = j + 2 < H ? j + 2 : H - 1;
            const int64_t xlo = i > 0 ? i - 1 : 0, xhi = i + 2 < W ? i + 2 : W - 1;
            const int64_t zlo = kk > 0 ? kk - 1 : 0, zhi = kk + 2 < L ? kk + 2 : L - 1;
            const int64_t cy0 = win_origin(ylo, yhi, v.WY, H), cx0 = win_origin(xlo, xhi, v.WX, W),
                          cz0 = win_origin(zlo, zhi, v.WZ, L);
            if (!holds(cur, ylo, xlo, zlo, yhi, xhi, zhi)) {
                const int nb = seq == 0 ? 0 : 1 - cur;
                bool have = false;
                if (pending) {
                    pending = false;
                    if (!wait_built()) { status = kGdmError; break; }
                    have = holds(nb, ylo, xlo, zlo, yhi, xhi, zhi);
                }
                if (!have) {
                    issue(nb, cy0, cx0, cz0);
                    if (!wait_built()) { status = kGdmError; break; }
                }
                cur = nb;
                v.w = reinterpret_cast<const R*>(sl.wbuf[cur]);
                v.y0 = oy[cur];
                v.x0 = ox[cur];
                v.z0 = oz[cur];
            }
            // near an inner edge of the current window: build the window centred here, meanwhile
            if (!pending && ((ylo - v.y0 < kPre3 && v.y0 > 0) || (v.y0 + v.WY - 1 - yhi < kPre3 && v.y0 + v.WY < H) ||
                             (xlo - v.x0 < kPre3 && v.x0 > 0) || (v.x0 + v.WX - 1 - xhi < kPre3 && v.x0 + v.WX < W) ||
                             (zlo - v.z0 < kPre3 && v.z0 > 0) || (v.z0 + v.WZ - 1 - zhi < kPre3 && v.z0 + v.WZ < L)) &&
                (cy0 != v.y0 || cx0 != v.x0 || cz0 != v.z0)) {
                issue(1 - cur, cy0, cx0, cz0);
                pending = true;
            }
            set_bounds();
        }
        EIK_P3PROBE(0);
        const bool rin = rx >= 0 && ry >= 0 && rz >= 0 && rx < W && ry < H && rz < L;
        // per-lane gather, kept in registers: lanes 0..23 the two T samples of one np.gradient value
        // (axis, corner), lanes 24..30 the node and its six neighbours (:244-252).  (The last two
        // path points, which the pops of :238-240 test, are (gx, gy, gz) and (p2x, p2y, p2z).)
        double t_hi = 0.0, t_lo = 0.0, gscale = 0.5, nv = 0.0;
        bool bad = false;
        if (ry >= 1 && ry + 1 < H && rx >= 1 && rx + 1 < W && rz >= 1 && rz + 1 < L) {
            // interior rint node: its six neighbours are in range (no wrap, none bad) and, like the
            // cube, inside the window -- every lane reads window cells at a lane-constant offset,
            // the same code on every lane (lanes 24..30 with stride 0 read their cell twice)
            const bool grad = lane < 24;
            const int base = grad ? (((int)(j - v.y0) * v.WX + (int)(i - v.x0)) * v.WZ + (int)(kk - v.z0))
                                  : (((int)(ry - v.y0) * v.WX + (int)(rx - v.x0)) * v.WZ + (int)(rz - v.z0));
            const int64_t pc = (g_ax == 0 ? (int64_t)j : g_ax == 1 ? (int64_t)i : (int64_t)kk) + g_c;
            const int64_t len = g_ax == 0 ? H : g_ax == 1 ? W : L;
            const bool first = pc == 0, last = !first && pc == len - 1;
            const int idx = lane < 31 ? base + g_off : base;
            const R* w = v.w;
            t_hi = (double)w[idx + (last ? 0 : g_str)];
            t_lo = (double)w[idx - (first ? 0 : g_str)];
            gscale = first || last ? 1.0 : 0.5;  // (/ 1.0 at the ends, / 2.0 inside: both exact)
            nv = t_hi;
        } else {
        if (lane >= 24 && lane < 31) {
            if (rin) {
                const int q = lane - 25;  // -1: the node; 0..5: y-1, y+1, x-1, x+1, z-1, z+1 (:244-252)
                int64_t cx = rx, cy = ry, cz = rz;
                if (q >= 0) {
                    const int64_t sg = (q & 1) ? 1 : -1;
                    cy += (q >> 1) == 0 ? sg : 0;
                    cx += (q >> 1) == 1 ? sg : 0;
                    cz += (q >> 1) == 2 ? sg : 0;
                }
                if (cx < 0) cx += W;  // python negative indices wrap
                if (cy < 0) cy += H;
                if (cz < 0) cz += L;
                bad = cx >= W || cy >= H || cz >= L;
                nv = bad ? __builtin_nan("") : v.at(cy, cx, cz);
            }
        }
        if (lane < 24) {
            const int axis = lane >> 3, cj = (lane >> 2) & 1, ci = (lane >> 1) & 1, ck = lane & 1;
            const int64_t y = j + cj, x = i + ci, z = kk + ck;
            const int64_t len = axis == 0 ? H : axis == 1 ? W : L;
            const int64_t p = axis == 0 ? y : axis == 1 ? x : z;
            const bool first = p == 0, last = !first && p == len - 1;
            const int64_t dlo = first ? 0 : 1, dhi = last ? 0 : 1;
            t_hi = v.atw(y + (axis == 0) * dhi, x + (axis == 1) * dhi, z + (axis == 2) * dhi);
            t_lo = v.atw(y - (axis == 0) * dlo, x - (axis == 1) * dlo, z - (axis == 2) * dlo);
            gscale = first || last ? 1.0 : 0.5;  // (/ 1.0 at the ends, / 2.0 inside: both exact)
        }
        }
        // Integer-node step (the C5 regime: on a z-padded few-layer volume every step is the
        // integer descent).  At a point whose three coordinates are integers every fraction of
        // the trilinear interpolation is 0, so each of dx, dy, dz is a0 + a1*0 + ... + a7*0*0*0:
        // NaN exactly when one of its coefficients is not finite (a*0 = NaN), i.e. when one of
        // its eight np.gradient samples is (every corner enters some a1..a7), i.e. when one of
        // their T samples is; otherwise a0.  So the fallback is taken iff a lane's T sample is not
        // finite -- a ballot, no interpolation and no lane exchange through LDS.  When it is
        // taken with the node reached and in range, no neighbour out of range and some
        // neighbour lower, the step is the descent below, in the reference's order with the
        // same operations as the general path (which handles every other case).
        double dx = 0.0, dy = 0.0, dz = 0.0;
        bool intstep = false;
        int best = -1;
        double tnode = 0.0;
        if (gx == (double)i && gy == (double)j && gz == (double)kk && rin) {
            const unsigned long long nonfin =
                __ballot(lane < 24 && !(__builtin_isfinite(t_hi) && __builtin_isfinite(t_lo)));
            const unsigned long long badm = __ballot(lane >= 24 && lane < 31 && bad);
            tnode = readlane_f64(nv, 24);
            if (nonfin != 0ull && badm == 0ull && !__builtin_isinf(tnode)) {
                double curT = tnode;
#pragma unroll
                for (int q = 0; q < 6; ++q) {  // the reference's ordered scan
                    const double tc = readlane_f64(nv, 25 + q);
                    if (tc < curT) {
                        curT = tc;
                        best = q;
                    }
                }
                intstep = best >= 0;
            }
        }
        if (intstep) {
            const int64_t nx = rx, ny = ry, nz = rz;
            bool deep = false;  // as the NaN branch below with fast = true
            if (n > 0 && sq3(gx - nx, gy - ny, gz - nz) < 1.0) {
                --n;
                if (n > 0 && sq3(p2x - nx, p2y - ny, p2z - nz) < 1.0) {
                    --n;
                    deep = true;
                }
            }
            if (deep)
                while (n > 0 && sq3(point(n - 1, 0) - nx, point(n - 1, 1) - ny, point(n - 1, 2) - nz) < 1.0) --n;
            if (n >= a.cap) { status = kGdmError; break; }
            if (n < lo) lo = n;
            put(n, (double)nx, (double)ny, (double)nz);
            ++n;
            gx = (double)nx;
            gy = (double)ny;
            gz = (double)nz;
        } else {
        if (lane < 24) gsh[lane >> 3][lane & 7] = (t_hi - t_lo) * gscale;
        if (lane >= 24 && lane < 31 && rin) {
            nsh[lane - 24] = nv;
            nbad[lane - 24] = bad;
        }
        wave_lds_sync();
        dx = tri3(gsh[1], gx - i, gy - j, gz - kk);
        dy = tri3(gsh[0], gx - i, gy - j, gz - kk);
        dz = tri3(gsh[2], gx - i, gy - j, gz - kk);
        EIK_P3PROBE(1);
        if (__builtin_isnan(dx) || __builtin_isnan(dy) || __builtin_isnan(dz)) {  // :212-253
            // int(round(NaN)) raises ValueError, int(round(+-inf)) OverflowError (:213-215), the
            // path as it stands.  (The points popped below were current points of earlier steps:
            // finite and in (-1, 2^31), so their 64-bit conversions are exact.)
            if (!gfin) { status = kGdmError; break; }
            int64_t nx = rx, ny = ry, nz = rz;
            bool err = false;
            // fast: the node is in range and reached -- no back-tracking, the gathered values apply
            const bool fast = rin && !__builtin_isinf(nsh[0]);
            if (!fast) {
                for (;;) {
                    if (nx < 0 || ny < 0 || nz < 0 || nx >= W || ny >= H || nz >= L) { err = true; break; }
                    if (!__builtin_isinf(v.at(ny, nx, nz))) break;
                    --n;
                    if (n == 0) { err = true; break; }
                    nx = (int64_t)__builtin_rint(point(n - 1, 0));
                    ny = (int64_t)__builtin_rint(point(n - 1, 1));
                    nz = (int64_t)__builtin_rint(point(n - 1, 2));
                }
                if (err) { status = kGdmError; break; }
            }
            bool deep = !fast;  // pops beyond the two gathered points read the ring
            if (fast && n > 0 && sq3(gx - nx, gy - ny, gz - nz) < 1.0) {
                --n;
                if (n > 0 && sq3(p2x - nx, p2y - ny, p2z - nz) < 1.0) {
                    --n;
                    deep = true;
                }
            }
            if (deep)
                while (n > 0 && sq3(point(n - 1, 0) - nx, point(n - 1, 1) - ny, point(n - 1, 2) - nz) < 1.0) --n;
            if (n >= a.cap) { status = kGdmError; break; }
            if (n < lo) lo = n;
            put(n, (double)nx, (double)ny, (double)nz);
            ++n;
            if (!fast) {  // the six neighbours of a back-tracked node, in parallel (lanes 0..5)
                if (lane < 6) {
                    int64_t cx = nx + off[lane][0], cy = ny + off[lane][1], cz = nz + off[lane][2];
                    if (cx < 0) cx += W;  // python negative indices wrap
                    if (cy < 0) cy += H;
                    if (cz < 0) cz += L;
                    const bool bad = cx >= W || cy >= H || cz >= L;
                    nsh[lane + 1] = bad ? __builtin_nan("") : v.at(cy, cx, cz);
                    nbad[lane + 1] = bad;
                }
                wave_lds_sync();
            }
            double curT = fast ? nsh[0] : v.at(ny, nx, nz);
            for (int q = 0; q < 6; ++q) {  // the reference's ordered scan
                if (nbad[q + 1]) { err = true; break; }
                const double tc = nsh[q + 1];
                if (tc < curT) {
                    curT = tc;
                    dx = ustep[q][0];
                    dy = ustep[q][1];
                    dz = ustep[q][2];
                }
            }
            wave_lds_sync();  // nsh / nbad are rewritten by the next step
            if (err) { status = kGdmError; break; }
            gx = (double)nx;
            gy = (double)ny;
            gz = (double)nz;
        }
        }
        EIK_P3PROBE(2);
        double ax, ay, az;
        if (intstep) {  // the tail below for the move `best`, from the table
            double m0 = 0.0, m1 = 0.0, m2 = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (q == best) {
                    m0 = mstep[q][0];
                    m1 = mstep[q][1];
                    m2 = mstep[q][2];
                }
            ax = gx - m0;
            ay = gy - m1;
            az = gz - m2;
        } else {
            const double nrm = __builtin_sqrt(dx * dx + dy * dy + dz * dz);  // :255
            if (nrm < 0.01) {
                ax = gx - tau * (dx / nrm);
                ay = gy - tau * (dy / nrm);
                az = gz - tau * (dz / nrm);
            } else {  // unnormalised step (:262-264)
                ax = gx - tau * dx;
                ay = gy - tau * dy;
                az = gz - tau * dz;
            }
        }
        if (n >= a.cap) { status = kGdmError; break; }
        put(n, ax, ay, az);
        ++n;
        if (n - lo > kRing) lo = n - kRing;
        p2x = gx;  // (gx, gy, gz) is point n - 2 now
        p2y = gy;
        p2z = gz;
        gx = ax;
        gy = ay;
        gz = az;
        if (__builtin_isnan(ax) || __builtin_isnan(ay) || __builtin_isnan(az)) { status = kGdmError; break; }
        if (sq3(ax - a.end[0], ay - a.end[1], az - a.end[2]) < 2.25) break;  // :266-267
        run = int_moves && intstep;
    }
    if (pending) wait_built();  // no build may still be writing when the builders are told to quit
    __hip_atomic_store(&sl.req_seq, -1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    // as the 2D walker: a loop that ended (steps or stop radius) with no row left for `end` is out
    // of point budget
    if (status == kGdmDone && n >= a.cap) status = kGdmError;
    if (lead) {
        if (status == kGdmDone && n < a.cap) {  // :269
            out[3 * n] = a.end[0];
            out[3 * n + 1] = a.end[1];
            out[3 * n + 2] = a.end[2];
            ++n;
        }
        *a.n_out = n;
        *a.status = status;
    }
    EIK_P3FLUSH;
}

hipError_t gdm3d(const Gdm3dArgs& a, bool f64, hipStream_t st) {
    if (f64)
        hipLaunchKernelGGL(gdm3d_kernel<double>, dim3(1), dim3(kP3Threads), 0, st, a);
    else
        hipLaunchKernelGGL(gdm3d_kernel<float>, dim3(1), dim3(kP3Threads), 0, st, a);
    return hipGetLastError();
}

hipError_t gdm3d_batch(const GdmBatchArgs& a, bool f64, hipStream_t st) {
    if (f64)
        hipLaunchKernelGGL((gdm3d_kernel<double, GdmBatchArgs>), dim3((unsigned)a.P), dim3(kP3Threads), 0, st, a);
    else
        hipLaunchKernelGGL((gdm3d_kernel<float, GdmBatchArgs>), dim3((unsigned)a.P), dim3(kP3Threads), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- full-field gradient
__global__ void gradient2d_kernel(const double* __restrict__ T, int64_t H, int64_t W, double* __restrict__ gnx,
                                  double* __restrict__ gny) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= H * W) return;
    const int64_t j = idx / W, i = idx - (idx / W) * W;
    double a, b;
    grad_at<double>(T, H, W, j, i, a, b);
    gnx[idx] = a;
    gny[idx] = b;
}

hipError_t gradient2d(const double* T, int64_t H, int64_t W, double* gnx, double* gny, hipStream_t st) {
    const int64_t n = H * W;
    hipLaunchKernelGGL(gradient2d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, H, W, gnx, gny);
    return hipGetLastError();
}

}  // namespace eik
