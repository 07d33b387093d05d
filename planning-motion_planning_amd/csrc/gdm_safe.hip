// gdm_safe.hip -- the obstacle-safe 2D walker (eik_path2d_safe_*) on gfx950: its own
// kernel next to gdm.hip's reference-faithful walker.  The two run one copy (gdm_walk.hpp) of the
// step's arithmetic (walk_step_*), the window state (Walk2Win) and the builders.
//
// The rule (no reference counterpart beyond the cited lines; tests/path_safe_np.py restates it on the
// host).  G' is computeGradient's (Gnx, Gny) with NaN at every node whose T is +inf.  Per iteration,
// with p the last point:
//   * gradient step (FastMarching.py:175-176, :220-230 -- the default walker's walk_step_*: its bits)
//     unless the interpolation of G' at p is NaN (a corner it uses is impassable, or the reference's
//     own 0/0) or the walk is in integer mode;
//   * else the fallback of :178-218 as intended (FastMarching3D.py:212-264 runs it): n = rint(p); while
//     T[n] is +inf drop the last point and take n from the one before (none left: ERROR); drop the
//     points closer than 1 to n; append n; append the 4-neighbour with the smallest T strictly below
//     T[n] (scan y-1, y+1, x-1, x+1, first wins ties; none: STUCK);
//   * stop within 1.5 of `end` (:231);
//   * stall rule: T at the nearest node of the new point has to fall below its running minimum
//     within S = max(16, ceil(8 / tau)) iterations, else the walk is in integer mode for good.
// Integer descent strictly lowers T, so it ends at a seed or says STUCK.
//
// Layout: gdm.hip's (gdm_walk.hpp) -- one workgroup, wave 0 walks, 15 builder waves fill two 64 x 64
// LDS windows of the gradient, prefetched kPrefetch nodes ahead; the builders write the NaN of an
// impassable node (build_window<R, true>), so the blocked test is the NaN test the step has anyway.
// T at nodes (the stall rule, the fallback, integer mode) is read from global memory: two more
// windows of fp64 T would take 64 KiB of LDS next to the 128 KiB of gradient windows, and a CU has
// 160 KiB.  The stall rule's load is kept off the step's dependent chain instead: it is issued when
// a step's point is known and consumed after the NEXT step's arithmetic, whose mode is all it decides.
#include "eik_common.hpp"
#include "eik_kernels.hpp"

#pragma clang fp contract(off)

#include "gdm_walk.hpp"

namespace eik {

__device__ __forceinline__ const Gdm2dArgs& safe_walk(const GdmSafeArgs& s) { return s.a; }
__device__ __forceinline__ const GdmBatchArgs& safe_walk(const GdmSafeBatchArgs& s) { return s.b; }
__device__ __forceinline__ int64_t* safe_info(const GdmSafeArgs& s) { return s.info; }
__device__ __forceinline__ int64_t* safe_info(const GdmSafeBatchArgs& s) {
    return s.info ? s.info + 4 * (int64_t)blockIdx.x : nullptr;
}

// One safe walk by one workgroup: A = GdmSafeArgs (one path) or GdmSafeBatchArgs (workgroup p walks
// descriptor p into its own slab, as gdm2d_kernel's grid form).  Every lane of the walker wave runs
// the same uniform code on the same values (loads are broadcasts, stores hit one address with one
// value), so the path edits of the fallback need no hand-over between lanes.
template <typename R, typename A>
__global__ __launch_bounds__(kPathThreads) void gdm2d_safe_kernel(A arg) {
    const Gdm2dArgs a = path_args<R>(safe_walk(arg));
    int64_t* const info = safe_info(arg);
    const long stall = arg.stall;
    __shared__ PathLds s;
    const R* __restrict__ T = static_cast<const R*>(a.T);
    const int64_t H = a.H, W = a.W;
    if (threadIdx.x == 0) {
        s.req_seq = 0;
        s.done = 0;
    }
    __syncthreads();
    if (threadIdx.x >= 64) {
        path_builder<R, true>(s, T, H, W);
        return;
    }
    const bool lead = threadIdx.x == 0;
    double* out = a.out;
    int status = kGdmDone;
    double px = a.ix, py = a.iy;
    out[0] = px;
    out[1] = py;
    int64_t n = 1;
    const double tau = a.tau;
    Walk2Win win(s, H, W);
    // the cell (i, j) of a valid point left the fast bounds: switch / prefetch windows; false: a build
    // never finished (status set)
    auto slow_step = [&](int64_t i, int64_t j) -> bool {
        if (win.cross(i, j)) return true;
        status = kGdmError;
        return false;
    };
    // ---- the rule
    // a NaN point, or one whose interpolation cell leaves the raster (trunc(x) + 1 >= W <=> x >= W - 1)
    auto bad = [&](double x, double y) { return !(x >= 0.0 && y >= 0.0 && x < (double)(W - 1) && y < (double)(H - 1)); };
    auto stop_at = [&](double x, double y) {  // :231  sqrt(e) < 1.5 <=> e < 2.25 (correctly rounded sqrt)
        const double ex = x - a.ex, ey = y - a.ey;
        return ex * ex + ey * ey < 2.25;
    };
    const double inf = __builtin_inf();
    int64_t fallbacks = 0, dropped = 0, int_from = -1;
    long stale = 0;
    bool integer = false, reached = false, have_tq = false;
    double tq = inf;  // T at the nearest node of the last point: the stall rule's pending operand
    double tlow = bad(px, py) ? inf : tv(T, W, (int64_t)__builtin_rint(py), (int64_t)__builtin_rint(px));
    const long kmax = a.steps < a.cap - 1 ? a.steps : a.cap - 1;
    long k = 0;
    auto stale_test = [&]() {  // of the iteration before: decides the mode of iteration k
        if (!have_tq) return;
        have_tq = false;
        if (tq < tlow) {
            tlow = tq;
            stale = 0;
        } else if (++stale >= stall) {
            integer = true;
            int_from = k;
        }
    };
    // The fallback at p = (px, py), a valid point.  false: status set (ERROR: no point left; STUCK: no
    // lower neighbour).  Else (px, py) is the child node and tq its T.
    auto fallback = [&]() -> bool {
        ++fallbacks;
        int64_t nx = (int64_t)__builtin_rint(px), ny = (int64_t)__builtin_rint(py);  // half to even
        while (__builtin_isinf(tv(T, W, ny, nx))) {
            --n;
            ++dropped;
            if (n == 0) { status = kGdmError; return false; }
            nx = (int64_t)__builtin_rint(out[2 * (n - 1)]);  // every kept point is a valid one: in the raster
            ny = (int64_t)__builtin_rint(out[2 * (n - 1) + 1]);
        }
        while (n > 0 && norm2(out[2 * (n - 1)] - (double)nx, out[2 * (n - 1) + 1] - (double)ny) < 1) {
            --n;
            ++dropped;
        }
        if (n + 2 > a.cap) { status = kGdmError; return false; }  // (a fallback drops before it appends two)
        out[2 * n] = (double)nx;
        out[2 * n + 1] = (double)ny;
        ++n;
        double best = tv(T, W, ny, nx);
        int64_t bx = -1, by = -1;
        const double tn = ny > 0 ? tv(T, W, ny - 1, nx) : inf, ts = ny + 1 < H ? tv(T, W, ny + 1, nx) : inf;
        const double tw = nx > 0 ? tv(T, W, ny, nx - 1) : inf, te = nx + 1 < W ? tv(T, W, ny, nx + 1) : inf;
        if (tn < best) { best = tn; bx = nx; by = ny - 1; }
        if (ts < best) { best = ts; bx = nx; by = ny + 1; }
        if (tw < best) { best = tw; bx = nx - 1; by = ny; }
        if (te < best) { best = te; bx = nx + 1; by = ny; }
        if (bx < 0) { status = kGdmStuck; return false; }
        out[2 * n] = (double)bx;
        out[2 * n + 1] = (double)by;
        ++n;
        px = (double)bx;
        py = (double)by;
        tq = best;
        return true;
    };
    // ---- gradient phase
    constexpr unsigned kWinBytes = sizeof(s.g[0]);
    while (k < kmax) {
        // Run loop of ordinary steps, one exit branch each (the default walker's single-exit form): the
        // step and the stall rule's pending test are computed before anything is known to be special --
        // a cell outside the fast bounds (window bookkeeping, a bad point), operands outside the fast
        // arithmetic's domain, a NaN gradient, the stop radius, the last iteration, the stall rule
        // firing -- and any of those leaves with nothing committed; the reference-structured iteration
        // below then takes that iteration with the same decisions.  The LDS address of a cell outside
        // the bounds is clamped into the window (its values are discarded), the stall rule's node into
        // the raster (a point off the raster leaves before its T is used).
        // Code placement, this one instantiation only.  The run loop below and the integer-mode loop
        // are sensitive to where they start: in <double, GdmSafeArgs> the compiler's code ahead of them
        // is one dword shorter than it was before the walkers shared Walk2Win, and with byte-identical
        // loops four bytes earlier the fp64 single walk measured 1.4-1.9 % (gradient phase) and 4 %
        // (integer mode) slower -- twice as many of the loops' 8-byte instructions then cross a 32 B /
        // 64 B fetch line.  One dword here and ten ahead of the integer-mode loop (below), all
        // outside the loops, put both loops back at the addresses they had; the run loops of the other
        // three instantiations kept their start (mod 32) and get nothing.  This is tied to this
        // compiler's output: when the code ahead of the loops changes again, measure
        // (tools/path_safe_ab.py) and drop or move the pads.
        if constexpr (std::is_same_v<R, double> && std::is_same_v<A, GdmSafeArgs>) asm volatile("s_nop 0");
        while (have_tq) {
            const uint32_t i = (uint32_t)__builtin_trunc(px), j = (uint32_t)__builtin_trunc(py);
            const bool in = (int)(px >= 0.0) & (int)(py >= 0.0) & (int)((int)i >= win.lo_x) & (int)((int)i <= win.hi_x) &
                            (int)((int)j >= win.lo_y) & (int)((int)j <= win.hi_y);
            unsigned off = (unsigned)(((int)j - win.cy0i) * kPW + ((int)i - win.cx0i)) * (unsigned)sizeof(double2);
            off = off <= kWinBytes - (kPW + 2) * sizeof(double2) ? off : 0u;  // unsigned: negatives too
            const double2* g = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(s.g[win.cur]) + off);
            bool odd;
            const WalkStep o = walk_step_rs(g[0], g[1], g[kPW], g[kPW + 1], px - (double)i, py - (double)j, px, py, tau, odd);
            const bool lower = tq < tlow;
            const double ntlow = lower ? tq : tlow;
            const long nstale = lower ? 0 : stale + 1;
            const bool leave = (int)!in | (int)odd | (int)__builtin_isnan(o.dx + o.dy) | (int)stop_at(o.sx, o.sy) |
                               (int)(k + 1 >= kmax) | (int)(nstale >= stall);
            if (leave) break;
            tlow = ntlow;
            stale = nstale;
            out[2 * n] = o.sx;
            out[2 * n + 1] = o.sy;
            ++n;
            px = o.sx;
            py = o.sy;
            ++k;
            int nx = (int)__builtin_rint(px), ny = (int)__builtin_rint(py);
            nx = nx < 0 ? 0 : nx > (int)W - 1 ? (int)W - 1 : nx;
            ny = ny < 0 ? 0 : ny > (int)H - 1 ? (int)H - 1 : ny;
            tq = tv(T, W, ny, nx);
        }
        if (bad(px, py)) { ++k; status = kGdmError; break; }
        const int64_t i = (int64_t)px, j = (int64_t)py;
        if (i < win.lo_x || i > win.hi_x || j < win.lo_y || j > win.hi_y) {
            if (!slow_step(i, j)) { ++k; break; }
        }
        const int li = (int)i - win.cx0i, lj = (int)j - win.cy0i;
        const double fa = px - (double)i, fb = py - (double)j;
        const auto& gw = s.g[win.cur];
        const double2 g00 = gw[lj][li], g01 = gw[lj][li + 1], g10 = gw[lj + 1][li], g11 = gw[lj + 1][li + 1];
        bool odd;
        WalkStep o = walk_step_rs(g00, g01, g10, g11, fa, fb, px, py, tau, odd);
        if (odd) o = walk_step_exact(g00, g01, g10, g11, fa, fb, px, py, tau);
        stale_test();  // its load had the step's arithmetic to arrive
        ++k;
        if (integer || __builtin_isnan(o.dx) || __builtin_isnan(o.dy)) {
            if (!fallback()) break;
            if (stop_at(px, py)) { reached = true; break; }
            if (integer) break;  // the run loop below takes over
            have_tq = true;      // tq = T[child]
            continue;
        }
        out[2 * n] = o.sx;
        out[2 * n + 1] = o.sy;
        ++n;
        px = o.sx;
        py = o.sy;
        if (stop_at(px, py)) { reached = true; break; }
        if (!bad(px, py)) {
            tq = tv(T, W, (int64_t)__builtin_rint(py), (int64_t)__builtin_rint(px));
            have_tq = true;
        }
    }
    if (status == kGdmDone && !reached && !integer) stale_test();  // the budget ran out: info[2] as the rule's
    // ---- integer mode, a run loop as gdm3d_kernel's scalar integer descent: the last two points are
    // a node and its child one cell apart, so a fallback drops the child, appends it again and appends
    // its lowest neighbour -- one row per iteration, no gradient, four T reads
    if (integer && status == kGdmDone && !reached) {
        int64_t cx = (int64_t)px, cy = (int64_t)py;
        double tc = tq;
        // (code placement, as ahead of the gradient phase's run loop: ten dwords, once per walk)
        if constexpr (std::is_same_v<R, double> && std::is_same_v<A, GdmSafeArgs>)
            asm volatile(".rept 10\n s_nop 0\n .endr");
        while (k < kmax) {
            ++k;
            if (cx + 1 >= W || cy + 1 >= H || n >= a.cap) { status = kGdmError; break; }
            ++fallbacks;
            ++dropped;
            const double tn = cy > 0 ? tv(T, W, cy - 1, cx) : inf, ts = tv(T, W, cy + 1, cx);
            const double tw = cx > 0 ? tv(T, W, cy, cx - 1) : inf, te = tv(T, W, cy, cx + 1);
            double best = tc;
            int64_t bx = -1, by = -1;
            if (tn < best) { best = tn; bx = cx; by = cy - 1; }
            if (ts < best) { best = ts; bx = cx; by = cy + 1; }
            if (tw < best) { best = tw; bx = cx - 1; by = cy; }
            if (te < best) { best = te; bx = cx + 1; by = cy; }
            if (bx < 0) { status = kGdmStuck; break; }
            out[2 * n] = (double)bx;
            out[2 * n + 1] = (double)by;
            ++n;
            cx = bx;
            cy = by;
            tc = best;
            if (stop_at((double)cx, (double)cy)) { reached = true; break; }
        }
    }
    // a budget that ran out short of the stop radius: iterations -> STUCK, rows -> ERROR (as the default)
    if (status == kGdmDone && !reached) status = kmax == a.steps ? kGdmStuck : kGdmError;
    __hip_atomic_store(&s.req_seq, -1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);  // builders exit
    if (lead) {
        if (status == kGdmDone && n < a.cap) {  // :234
            out[2 * n] = a.ex;
            out[2 * n + 1] = a.ey;
            ++n;
        }
        *a.n_out = n;
        *a.status = status;
        if (info) {
            info[0] = fallbacks;
            info[1] = dropped;
            info[2] = int_from;
            info[3] = k;
        }
    }
}

hipError_t gdm2d_safe(const GdmSafeArgs& a, bool f64, hipStream_t st) {
    if (f64)
        hipLaunchKernelGGL((gdm2d_safe_kernel<double, GdmSafeArgs>), dim3(1), dim3(kPathThreads), 0, st, a);
    else
        hipLaunchKernelGGL((gdm2d_safe_kernel<float, GdmSafeArgs>), dim3(1), dim3(kPathThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t gdm2d_safe_batch(const GdmSafeBatchArgs& a, bool f64, hipStream_t st) {
    const dim3 g((unsigned)a.b.P), b(kPathThreads);
    if (f64)
        hipLaunchKernelGGL((gdm2d_safe_kernel<double, GdmSafeBatchArgs>), g, b, 0, st, a);
    else
        hipLaunchKernelGGL((gdm2d_safe_kernel<float, GdmSafeBatchArgs>), g, b, 0, st, a);
    return hipGetLastError();
}

}  // namespace eik
