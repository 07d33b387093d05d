// replan.hip -- incremental 2D re-solve after local cost changes.
//
// The Eikonal field is causal: a cell's value depends only on neighbours with smaller T.  After
// the cost changed inside K rectangles, only the numerical domain of dependence of the cells whose
// cost may have gone up -- the CONE -- has to be recomputed:
//
//   cone = closure of "p joins if a 4-neighbour q in the cone has T_old(q) <= T_old(p), p finite,
//          p not the goal", seeded with the finite-T cells of the EIK_CHANGE_ANY rectangles.
//          (The goal is excluded in the seed kernel AND in the flood: beside zero-cost cells, whose T
//          is 0 too, the tie 0 <= 0 would otherwise reach it and the reset would wipe the source.)
//
// Cells outside the cone keep T_old, cone cells restart from +inf: that state is a supersolution of
// the new problem, and the solver's monotone T = min(T, solve) iteration descends from it to the new
// fixed point.  Lowered costs need no reset at all (T_old is a supersolution already): their tiles
// are only queued.
//
// Kernels, in stream order (eikonal_api.cpp eik_fim2d_update):
//   prep (phase 0)   queue words cleared for the flood, T untouched
//   seed             sign bit set on the seed cells; every tile overlapping an ANY rectangle dilated
//                    by one cell queued
//   flood            ONE persistent launch on the tile engine of fim_engine.hpp (FIFO form): a tile
//                    visit stages T (+1-cell ring) in LDS as bit patterns, carries the marks with
//                    four skewed quadrant sweeps (one wave per direction) until a pass adds none,
//                    stores the newly marked cells and queues a neighbour when a newly marked edge
//                    cell has T <= the neighbour's adjacent, unmarked cell
//   prep (phase 1)   queue words cleared again, as fim2d_init_kernel does, T untouched
//   reset            over the tiles the flood recorded: marked cells -> +inf, the edge-column copies
//                    rewritten, the tile queued for the solve (kSelf | kVisited) when it has a reset
//                    cell and a finite kept cell in the tile or on its ring, keyed by the smallest
//   rects            every tile overlapping a rectangle (either kind) queued when one of its
//                    finite-cost rectangle cells has a finite kept 4-neighbour (a lowered or opened
//                    cell can only improve from such a neighbour)
//
// The mark is the sign bit of T in place: T >= 0, so a set sign bit means "in the cone" and |T| is the
// old value; non-negative IEEE values order as unsigned integers, so the flood compares bit patterns
// and the cone is a deterministic function of T_old.  Cross-workgroup visibility inside the flood
// follows the engine's recipe: sc1 loads and stores, s_waitcnt vmcnt(0) in every storing wave and a
// workgroup barrier before any activation atomic.
#include "fim_engine.hpp"

namespace eik {

template <typename R>
struct Bits {
    using U = typename Real<R>::U;
    static constexpr U sign = U(1) << (8 * sizeof(U) - 1);
    static constexpr U inf = sizeof(R) == 8 ? (U)0x7ff0000000000000ull : (U)0x7f800000u;
    static __device__ __forceinline__ U of(R v) {
        if constexpr (sizeof(R) == 8) return (U)__double_as_longlong(v);
        else return __float_as_uint(v);
    }
    static __device__ __forceinline__ R val(U b) {
        if constexpr (sizeof(R) == 8) return __longlong_as_double((long long)b);
        else return __uint_as_float(b);
    }
};

// a tile the cone reaches: listed once (the reset kernel runs over this list only)
__device__ __forceinline__ void record_tile(const ReplanArgs& r, int tile) {
    if (__hip_atomic_load(&r.rflag[tile], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
    if (atomicExch(&r.rflag[tile], 1u) == 0u) {
        const unsigned long long pos = atomicAdd(&r.info[1], 1ull);
        r.rlist[pos] = tile;
    }
}

// qpush that counts the tiles it newly queued (info[3])
__device__ __forceinline__ void push_counted(const Fim2dArgs& a, const ReplanArgs& r, int tile, unsigned trig, float k) {
    unsigned kold = 0x7f800000u;
    const unsigned old = a.bctl ? qpush_issue_key(a, tile, trig, k, kold) : qpush_issue(a, tile, trig);
    qpush_complete(a, tile, old, k, kold);
    if ((old & (kPending | kBusy)) == 0u) atomicAdd(&r.info[3], 1ull);
}

// ------------------------------------------------------------------------------- prep
// The queue's control words, visit counters, slots, keys and per-tile state cleared as
// fim2d_init_kernel clears them, except that T and the edge columns stay and a tile keeps kVisited.
// phase 0 (before the flood): also the update's own words; phase 1 (before the restart): the
// flood's visit count is kept in info[2].
__global__ __launch_bounds__(256) void replan_prep_kernel(Fim2dArgs a, ReplanArgs r, int phase) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0) {
        const unsigned long long v = a.visits[0];
        __syncthreads();
        const int t = threadIdx.x;
        // (the visit counters too; a flood that failed keeps its error word: the solve's launch then
        // ends at once and reports it)
        if (t < (int)(kQueueCtlBytes / 4) && !(phase == 1 && t == 192 / 4)) reinterpret_cast<unsigned*>(a.qhead)[t] = 0u;
        if (t < 4) a.counts[t] = 0;
        if (t < 6 && phase == 0) r.info[t] = 0ull;
        if (t == 0 && phase == 1) r.info[2] = v;
    }
    for (int64_t i = i0; i < a.capacity; i += stride) {
        a.mark[i] = 0u;
        a.key[i] = 0x7f800000u;
        a.qstate[i] &= kVisited;
        if (phase == 0) r.rflag[i] = 0u;
    }
    for (int64_t i = i0; i <= (int64_t)a.qmask; i += stride) a.qslot[i] = 0u;
}

// ------------------------------------------------------------------------------- seed
// blockIdx.x: rectangle; blockIdx.y: a share of its cells and tiles
template <typename R>
__global__ __launch_bounds__(256) void replan_seed_kernel(Fim2dArgs a, ReplanArgs r) {
    using B = Bits<R>;
    using U = typename B::U;
    const ReplanRect q = r.rects[blockIdx.x];
    if (q.kind != kChangeAny) return;
    U* const Tb = static_cast<U*>(a.T);
    const int64_t gx = r.gx, gy = r.gy;
    const int64_t w = q.x1 - q.x0, n = w * (int64_t)(q.y1 - q.y0);
    const int64_t stride = (int64_t)gridDim.y * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < n; i += stride) {
        const int64_t y = q.y0 + i / w, x = q.x0 + i % w;
        if (x == gx && y == gy) continue;  // the goal is never a seed
        const U v = Tb[y * a.W + x];
        if (v < B::inf) {  // finite, not yet marked (by an overlapping rectangle)
            Tb[y * a.W + x] = v | B::sign;
            record_tile(r, (int)(y / kTile) * a.ntx + (int)(x / kTile));
        }
    }
    // the tiles of the rectangle dilated by one cell: a seed on a tile's edge is its neighbour's ring
    const int64_t dx0 = q.x0 > 0 ? q.x0 - 1 : 0, dy0 = q.y0 > 0 ? q.y0 - 1 : 0;
    const int64_t dx1 = q.x1 < a.W ? q.x1 : a.W - 1, dy1 = q.y1 < a.H ? q.y1 : a.H - 1;  // inclusive
    const int64_t tx0 = dx0 / kTile, ty0 = dy0 / kTile, ntx = dx1 / kTile - tx0 + 1, nty = dy1 / kTile - ty0 + 1;
    for (int64_t i = i0; i < ntx * nty; i += stride)
        qpush(a, (int)((ty0 + i / ntx) * a.ntx + tx0 + i % ntx), kSelf);
}

// ------------------------------------------------------------------------------- flood
template <typename R>
struct FloodLds {
    typename Real<R>::U t[kLds * kLds];  // bit patterns of the tile + ring; sign bit: in the cone
    int tile;
    unsigned chg, flags, any;
};

// One quadrant sweep of the marks, skewed like the solve's (lane l = column, step s = row s - l): the
// upstream y cell is the lane's own previous result, the upstream x cell lane l - 1's previous result
// through the DPP wave shift (lane 0: the ring column), both in registers -- the step's dependent
// chain has no LDS round trip.  The lane's own cells (and lane 0's ring cells) come from LDS a group
// of kFloodGroup steps ahead: a mark another wave sets meanwhile is a stale read, which only leaves
// work for the next pass (a pass that changed nothing wrote nothing, so its reads were exact).
// Marks travel along non-decreasing T, so one pass carries them along any path that is monotone in
// this quadrant's two directions.  Concurrent waves only ever OR the same bit into a cell.
constexpr int kFloodGroup = 8;
template <typename R, int DX, int DY>
__device__ __forceinline__ bool flood_sweep(typename Real<R>::U* t, int lane) {
    using B = Bits<R>;
    using U = typename B::U;
    static_assert((2 * kTile) % kFloodGroup == 0, "whole groups");
    const int x = (DX > 0 ? lane : kTile - 1 - lane) + 1;  // LDS column
    auto lrow = [](int k) { return (DY > 0 ? k : kTile - 1 - k) + 1; };  // LDS row of the sweep's k-th row
    bool changed = false;
    U cur = t[(DY > 0 ? 0 : kLds - 1) * kLds + x];  // the ring row upstream of the first row
#pragma unroll 1
    for (int s0 = 0; s0 < 2 * kTile; s0 += kFloodGroup) {
        U own[kFloodGroup], ring[kFloodGroup];
#pragma unroll
        for (int u = 0; u < kFloodGroup; ++u) {
            const int k = s0 + u - lane;
            const int kc = k < 0 ? 0 : k > kTile - 1 ? kTile - 1 : k;
            own[u] = t[lrow(kc) * kLds + x];
            ring[u] = t[lrow(kc) * kLds + x - DX];  // (lane 0's is the ring column, which no sweep writes)
        }
#pragma unroll
        for (int u = 0; u < kFloodGroup; ++u) {
            const int k = s0 + u - lane;
            const bool valid = k >= 0 && k < kTile;
            const U ux = B::of(wave_shr1(B::val(cur), B::val(ring[u]))), uy = cur;
            U v = own[u];
            const bool mx = (ux & B::sign) && (ux & ~B::sign) <= v;
            const bool my = (uy & B::sign) && (uy & ~B::sign) <= v;
            if (valid && v < B::inf && (mx || my)) {  // finite, unmarked, and a marked upstream cell at or below it
                v |= B::sign;
                t[lrow(k) * kLds + x] = v;
                changed = true;
            }
            cur = valid ? v : cur;
        }
    }
    return changed;
}

// Stage, flood and write back one tile; leaves the neighbour activations in L.flags (bits 0..3:
// N / S / W / E) and "marked something" in L.any.  Ends with every wave's stores drained and a
// workgroup barrier.
template <typename R>
__device__ __forceinline__ void flood_tile(const Fim2dArgs& a, const ReplanArgs& r, int tile, FloodLds<R>& L) {
    using B = Bits<R>;
    using U = typename B::U;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
    // (cell indices fit 32 bits: the persistent mode's rasters are below 2^32 bytes)
    const int y0 = ty * kTile, x0 = tx * kTile, H = (int)a.H, W = (int)a.W;
    const TMem<R, true> T(static_cast<R*>(a.T), a.H * a.W);
    // The goal is staged as +inf: it is never marked (p not the goal -- its T = 0 is the boundary
    // condition, and with zero costs beside it a tie 0 <= 0 would reach it), and as an unmarked cell it
    // hands no mark on, so to the flood it is a cell that is not there.
    const int ggx = (int)r.gx, ggy = (int)r.gy;
    // cell j of this thread: LDS index tid + j * kThreads; out of the raster and the ring's corners: +inf
    auto pos = [&](int i, unsigned& cell) {
        const int ly = i / kLds, lx = i - ly * kLds;
        const int gy = y0 + ly - 1, gx = x0 + lx - 1;
        const bool corner = (ly == 0 || ly == kLds - 1) && (lx == 0 || lx == kLds - 1);
        cell = (unsigned)gy * (unsigned)W + (unsigned)gx;
        return !corner && gy >= 0 && gy < H && gx >= 0 && gx < W && !(gx == ggx && gy == ggy);
    };
    // every global load of the visit is issued before the first LDS store (the compiler does not move
    // the sc1 buffer loads across LDS stores: interleaved, each would be a serial round trip)
    constexpr int kPer = (kLds * kLds + kThreads - 1) / kThreads;
    U st[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = tid + j * kThreads;
        unsigned cell;
        st[j] = B::inf;
        if (i < kLds * kLds && pos(i, cell)) st[j] = B::of(T.ld(cell));
    }
    unsigned mine = 0u;  // bit j: marked when staged
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = tid + j * kThreads;
        if (i < kLds * kLds) L.t[i] = st[j];
        if (st[j] & B::sign) mine |= 1u << j;
    }
    if (tid == 0) {
        L.flags = 0u;
        L.any = 0u;
        L.chg = 0u;
    }
    // no mark in the tile or on its ring (a tile queued for a seed rectangle's dilation, or for an
    // edge its neighbour's flood has since covered): nothing can spread
    if (!__syncthreads_or(mine != 0u)) return;
    for (;;) {
        bool ch;
        if (wave == 0)      ch = flood_sweep<R, +1, +1>(L.t, lane);
        else if (wave == 1) ch = flood_sweep<R, -1, +1>(L.t, lane);
        else if (wave == 2) ch = flood_sweep<R, +1, -1>(L.t, lane);
        else                ch = flood_sweep<R, -1, -1>(L.t, lane);
        if (__any(ch) && lane == 0) atomicOr(&L.chg, 1u);
        __syncthreads();
        const unsigned c = L.chg;
        __syncthreads();  // everyone has read it
        if (!c) break;    // uniform
        if (tid == 0) L.chg = 0u;
        __syncthreads();
    }
    // newly marked cells of the tile: stored, and tested against the ring where they lie on an edge
    // (the neighbour's adjacent cell as staged: finite and unmarked -- a stale "unmarked" only costs a
    // visit that finds nothing to do)
    unsigned fl = 0u;
    for (int i = tid, j = 0; i < kLds * kLds; i += kThreads, ++j) {
        const int ly = i / kLds, lx = i - ly * kLds;
        if (ly < 1 || ly > kTile || lx < 1 || lx > kTile) continue;
        const U v = L.t[i];
        if (!(v & B::sign) || ((mine >> j) & 1u)) continue;
        T.st((unsigned)(y0 + ly - 1) * (unsigned)W + (unsigned)(x0 + lx - 1), B::val(v));  // (marked => finite => inside the raster)
        fl |= 16u;
        const U m = v & ~B::sign;
        auto hit = [&](int h) { return L.t[h] < B::inf && m <= L.t[h]; };
        if (ly == 1 && hit(i - kLds)) fl |= 1u;
        if (ly == kTile && hit(i + kLds)) fl |= 2u;
        if (lx == 1 && hit(i - 1)) fl |= 4u;
        if (lx == kTile && hit(i + 1)) fl |= 8u;
    }
    if (fl & 15u) atomicOr(&L.flags, fl & 15u);
    if (fl & 16u) atomicOr(&L.any, 1u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

template <typename R>
__global__ __launch_bounds__(kThreads) void replan_flood_kernel(Fim2dArgs a, ReplanArgs r) {
    __shared__ FloodLds<R> L;
    // the flood's queue is the plain FIFO: stated here, the engine's band, fresh-first and live
    // branches fold away (and their kernel arguments leave the scalar registers: no spills)
    a.bctl = nullptr;
    a.fresh_first = 0;
    a.qhold = nullptr;
    int tile = -1;
    for (;;) {
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            if (tile >= 0) {  // retire the previous tile: activations, then the finish
                const unsigned f = L.flags;
                const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
                if (lane == 1 && (f & 1u) && ty > 0) qpush(a, tile - a.ntx, kFromS);
                if (lane == 2 && (f & 2u) && ty + 1 < a.nty) qpush(a, tile + a.ntx, kFromN);
                if (lane == 3 && (f & 4u) && tx > 0) qpush(a, tile - 1, kFromE);
                if (lane == 4 && (f & 8u) && tx + 1 < a.ntx) qpush(a, tile + 1, kFromW);
                if (lane == 0 && L.any) record_tile(r, tile);
                // the activations' counter increments complete before the finish decrements
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) {
                    qfinish(a, tile);
                    charge_visits(a, 1ull);  // the visit budget bounds the flood like a solve
                }
            }
            if (lane == 0) {
                unsigned trig = 0u;
                L.tile = qgrab(a, trig);
            }
        }
        __syncthreads();
        tile = L.tile;
        if (tile < 0) break;  // uniform: the flood has ended (or failed: qerror)
        flood_tile<R>(a, r, tile, L);
    }
}

// ------------------------------------------------------------------------------- reset
// Over the recorded tiles: marked cells -> +inf (counted in info[0]), the tile's edge-column copies
// rewritten from T, and the tile queued for the solve when a finite kept cell lies in it or on its
// ring -- keyed by the smallest such value.  A ring cell that its own tile's block is resetting at
// the same time reads as marked or as +inf: not kept either way.
template <typename R>
__global__ __launch_bounds__(kThreads) void replan_reset_kernel(Fim2dArgs a, ReplanArgs r) {
    using B = Bits<R>;
    using U = typename B::U;
    __shared__ U s_key;
    __shared__ unsigned s_cells;
    U* const Tb = static_cast<U*>(a.T);
    U* const Eb = static_cast<U*>(a.ecol);
    const int tid = threadIdx.x;
    const int count = (int)r.info[1];
    for (int it = blockIdx.x; it < count; it += gridDim.x) {
        const int tile = r.rlist[it];
        const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
        const int64_t y0 = (int64_t)ty * kTile, x0 = (int64_t)tx * kTile;
        if (tid == 0) {
            s_key = B::inf;
            s_cells = 0u;
        }
        __syncthreads();
        U kmin = B::inf;
        unsigned cells = 0u;
        for (int i = tid; i < kLds * kLds; i += kThreads) {
            const int ly = i / kLds, lx = i - ly * kLds;
            const int64_t gy = y0 + ly - 1, gx = x0 + lx - 1;
            const bool corner = (ly == 0 || ly == kLds - 1) && (lx == 0 || lx == kLds - 1);
            if (corner || gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) continue;
            const bool interior = ly >= 1 && ly <= kTile && lx >= 1 && lx <= kTile;
            U v = Tb[gy * a.W + gx];
            if (gx == r.gx && gy == r.gy) v &= ~B::sign;  // (never marked, and never reset: the source)
            if (v & B::sign) {
                v = B::inf;
                if (interior) {
                    Tb[gy * a.W + gx] = B::inf;
                    ++cells;
                }
            }
            if (interior && (lx == 1 || lx == kTile))
                Eb[((int64_t)tile * 2 + (lx == 1 ? 0 : 1)) * kTile + ly - 1] = v;
            kmin = v < kmin ? v : kmin;
        }
        if (kmin < B::inf) atomicMin(&s_key, kmin);
        if (cells) atomicAdd(&s_cells, cells);
        __syncthreads();
        if (tid == 0) {
            atomicAdd(&r.info[0], (unsigned long long)s_cells);
            if (s_cells && s_key < B::inf) push_counted(a, r, tile, kSelf | kVisited, (float)B::val(s_key));
        }
        __syncthreads();
    }
}

// Every tile overlapping a rectangle of either kind: queued for the solve when one of the
// rectangle's cells in it has a finite cost and a finite kept 4-neighbour, keyed by the smallest such
// neighbour.  Runs after the reset kernel (marked cells are +inf by now).  blockIdx.x: rectangle.
template <typename R>
__global__ __launch_bounds__(kThreads) void replan_rects_kernel(Fim2dArgs a, ReplanArgs r) {
    using B = Bits<R>;
    using U = typename B::U;
    __shared__ U s_key;
    const ReplanRect q = r.rects[blockIdx.x];
    const U* const Tb = static_cast<const U*>(a.T);
    const R* const cost = static_cast<const R*>(a.cost);
    const int tid = threadIdx.x;
    const int64_t tx0 = q.x0 / kTile, ty0 = q.y0 / kTile;
    const int64_t ntx = (q.x1 - 1) / kTile - tx0 + 1, nty = (q.y1 - 1) / kTile - ty0 + 1;
    for (int64_t t = blockIdx.y; t < ntx * nty; t += gridDim.y) {
        const int64_t ty = ty0 + t / ntx, tx = tx0 + t % ntx;
        const int64_t xa = q.x0 > tx * kTile ? q.x0 : tx * kTile, xb = q.x1 < (tx + 1) * kTile ? q.x1 : (tx + 1) * kTile;
        const int64_t ya = q.y0 > ty * kTile ? q.y0 : ty * kTile, yb = q.y1 < (ty + 1) * kTile ? q.y1 : (ty + 1) * kTile;
        if (tid == 0) s_key = B::inf;
        __syncthreads();
        U kmin = B::inf;
        const int w = (int)(xb - xa), n = w * (int)(yb - ya);
        for (int i = tid; i < n; i += kThreads) {
            const int64_t y = ya + i / w, x = xa + i % w;
            if (!(cost[y * a.W + x] < Real<R>::inf())) continue;
            auto nb = [&](int64_t yy, int64_t xx) {
                if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) return;
                const U v = Tb[yy * a.W + xx];
                kmin = v < kmin ? v : kmin;  // (no marked cell is left: the bit patterns are values)
            };
            nb(y - 1, x);
            nb(y + 1, x);
            nb(y, x - 1);
            nb(y, x + 1);
        }
        if (kmin < B::inf) atomicMin(&s_key, kmin);
        __syncthreads();
        if (tid == 0 && s_key < B::inf)
            push_counted(a, r, (int)(ty * a.ntx + tx), kSelf | kVisited, (float)B::val(s_key));
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------- adopt
// A field the caller states is converged: the edge-column copies built from T, kVisited on every
// tile with a finite cell (a tile without it skips its first T read, fim2d.hip kFreshSkip).
template <typename R>
__global__ __launch_bounds__(kThreads) void replan_adopt_kernel(Fim2dArgs a) {
    using B = Bits<R>;
    using U = typename B::U;
    __shared__ unsigned s_fin;
    const U* const Tb = static_cast<const U*>(a.T);
    U* const Eb = static_cast<U*>(a.ecol);
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < a.capacity; tile += gridDim.x) {
        const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
        const int64_t y0 = (int64_t)ty * kTile, x0 = (int64_t)tx * kTile;
        if (tid == 0) s_fin = 0u;
        __syncthreads();
        bool fin = false;
        for (int i = tid; i < kTile * kTile; i += kThreads) {
            const int ry = i / kTile, cx = i - ry * kTile;
            const int64_t gy = y0 + ry, gx = x0 + cx;
            const U v = gy < a.H && gx < a.W ? Tb[gy * a.W + gx] : B::inf;
            fin |= v < B::inf;
            if (cx == 0 || cx == kTile - 1) Eb[((int64_t)tile * 2 + (cx == 0 ? 0 : 1)) * kTile + ry] = v;
        }
        if (fin) atomicOr(&s_fin, 1u);
        __syncthreads();
        if (tid == 0) a.qstate[tile] = s_fin ? kVisited : 0u;
        __syncthreads();
    }
}

// ------------------------------------------------------------- seed sets
// The re-solve of a field that a seed LIST produced (eik_fim2d_update_seeds), for a list that may have
// changed with the cost.  Roots take the goal's place.  The host's diff (seed_diff.cpp) names every
// distinct cell of the old list with b_old, the smallest (R)t0 of the old seeds on it, and its class:
// keep (b_new <= b_old) or release.  With r.gx = r.gy = -1 the goal tests above never fire, and three
// plain grid kernels around them, ordered by the stream, make the kernels above see what they need:
//
//   roots    before the seed kernel.  An entry whose cell does not hold b_old bit for bit is a dominated
//            seed, an ordinary cell: nothing.  A kept ROOT is lifted to +inf -- to the seed kernel and
//            the flood a cell that is not there, never marked and handing no mark on, as the staged goal
//            is -- and the entry is flagged.  A released root is a cone seed like a finite cell of an ANY
//            rectangle: sign bit, its tile recorded, the tiles of the cell dilated by one queued.
//   unlift   after the flood, before the reset: flagged entries get b_old back, so that the reset and
//            the rectangles kernel find the spared roots as finite kept cells, key their pushes by them
//            and rewrite the edge columns with the roots in them.
//   reseed   after the rectangles kernel, one thread per seed of the NEW list: T = min(T, b_new) on the
//            bit pattern (and the edge column's copy); only a seed that lowered its cell queues its tile
//            and the neighbours across the sides it lies on, as fim2d_seeds_kernel does.
template <typename R>
__global__ __launch_bounds__(256) void replan_roots_kernel(Fim2dArgs a, ReplanArgs r, RootDesc* __restrict__ roots, int n) {
    using B = Bits<R>;
    using U = typename B::U;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const RootDesc d = roots[k];
    // (the host checked: 0 <= x < W, 0 <= y < H; one entry per cell, so no two threads share one)
    U* const p = static_cast<U*>(a.T) + ((int64_t)d.y * a.W + d.x);
    const U v = *p;
    if (v != B::of((R)d.b_old)) return;  // undercut by another seed's wave: not a root
    if (d.cls == kRootKeep) {
        *p = B::inf;
        roots[k].lifted = 1u;
        return;
    }
    *p = v | B::sign;
    const int ty = d.y / kTile, tx = d.x / kTile, ry = d.y % kTile, cx = d.x % kTile;
    const int tile = ty * a.ntx + tx;
    record_tile(r, tile);
    qpush(a, tile, kSelf);
    // a root on a tile's edge lies on its neighbour's ring
    if (ry == 0 && ty > 0) qpush(a, tile - a.ntx, kSelf);
    if (ry == kTile - 1 && ty + 1 < a.nty) qpush(a, tile + a.ntx, kSelf);
    if (cx == 0 && tx > 0) qpush(a, tile - 1, kSelf);
    if (cx == kTile - 1 && tx + 1 < a.ntx) qpush(a, tile + 1, kSelf);
}

template <typename R>
__global__ __launch_bounds__(256) void replan_unlift_kernel(Fim2dArgs a, const RootDesc* __restrict__ roots, int n) {
    using B = Bits<R>;
    using U = typename B::U;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const RootDesc d = roots[k];
    if (d.lifted) static_cast<U*>(a.T)[(int64_t)d.y * a.W + d.x] = B::of((R)d.b_old);
}

template <typename R>
__global__ __launch_bounds__(256) void replan_reseed_kernel(Fim2dArgs a, ReplanArgs r, const SeedDesc* __restrict__ seeds, int K) {
    using B = Bits<R>;
    using U = typename B::U;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const SeedDesc s = seeds[k];
    // (the host checked: inside the raster, t0 finite, >= 0 and rounded to R; one map, persistent mode)
    const R t0 = (R)s.t0;
    const U bits = B::of(t0);
    const int cx = s.x % kTile, ry = s.y % kTile;
    const int tile = (s.y / kTile) * a.ntx + s.x / kTile;
    const U old = atomicMin(static_cast<U*>(a.T) + ((int64_t)s.y * a.W + s.x), bits);
    if (a.ecol && (cx == 0 || cx == kTile - 1))
        atomicMin(static_cast<U*>(a.ecol) + (((int64_t)tile * 2 + (cx == 0 ? 0 : 1)) * kTile + ry), bits);
    if (!(old > bits)) return;  // lowered nothing: queues nothing
    const float key = (float)t0;
    push_counted(a, r, tile, kSelf | kVisited, key);
    activate_seed_sides(a, tile, ry, cx, kTile, key);
}

// ------------------------------------------------------------------------- host launchers
hipError_t replan_prep(const Fim2dArgs& a, const ReplanArgs& r, int phase, hipStream_t st) {
    static_assert(kQueueCtlBytes / 4 <= 256, "block 0 clears the queue words");
    const int64_t n = std::max<int64_t>(a.capacity, (int64_t)a.qmask + 1);
    hipLaunchKernelGGL(replan_prep_kernel, dim3((int)std::min<int64_t>(256, (n + 255) / 256)), dim3(256), 0, st, a, r, phase);
    return hipGetLastError();
}

hipError_t replan_seed(const Fim2dArgs& a, const ReplanArgs& r, bool f64, hipStream_t st) {
    if (r.K < 1) return hipSuccess;  // (a seeded update with released roots and no rectangle)
    if (f64)
        hipLaunchKernelGGL(replan_seed_kernel<double>, dim3(r.K, 32), dim3(256), 0, st, a, r);
    else
        hipLaunchKernelGGL(replan_seed_kernel<float>, dim3(r.K, 32), dim3(256), 0, st, a, r);
    return hipGetLastError();
}

int replan_flood_resident(bool f64, int cus) {
    int per_cu = 0;
    const hipError_t e = f64 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, replan_flood_kernel<double>, kThreads, 0)
                             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, replan_flood_kernel<float>, kThreads, 0);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    return per_cu * cus;
}

hipError_t replan_flood(const Fim2dArgs& a, const ReplanArgs& r, bool f64, int grid, hipStream_t st) {
    if (f64)
        hipLaunchKernelGGL(replan_flood_kernel<double>, dim3(grid), dim3(kThreads), 0, st, a, r);
    else
        hipLaunchKernelGGL(replan_flood_kernel<float>, dim3(grid), dim3(kThreads), 0, st, a, r);
    return hipGetLastError();
}

hipError_t replan_reset(const Fim2dArgs& a, const ReplanArgs& r, bool f64, hipStream_t st) {
    const int grid = (int)std::min<int64_t>(1024, a.capacity);
    if (f64) {
        hipLaunchKernelGGL(replan_reset_kernel<double>, dim3(grid), dim3(kThreads), 0, st, a, r);
        if (r.K > 0) hipLaunchKernelGGL(replan_rects_kernel<double>, dim3(r.K, 16), dim3(kThreads), 0, st, a, r);
    } else {
        hipLaunchKernelGGL(replan_reset_kernel<float>, dim3(grid), dim3(kThreads), 0, st, a, r);
        if (r.K > 0) hipLaunchKernelGGL(replan_rects_kernel<float>, dim3(r.K, 16), dim3(kThreads), 0, st, a, r);
    }
    return hipGetLastError();
}

hipError_t replan_adopt(const Fim2dArgs& a, bool f64, hipStream_t st) {
    const int grid = (int)std::min<int64_t>(4096, a.capacity);
    if (f64)
        hipLaunchKernelGGL(replan_adopt_kernel<double>, dim3(grid), dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(replan_adopt_kernel<float>, dim3(grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t replan_roots(const Fim2dArgs& a, const ReplanArgs& r, bool f64, RootDesc* d_roots, int64_t n, hipStream_t st) {
    const int grid = (int)((n + 255) / 256);
    if (f64)
        hipLaunchKernelGGL(replan_roots_kernel<double>, dim3(grid), dim3(256), 0, st, a, r, d_roots, (int)n);
    else
        hipLaunchKernelGGL(replan_roots_kernel<float>, dim3(grid), dim3(256), 0, st, a, r, d_roots, (int)n);
    return hipGetLastError();
}

hipError_t replan_unlift(const Fim2dArgs& a, bool f64, const RootDesc* d_roots, int64_t n, hipStream_t st) {
    const int grid = (int)((n + 255) / 256);
    if (f64)
        hipLaunchKernelGGL(replan_unlift_kernel<double>, dim3(grid), dim3(256), 0, st, a, d_roots, (int)n);
    else
        hipLaunchKernelGGL(replan_unlift_kernel<float>, dim3(grid), dim3(256), 0, st, a, d_roots, (int)n);
    return hipGetLastError();
}

hipError_t replan_reseed(const Fim2dArgs& a, const ReplanArgs& r, bool f64, const SeedDesc* d_seeds, int64_t K, hipStream_t st) {
    const int grid = (int)((K + 255) / 256);
    if (f64)
        hipLaunchKernelGGL(replan_reseed_kernel<double>, dim3(grid), dim3(256), 0, st, a, r, d_seeds, (int)K);
    else
        hipLaunchKernelGGL(replan_reseed_kernel<float>, dim3(grid), dim3(256), 0, st, a, r, d_seeds, (int)K);
    return hipGetLastError();
}

}  // namespace eik
