// cost_diff.hip -- what changed between two cost rasters, per solver tile.
//
// cost_diff_tiles_kernel: one workgroup of 256 threads per 64 x 64 tile, each wave 16 rows; both rasters
// are read once, 16 bytes per lane, and every tile writes its own 32-byte record -- no atomics, no
// cross-workgroup traffic, a deterministic function of the two rasters.  cost_diff_compact_kernel: one
// workgroup, an ordered scan of the records into the totals and the changed tiles' list.
// Plain grid launches only.
#include <hip/hip_runtime.h>

#include <climits>

#include "eik_common.hpp"
#include "eik_kernels.hpp"

namespace eik {

namespace {

constexpr int kDiffWaves = kThreads / 64;       // 4
constexpr int kDiffRows = kTile / kDiffWaves;   // rows of a tile per wave: 16

template <typename R, int V>
struct DiffVec;  // V cells of R in one load
template <>
struct DiffVec<double, 2> {
    typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct DiffVec<float, 4> {
    typedef float type __attribute__((ext_vector_type(4)));
};
template <typename R>
struct DiffVec<R, 1> {
    typedef R type;
};

template <typename R, int V>
__device__ __forceinline__ R diff_lane(const typename DiffVec<R, V>::type& v, int j) {
    if constexpr (V == 1)
        return v;
    else
        return v[j];
}

template <bool NT, typename T>
__device__ __forceinline__ T diff_load(const T* p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

// per-lane state of the tile's reduction: the box as min / max cell (inclusive), and the counts
struct DiffAcc {
    int x0, y0, x1, y1;
    unsigned changed, raised, invalid;
};

__device__ __forceinline__ void diff_wave_reduce(DiffAcc& a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a.x0 = min(a.x0, __shfl_xor(a.x0, m));
        a.y0 = min(a.y0, __shfl_xor(a.y0, m));
        a.x1 = max(a.x1, __shfl_xor(a.x1, m));
        a.y1 = max(a.y1, __shfl_xor(a.y1, m));
        a.changed += __shfl_xor(a.changed, m);
        a.raised += __shfl_xor(a.raised, m);
        a.invalid += __shfl_xor(a.invalid, m);
    }
}

// V cells per lane and load: a row of the tile takes 64 / V lanes, a wave covers V rows per load and its
// 16 rows in 16 / V loads per raster, four of them issued before their compares.  V > 1 needs W % V == 0 and
// 16-byte aligned rasters (the launcher checks): a vector then lies wholly inside or outside the raster.
template <typename R, int V, bool NT>
__global__ __launch_bounds__(kThreads) void cost_diff_tiles_kernel(const R* __restrict__ old_c, const R* __restrict__ new_c,
                                                                   int64_t H, int64_t W, int ntx,
                                                                   DiffRecord* __restrict__ rec) {
    typedef typename DiffVec<R, V>::type Vec;
    constexpr int kLanesRow = kTile / V;  // lanes per tile row
    constexpr int kLoads = kDiffRows / V;
    constexpr int kBatch = kLoads < 4 ? kLoads : 4;
    __shared__ DiffAcc part[kDiffWaves];
    const int tile = blockIdx.x;
    const int tx = tile % ntx, ty = tile / ntx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t x = (int64_t)tx * kTile + (lane % kLanesRow) * V;
    const int64_t yb = (int64_t)ty * kTile + wave * kDiffRows + lane / kLanesRow;
    const bool xin = x < W;  // (the whole vector: W % V == 0)

    DiffAcc a{INT_MAX, INT_MAX, -1, -1, 0u, 0u, 0u};
    // kBatch loads per raster in flight per lane, then their compares (all 16 / V at once cost fp64 236 VGPRs)
#pragma unroll 1
    for (int b0 = 0; b0 < kLoads; b0 += kBatch) {
        Vec vo[kBatch], vn[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            const int64_t y = yb + (int64_t)(b0 + i) * V;
            if (xin && y < H) {
                const int64_t off = y * W + x;
                vo[i] = diff_load<NT>(reinterpret_cast<const Vec*>(old_c + off));
                vn[i] = diff_load<NT>(reinterpret_cast<const Vec*>(new_c + off));
            } else {  // a cut tile's cells past the south / east edge: equal and valid
                vo[i] = Vec(0);
                vn[i] = Vec(0);
            }
        }
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            const int y = (int)(yb + (int64_t)(b0 + i) * V);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const R o = diff_lane<R, V>(vo[i], j), n = diff_lane<R, V>(vn[i], j);
                const bool inv = !(n >= R(0));    // NaN or negative (-0 is valid)
                const bool ch = (o != n) || inv;  // as values: +0 == -0, inf == inf, NaN differs from all
                if (ch) {
                    const int xc = (int)x + j;
                    a.x0 = min(a.x0, xc);
                    a.x1 = max(a.x1, xc);
                    a.y0 = min(a.y0, y);
                    a.y1 = max(a.y1, y);
                }
                a.changed += ch;
                a.raised += n > o;
                a.invalid += inv;
            }
        }
    }
    diff_wave_reduce(a);
    if (lane == 0) part[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kDiffWaves; ++w) {
            const DiffAcc b = part[w];
            a.x0 = min(a.x0, b.x0);
            a.y0 = min(a.y0, b.y0);
            a.x1 = max(a.x1, b.x1);
            a.y1 = max(a.y1, b.y1);
            a.changed += b.changed;
            a.raised += b.raised;
            a.invalid += b.invalid;
        }
        DiffRecord r;
        const bool any = a.changed != 0;
        r.x0 = any ? a.x0 : 0;
        r.y0 = any ? a.y0 : 0;
        r.x1 = any ? a.x1 + 1 : 0;
        r.y1 = any ? a.y1 + 1 : 0;
        r.changed = a.changed;
        r.raised = a.raised;
        r.invalid = a.invalid;
        r.tile = tile;
        rec[tile] = r;  // one 32-byte struct store
    }
}

// One workgroup: chunks of kCompactThreads records in tile order; a changed record's slot in the list is
// the changed records before it (the chunks before, then a ballot + LDS scan inside the chunk).
constexpr int kCompactThreads = 1024;
__global__ __launch_bounds__(kCompactThreads) void cost_diff_compact_kernel(const DiffRecord* __restrict__ rec, int tiles,
                                                                            DiffRecord* __restrict__ out) {
    constexpr int kWaves = kCompactThreads / 64;
    __shared__ unsigned wcount[kWaves];
    __shared__ unsigned long long tot[kWaves][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned base = 0;  // changed tiles of the chunks before (the same in every thread)
    unsigned long long changed = 0, raised = 0, invalid = 0;
    for (int c0 = 0; c0 < tiles; c0 += kCompactThreads) {
        const int i = c0 + (int)threadIdx.x;
        DiffRecord r{};
        if (i < tiles) r = rec[i];
        const bool flag = r.changed != 0;
        const unsigned long long bal = __ballot(flag);
        if (lane == 0) wcount[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const unsigned n = wcount[w];
            before += w < wave ? n : 0u;
            all += n;
        }
        if (flag) {
            const unsigned slot = base + before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
            out[1 + slot] = r;
            changed += r.changed;
            raised += r.raised;
            invalid += r.invalid;
        }
        base += all;
        __syncthreads();  // wcount is rewritten by the next chunk
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        changed += __shfl_xor(changed, m);
        raised += __shfl_xor(raised, m);
        invalid += __shfl_xor(invalid, m);
    }
    if (lane == 0) {
        tot[wave][0] = changed;
        tot[wave][1] = raised;
        tot[wave][2] = invalid;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        DiffHeader h{0, 0, 0, base};
        for (int w = 0; w < kWaves; ++w) {
            h.changed += tot[w][0];
            h.raised += tot[w][1];
            h.invalid += tot[w][2];
        }
        *reinterpret_cast<DiffHeader*>(out) = h;
    }
}

template <typename R, int V>
hipError_t launch_tiles(const void* d_old, const void* d_new, int64_t H, int64_t W, int ntx, int nty, DiffRecord* rec, bool nt,
                        hipStream_t st) {
    const dim3 grid((unsigned)(ntx * nty)), block(kThreads);
    if (nt)
        hipLaunchKernelGGL((cost_diff_tiles_kernel<R, V, true>), grid, block, 0, st, (const R*)d_old, (const R*)d_new, H, W, ntx,
                           rec);
    else
        hipLaunchKernelGGL((cost_diff_tiles_kernel<R, V, false>), grid, block, 0, st, (const R*)d_old, (const R*)d_new, H, W,
                           ntx, rec);
    return hipGetLastError();
}

}  // namespace

hipError_t cost_diff_tiles(const void* d_old, const void* d_new, bool f64, int64_t H, int64_t W, int ntx, int nty,
                           DiffRecord* rec, bool nt, hipStream_t st) {
    if (H < 1 || W < 1 || ntx != (W + kTile - 1) / kTile || nty != (H + kTile - 1) / kTile) return hipErrorInvalidValue;
    const size_t cell = f64 ? 8 : 4;
    const bool wide = (((uintptr_t)d_old | (uintptr_t)d_new) & 15u) == 0 && (W * cell) % 16 == 0;
    if (f64) return wide ? launch_tiles<double, 2>(d_old, d_new, H, W, ntx, nty, rec, nt, st)
                         : launch_tiles<double, 1>(d_old, d_new, H, W, ntx, nty, rec, nt, st);
    return wide ? launch_tiles<float, 4>(d_old, d_new, H, W, ntx, nty, rec, nt, st)
                : launch_tiles<float, 1>(d_old, d_new, H, W, ntx, nty, rec, nt, st);
}

hipError_t cost_diff_compact(const DiffRecord* rec, int tiles, DiffRecord* out, hipStream_t st) {
    if (tiles < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cost_diff_compact_kernel, dim3(1), dim3(kCompactThreads), 0, st, rec, tiles, out);
    return hipGetLastError();
}

}  // namespace eik
