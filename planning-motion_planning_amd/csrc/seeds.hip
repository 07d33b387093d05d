// seeds.hip -- multi-source 2D solves: a solve seeded from a SET of cells, each with
// a start value T0 >= 0, and the nearest-seed label of every cell of the converged field.
//
// The sweep itself needs nothing new: a write-back keeps min(old, new) and no visit treats a source
// cell specially, so the field of a seed set is the fixed point the ordinary solve reaches from
// "T = +inf, T[seed k] = min T0_k".  Everything is in how the solve is seeded:
//
//   fim2d_seeds_kernel   after fim2d_init with no goal (T = +inf, queue and marks cleared): one thread
//                        per seed lowers T (and the tile's edge-column copy) to T0 with an atomic min on
//                        the bit pattern, and activates the seed's tile -- and the neighbour across every
//                        tile side the seed lies on -- with key T0.
//
// and one post-pass on the converged field:
//
//   labels               label[c] = the seed whose wave reached c first, by the rule of include/eikonal.h:
//                        parents (the lowest strictly lower 4-neighbour), roots (seeds that hold their
//                        own T0), pointer jumping to the roots, a gather of the roots' labels.
//   labels3d             the same rule on a volume with 6 neighbours (§3.16; its seeding is fim3d.hip's):
//                        parent and root kernels of its own, the jumping and the gather shared.
#include "fim_engine.hpp"

namespace eik {

template <typename R>
struct SeedBits {
    using U = typename Real<R>::U;
    static __device__ __forceinline__ U of(R v) {
        if constexpr (sizeof(R) == 8) return (U)__double_as_longlong(v);
        else return __float_as_uint(v);
    }
};

// ------------------------------------------------------------------------------- seeding
// One thread per seed.  T0 >= 0, so values order like their bit patterns and the atomic min is an
// unsigned one: of two seeds on one cell the lower holds, in any order of arrival.  The pushes are
// the engine's own (qpush / enqueue): a tile named by several seeds, or activated from a neighbour's
// seed and holding its own, ends with the OR of the triggers and ONE queue entry -- only the push that
// finds the state word without kPending queues it (qpush_complete); with priority bands a later push
// a whole band lower adds its decrease-key entry, as any activation does.  kVisited: a tile without it
// skips its first T read (fim2d.hip kFreshSkip) and would lose the seed.
template <typename R>
__global__ __launch_bounds__(256) void fim2d_seeds_kernel(Fim2dArgs a, const SeedDesc* __restrict__ seeds, int K) {
    using U = typename SeedBits<R>::U;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const SeedDesc s = seeds[k];
    // (the host checked: 0 <= x < W, 0 <= y < H, 0 <= map < B, t0 finite and >= 0 in R)
    const R t0 = (R)s.t0;
    const U bits = SeedBits<R>::of(t0);
    const int cx = s.x % kTile, ry = s.y % kTile;
    const int tile = s.map * a.tiles_per_map + (s.y / kTile) * a.ntx + s.x / kTile;
    atomicMin(static_cast<U*>(a.T) + ((int64_t)s.map * a.H * a.W + (int64_t)s.y * a.W + s.x), bits);
    // the edge columns' copy (read by the solvers that keep one, fim2d.hip kEcol; the others never look)
    if (a.ecol && (cx == 0 || cx == kTile - 1))
        atomicMin(static_cast<U*>(a.ecol) + (((int64_t)tile * 2 + (cx == 0 ? 0 : 1)) * kTile + ry), bits);
    const float key = (float)t0;  // (a double past the float range: +inf, the last band)
    if (a.mode == kModePersistent) {
        qpush(a, tile, kSelf | kVisited, key);
    } else {
        atomicMin(&a.key[tile], __float_as_uint(key));
        if (atomicMax(&a.mark[tile], 1u) < 1u) {  // onto list 0 once
            const int pos = atomicAdd(&a.counts[0], 1);
            a.lists[pos] = tile;
        }
    }
    activate_seed_sides(a, tile, ry, cx, kTile, key);
}

// ------------------------------------------------------------------------------- labels
// Cell i of the B maps: its parent (itself: no parent) and label -1.
template <typename R>
__global__ __launch_bounds__(256) void labels_parent_kernel(LabelArgs l) {
    const R* const T = static_cast<const R*>(l.T);
    const int64_t hw = l.H * l.W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < l.n; i += stride) {
        const int64_t r = i % hw;
        const int64_t y = r / l.W, x = r - y * l.W;
        const R t = T[i];
        R best = t;
        int64_t p = i;
        if (t < Real<R>::inf()) {
            // the smallest neighbour strictly below t; of equal ones the first of x-1, x+1, y-1, y+1
            auto nb = [&](bool in, int64_t j) {
                if (!in) return;
                const R v = T[j];
                if (v < best) {
                    best = v;
                    p = j;
                }
            };
            nb(x > 0, i - 1);
            nb(x + 1 < l.W, i + 1);
            nb(y > 0, i - l.W);
            nb(y + 1 < l.H, i + l.W);
        }
        l.par[i] = (int)p;
        l.label[i] = -1;
    }
}

// Seed k is a root when T at its cell is its T0 bit for bit: the cell is its own parent and takes the
// lowest such k (an unsigned min: -1 is the largest).
template <typename R>
__global__ __launch_bounds__(256) void labels_root_kernel(LabelArgs l) {
    using U = typename SeedBits<R>::U;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= l.K) return;
    const SeedDesc s = l.seeds[k];
    const int64_t i = (int64_t)s.map * l.H * l.W + (int64_t)s.y * l.W + s.x;
    if (static_cast<const U*>(l.T)[i] != SeedBits<R>::of((R)s.t0)) return;  // undercut by another seed's wave
    l.par[i] = (int)i;
    atomicMin(reinterpret_cast<unsigned*>(l.label) + i, (unsigned)k);
}

// Pointer jumping, pass p: par[i] = par[par[i]], in place.  A value read may be this pass's or the
// last one's -- either is an ancestor at least as far as the last pass left it, so after pass p every
// cell points at its chain's end or at least 2^(p+1) links up, and ceil(log2(H W)) passes reach the
// ends of the longest possible chain.  The host launches that many; a pass that finds the flag of the
// pass before it clear (nothing moved: every cell points at its chain's end) returns at once.
__global__ __launch_bounds__(256) void labels_jump_kernel(LabelArgs l, int pass) {
    if (pass > 0 && l.flags[pass - 1] == 0u) return;  // uniform across the launch
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool moved = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < l.n; i += stride) {
        const int q = l.par[i];
        if (q == (int)i) continue;
        const int g = l.par[q];
        if (g != q) {
            l.par[i] = g;
            moved = true;
        }
    }
    if (__any(moved) && (threadIdx.x & 63) == 0) l.flags[pass] = 1u;
}

// label[i] = label[chain's end].  In place: an end is its own parent and keeps its value (a root's
// label, or -1 for a cell with no strictly lower neighbour), and only ends are read.
__global__ __launch_bounds__(256) void labels_gather_kernel(LabelArgs l) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < l.n; i += stride) {
        const int q = l.par[i];
        if (q != (int)i) l.label[i] = l.label[q];
    }
}

// ------------------------------------------------------------------------------- labels, 3D
// The same rule on one [H][W][L] volume (z fastest) with 6 neighbours.  Only the parents
// and the roots know the dimension: pointer jumping and the gather above work on cell indices.
// Cell i: its parent (itself: no parent) and label -1.
template <typename R>
__global__ __launch_bounds__(256) void labels3d_parent_kernel(Label3Args l) {
    const R* const T = static_cast<const R*>(l.T);
    const int64_t wl = l.W * l.L;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < l.n; i += stride) {
        const int64_t z = i % l.L, xy = i / l.L, x = xy % l.W, y = xy / l.W;
        const R t = T[i];
        R best = t;
        int64_t p = i;
        if (t < Real<R>::inf()) {
            // the smallest neighbour strictly below t; of equal ones the first of x-1, x+1, y-1, y+1, z-1,
            // z+1 (the order of fim3d.hip's faces)
            auto nb = [&](bool in, int64_t j) {
                if (!in) return;
                const R v = T[j];
                if (v < best) {
                    best = v;
                    p = j;
                }
            };
            nb(x > 0, i - l.L);
            nb(x + 1 < l.W, i + l.L);
            nb(y > 0, i - wl);
            nb(y + 1 < l.H, i + wl);
            nb(z > 0, i - 1);
            nb(z + 1 < l.L, i + 1);
        }
        l.par[i] = (int)p;
        l.label[i] = -1;
    }
}

// Seed k is a root when T at its cell is its T0 bit for bit (labels_root_kernel's rule)
template <typename R>
__global__ __launch_bounds__(256) void labels3d_root_kernel(Label3Args l) {
    using U = typename SeedBits<R>::U;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= l.K) return;
    const Seed3Desc s = l.seeds[k];
    const int64_t i = (s.y * l.W + s.x) * l.L + s.z;
    if (static_cast<const U*>(l.T)[i] != SeedBits<R>::of((R)s.t0)) return;  // undercut by another seed's wave
    l.par[i] = (int)i;
    atomicMin(reinterpret_cast<unsigned*>(l.label) + i, (unsigned)k);
}

// ------------------------------------------------------------------------- host launchers
int labels3d_passes(int64_t n) {
    int p = 1;
    while (p < kLabelPasses && (1ll << p) < n) ++p;
    return p;
}

hipError_t labels3d(const Label3Args& l, bool f64, hipStream_t st) {
    hipError_t e = hipMemsetAsync(l.flags, 0, sizeof(unsigned) * kLabelPasses, st);
    if (e != hipSuccess) return e;
    const int grid = (int)std::min<int64_t>(8192, (l.n + 255) / 256);
    const int kgrid = (l.K + 255) / 256;
    if (f64) {
        hipLaunchKernelGGL(labels3d_parent_kernel<double>, dim3(grid), dim3(256), 0, st, l);
        hipLaunchKernelGGL(labels3d_root_kernel<double>, dim3(kgrid), dim3(256), 0, st, l);
    } else {
        hipLaunchKernelGGL(labels3d_parent_kernel<float>, dim3(grid), dim3(256), 0, st, l);
        hipLaunchKernelGGL(labels3d_root_kernel<float>, dim3(kgrid), dim3(256), 0, st, l);
    }
    // the dimension-free half: the jump and gather kernels read par, label, flags and n only
    LabelArgs j{};
    j.n = l.n;
    j.par = l.par;
    j.label = l.label;
    j.flags = l.flags;
    const int passes = labels3d_passes(l.n);
    for (int p = 0; p < passes; ++p) hipLaunchKernelGGL(labels_jump_kernel, dim3(grid), dim3(256), 0, st, j, p);
    hipLaunchKernelGGL(labels_gather_kernel, dim3(grid), dim3(256), 0, st, j);
    return hipGetLastError();
}

hipError_t fim2d_start_seeds(const Fim2dArgs& a, bool f64, const SeedDesc* d_seeds, int64_t K, hipStream_t st) {
    const int grid = (int)((K + 255) / 256);
    if (f64)
        hipLaunchKernelGGL(fim2d_seeds_kernel<double>, dim3(grid), dim3(256), 0, st, a, d_seeds, (int)K);
    else
        hipLaunchKernelGGL(fim2d_seeds_kernel<float>, dim3(grid), dim3(256), 0, st, a, d_seeds, (int)K);
    return hipGetLastError();
}

int labels2d_passes(int64_t H, int64_t W) {
    int p = 1;
    while (p < kLabelPasses && (1ll << p) < H * W) ++p;
    return p;
}

hipError_t labels2d(const LabelArgs& l, bool f64, hipStream_t st) {
    hipError_t e = hipMemsetAsync(l.flags, 0, sizeof(unsigned) * kLabelPasses, st);
    if (e != hipSuccess) return e;
    const int grid = (int)std::min<int64_t>(8192, (l.n + 255) / 256);
    const int kgrid = (l.K + 255) / 256;
    if (f64) {
        hipLaunchKernelGGL(labels_parent_kernel<double>, dim3(grid), dim3(256), 0, st, l);
        hipLaunchKernelGGL(labels_root_kernel<double>, dim3(kgrid), dim3(256), 0, st, l);
    } else {
        hipLaunchKernelGGL(labels_parent_kernel<float>, dim3(grid), dim3(256), 0, st, l);
        hipLaunchKernelGGL(labels_root_kernel<float>, dim3(kgrid), dim3(256), 0, st, l);
    }
    const int passes = labels2d_passes(l.H, l.W);
    for (int p = 0; p < passes; ++p) hipLaunchKernelGGL(labels_jump_kernel, dim3(grid), dim3(256), 0, st, l, p);
    hipLaunchKernelGGL(labels_gather_kernel, dim3(grid), dim3(256), 0, st, l);
    return hipGetLastError();
}

}  // namespace eik
