// api_internal.hpp -- what the files of the C ABI's host code share (eikonal_api.cpp and the api_*.cpp split
// off it): the context and solver objects behind the ABI's opaque handles, the error helpers
// and the declarations of the helpers that more than one file calls.  Included by those files only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eikonal.h"
#include "eik_common.hpp"
#include "eik_kernels.hpp"

using namespace eik;

int rover_assemble(const double* pathS, int64_t nS, const double* pathG, int64_t nG, const double* Z, int64_t H,
                   int64_t W, const eik_rover_query* q, double* path_xyz, double* heading, int64_t cap, int64_t* n_out,
                   double zmin_known);  // rover.cpp

// Everything internal lives in one namespace of hidden visibility: the split adds no dynamic symbol.
namespace eik_api __attribute__((visibility("hidden"))) {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

class CopyPool;  // eikonal_api.cpp

// Descriptors of one batched path call (eik_path*_batch_dev): a pinned host block and its device
// twin.  The call fills h, copies it to d on the caller's stream, launches, and records ev; the
// block is free again once ev has completed (stage_desc).
struct DescBlock {
    GdmDesc* h = nullptr;
    GdmDesc* d = nullptr;
    int64_t cap = 0;
    hipEvent_t ev = nullptr;
};

// The seeds of one multi-source call (eik_fim2d_start_seeds, eik_labels2d_dev), or the root entries of one
// seeded update (eik_fim2d_update_seeds): a pinned host block and its device twin, grown on demand; ev
// marks the block's last upload (waited for before reuse).
template <typename D>
struct Stage {
    D* h = nullptr;
    D* d = nullptr;
    int64_t cap = 0;
    hipEvent_t ev = nullptr;
    void release() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        if (ev) (void)hipEventDestroy(ev);
        h = d = nullptr;
        ev = nullptr;
        cap = 0;
    }
};

using SeedStage = Stage<SeedDesc>;
using RootStage = Stage<RootDesc>;
using Seed3Stage = Stage<Seed3Desc>;

}  // namespace eik_api

// The handles' objects are global (include/eikonal.h names them) and hold the types above, and the helpers
// below take the handles: hence the namespace's two parts.  The files that include this header are written in
// both namespaces.
using namespace eik_api;

struct eik_ctx {
    int device = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;
    std::string err;
    int max_rounds = 1;
    double tol = 0.0;
    double delta = 0.0;  // 0: unordered FIM
    int sync_every = 8;
    int mode = kModePersistent;  // EIK_OPT_MODE
    double qtimeout_s = 30.0;    // EIK_OPT_QTIMEOUT: persistent-mode spin limit
    unsigned long long max_visits = 0;  // EIK_OPT_MAX_VISITS (0: per-solver default)
    int passes = 0;              // EIK_OPT_PASSES: in-place passes per persistent visit (0: adaptive)
    bool fresh_first = false;    // EIK_OPT_FRESH_FIRST: fresh tiles jump a backlogged FIFO
    int sched = 1;               // EIK_OPT_SCHED: in-place scheduling of persistent visits
    int live_pack = 0;           // EIK_OPT_LIVE_PACK: the halo agent packs only idle tiles' edges
    // EIK_OPT_PRIO: the priority bands' width in units of 64 x the cost's geometric mean (0: the
    // plain FIFO; < 0, the default: default_prio() in fp64, on the layered solver and on one fp32 2D map of
    // >= kWideTiles tiles, else 0 in fp32 2D;
    // round 5's first default was 1 in fp64).  fp64 at 1: C2 2.44-2.50 -> 2.37 ms, C4 at
    // one GPU 10.5 -> 13.8 Gcells/s; 0.5 / 2 lose on C4 (6.9 / 12.9; profiles/r05i_prio_ab.log).  fp32
    // solves are twice as fast per pass and the one-dispatcher bands held them back: C2 fp32 1.6 ->
    // 1.9 ms, C4 fp32 18.7 -> 10.8 Gcells/s (profiles/r05j_bench.json) -- until the 128-entry dispatches of
    // round 6 (C4 fp32 with bands 18.4 -> 19.5).  Batches of > 2 maps: FIFO.
    // The layered solver's bands (both dtypes, default_prio()): C5 fp64 1.92 -> 3.65, fp32 4.73 -> 6.2
    // Gcells/s (profiles/r05ac_layered_prio_ab.log, r05ad_prio_width_ab.log).
    double prio = -1.0;
    int prio_ring = 0;           // EIK_OPT_PRIO_RING: slots per priority band (0: pow2 >= 2 x the tiles)
    int prio_dispatch = 0;       // EIK_OPT_PRIO_DISPATCH: band entries per dispatch (0: 128 on maps of >= kWideTiles, else 16)
    int wide = -1;               // EIK_OPT_WIDE: the fp32 2D persistent kernel's form (< 0: by size, wide_form())
    int64_t last_form[4] = {};   // eik_last_form: wide form launched, bands set up, pass cap, dispatch batch
    // EIK_OPT_LAYER_PLANAR (default 1): the layered solver works on layer-planar copies.  C5 kernel
    // traffic per launch 9.06 -> 3.92 GB (fp32), 20.3 -> 8.6 GB (fp64), the time within noise
    // (the layered sweep is VALU-bound; profiles/r05c_pmc_traffic_c5*.json, r05h_prio_planar_ab.log)
    int layer_planar = 1;
    int seeds_layered = 0;       // EIK_OPT_SEEDS_LAYERED: eik_fim3d_solve_seeds routes as eik_fim3d_solve does
    int64_t last_solver3[4] = {};  // eik_fim3d_last_solver: layered solver ran, z0, nl, bands set up
    DevBuf lp_cost, lp_T;        // those copies (solve_layered)
    int path_loop = 4;           // EIK_OPT_PATH_LOOP: 2D walker loop form (4: lane pairs, round 5,
                                 // 0.405 -> 0.30 us/step on the bench path, profiles/r05k_walker_ab.log)
    int timing = 0;
    int grid = 0;
    eik_stats last{};
    eik_fim2d* cached = nullptr;  // solver reused by the host-buffer entry points
    eik_fim2d* cached_l = nullptr;  // queue state of the layered 3D solver (fim2dl.hip), fp32 tiles
    eik_fim2d* cached_l64 = nullptr;  // the same for the fp64 layered solver's 40-row tiles
    eik_fim2d* cached_fronts = nullptr;  // coarse B = 2 solver of the capped bidirectional fronts
    double fronts_cap = 1.25;          // EIK_OPT_FRONTS_CAP: cap margin (0: full fronts)
    DevBuf fronts;                     // capped fronts: coarse cost (2 maps) | coarse T (2 maps) | FrontsCheck
    int64_t fronts_info[10] = {};      // eik_fronts_info: capped, fallback, kept G / S, members G / S,
                                       // band cells G / S, band relaxation sweeps G / S
    bool exact_band = false;           // EIK_OPT_EXACT_BAND: replay the reference's band (bidir_exact.hip)
    DevBuf exact;                      // its scratch: events, ranks, sort keys
    unsigned long long exact_info[5] = {};  // eik_exact_info: passes, sweeps G / S, tie launches, microseconds
    DevBuf cm_u8, cm_i32, cm_f32, cm_f64;  // cost-builder scratch
    DevBuf arm;                            // end-effector volume scratch (arm.hip)
    int resident_l[2][5] = {};  // co-resident workgroups of fim2dl_persist_kernel<R, nl> (f32, f64)
    DevBuf cost, T, T2, goals, work, misc;
    DevBuf l3, c3, m3, v3;             // 3D solver scratch (lists, counts, marks, visits)
    int max_passes3 = 24;
    int* h3 = nullptr;                 // 3D solver: pinned count + visits words (made once)
    DevBuf q3ctl, q3slot, q3state, q3vis;  // 3D persistent driver: tile FIFO (fim_engine.hpp)
    unsigned* h_q3 = nullptr;          // pinned copy of q3ctl + the two visit counters
    int resident3[2] = {0, 0};         // co-resident workgroups of fim3d_persist_kernel (f32, f64)
    hipStream_t stream2 = nullptr;     // second stream: the rover path's two walks run side by side
    // pinned staging of large host <-> device copies (host_to_dev / dev_to_host)
    char* stage[2] = {nullptr, nullptr};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    CopyPool* pool = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t e3[2] = {nullptr, nullptr};
    // the cost diff (cost_diff.hip): every tile's record, the totals + the changed tiles'
    // list, the list's pinned copy (1 + max(kMaxRects, tiles) records) and the kernels' timing events
    DevBuf diff_rec, diff_out, cost2;  // (cost2: the host entries' old cost)
    DiffRecord* h_diff = nullptr;
    int64_t h_diff_cap = 0;
    hipEvent_t ev_diff[2] = {nullptr, nullptr};
    // EIK_OPT_DIFF_LOADS: non-temporal loads by default -- 16384^2 fp64 0.75-0.77 -> 0.66-0.71 ms, 4096^2 fp64
    // 0.057-0.066 -> 0.049-0.062 ms, fp32 equal (profiles/cost_diff_ab.log)
    bool diff_nt = true;
    double diff_share = -1.0;          // EIK_OPT_DIFF_SHARE (< 0: kDiffFullShare)
    SeedStage lab_seeds;               // eik_labels2d_dev: its seeds, and its scratch (parents | pass flags)
    DevBuf lab_work, lab_out;          // (lab_out: the host entries' device labels)
    Seed3Stage seeds3, lab_seeds3;     // eik_fim3d_solve_seeds / eik_labels3d_dev: their seeds (scratch: lab_work)
    std::vector<DescBlock> desc;       // batched paths: descriptor blocks in flight or free (stage_desc)
    size_t desc_next = 0;
};

struct eik_fim2d {
    eik_ctx* ctx = nullptr;
    int64_t B = 0, H = 0, W = 0;
    bool f64 = false;
    Fim2dArgs a{};
    hipStream_t stream = nullptr;
    DevBuf lists, counts, mark, edge, goals, key;
    DevBuf ecol;                         // every tile's two edge columns (Fim2dArgs::ecol)
    DevBuf qctl, qslot, qstate;          // persistent-mode FIFO
    DevBuf bslot, bctl;                  // priority bands (EIK_OPT_PRIO)
    int* h_counts = nullptr;             // pinned
    unsigned* h_q = nullptr;             // pinned copy of qctl
    unsigned long long* h_visits = nullptr;
    int64_t* h_goals = nullptr;          // pinned: the goals' upload does not stall the host
    int64_t iterations = 0, host_syncs = 0, max_iters = 0;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    std::vector<hipEvent_t> ev_pool;     // per-launch timing pairs (timing option)
    size_t ev_used = 0;
    double sweep_ms = 0.0, solve_ms = 0.0;
    bool started = false;
    bool defer_sync = false;             // eik_fim2d_solve: the launch's read-back syncs with the finish
    bool need_rewind = false;            // a launch without its queue rewind ran since the last init
    bool band_overflow = false;          // the last launch stopped on a full priority band (qerror bit 4)
    bool no_bands = false;               // ... so this solver's next starts use the FIFO
    // a seed set started the bound solve (eik_fim2d_start_seeds): eik_fim2d_update knows one goal only,
    // eik_fim2d_update_seeds re-solves it
    bool seeded = false;
    SeedStage sd;                        // its seeds
    std::vector<SeedDesc> bound;         // the bound seed list (host copy: start_seeds, adopt_seeds, update_seeds)
    RootStage roots;                     // eik_fim2d_update_seeds: the old list's cells (seed_diff.hpp)
    int64_t last_active = -1;            // tiles left by the last persistent launch read back (-1: none yet, or it failed)
    // incremental re-solve (replan.hip): descriptors (pinned + device), recorded tiles, counters
    DevBuf rp_rects, rp_list, rp_flag, rp_info;
    ReplanRect* h_rects = nullptr;       // pinned [kMaxRects]
    unsigned long long* h_info = nullptr;  // pinned [6]
    hipEvent_t ev_rp[2] = {nullptr, nullptr};
    bool rp_timed = false, rp_fallback = false;  // events recorded; the last resolve ended in a full solve
    int flood_grid = 0;                  // co-resident workgroups of the flood kernel
    int persist_grid = 0;                // co-resident workgroups of the persistent kernel
    int64_t diff_info[8] = {};           // eik_fim2d_diff_info: of the last eik_fim2d_resolve_cost
    bool persist_wide = false;           // ... of which form (EIK_OPT_WIDE can change it between solves)
    // live domain decomposition: hold word on the device, mailbox of the halo agent on the host
    DevBuf hold;
    LiveBox* box = nullptr;              // pinned, coherent
    bool live_on = false;
    // a layered volume's block (eik_fim3dl_create: the layered solver, fim2dl.hip): nl > 0
    int lnl = 0, lz0 = 0;
    int64_t lL = 1;
};

namespace eik_api __attribute__((visibility("hidden"))) {

int set_err(eik_ctx* c, int code, const char* fmt, ...);  // eikonal_api.cpp

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_err((ctx), e_ == hipErrorOutOfMemory ? EIK_ERR_NOMEM : EIK_ERR_HIP, "%s: %s (%s:%d)", \
                           #expr, hipGetErrorString(e_), __FILE__, __LINE__);                      \
    } while (0)

// the staged copies' chunk (host_to_dev / dev_to_host): the pinned ring holds two of them
constexpr size_t kStageChunk = 8ull << 20;
constexpr double kFrontsMargin = 1.25;  // capped bidirectional fronts (solve_fronts)
// words of a solver's queue control block (kQueueCtlBytes, read back into h_q / h_q3 after a persistent
// launch): the active tiles' count at byte 128, the error bits at byte 192
constexpr int kQActiveWord = 128 / 4;
constexpr int kQErrorWord = 192 / 4;

// A pair of timing events that one call makes for itself (the exact replays): the call creates them here, and
// they are destroyed with the scope, whichever way the call returns.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// ---- eikonal_api.cpp's helpers that the api_*.cpp files call
hipError_t host_to_dev(eik_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
hipError_t dev_to_host(eik_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
int get_solver(eik_ctx* c, int64_t B, int64_t H, int64_t W, int dtype, eik_fim2d** out);
int solve_fronts(eik_ctx* c, eik_fim2d* f, double* dcost, double* dT, const int64_t g[4], int64_t H, int64_t W,
                 unsigned long long* best);
int fim3d_solve_one(eik_ctx* c, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int dtype,
                    const int64_t goal[3], hipStream_t st, int64_t stop_off);
int64_t early_offset(const int64_t goal[3], const int64_t start[3], int64_t H, int64_t W, int64_t L);

// Costs must be >= 0 or +inf (negative or NaN: EIK_ERR_ARG).  Checked on the device copy `dev`
// of the host array `cost` (a host scan of a 4096^2 f64 raster took ~19 ms at one core's memory
// bandwidth): one short kernel and an 8-byte read-back, before anything is solved.
template <typename R>
int check_cost(eik_ctx* c, const R* cost, const void* dev, int64_t n, hipStream_t st) {
    HIPCHK(c, c->misc.ensure(64));
    unsigned long long* first = (unsigned long long*)c->misc.p + 7;  // (words 0..: the join's)
    HIPCHK(c, cost_check(dev, n, sizeof(R) == 8, first, st));
    unsigned long long i = 0;
    HIPCHK(c, hipMemcpyAsync(&i, first, sizeof i, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (i != ~0ull)
        return set_err(c, EIK_ERR_ARG, "cost[%ld] = %g: costs must be >= 0 or +inf", (long)i, (double)cost[i]);
    return EIK_OK;
}

}  // namespace eik_api
