/*
 * eikonal.h -- C ABI of the MI355X-native Eikonal cost-to-go solver (libeikonal.so).
 *
 * The drop-in boundary for the hot path of esa-prl/planning-motion_planning:
 *   src/FastMarching/FastMarching.py   (2D FMM + gradient-descent path)
 *   src/FastMarching/FastMarching3D.py (3D FMM + path)
 * reached from Python through ctypes (planning-motion_planning_amd/FastMarching/, same module
 * and function names as the reference) and from C++ directly (include/MotionPlanning.hpp
 * users, Rock components).  Plain C: pointers + sizes, no exceptions, no torch types.
 *
 * Conventions (identical to the reference):
 *   - rasters are row-major [y][x] (3D: [y][x][z]); nodes are (x, y(, z));
 *   - cost = +inf marks an impassable cell (FastMarching.py:93-94); costs must be >= 0;
 *   - T = +inf marks an unreached cell;
 *   - out-of-range neighbours read as +inf (the reference instead relies on an inf border,
 *     Coupled_motion_planner.py:1213-1216, and wraps/raises without one).
 * Every function returns an eik_status (0 = OK); on error eik_last_error() describes it.
 * One context per host thread; a context owns its device buffers and HIP stream.
 * Host-buffer entry points (eik_tmap*, eik_path*, eik_gradient*) are synchronous.
 * Device entry points (eik_fim2d_*, eik_path2d_dev) take device pointers and a hipStream_t
 * (passed as void*, used as given: NULL is the default null stream, as in HIP) and are
 * asynchronous unless noted.
 */
#ifndef EIKONAL_H_
#define EIKONAL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    EIK_OK = 0,
    EIK_ERR_ARG = -1,         /* bad argument (shape, index, negative cost, NULL pointer)     */
    EIK_ERR_HIP = -2,         /* HIP runtime / launch failure                                  */
    EIK_ERR_NOMEM = -3,       /* device or host allocation failed                               */
    EIK_ERR_NOCONVERGE = -4,  /* iteration cap reached (e.g. negative cost on a device buffer)  */
    EIK_ERR_UNREACHABLE = -5, /* bidirectional fronts never meet (reference: UnboundLocalError) */
    EIK_ERR_NODEVICE = -6     /* no HIP device / library built without one                       */
} eik_status;

typedef enum { EIK_F32 = 0, EIK_F64 = 1 } eik_dtype;

/* path status (eik_path2d / eik_path3d), mirrors the reference's exits */
typedef enum {
    EIK_PATH_DONE = 0,     /* stop radius (< 1.5 cells) or step budget hit; end appended (:231-234):
                              always with n_out <= cap, `end` being row n_out - 1                */
    EIK_PATH_FALLBACK = 1, /* NaN gradient: the reference's fallback returns a truncated path
                              (numpy-2 behaviour of FastMarching.py:178-218)                       */
    EIK_PATH_ERROR = 2,    /* the reference raises out of getPathGDM: a NaN point, an index out of
                              range (also a coordinate <= -1, which numpy's uint32 cast turns
                              into an index past every axis, and any coordinate >= 2^31; 2D: also
                              an infinite coordinate at the top of a step, computeGradient's
                              int(point)), 3D: int(round()) of a NaN or infinite coordinate in the
                              NaN branch; the path as it stands is returned.  A coordinate in
                              (-1, 0) is cell 0 with a negative fraction and walks on.
                              Also: out of point budget -- the walk has no row left for its next
                              point or, after the stop radius or the last step, for `end`:
                              n_out == cap, the first cap rows of the walk                        */
    EIK_PATH_STUCK = 3     /* eik_path2d_safe_* only: no lower neighbour to descend to, or the
                              iteration budget ran out short of the stop radius; end NOT appended   */
} eik_path_status;

typedef struct eik_ctx eik_ctx;
typedef struct eik_fim2d eik_fim2d;

typedef struct {
    int64_t iterations;   /* solver launches of the last solve (list mode: outer iterations) */
    int64_t tile_visits;  /* 64x64 tile visits of the last solve                                */
    int64_t host_syncs;   /* active-count read-backs                                            */
    double solve_ms;      /* device time of the last solve (hipEvents, init..converged)         */
    double sweep_ms;      /* summed device time of the sweep launches (timing option on)        */
    double bytes_alg;     /* algorithmic bytes of the sweep launches (tile_visits x bytes/visit) */
    int64_t inplace_passes; /* persistent mode: extra in-place passes of busy tiles (halo refresh
                               + sweep + write-back of the tile already in LDS)                 */
    int64_t fresh_visits; /* persistent mode: tile visits (among tile_visits) that read no T --
                             the tile's first visit, T still +inf (bytes_alg counts them so)    */
} eik_stats;

/* options (eik_set_option) */
typedef enum {
    EIK_OPT_MAX_ROUNDS = 0,  /* sweep rounds per tile visit before re-enqueueing (default 1)   */
    EIK_OPT_SYNC_EVERY = 1,  /* sweep launches between active-count read-backs (default 8)     */
    EIK_OPT_TIMING = 2,      /* 1: time each sweep launch with hipEvents (for the roofline)     */
    EIK_OPT_GRID = 3,        /* workgroups per sweep launch (default 4 x CUs)                   */
    EIK_OPT_TOL = 4,         /* relative change below which a cell does not (re)activate tiles  */
    EIK_OPT_DELTA = 5,       /* ordered mode: per launch, only tiles whose entering T is within
                                delta of the smallest pending one are swept (0: off; > 0 forces
                                EIK_MODE_LIST)                                                  */
    EIK_OPT_MODE = 6,        /* EIK_MODE_PERSISTENT (default): one launch per solve over a device
                                FIFO of tiles; EIK_MODE_LIST: one launch per outer iteration   */
    EIK_OPT_QTIMEOUT = 7,    /* persistent mode: seconds a workgroup may wait on the FIFO before
                                the solve fails with EIK_ERR_HIP instead of hanging (default 30) */
    EIK_OPT_MAX_VISITS = 8,  /* persistent mode: tile visits after which a solve fails with
                                EIK_ERR_NOCONVERGE (0: default 1024 x tiles + 2^20; 2D solves: x the
                                raster's elongation, (tile columns + tile rows) / (2 sqrt(tiles)),
                                where that exceeds 1)                                          */
    EIK_OPT_PASSES = 9,      /* persistent mode: sweep passes a visit may run in place while its
                                tile keeps changing before it is re-queued (0, the default:
                                40 for a single map, 16 for a single fp32 map of >= 16384
                                tiles, 2 for a batch of maps)                                  */
    EIK_OPT_FRESH_FIRST = 10,/* persistent mode: 1 queues a tile's first activation ahead of
                                re-visits while the queue has a backlog (default 0: one FIFO)  */
    EIK_OPT_SCHED = 11,      /* persistent mode, bit mask: 1 = a busy tile serves activations that
                                reach it in place (no re-queued visit); 2 = after a visit's first
                                pass, neighbour activations wait for the visit's end (default 1:
                                profiles/r02d_grab_sched_ab.log)                                 */
    EIK_OPT_PATH_LOOP = 12,  /* 2D path kernel, the loop form: 0 = the loop in the reference's
                                statement order; 1 = one exit branch per step (the step is
                                computed before its special cases are tested), the compiler's f64
                                sqrt / division; 2 = form 1 with the sqrt / division free of range
                                handling inside their safe domain; 3 = form 2 with both divisions
                                taken from the square roots' reciprocals (div_rs, checked by
                                eik_selftest_walker_math); 4 (default) = form 3 on lane pairs,
                                x on even lanes, y on odd, one-correction square roots.  Same
                                path bits in all five: 4 is the walker, 3 .. 0 the slower forms it
                                is tested against.                                              */
    EIK_OPT_FRONTS_CAP = 13, /* biComputeTmap / rover path, rasters >= 2^20 cells: 1 (default) solves
                                each front only up to a cap on T estimated from a coarse copy of
                                the raster (x 1.25) and falls back to the full solve when the
                                capped fields cannot be shown to give the full fields' join; a
                                value v > 1: the same with margin v; 0 = full fronts            */
    EIK_OPT_LIVE_PACK = 14,  /* live domain decomposition (eik_fim2d_live_pack): 0 (default) = the
                                halo agent stores every edge cell each round; 1 = only the cells
                                of tiles that are neither pending nor busy (converged edges), so a
                                neighbour is not re-activated by every intermediate refinement
                                (a round whose snapshot had no tile pending or busy packs all)   */
    EIK_OPT_PRIO = 15,       /* 2D persistent solves of one or two maps and the layered 3D solver:
                                v > 0 serves waiting tiles lowest entering T first, in 64 bands of
                                width v x 64 x the geometric mean of the finite costs
                                (fim_engine.hpp "priority bands"); 0 = the FIFO; < 0 (default) =
                                0.25 x max(1, sqrt(H W) / 4096) for fp64 2D solves of rasters
                                of >= 4096^2 cells (any size for a decomposition block), one
                                fp32 2D map of >= 16384 tiles and layered solves of >= 3072^2
                                in either dtype; else the FIFO                                   */
    EIK_OPT_LAYER_PLANAR = 16, /* few-layer 3D volumes (the layered solver): 1 (default) solves on
                                layer-planar copies [nl][H][W] of the solved layers (one copy in,
                                one out per solve; every tile-row access one contiguous run per
                                layer); 0 = in the volume's [y][x][L] layout                     */
    EIK_OPT_PRIO_RING = 17,  /* slots per priority band (rounded up to a power of two; 0, the
                                default: >= 2 x the tiles).  A band whose ring fills stops the
                                launch; eik_fim2d_solve then solves again with the FIFO.         */
    EIK_OPT_PRIO_DISPATCH = 18, /* band entries moved to the FIFO per dispatch, 1..128 (0, the
                                default: 128 on maps of >= 16384 tiles, else 16)                */
    EIK_OPT_EXACT_BAND = 19, /* biComputeTmap / rover path and fp64 FM3D early exits: 1 replays the
                                reference's sequential narrow band in pop order from the converged
                                fields (csrc/bidir_exact.hip): its tentative band values, its LIFO
                                order of equal T and so its nodeJoin / closed set, bit for bit; 0
                                (default) = band cells at their final (2D: relaxed) values (GPU <=
                                reference <= 1.03 x GPU), ties by node index / strict < T[start] */
    EIK_OPT_WIDE = 20,       /* fp32 2D persistent solves: which form of the kernel is launched
                                (and the co-resident workgroup count that goes with it).  < 0
                                (default) = by size: the 4-waves-per-SIMD form on maps of >= 16384
                                tiles, else the narrow form; 0 = always the narrow form; 1 =
                                always the 4-waves-per-SIMD form.  The pass cap, the bands and the
                                dispatch batch keep their own defaults (EIK_OPT_PASSES, _PRIO,
                                _PRIO_DISPATCH); fp64 solves ignore it.                          */
    EIK_OPT_DIFF_LOADS = 21, /* the cost diff's loads (eik_cost_diff_dev, eik_fim2d_resolve_cost): 1
                                (default) non-temporal, 0 plain; same results (tools/cost_diff_ab.py) */
    EIK_OPT_DIFF_SHARE = 22, /* eik_fim2d_resolve_cost solves from scratch when more than this share
                                of the raster's tiles changed; < 0 (default): the measured constant
                                (DESIGN.md §3.15); >= 1: never                                      */
    EIK_OPT_SEEDS_LAYERED = 23 /* eik_fim3d_solve_seeds / eik_tmap3d_seeds_*: 0 (default) = always the
                                general 3D solver; 1 = few-layer volumes go to the layered solver by
                                eik_fim3d_solve's own rule when every seed's z lies among the solved
                                layers (eik_fim3d_last_solver tells which ran)     */
} eik_option;

typedef enum { EIK_MODE_LIST = 0, EIK_MODE_PERSISTENT = 1 } eik_mode;

/* ---- context: replaces MotionPlanning::initPython / shutDownPython (MotionPlanning.cpp:5-29,
 *      :93-100) as the owner of solver state; one per host thread -------------------------- */
int eik_create(int device, eik_ctx** out);
void eik_destroy(eik_ctx* ctx);
const char* eik_last_error(const eik_ctx* ctx);
int eik_set_option(eik_ctx* ctx, int option, double value);
int eik_get_stats(const eik_ctx* ctx, eik_stats* out);
const char* eik_version(void);

/* ---- host-buffer drop-ins of FastMarching.py ------------------------------------------- */

/* computeTmap(costMap, goal, start) FastMarching.py:92-112 -> full arrival field T (the
 * reference raises at :107; this is its intended semantics with no early exit).
 * cost, T: H*W row-major.  f32: fp32 compute; f64: fp64 compute. */
int eik_tmap2d_f32(eik_ctx* ctx, const float* cost, int64_t H, int64_t W, int64_t gx, int64_t gy, float* T);
int eik_tmap2d_f64(eik_ctx* ctx, const double* cost, int64_t H, int64_t W, int64_t gx, int64_t gy, double* T);

/* biComputeTmap(costMap, goal, start) FastMarching.py:114-162 -> (TmapG, TmapS, nodeJoin).
 * nodeJoin is the first node popped by one front that the other front had already closed,
 * evaluated on the device from the two fields' pop ranks (the meeting iteration k).  TmapG/TmapS
 * are the fronts' PARTIAL fields at that iteration, as the reference returns them: the source and
 * its k first pops (rank <= k) and the narrow band around them at their values, +inf elsewhere
 * (fp64; band values relaxed and exact ties of T ranked by node index, or with EIK_OPT_EXACT_BAND
 * the reference's own band values, LIFO ties and nodeJoin). */
int eik_tmap2d_bidir_f64(eik_ctx* ctx, const double* cost, int64_t H, int64_t W, int64_t gx, int64_t gy,
                         int64_t sx, int64_t sy, double* TG, double* TS, uint32_t join[2]);

/* The join step of biComputeTmap alone (FastMarching.py:141-162) from two given FULL fields
 * TG (goal front) and TS (start front), H*W fp64 each (+inf = unreached): nodeJoin and the two
 * partial fields TGp / TSp, exactly as eik_tmap2d_bidir_f64 forms them after its solve.  members
 * (optional): the cells ranked per front -- the join bounds the meeting iteration first and sorts
 * only the cells under the bound (csrc/bidir.hip).  EIK_ERR_UNREACHABLE when no cell is finite in
 * both fields. */
int eik_bidir_join_f64(eik_ctx* ctx, const double* TG, const double* TS, int64_t H, int64_t W, double* TGp,
                       double* TSp, uint32_t join[2], int64_t members[2]);

/* How the last biComputeTmap / rover path formed its fronts: out[0] 1 = capped fronts, out[1] 1 =
 * the capped result was replaced by the full solve, out[2..3] cells kept under the caps (goal,
 * start front), out[4..5] cells the join ranked per front, out[6..7] band cells relaxed per front,
 * out[8..9] the band relaxation's sweeps per front. */
int eik_fronts_info(const eik_ctx* ctx, int64_t out[10]);

/* The last biComputeTmap / rover path's / FM3D early exit's exact band replay (EIK_OPT_EXACT_BAND): out[0] re-ranking
 * passes, out[1..2] relaxation sweeps (goal, start front), out[3] tie-run launches, out[4] its
 * device time in microseconds; all 0 when it did not run. */
int eik_exact_info(const eik_ctx* ctx, int64_t out[5]);

/* What the last 2D solve started on the context (eik_fim2d_start and every entry point that goes
 * through it; the internal coarse solve of the capped fronts and the cost builder's do not count)
 * took: out[0] 1 = the 4-waves-per-SIMD fp32 form was launched, out[1] 1 = priority bands were set
 * up, out[2] the pass cap, out[3] the bands' dispatch batch (0 without bands). */
int eik_last_form(const eik_ctx* ctx, int64_t out[4]);

/* B independent maps (goal sweep / terrain Monte-Carlo): cost, T: B*H*W; goals: B x (x, y). */
int eik_tmap2d_batch_f32(eik_ctx* ctx, const float* cost, int64_t B, int64_t H, int64_t W, const int64_t* goals,
                         float* T);

/* getPathGDM(T, init, end, tau) FastMarching.py:164-236 on an fp64 field.
 * out: cap x 2 (x, y) rows; *n_out rows written; *status an eik_path_status. */
int eik_path2d_f64(eik_ctx* ctx, const double* T, int64_t H, int64_t W, const double init[2], const double end[2],
                   double tau, double* out, int64_t cap, int64_t* n_out, int* status);

/* computeGradient(T) FastMarching.py:242-300 (point = [] -> whole field): Gnx, Gny. */
int eik_gradient2d_f64(eik_ctx* ctx, const double* T, int64_t H, int64_t W, double* gnx, double* gny);

/* ---- host-buffer drop-ins of FastMarching3D.py ----------------------------------------- */

/* FastMarching3D.computeTmap :126-145 without its early exit -> the full field T (what the
 * reference returns when `start` is never popped).  cost, T: H*W*L row-major [y][x][z];
 * goal = (x, y, z). */
int eik_tmap3d_f32(eik_ctx* ctx, const float* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3], float* T);
int eik_tmap3d_f64(eik_ctx* ctx, const double* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3],
                   double* T);

/* FastMarching3D.computeTmap(costMap, goal, start) :126-145 as the planner calls it
 * (Coupled_motion_planner.py:1636): the loop breaks once `start` is popped (:141), so T is the
 * PARTIAL field -- cells popped before `start` (T < T[start]) and `start` at their final values,
 * the narrow band (finite cost, a closed 6-neighbour) at its converged full-field value -- <= the
 * reference's tentative value, which depends on its sequential update order --
 * and +inf elsewhere (eik_fim3d_early_exit).  fp64 with EIK_OPT_EXACT_BAND: the reference's own
 * closed set and band values, replayed in pop order (masks identical, values within 1e-11).
 * start == goal, a start outside the volume or an unreachable start -> the full field, as in the
 * reference (it never pops such a start). */
int eik_tmap3d_early_f32(eik_ctx* ctx, const float* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3],
                         const int64_t start[3], float* T);
int eik_tmap3d_early_f64(eik_ctx* ctx, const double* cost, int64_t H, int64_t W, int64_t L, const int64_t goal[3],
                         const int64_t start[3], double* T);

/* FastMarching3D.getPathGDM(T, init, end, tau) :198-271 on an fp64 field: out cap x 3 rows. */
int eik_path3d_f64(eik_ctx* ctx, const double* T, int64_t H, int64_t W, int64_t L, const double init[3],
                   const double end[3], double tau, double* out, int64_t cap, int64_t* n_out, int* status);

/* ---- device-resident solver (bench, multi-GPU domain decomposition, C++ hosts) ---------- */

/* A solver for B maps of H x W in `dtype`; owns the active lists, marks and counters. */
int eik_fim2d_create(eik_ctx* ctx, int64_t B, int64_t H, int64_t W, int dtype, eik_fim2d** out);
void eik_fim2d_destroy(eik_fim2d* fim);

/* Ghost strips for a subdomain of a decomposed raster (device pointers, NULL = +inf border):
 * north/south length W, west/east length H.  Values are min-merged by eik_fim2d_merge_ghost. */
/* A block of a domain-decomposed few-layer 3D volume ([H][W][L], layers z0 .. z0+nl-1 solved: the
 * layered solver; FastMarching3D.py:19-145 semantics; SURVEY §8(e) "C5: split x-y only, layers stay
 * together").  The handle is an eik_fim2d: eik_fim2d_set_ghosts (strips of nl values per edge cell,
 * [i][z]), eik_fim2d_iterate (one persistent launch to local convergence), eik_fim2d_pack_edges,
 * eik_fim2d_merge_ghost, eik_fim2d_active, eik_fim2d_stats and eik_fim2d_destroy apply; start with
 * eik_fim3dl_start (goal (x, y, z), z absolute; x < 0: the goal is in another block). */
int eik_fim3dl_create(eik_ctx* ctx, int64_t H, int64_t W, int64_t L, int z0, int nl, int dtype, eik_fim2d** out);
int eik_fim3dl_start(eik_fim2d* f, const void* d_cost, void* d_T, const int64_t goal[3], void* stream);

/* Diagnostics: the queue counters of the solver's last persistent launch (builds with -DEIK_QDEBUG=1:
 * FIFO claims, stale FIFO entries, band dispatches, decrease-key entries, band puts at out[3..7];
 * zeros otherwise).  tools/prio_probe.py. */
int eik_fim2d_qcount(const eik_fim2d* f, uint64_t out[8]);

int eik_fim2d_set_ghosts(eik_fim2d* fim, void* north, void* south, void* west, void* east);

/* Bind device cost/T (B*H*W of dtype), set T = inf, T[goal] = 0, seed the goal tiles.
 * goals: host array B x (x, y); a goal outside the map seeds nothing (subdomain w/o goal). */
int eik_fim2d_start(eik_fim2d* fim, const void* d_cost, void* d_T, const int64_t* goals, void* stream);

/* Run up to max_iters outer iterations (stops early when no tile is active); *active gets the
 * number of tiles active for the next iteration (synchronises the stream). */
int eik_fim2d_iterate(eik_fim2d* fim, int64_t max_iters, int64_t* active);

/* start + iterate to convergence (synchronous). */
int eik_fim2d_solve(eik_fim2d* fim, const void* d_cost, void* d_T, const int64_t* goals, void* stream);

/* Halo exchange helpers (async on the bound stream): copy edge rows/columns of T into send
 * strips; min-merge a received strip into ghost `side` (0 N, 1 S, 2 W, 3 E) and activate the
 * edge tiles whose ghost decreased. */
int eik_fim2d_pack_edges(eik_fim2d* fim, void* north, void* south, void* west, void* east);
int eik_fim2d_merge_ghost(eik_fim2d* fim, int side, const void* recv);
/* number of tiles active for the next iteration (synchronises the stream) */
int eik_fim2d_active(eik_fim2d* fim, int64_t* active);
/* statistics of the current/last solve (synchronises the stream to read the visit counter) */
int eik_fim2d_stats(eik_fim2d* fim, eik_stats* out);

/* Incremental re-solve after local cost changes (replanning; no reference counterpart, DESIGN.md
 * §3.12).  The solver holds a converged field: its last solve ended with 0 active tiles, or the field
 * was bound with eik_fim2d_adopt.  The caller has written the new costs into the bound cost buffer on
 * the same stream and names K rectangles (x0, y0, x1, y1), half-open, clipped to the raster, that hold
 * every changed cell, each with a kind:
 *   EIK_CHANGE_ANY      a cost in the rectangle may have gone up (always safe to say)
 *   EIK_CHANGE_LOWERED  the caller guarantees that no cost in the rectangle went up
 * Only the cells whose old value depended on a cell of an ANY rectangle are reset and solved again;
 * the rest of T is kept.  The result is the fixed point of the new cost -- exact for EIK_OPT_TOL = 0
 * (the default); with a tolerance the kept cells carry the old solve's tolerance.
 *
 * One map (B = 1), no ghost strips, not a layered block, persistent mode (EIK_OPT_MODE, and a raster
 * within its 32-bit offsets), either dtype, FIFO or priority bands.  Anything else -- a solver never
 * started or adopted, a last solve that did not converge, a rectangle with x1 <= x0 or y1 <= y0 or
 * wholly outside the raster, a kind other than 0 / 1, K > 1024 -- is EIK_ERR_ARG with a message, and
 * nothing is launched.
 *
 * eik_fim2d_update   asynchronous: invalidates and queues the restart; eik_fim2d_iterate then converges
 *                    it.  kinds == NULL: all ANY.  K == 0: a no-op, the solver stays converged.  The
 *                    descriptors are staged through a pinned block: rects / kinds may be reused at once.
 * eik_fim2d_resolve  update + iterate to convergence (synchronous); a full priority-band ring falls back
 *                    to a full FIFO solve, as in eik_fim2d_solve.
 *                    If the invalidation itself fails (its tile-visit budget, EIK_OPT_MAX_VISITS, or a queue
 *                    wait past EIK_OPT_QTIMEOUT), the following iterate / this resolve returns that error
 *                    and the bound T is INVALID: it may hold sign-marked (negative) values and a partly
 *                    reset cone.  The same holds after any other error of the re-solve.  Solve from
 *                    scratch (eik_fim2d_solve) before the field or a further update is used.
 * eik_fim2d_adopt    binds d_cost / d_T where d_T is, by the caller's word, the converged field of some
 *                    earlier cost of this raster for `goals`; nothing is solved.
 * eik_fim2d_update_info  of the last update: out[0] cells invalidated, [1] tiles holding them, [2] tile
 *                    visits of the invalidation flood, [3] tiles queued for the solve, [4] device time
 *                    of the invalidation in microseconds, [5] 1 when eik_fim2d_resolve fell back to a
 *                    full solve, else 0 (synchronises the stream). */
typedef enum { EIK_CHANGE_ANY = 0, EIK_CHANGE_LOWERED = 1 } eik_change;
int eik_fim2d_update(eik_fim2d* fim, const int64_t* rects, const int* kinds, int64_t K, void* stream);
int eik_fim2d_resolve(eik_fim2d* fim, const int64_t* rects, const int* kinds, int64_t K, void* stream);
int eik_fim2d_adopt(eik_fim2d* fim, const void* d_cost, void* d_T, const int64_t* goals, void* stream);
int eik_fim2d_update_info(eik_fim2d* fim, int64_t out[6]);
/* Host buffers: cost_new and the converged field T of the earlier cost go up, T comes back as the
 * field of cost_new (adopt + resolve on the context's cached solver). */
int eik_tmap2d_update_f32(eik_ctx* ctx, const float* cost_new, float* T_inout, int64_t H, int64_t W, int64_t gx,
                          int64_t gy, const int64_t* rects, const int* kinds, int64_t K);
int eik_tmap2d_update_f64(eik_ctx* ctx, const double* cost_new, double* T_inout, int64_t H, int64_t W, int64_t gx,
                          int64_t gy, const int64_t* rects, const int* kinds, int64_t K);

/* Multi-source 2D solves (no reference counterpart): the field of a SET of K seeds,
 * seed k at cell (x, y) of map map_of[k] with start value t0[k] >= 0,
 *     T = min_k (t0[k] + cost-to-go from seed k)
 * as the solver's own discrete fixed point -- which lies below the pointwise minimum of K single-source
 * fields wherever a cell takes its x neighbour from one seed's wave and its y neighbour from another's.
 * A goal region, several candidate goals, a docking line; t0 carries a cost already spent elsewhere.
 * Two seeds may name one cell (the lower t0 holds); a seed that another seed's wave undercuts is
 * dominated (T there ends below its t0).  A seed on a +inf-cost cell keeps its t0.
 *
 * seeds: K x (x, y), host.  t0: K host doubles, rounded to the solver's dtype, or NULL (all 0).  map_of:
 * K host int32, or NULL (needs B == 1).  The host arrays are read before the call returns and go to the
 * device in stream order through a pinned block.  Options, statistics, the visit budget, the priority
 * bands (the seeds' keys are their t0) and eik_last_form behave as in any solve.
 *
 * EIK_ERR_ARG, with a message naming the offending index and nothing launched: K < 1 or K > 2^24, a
 * NULL pointer, a seed outside the raster (stricter than the single goal, whose "outside = seeds
 * nothing" exists for decomposition blocks), map_of[k] outside [0, B), map_of == NULL with B > 1, a t0
 * that is negative, NaN or +inf or (fp32 solver) rounds to +inf, a layered block, a solver with ghost
 * strips bound.
 *
 * eik_fim2d_start_seeds  asynchronous; eik_fim2d_iterate then converges it.
 * eik_fim2d_solve_seeds  start + iterate to convergence (synchronous); a full priority-band ring falls
 *                        back to the FIFO with the same seeds, as in eik_fim2d_solve.
 * Replanning after a seeded solve: eik_fim2d_update_seeds / eik_fim2d_resolve_seeds below, which take
 * cost changes and seed-list changes.  The single-goal calls stay single-goal: after a seeded start,
 * eik_fim2d_update, eik_fim2d_resolve and eik_tmap2d_update_* (the context's cached solver after
 * eik_tmap2d_seeds_*) return EIK_ERR_ARG ("the bound solve has a seed set") until an eik_fim2d_start /
 * eik_fim2d_solve / eik_fim2d_adopt (any single-goal host solve on the context) binds a single-goal
 * solve again.
 * Not covered: the layered solver, the bidirectional fronts, a seeded eik_plan2d_batch.  3D volumes:
 * eik_fim3d_solve_seeds below (one volume on the general 3D solver or, with EIK_OPT_SEEDS_LAYERED, on the
 * layered one; no 3D replanning, no B > 1, no early exit with a seed set). */
int eik_fim2d_start_seeds(eik_fim2d* fim, const void* d_cost, void* d_T, const int64_t* seeds, const double* t0,
                          const int32_t* map_of, int64_t K, void* stream);
int eik_fim2d_solve_seeds(eik_fim2d* fim, const void* d_cost, void* d_T, const int64_t* seeds, const double* t0,
                          const int32_t* map_of, int64_t K, void* stream);

/* Nearest-seed labels: which seed does each cell of a converged field belong to (the nearest goal
 * under the cost, the Voronoi partition of the seeds, the `end` to pass to getPathGDM for a start).
 * d_T: the converged field of B maps of H x W in dtype (fewer than 2^31 cells in all), device; seeds,
 * t0, map_of, K: the seed list that produced it, checked as above; d_label: int32 [B][H][W], device.
 * Asynchronous on `stream`, no read-back.  The context owns the scratch: calls on one stream simply
 * queue up, calls on different streams must not overlap.
 * The rule:
 *   Root.   Cell c is a root with label k when seed k lies on c and T[c] == (R)t0_k bit for bit.  Of
 *           several such k, the lowest wins.  A seed that another seed's wave undercut
 *           (T[c] < t0_k) is not a root.
 *   Parent. Otherwise, the parent of a finite cell is its 4-neighbour with the smallest T strictly
 *           below T[c].  Among equal candidates the first in the order x-1, x+1, y-1, y+1 wins.  The
 *           label of c is the label of its parent.
 *   Unlabelled cells.  label = -1 for: a cell with T = +inf; a finite non-root cell with no strictly
 *           lower neighbour (a zero-cost plateau, or fp32 rounding of T + c to T); everything whose
 *           parent chain ends in such a cell.
 * Parents strictly decrease T, so they form a forest; the labels are a deterministic function of T and
 * the seed list. */
int eik_labels2d_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, const int64_t* seeds,
                     const double* t0, const int32_t* map_of, int64_t K, int32_t* d_label, void* stream);

/* Host buffers, one map: cost in, the seeded field T and (labels != NULL) its labels out. */
int eik_tmap2d_seeds_f32(eik_ctx* ctx, const float* cost, int64_t H, int64_t W, const int64_t* seeds, const double* t0,
                         int64_t K, float* T, int32_t* labels);
int eik_tmap2d_seeds_f64(eik_ctx* ctx, const double* cost, int64_t H, int64_t W, const int64_t* seeds, const double* t0,
                         int64_t K, double* T, int32_t* labels);

/* Replanning for goal sets: the incremental re-solve of a seeded field after cost changes AND seed-list
 * changes (no reference counterpart).  A goal dropped (sample collected, site ruled
 * out), added, or its start value changed is the same kind of event as a cost change.
 *
 * The solver remembers the bound seed list as a host copy: eik_fim2d_start_seeds / eik_fim2d_solve_seeds
 * set it, eik_fim2d_adopt_seeds sets it, every successful eik_fim2d_update_seeds replaces it.
 *
 * The rule.  One map.  The OLD seed list produced the converged field T_old.  The NEW list may be the
 * same.  For a cell c, b_old(c) is the smallest (R)t0 of the old seeds on c, or +inf if there is none.
 * b_new(c) is the same for the new list.  R is the solver's dtype and values compare as bit patterns.
 *   Root.           c is an old root when b_old(c) is finite and T_old[c] == b_old(c) bit for bit.  This
 *                   is the label rule's root.  A dominated seed, with T_old[c] < b_old(c), is an
 *                   ordinary cell.
 *   Spared root.    An old root with b_new(c) <= b_old(c).  It is never in the cone and hands no mark
 *                   on.  Its value is a boundary condition and its own cost is not used.  The single
 *                   goal of eik_fim2d_update is the case K = 1, t0 = 0.
 *   Released root.  An old root with b_new(c) > b_old(c), where removal means +inf.  It is a cone seed.
 *   Cone.           The cone is the closure of "p joins if a 4-neighbour q in the cone has
 *                   T_old(q) <= T_old(p), p finite, p not a spared root".  It is seeded with the
 *                   finite-T_old cells of the EIK_CHANGE_ANY rectangles and with the released roots.
 *   Restart state.  +inf on the cone and T_old elsewhere, then T[c] = min(T[c], b_new(c)) at every new
 *                   seed.  This state is a supersolution of the new problem.  The ordinary persistent
 *                   solve descends from it to the fixed point of the new cost and new list, which is
 *                   the field eik_fim2d_solve_seeds would give.
 *   Lowering edits. Lowered rectangles, added seeds and lowered t0 need no reset.
 *
 * rects, kinds, K: exactly as in eik_fim2d_update (semantics, kinds, clipping, K <= 1024).  seeds, t0,
 * Ks: the new list, checked as in eik_fim2d_start_seeds (a message names the offending index);
 * seeds == NULL with Ks == 0: the list stays as it is.  K == 0 with an unchanged list is a no-op:
 * nothing is queued, T keeps its bits, the info is zero and the solver stays converged.
 *
 * EIK_ERR_ARG with a message and nothing launched: everything eik_fim2d_update refuses (B > 1, ghost
 * strips, a layered block, not the persistent mode, a solver never started or adopted, a last solve that
 * did not converge, bad rectangles), a bad seed list, and a bound solve without a seed set ("the bound
 * solve has a single goal: eik_fim2d_update, or eik_fim2d_adopt_seeds first").
 *
 * eik_fim2d_adopt_seeds    binds d_cost / d_T where d_T is, by the caller's word, the converged field of
 *                          some earlier cost of this raster for this seed list; nothing is solved.
 * eik_fim2d_update_seeds   asynchronous: invalidates, re-seeds and queues the restart; eik_fim2d_iterate
 *                          then converges it.  The host arrays may be reused at once.
 * eik_fim2d_resolve_seeds  update + iterate to convergence (synchronous); a full priority-band ring
 *                          falls back to a full eik_fim2d_solve_seeds of the new list on the FIFO
 *                          (eik_fim2d_update_info out[5] = 1).
 * eik_fim2d_update_info    as for eik_fim2d_update: the cells invalidated include the released roots,
 *                          the tiles queued include those the new seeds queued.
 * Failures are those of eik_fim2d_resolve: after an error of the invalidation or of the re-solve the
 * bound T is INVALID -- it may hold sign-marked (negative) values and a partly reset cone, and spared
 * roots that were lifted for the invalidation may read +inf.  Solve from scratch
 * (eik_fim2d_solve_seeds) before the field or a further update is used.
 * Not covered: B > 1, the layered solver, 3D replanning (eik_fim3d_solve_seeds solves from scratch), a
 * seeded eik_plan2d_batch. */
int eik_fim2d_adopt_seeds(eik_fim2d* fim, const void* d_cost, void* d_T, const int64_t* seeds, const double* t0,
                          int64_t Ks, void* stream);
int eik_fim2d_update_seeds(eik_fim2d* fim, const int64_t* rects, const int* kinds, int64_t K, const int64_t* seeds,
                           const double* t0, int64_t Ks, void* stream);
int eik_fim2d_resolve_seeds(eik_fim2d* fim, const int64_t* rects, const int* kinds, int64_t K, const int64_t* seeds,
                            const double* t0, int64_t Ks, void* stream);
/* Host buffers: cost_new and T, the converged field of the earlier cost for the old list, go up; T comes
 * back as the field of cost_new for the new list (adopt_seeds with the old list, then resolve_seeds with
 * the new one, on the context's cached solver).  seeds_new == NULL with K_new == 0: the list is
 * unchanged.  labels != NULL: the labels of the new list, taken while the field is on the device. */
int eik_tmap2d_update_seeds_f32(eik_ctx* ctx, const float* cost_new, float* T_inout, int64_t H, int64_t W,
                                const int64_t* seeds_old, const double* t0_old, int64_t K_old, const int64_t* seeds_new,
                                const double* t0_new, int64_t K_new, const int64_t* rects, const int* kinds, int64_t K,
                                int32_t* labels);
int eik_tmap2d_update_seeds_f64(eik_ctx* ctx, const double* cost_new, double* T_inout, int64_t H, int64_t W,
                                const int64_t* seeds_old, const double* t0_old, int64_t K_old, const int64_t* seeds_new,
                                const double* t0_new, int64_t K_new, const int64_t* rects, const int* kinds, int64_t K,
                                int32_t* labels);

/* Rectangle-free replanning (no reference counterpart): a device diff of two cost rasters
 * names the rectangles and kinds that eik_fim2d_update needs, so the chain eik_costmap_dev ->
 * eik_fim2d_resolve_cost -> walk never leaves the device.
 *
 * Per cell: changed when old != new as values (+0 equals -0, +inf equals +inf); raised when new > old
 * (finite -> +inf is raised, +inf -> finite is lowered); invalid when new is NaN or < 0 (an invalid cell
 * counts as changed).  Per solver tile of 64 x 64 cells: the bounding box of its changed cells.
 * The rule from tiles to rectangles.  A changed tile's rectangle is its bounding box, of kind
 * EIK_CHANGE_ANY if the tile has a raised cell, else EIK_CHANGE_LOWERED.  More than cap rectangles: the
 * union per block of 2 x 2 tiles, aligned to the tile grid's origin -- the bounding box of the members,
 * ANY if any member is ANY -- then 4 x 4, 8 x 8, ... until at most cap are left.  Rectangles are emitted
 * in ascending (block row, block column).  The result is a deterministic function of the two rasters.
 *
 * What changed between two device rasters of one shape.  Synchronous (the records are read back).
 * rects: cap x (x0, y0, x1, y1) half-open, kinds: cap, *K rectangles written (0: the rasters are equal).
 * info[0] cells changed, [1] cells raised, [2] cells of d_new that are NaN or negative, [3] tiles
 * changed, [4] block side in tiles after coarsening (1, 2, 4, ...; 0 when K == 0), [5] device time in
 * microseconds.  1 <= cap <= 1024.  Invalid cells do not fail this call: info[2] reports them. */
int eik_cost_diff_dev(eik_ctx* ctx, const void* d_old, const void* d_new, int dtype, int64_t H, int64_t W,
                      int64_t* rects, int* kinds, int64_t cap, int64_t* K, int64_t info[6], void* stream);

/* Re-solve for a new cost raster without naming what changed.  d_cost_new is diffed against the bound
 * cost.  Then the solver is bound to d_cost_new (the old buffer is the caller's again: two buffers in
 * ping-pong, e.g. eik_costmap_dev's output) and re-solved with the rectangles and kinds of the diff.
 * A bound single goal goes through eik_fim2d_resolve.  A bound seed set goes through
 * eik_fim2d_resolve_seeds with the list unchanged.  Synchronous.
 *
 * EIK_ERR_ARG with a message and nothing launched: everything eik_fim2d_update refuses (B > 1, ghost
 * strips, a layered block, not the persistent mode, a solver never started or adopted, a last solve that
 * did not converge), and d_cost_new == NULL.
 * Invalid new costs (NaN or negative): EIK_ERR_ARG, the message names their count and the first such
 * cell; nothing is rebound, no update is launched and T keeps its bits.
 * Equal rasters: the solver is rebound, no update is queued, T keeps its bits, eik_fim2d_update_info is
 * zero and the solver stays converged (the K == 0 contract of eik_fim2d_update).
 * When the changed tiles, of either kind, are more than a share of the raster's tiles (DESIGN.md §3.15;
 * EIK_OPT_DIFF_SHARE) and more than 16, the solver is rebound and solves from scratch with the bound goal
 * or seed list (eik_fim2d_solve / eik_fim2d_solve_seeds on the new buffer); no rectangle list is built.
 * Failures after the rebind are those of eik_fim2d_resolve: the bound T is INVALID until a solve from
 * scratch (eik_fim2d_solve / eik_fim2d_solve_seeds on d_cost_new).
 *
 * eik_fim2d_diff_info  out[0..5]: info[0..5] of the last eik_fim2d_resolve_cost's diff, [6] 1 = it solved
 *                      from scratch by the share rule, [7] rectangles passed on.
 * Not covered: a windowed rebuild of the cost raster itself, B > 1, layered and 3D solvers, the
 * bidirectional fronts. */
int eik_fim2d_resolve_cost(eik_fim2d* fim, const void* d_cost_new, void* stream);
int eik_fim2d_diff_info(eik_fim2d* fim, int64_t out[8]);

/* Host buffers: both costs and T, the converged field of cost_old for the goal, go up; T comes back as the
 * field of cost_new (adopt on cost_old, then eik_fim2d_resolve_cost, on the context's cached solver). */
int eik_tmap2d_update_cost_f32(eik_ctx* ctx, const float* cost_old, const float* cost_new, float* T_inout,
                               int64_t H, int64_t W, int64_t gx, int64_t gy);
int eik_tmap2d_update_cost_f64(eik_ctx* ctx, const double* cost_old, const double* cost_new, double* T_inout,
                               int64_t H, int64_t W, int64_t gx, int64_t gy);

/* Live domain decomposition (no reference counterpart: the multi-GPU split of SURVEY.md §8(e)).
 * eik_fim2d_launch(fim, 1) starts ONE persistent launch on the bound stream and returns at once.
 * Its last workgroup is a halo agent serving a pinned host mailbox while the others solve; the
 * launch keeps serving its tile FIFO -- idle included -- until eik_fim2d_release.  Per round:
 *   live_pack(p)   the agent snapshots "tiles pending or busy", then stores the four edges of T
 *                  into send[p][side] (the neighbours' receive strips, e.g. eik_ipc_open'ed)
 *   (host barrier: every rank has packed)
 *   live_merge(p)  the agent min-merges recv[p][side] into the ghosts and queues the edge tiles
 *                  whose ghost dropped; *active = the pack's snapshot, *changed = ghosts lowered
 * The raster is converged when, in one round, every rank reports active == 0 and changed == 0.
 * eik_fim2d_live_bind sets the strips (index parity * 4 + side, NULL = no neighbour) before the
 * launch.  live = 0 is one ordinary persistent launch without the trailing synchronisation. */
int eik_fim2d_live_bind(eik_fim2d* fim, void* const send[8], void* const recv[8]);
int eik_fim2d_launch(eik_fim2d* fim, int live);
int eik_fim2d_live_pack(eik_fim2d* fim, int parity);
int eik_fim2d_live_merge(eik_fim2d* fim, int parity, int64_t* active, int64_t* changed);
/* end the live launch: wait for it on the bound stream; *active = tiles left (0 when converged) */
int eik_fim2d_release(eik_fim2d* fim, int64_t* active);

/* Sum of one integer over the `world` ranks of one node, through a shared-memory segment of
 * 64 * world bytes (zeroed before first use); round = 1, 2, ... on every rank in step.  Returns
 * EIK_ERR_HIP after timeout_s without the others.  (Per-round vote of the live decomposition.) */
int eik_node_allreduce(void* shm, int rank, int world, uint64_t round, int64_t value, int64_t* sum, double timeout_s);
/* the segment: POSIX shm `name` of `bytes` (create != 0: new and zeroed), mapped at *addr */
int eik_node_shm_open(const char* name, int64_t bytes, int create, void** addr);
int eik_node_shm_close(void* addr, int64_t bytes);
int eik_node_shm_unlink(const char* name);

/* Page-locked host memory for the drop-in's returned fields (FastMarching.computeTmap, ...): the
 * host entry points copy a registered pinned buffer as ONE DMA at PCIe speed instead of through
 * their staging ring (host threads memcpy'ing 8 MiB chunks), e.g. a field returned by
 * eik_tmap2d_f64 and handed back to eik_path2d_f64.  Thread-safe; no context needed. */
int eik_host_alloc(int64_t bytes, void** out);
int eik_host_free(void* p);

/* Device buffers shared between the processes of one node (hipIpc handles, 64 bytes). */
int eik_ipc_alloc(eik_ctx* ctx, int64_t bytes, void** d_ptr, unsigned char handle[64]);
int eik_ipc_free(eik_ctx* ctx, void* d_ptr);
int eik_ipc_open(eik_ctx* ctx, const unsigned char handle[64], void** d_ptr);
int eik_ipc_close(eik_ctx* ctx, void* d_ptr);

/* Self-test (no reference counterpart): the 2D path kernel's fast-path f64 square root,
 * division and interpolation against the exact forms they replace, on n pseudo-random inputs
 * each from their domain (gdm.hip walker_math_selftest_kernel); counts[0..2] = mismatches of
 * each (0 expected), counts[3] = samples evaluated (n), counts[4] = mismatches of the division
 * taken from the square root's reciprocal (path loop forms 3-4), counts[5] = mismatches of the
 * one-correction square root (form 4); 0 expected in both. */
int eik_selftest_walker_math(eik_ctx* ctx, int64_t n, uint64_t seed, int64_t counts[6]);

/* getPathGDM on a device-resident field; out/n_out/status are device pointers. */
int eik_path2d_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t H, int64_t W, const double init[2],
                   const double end[2], double tau, double* d_out, int64_t cap, int64_t* d_n_out, int* d_status,
                   void* stream);

/* ---- batched paths: P getPathGDM walks in one launch (no reference counterpart) -----------
 * d_T holds B fields of one shape ([B][H][W], dtype); path p walks field map_of[p] from
 * inits[p] to ends[p] (P x 2 rows of (x, y)) into d_out + p * cap * 2, d_n_out[p], d_status[p]
 * (an eik_path_status per path: one path that errors or falls back does not fail the call).  Every
 * path is bit-identical to eik_path2d_dev on its field with the same tau and cap.
 * map_of, inits, ends are HOST arrays of P entries, read before the call returns and put on the
 * device in stream order (calls issued back to back on one stream need no synchronisation between
 * them); map_of == NULL: path p walks field p when P == B, field 0 when B == 1.
 * EIK_ERR_ARG (checked on the host, nothing launched): a map_of entry outside [0, B), map_of NULL
 * with P != B and B > 1, P < 1, cap < 2, H or W < 3, tau <= 0, a NULL pointer.
 * One workgroup per path on its own CU: P above the CU count runs in rounds.  Async on `stream`. */
int eik_path2d_batch_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, int64_t P,
                         const int32_t* map_of, const double* inits, const double* ends, double tau, double* d_out,
                         int64_t cap, int64_t* d_n_out, int* d_status, void* stream);

/* The same on host buffers (synchronous): T: B*H*W fp64, uploaded once; out: P x cap x 2, of which
 * path p's first n_out[p] rows are written (the rest is left as it was); n_out, status: P. */
int eik_path2d_batch_f64(eik_ctx* ctx, const double* T, int64_t B, int64_t H, int64_t W, int64_t P,
                         const int32_t* map_of, const double* inits, const double* ends, double tau, double* out,
                         int64_t cap, int64_t* n_out, int* status);

/* ---- obstacle-safe 2D paths (no reference counterpart beyond the cited lines) ---------------
 * getPathGDM stops at, tunnels through or stalls beside +inf cells (it is the reference's walk,
 * kept bit for bit above).  These entries walk the same field by a rule that does not:
 *   G' = computeGradient's (Gnx, Gny) with NaN at every node whose T is +inf.  Per iteration
 *   (round(15000 / tau) of them), p the last point:
 *     - the reference's step (:175-176, :220-230, the default walker's bits) unless the
 *       interpolation of G' at p is NaN or the walk is in integer mode;
 *     - else the fallback of :178-218 as intended (FastMarching3D.py:212-264): n = rint(p), half to
 *       even; while T[n] is +inf drop the last point and take n from the one before (none left:
 *       EIK_PATH_ERROR); drop the points closer than 1 to n; append n; append the 4-neighbour of n
 *       with the smallest T strictly below T[n] (scanned y-1, y+1, x-1, x+1, the first wins ties;
 *       none: EIK_PATH_STUCK);
 *     - stop within 1.5 of end (EIK_PATH_DONE, end appended);
 *     - stall rule: when T at the nearest node of the new point has not fallen below its running
 *       minimum for S = max(16, ceil(8 / tau)) iterations in a row, every later iteration takes
 *       the fallback (integer mode).
 *   A NaN point, a negative coordinate or an interpolation cell outside the raster is
 *   EIK_PATH_ERROR; a budget that runs out short of the stop radius is EIK_PATH_STUCK (rows: ERROR).
 *   Rows grow by at most one per iteration, so cap is the default walker's.
 * Guarantee: with tau <= 0.5, a converged field and finite T[init], the status is DONE or STUCK by
 * budget, and no emitted point has a +inf node as its nearest node.  Segments between points are
 * NOT swept: a step may pass the gap between two impassable cells that touch only at a corner.
 * The path equals getPathGDM's up to the first blocked step or stall and differs only from there on.
 * tau: 0 < tau <= 1 (a step longer than a cell cannot be made safe by sampling points), else
 * EIK_ERR_ARG, as everything eik_path2d_dev / eik_path2d_batch_dev check.
 * info (nullable; int64[4] per path): fallbacks taken, points dropped, the first iteration run in
 * integer mode (-1: never), iterations run.  Layout, staging and rounds as the entries above. */
int eik_path2d_safe_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t H, int64_t W, const double init[2],
                        const double end[2], double tau, double* d_out, int64_t cap, int64_t* d_n_out, int* d_status,
                        int64_t* d_info, void* stream);
int eik_path2d_safe_f64(eik_ctx* ctx, const double* T, int64_t H, int64_t W, const double init[2], const double end[2],
                        double tau, double* out, int64_t cap, int64_t* n_out, int* status, int64_t info[4]);
int eik_path2d_safe_batch_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, int64_t P,
                              const int32_t* map_of, const double* inits, const double* ends, double tau,
                              double* d_out, int64_t cap, int64_t* d_n_out, int* d_status, int64_t* d_info,
                              void* stream);
int eik_path2d_safe_batch_f64(eik_ctx* ctx, const double* T, int64_t B, int64_t H, int64_t W, int64_t P,
                              const int32_t* map_of, const double* inits, const double* ends, double tau, double* out,
                              int64_t cap, int64_t* n_out, int* status, int64_t* info);

/* FastMarching3D.getPathGDM, batched as above: d_T [B][H][W][L]; inits, ends: P x 3 (x, y, z);
 * d_out: P x cap x 3.  Every path is bit-identical to eik_path3d_dev.  EIK_ERR_ARG as above, with
 * H, W or L < 1 for the shape. */
int eik_path3d_batch_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t B, int64_t H, int64_t W, int64_t L,
                         int64_t P, const int32_t* map_of, const double* inits, const double* ends, double tau,
                         double* d_out, int64_t cap, int64_t* d_n_out, int* d_status, void* stream);
int eik_path3d_batch_f64(eik_ctx* ctx, const double* T, int64_t B, int64_t H, int64_t W, int64_t L, int64_t P,
                         const int32_t* map_of, const double* inits, const double* ends, double tau, double* out,
                         int64_t cap, int64_t* n_out, int* status);

/* End to end on B maps (terrain Monte-Carlo, goal sweep): eik_tmap2d_batch_f32's solve, the fields
 * kept on the device, then one batched walk from starts[b] (B x 2 doubles) to goals[b] (B x 2,
 * (x, y)) on fp32 field b.  paths: B x cap x 2, n_out, status: B (per map; a start outside map b is
 * that path's EIK_PATH_ERROR).  Only the paths come back, and the B*H*W fields too when T_out is
 * not NULL.  Synchronous. */
int eik_plan2d_batch_f32(eik_ctx* ctx, const float* cost, int64_t B, int64_t H, int64_t W, const int64_t* goals,
                         const double* starts, double tau, double* paths, int64_t cap, int64_t* n_out, int* status,
                         float* T_out);

/* 3D solve on device buffers (synchronous: returns after convergence; stats via
 * eik_get_stats). */
int eik_fim3d_solve(eik_ctx* ctx, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int dtype,
                    const int64_t goal[3], void* stream);

/* Goal sets for 3D solves (no reference counterpart): the field of a SET of K seeds in
 * one volume, seed k at cell (x, y, z) with start value t0[k] >= 0,
 *     T = min_k (t0[k] + cost-to-go from seed k)
 * as the solver's own discrete fixed point (below the pointwise minimum of K single-goal fields, as in
 * 2D above), and the nearest-goal label of every cell.  Several admissible final arm waypoints, each with
 * a penalty: one field and the partition, not K solves.
 * Two seeds may name one cell (the lower t0 holds); a seed that another seed's wave undercuts is
 * dominated (T there ends below its t0).  A seed on a +inf-cost cell keeps its t0.
 *
 * seeds: K x (x, y, z), host.  t0: K host doubles, rounded to dtype, or NULL (all 0).  The host arrays
 * are read before the call returns and go to the device in stream order through a pinned block.
 *
 * eik_fim3d_solve_seeds  synchronous, like eik_fim3d_solve.  By default it always runs on the general 3D
 *                        solver -- the persistent driver while the volume is under 4 GiB and the context
 *                        is in persistent mode, else the list driver -- also for the few-layer volumes
 *                        that eik_fim3d_solve gives to the layered solver.  With EIK_OPT_SEEDS_LAYERED = 1
 *                        it routes as eik_fim3d_solve does for one goal: the layered solver takes the
 *                        volume when the context is in persistent mode, EIK_OPT_MAX_ROUNDS is 1, a tile
 *                        row band of the volume is under 4 GiB, the volume has at most 4 (fp32) / 3
 *                        (fp64) layers -- or two more, the first and last all +inf -- and every seed's z
 *                        lies among the solved layers; otherwise the general solver runs as before (a
 *                        seed in a padding layer feeds its z neighbour, and the layered solver never
 *                        reads the padding).  The field obeys the same bounds on either solver.
 *                        eik_get_stats, EIK_OPT_PASSES, EIK_OPT_GRID, EIK_OPT_QTIMEOUT and
 *                        EIK_OPT_MAX_VISITS behave as in eik_fim3d_solve (on the layered solver also
 *                        EIK_OPT_PRIO, with the seeds' t0 as keys, and EIK_OPT_LAYER_PLANAR).
 * eik_fim3d_last_solver  what the last 3D solve on the context (eik_fim3d_solve, eik_fim3d_solve_seeds and
 *                        the host entries above them) ran on: out[0] = 1 the layered solver, 0 the
 *                        general one; out[1] = z0, the first solved layer; out[2] = nl, the solved layers
 *                        (0 on the general solver); out[3] = 1 when priority bands were set up.
 * eik_labels3d_dev       the labels of a converged field d_T of H x W x L cells in dtype (fewer than 2^31
 *                        cells) for the seed list that produced it -> d_label, int32 [H][W][L], device.
 *                        Asynchronous on `stream`, no read-back.  The context owns the scratch (shared
 *                        with eik_labels2d_dev): calls on one stream queue up, calls on different streams
 *                        must not overlap.
 * The label rule is eik_labels2d_dev's with 6 neighbours:
 *   Root.   Cell c is a root with label k when seed k lies on c and T[c] == (R)t0_k bit for bit.  Of
 *           several such k, the lowest wins.  A seed that another seed's wave undercut is not a root.
 *   Parent. Otherwise, the parent of a finite cell is its 6-neighbour with the smallest T strictly
 *           below T[c].  Among equal candidates the first in the order x-1, x+1, y-1, y+1, z-1, z+1
 *           wins.  The label of c is the label of its parent.
 *   Unlabelled cells.  label = -1 for: a cell with T = +inf; a finite non-root cell with no strictly
 *           lower neighbour (a zero-cost plateau, or fp32 rounding of T + c to T); everything whose
 *           parent chain ends in such a cell.
 *
 * EIK_ERR_ARG, with a message naming the offending index and nothing launched: K < 1 or K > 2^24, a
 * NULL pointer, a seed outside the volume, a t0 that is negative, NaN or +inf or (fp32) rounds to +inf,
 * H, W or L < 1.
 * Not covered: seeds on decomposition blocks (eik_fim3dl_* handles), 3D replanning, B > 1 volumes per
 * call, early exit with a seed set. */
int eik_fim3d_solve_seeds(eik_ctx* ctx, const void* d_cost, void* d_T, int64_t H, int64_t W, int64_t L, int dtype,
                          const int64_t* seeds, const double* t0, int64_t K, void* stream);
int eik_fim3d_last_solver(const eik_ctx* ctx, int64_t out[4]);
int eik_labels3d_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t H, int64_t W, int64_t L, const int64_t* seeds,
                     const double* t0, int64_t K, int32_t* d_label, void* stream);

/* Host buffers, one volume: cost in, the seeded field T and (labels != NULL) its labels out. */
int eik_tmap3d_seeds_f32(eik_ctx* ctx, const float* cost, int64_t H, int64_t W, int64_t L, const int64_t* seeds,
                         const double* t0, int64_t K, float* T, int32_t* labels);
int eik_tmap3d_seeds_f64(eik_ctx* ctx, const double* cost, int64_t H, int64_t W, int64_t L, const int64_t* seeds,
                         const double* t0, int64_t K, double* T, int32_t* labels);

/* FastMarching3D.computeTmap's early exit at `start` (:141) on device buffers: d_T (a converged
 * full field from eik_fim3d_solve) -> d_Te (a different buffer), async on `stream`. */
int eik_fim3d_early_exit(eik_ctx* ctx, const void* d_cost, const void* d_T, void* d_Te, int64_t H, int64_t W,
                         int64_t L, int dtype, const int64_t goal[3], const int64_t start[3], void* stream);

/* FastMarching3D.getPathGDM on a device-resident field. */
int eik_path3d_dev(eik_ctx* ctx, const void* d_T, int dtype, int64_t H, int64_t W, int64_t L, const double init[3],
                   const double end[3], double tau, double* d_out, int64_t cap, int64_t* d_n_out, int* d_status,
                   void* stream);

/* ---- cost-raster builder (the solver's input producer) ----------
 * Coupled_motion_planner.py main(), :1101-1216: DEM -> surface normals -> slope obstacles ->
 * hole filling, disk erode/dilate -> 300 x obstacle + 10 x distance ramp -> 50 x 50 box blur ->
 * +inf border.  Constants default to the reference's (slope 0.20 rad, rover diagonal 0.9 m,
 * expansion 1 m, gradient 10, obstacle cost 300) when params is NULL. */
typedef struct {
    double slope_max;  /* rad, :1154 */
    double diagonal;   /* m, rover body diagonal (corridor erosion radius = diagonal / 2), :1172 */
    double expansion;  /* m, obstacle cost ramp radius, :1190 */
    double gradient;   /* ramp cost scale, :1202 */
    double high;       /* obstacle cost, :1187 */
} eik_costmap_params;

/* Z: H x W DEM (row-major, Zs of :1098-1101, spacing size / (n - 1) as linspace(0, size, n)).
 * cost_out: H x W, [y][x] -- the reference's cMap.T, i.e. the array it passes to
 * FM.biComputeTmap (:1222); obst_out (nullable): the final obstacle map (:1180-1184), 0/1. */
int eik_costmap_f64(eik_ctx* ctx, const double* Z, int64_t H, int64_t W, double resolution, double size,
                    const eik_costmap_params* params, double* cost_out, uint8_t* obst_out);
/* the same on device buffers, async on `stream` except the two hole-filling solves */
int eik_costmap_dev(eik_ctx* ctx, const double* d_Z, int64_t H, int64_t W, double resolution, double size,
                    const eik_costmap_params* params, double* d_cost, uint8_t* d_obst, void* stream);
/* The cost tail alone (:1180-1216; the code eik_costmap_* runs for it): obst is the H x W 0/1 obstacle
 * mask as it stands after :1177, H, W >= 3, resolution > 0.  cost_out [y][x] and obst_out (nullable)
 * as eik_costmap_f64 returns them. */
int eik_cost_tail_u8(eik_ctx* ctx, const uint8_t* obst, int64_t H, int64_t W, double resolution,
                     const eik_costmap_params* params, double* cost_out, uint8_t* obst_out);
/* surface_normal(resolution, size, z) :37-80 -> unit normals (H x W each) */
int eik_surface_normal_f64(eik_ctx* ctx, const double* Z, int64_t H, int64_t W, double size, double* Nx, double* Ny,
                           double* Nz);
/* image_filling(im) :82-94 (cv2.floodFill from (0, 0), 4-connected) on a 0/1 uint8 image */
int eik_image_fill_u8(eik_ctx* ctx, const uint8_t* im, int64_t H, int64_t W, uint8_t* out);
/* cv2.erode / cv2.dilate with the reference's structural_disk(radius) (Coupled_motion_planner.py:96-105,
 * :1168-1177, :1192) on a 0/1 uint8 mask: erode != 0 -> erosion; pixels outside the image take no part. */
int eik_disk_morph_u8(eik_ctx* ctx, const uint8_t* im, int64_t H, int64_t W, int radius, int erode, uint8_t* out);

/* ---- rover path of the planner -----------------------------------
 * Coupled_motion_planner.py main(), step 1 (:1097-1258): DEM -> cost raster (eik_costmap_*) ->
 * biComputeTmap(cMap.T, sample node, rover node) -> getPathGDM from nodeJoin to each end ->
 * roverPath = [flipud(pathS); pathG[1:]] in metres (res * (p + 1)), waypoints within 0.1 m of the
 * rover or the sample dropped, z = zp + Zs[round(y / res), round(x / res)], heading =
 * [initialHeading, atan2(dy, dx)...].  Nodes: pxm = int(round(xm / res - 1)) etc. (:1107-1117,
 * Python's round: half to even).  Defaults of the reference: zp 0.07 (:1132), tau 0.5 (:1225). */
typedef struct {
    double xm, ym;            /* sample position (m), :1107-1108                                 */
    double xr, yr;            /* rover position (m), :1115-1116                                  */
    double initial_heading;   /* rad, :1254                                                      */
    double resolution, size;  /* DEM spacing (m) and side (m) as main()'s arguments              */
    double zp;                /* height of the rover reference system above the floor, :1132     */
    double tau;               /* GDM step (cells), :1225-1226                                    */
} eik_rover_query;

/* Host-only tail of step 1 (no GPU, no context): from the two GDM paths (K x 2 cell coordinates,
 * pathS from nodeJoin to the rover node, pathG from nodeJoin to the sample node) and the DEM Z
 * (H x W, raw heights: the min shift of :1101 is applied here) to path_xyz (cap x 3, metres) and
 * heading (cap).  *n_out = rows written; EIK_ERR_ARG if cap is too small or a waypoint falls
 * outside Z (the reference raises IndexError there). */
int eik_rover_assemble(const double* pathS, int64_t nS, const double* pathG, int64_t nG, const double* Z, int64_t H,
                       int64_t W, const eik_rover_query* q, double* path_xyz, double* heading, int64_t cap,
                       int64_t* n_out);

/* The whole of step 1 on the GPU: cost raster, both fronts as one 2-map fp64 batch, the device
 * join, the two path kernels, then eik_rover_assemble on the host.  Z: H x W host DEM.  join
 * (nullable) receives nodeJoin; cost_out (nullable, H x W [y][x]) the cost raster.
 * EIK_ERR_UNREACHABLE when the rover cannot reach the sample. */
int eik_rover_path_f64(eik_ctx* ctx, const double* Z, int64_t H, int64_t W, const eik_rover_query* q,
                       const eik_costmap_params* params, double* path_xyz, double* heading, int64_t cap,
                       int64_t* n_out, uint32_t join[2], double* cost_out);

/* ---- end-effector cost volume of the planner ---------------------
 * Coupled_motion_planner.py main(), step 3 (:1462-1593): the arm's FM3D runs on
 * Cmap = GetObstMap(...)[0] * TunnelCost(...) over a small square area around the sample.  The
 * volume is [iy][ix][iz], sY x sX x sZ with sX == sY (the planner's area is square, :1519). */
typedef struct {
    int64_t sX, sY, sZ;              /* nodes per axis, :1528-1529                                 */
    double resX, resY, resZ;         /* m per node, :1532-1534                                     */
    double xm, ym;                   /* GetObstMap's sample test: columns with resX*i == xm or
                                        resY*j == ym are skipped (:329; the planner passes the
                                        global sample position)                                    */
    double rlim, rO, rm;             /* TunnelCost(Rlim, rO, rm, ...), :1577 (Rlim, rO, rm :1121-1124) */
    uint32_t final_wp[3];            /* sample node (x, y, z), :1574                                */
    uint32_t initial_wp[3];          /* end-effector start node (x, y, z), :1573                    */
} eik_arm_volume;

/* GetObstMap(ZsMap, resX, resY, resZ, sX, sY, sZ, newObstMap, xm, ym) :319-358.  ZsMap, newObstMap:
 * m x n (row j = y).  finalMap (2 / +inf), obstMap and groundMap (1 / +inf; nullable): sX*sY*sZ. */
int eik_arm_obst_map_f64(eik_ctx* ctx, const double* ZsMap, const double* newObstMap, int64_t m, int64_t n,
                         const eik_arm_volume* vol, double* finalMap, double* obstMap, double* groundMap);

/* TunnelCost(rlim, rO, rm, gamma2D, sX, sY, sZ, resX, resY, resZ, finalBaseHeading, finalWayPointArm,
 * initialWayPointArm) :505-725.  gamma2D, heading: npts x 3 (arm base positions in the area's frame,
 * (roll, pitch, yaw) per point).  Cmap: sY*sX*sZ (10 / tunnel cost / +inf), bit-identical to the
 * reference (tests/golden/arm.npz). */
int eik_arm_tunnel_cost_f64(eik_ctx* ctx, const double* gamma2D, const double* heading, int64_t npts,
                            const eik_arm_volume* vol, double* Cmap);

/* :1562-1593 on the GPU: Cmap = finalMap * tunnel on the device -> FM3D.computeTmap(Cmap,
 * finalWayPointArm, initialWayPointArm) -> FM3D.getPathGDM(T, initialWayPointArm, finalWayPointArm,
 * tau) -> path (cap x 3 node coordinates, before the planner's scaling and smoothing, :1588-1598).
 * The field is computeTmap's early-exit field at initialWayPointArm (eik_tmap3d_early_f64).
 * cost_out / T_out (nullable): the volume and that arrival field, sY*sX*sZ. */
int eik_arm_path_f64(eik_ctx* ctx, const double* ZsMap, const double* newObstMap, int64_t m, int64_t n,
                     const double* gamma2D, const double* heading, int64_t npts, const eik_arm_volume* vol, double tau,
                     double* path, int64_t cap, int64_t* n_out, int* status, double* cost_out, double* T_out);

/* FastMarching3D.computeTmap on B independent volumes of one shape in ONE solve (candidate fetch
 * poses): cost, T: B*H*W*L; goals: B x (x, y, z). */
int eik_tmap3d_batch_f64(eik_ctx* ctx, const double* cost, int64_t B, int64_t H, int64_t W, int64_t L,
                         const int64_t* goals, double* T);

/* ---- DEM ingest, host only: no GPU, no context --------------------
 * Coupled_motion_planner.py:1098-1099 reads PRL_DEM.txt as comma-separated rows with a Python
 * float() per value.  eik_load_dem_txt parses the same text with host threads (nthreads <= 0:
 * all cores), bit-identical values (correctly rounded parsing).  out == NULL: only H, W.
 * Errors: EIK_ERR_ARG, message from eik_io_last_error(). */
int eik_load_dem_txt(const char* path, double* out, int64_t cap, int64_t* H, int64_t* W, int nthreads);
const char* eik_io_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* EIKONAL_H_ */
