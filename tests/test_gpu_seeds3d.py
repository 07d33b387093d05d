"""Goal sets for 3D solves on the GPU (eik_fim3d_solve_seeds, eik_labels3d_dev, eik_tmap3d_seeds_*,
DESIGN.md §3.16).

The expected field of a seed set is tests/seeds3d_np.seeded_reference3: the fixed point from above of
T = min(T, update) with the update of FastMarching3D.py:59-75 -- NOT the minimum of single-goal fields,
which lies above it.  Bounds are the suite's (handoff3d.ATOL64 / RTOL32): reachability masks identical,
fp64 <= 1e-9 absolute, fp32 <= 2e-5 relative (costs go through float32, the t0 values are exact in
float32).  Labels are compared for exact equality with the numpy rule (seeds3d_np.label_rule3) applied to
the GPU's own field.

Every case runs in both dtypes on the persistent driver and in list mode; both contexts carry
EIK_OPT_QTIMEOUT 5, so a lost activation is an error and not a hang.

The plateau of the "chambers" case.  FastMarching3D.py:59-75 accepts no n at C = 0 (its test is
C^2 > sum (Tmax - Ti)^2 with a strict >, and the reference raises once its list is empty), so a cell of
cost exactly 0 has no value in the specification; the fp64 solver, which computes in the reference's own
arithmetic (solve3_ref), leaves it at +inf, and the fp32 solver's cancellation-free form takes its one-axis
branch a + C = a.  A plateau that is FINITE in both dtypes and in the specification therefore needs a cost
that is zero to working precision, not exactly: a corridor one cell wide of cost 2^-80 between +inf walls.
Its cells see one finite axis (n = 1), where (C^2 + w^2) - w^2 cannot be negative, and T + 2^-80 rounds to
T in either dtype: the corridor holds its entry's value all along, no cell has a strictly lower neighbour,
and the label is -1 inside it and behind it.  The block of cost exactly 0 is there as well: its labels are
-1 whatever its T is, and they must equal the rule on the device's own field.
"""
import ctypes
import functools

import numpy as np
import pytest

import handoff3d as HO
from seeds3d_np import (FIVE_SEEDS, FIVE_SHAPE, FIVE_T0, FIVE_UNDOMINATED, label_rule3, seeded_reference3, undominated3)
from test_seeds_abi import raster

pytestmark = pytest.mark.gpu

DRIVERS = ["persistent", "list"]
F64 = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
TINY = 2.0 ** -80  # exact in float32; T + TINY == T for every T >= 2^-56 (fp64) / 2^-103 (fp32)


def _context(driver):
    import eikonal
    from eikonal import _lib as L

    return eikonal.Context(0, options={"MODE": L.MODE_PERSISTENT if driver == "persistent" else L.MODE_LIST, "QTIMEOUT": 5})


@pytest.fixture(scope="module")
def ctxs():
    cs = {d: _context(d) for d in DRIVERS}
    for d, c in cs.items():
        c.driver = d  # (solve() checks that the driver asked for ran)
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module", params=DRIVERS)
def ctx(request, ctxs):
    return ctxs[request.param]


def dt(f64):
    return np.float64 if f64 else np.float32


def solve(c, cost, seeds, t0, f64, labels=True):
    """eik_fim3d_solve_seeds on device buffers, then eik_labels3d_dev on the field where it lies"""
    import torch
    from eikonal import _lib as L

    dev = torch.device("cuda", 0)
    cd = torch.from_numpy(np.array(cost, dt(f64), order="C")).to(dev)
    Td = torch.full_like(cd, float("nan"))
    H, W, Lz = cost.shape
    c.fim3d_solve_seeds(cd.data_ptr(), Td.data_ptr(), H, W, Lz, L.EIK_F64 if f64 else L.EIK_F32, seeds, t0,
                        torch.cuda.current_stream(dev).cuda_stream)
    s = c.stats()
    # the general solver on the driver asked for: the persistent driver is one launch with one host sync,
    # the list driver counts its sweeps; the layered solver (fresh_visits > 0) never
    assert s["fresh_visits"] == 0 and s["tile_visits"] > 0
    assert (s["host_syncs"] == 1 and s["iterations"] == 1) == (c.driver == "persistent"), s
    T = Td.cpu().numpy()
    if not labels:
        return T
    lab = c.labels3d(Td, seeds, t0)
    assert lab.dtype == torch.int32 and lab.shape == Td.shape
    return T, lab.cpu().numpy()


def close(T, R, f64):
    """the suite's bounds between a field and its expected values"""
    assert T.shape == R.shape
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    if not fin.any():
        return
    err = np.abs(T[fin].astype(np.float64) - R[fin])
    print(f"max abs err {err.max():.3e}")
    if f64:
        assert err.max() <= HO.ATOL64, err.max()
    else:
        rel = err / np.maximum(np.abs(R[fin]), 1e-30)
        rel[R[fin] == 0] = err[R[fin] == 0]
        print(f"max rel err {rel.max():.3e}")
        assert rel.max() <= HO.RTOL32, rel.max()


def _low(seeds, t0, k):
    """the lowest t0 named for seed k's cell"""
    return min(v for s, v in zip(seeds, t0) if tuple(s) == tuple(seeds[k]))


def check_seeded(T, R, seeds, t0, f64):
    """masks identical, the suite's bounds, and every seed's cell exactly its cell's lowest t0 where the
    reference says no other seed's wave undercut it, strictly below it otherwise"""
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    assert all(float(dt(f64)(v)) == v for v in t0), "the t0 values must be exact in float32"
    assert any(undominated3(R, seeds, t0)), "every case needs an undominated seed"
    for k, (x, y, z) in enumerate(seeds):
        low = _low(seeds, t0, k)
        if R[y, x, z] == low:
            assert T[y, x, z] == T.dtype.type(low), (k, T[y, x, z])
        else:
            assert T[y, x, z] < T.dtype.type(low), (k, T[y, x, z])
    close(T, R, f64)


def check_labels(lab, T, R, seeds, t0):
    """exact equality with the numpy rule on the GPU's own field; every undominated seed's cell carries its
    own k (the lowest k of equal seeds on one cell), a dominated seed's another seed's"""
    assert lab.dtype == np.int32
    want = label_rule3(T, seeds, t0)
    assert np.array_equal(lab, want), f"{(lab != want).sum()} labels differ from the rule"
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    und = undominated3(R, seeds, t0)
    for k, (x, y, z) in enumerate(seeds):
        first = min(j for j, s in enumerate(seeds) if tuple(s) == (x, y, z) and t0[j] == t0[k])
        if und[k]:
            assert lab[y, x, z] == first, (k, lab[y, x, z])
        else:
            assert lab[y, x, z] != k, k


# ---------------------------------------------------------------------------------- the cases
def _cut(shape):
    """three seeds at distinct t0 in a cut_cost3 volume (5 % +inf), the seeds' cells open"""
    H, W, Lz = shape
    seeds = [(1, 1, 0), (W - 2, H - 2, Lz - 1), (W // 2, H // 2, Lz // 2)]
    cost = HO.cut_cost3(shape, seeds[0], salt=3)
    for x, y, z in seeds:
        cost[y, x, z] = 1.0
    return cost, seeds, [0.0, 2.5, 1.0]


def _ball():
    """every cell within 5 of the centre tile's centre, all at 0: the ball reaches past the tile's y and z
    faces (rows 7 .. 17 of tile rows 8 .. 15), so many pushes land on one tile and its neighbours"""
    ys, xs, zs = np.mgrid[0:FIVE_SHAPE[0], 0:FIVE_SHAPE[1], 0:FIVE_SHAPE[2]]
    m = (xs - 24) ** 2 + (ys - 12) ** 2 + (zs - 12) ** 2 <= 25
    seeds = [(int(x), int(y), int(z)) for y, x, z in zip(*np.nonzero(m))]
    assert 480 <= len(seeds) <= 560 and {7, 17} <= {s[1] for s in seeds} and {7, 17} <= {s[2] for s in seeds}
    return raster(FIVE_SHAPE, 31), seeds, None


CHAMBER_SEEDS, CHAMBER_T0 = [(3, 3, 3), (40, 20, 20)], [0.0, 4.0]
CORRIDOR = (12, slice(2, 14), 12)   # cost[y, x, z]: one cell wide along x, between +inf walls
ZERO_BLOCK = (slice(3, 8), slice(6, 12), slice(15, 21))


def _chambers():
    """walls of +inf cost at x = 16 and x = 32: the chambers x < 16 and x > 32 hold a seed each, the one
    between them none.  In the first chamber, the plateau corridor and the block of cost exactly 0 of the
    module docstring."""
    cost = raster(FIVE_SHAPE, 11)
    cost[:, 16, :] = cost[:, 32, :] = np.inf
    cost[11:14, 2:14, 11:14] = np.inf
    cost[CORRIDOR] = TINY
    return cost, CHAMBER_SEEDS, CHAMBER_T0


def _inf_seed():
    cost = raster(FIVE_SHAPE, 12)
    cost[10, 30, 10] = np.inf  # the second seed's own cell
    return cost, [(3, 3, 3), (30, 10, 10)], [0.0, 2.0]


CASES = {
    "five": lambda: (raster(FIVE_SHAPE), FIVE_SEEDS, FIVE_T0),
    "cut17x33x9": lambda: _cut((17, 33, 9)),     # two z tiles, one of them a single layer
    "cut20x40x6": lambda: _cut((20, 40, 6)),     # 16 x 8 x 6 tiles
    "cut33x35x3": lambda: _cut((33, 35, 3)),     # 16 x 16 x 3 tiles: the single-goal entry's layered shape
    "ball": _ball,
    "pair": lambda: (raster(FIVE_SHAPE, 32), [(20, 9, 9), (20, 9, 9)], [7.0, 3.0]),
    "chambers": _chambers,
    "inf_seed": _inf_seed,
}


@functools.lru_cache(maxsize=None)
def case(name):
    cost, seeds, t0 = CASES[name]()
    R = seeded_reference3(cost, seeds, t0)
    cost.setflags(write=False)
    R.setflags(write=False)
    return cost, seeds, t0, R


@F64
@pytest.mark.parametrize("name", ["five", "cut17x33x9", "cut20x40x6", "cut33x35x3", "ball", "inf_seed"])
def test_field_and_labels(ctx, name, f64):
    cost, seeds, t0, R = case(name)
    T, lab = solve(ctx, cost, seeds, t0, f64)
    check_seeded(T, R, seeds, t0, f64)
    check_labels(lab, T, R, seeds, t0)
    if name == "five":
        assert undominated3(R, seeds, t0) == FIVE_UNDOMINATED
        assert lab[7, 15, 7] == 3  # (15, 7, 7): undercut from the first cell of the diagonal neighbour tile
        assert set(np.unique(lab)) == {0, 1, 3}
    if name == "ball":
        assert (lab >= 0).all() and len(np.unique(lab)) > 100
    if name == "inf_seed":
        assert T[10, 30, 10] == 2.0 and lab[10, 30, 10] == 1  # the seed on a +inf-cost cell keeps its t0


@F64
def test_two_seeds_on_one_cell(ctx, f64):
    """K = 2 on one cell at t0 = (7, 3): the lower value holds and the label is 1"""
    cost, seeds, t0, R = case("pair")
    T, lab = solve(ctx, cost, seeds, t0, f64)
    assert T[9, 20, 9] == 3.0 and lab[9, 20, 9] == 1
    check_seeded(T, R, seeds, t0, f64)
    check_labels(lab, T, R, seeds, t0)
    assert (lab == 1).all()


@F64
@pytest.mark.parametrize("face", HO.FACES)
def test_lone_exit(ctx, face, f64):
    """the one seed, at t0 = 5, lies on a tile face with every neighbour +inf but the one across that face:
    only the seeding can hand it over (for_goal_tiles).  Field = 5 + the single-goal oracle field."""
    goal = HO.lone3_goal(face)
    cost = HO.lone_exit_cost(HO.LONE3_SHAPE, goal, face)
    R = 5.0 + HO.oracle_field(("lone3", face), cost, goal)
    x, y, z = HO.lone_exit_cell(goal, face)
    assert np.isfinite(R[y, x, z]) and HO.corners_finite(R)
    T, lab = solve(ctx, cost, [goal], [5.0], f64)
    assert T[goal[1], goal[0], goal[2]] == 5.0
    close(T, R, f64)
    assert np.array_equal(lab, label_rule3(T, [goal], [5.0]))
    assert np.array_equal(lab >= 0, np.isfinite(R)) and lab[goal[1], goal[0], goal[2]] == 0


@F64
def test_chambers_and_plateau(ctx, f64):
    cost, seeds, t0, R = case("chambers")
    T, lab = solve(ctx, cost, seeds, t0, f64)
    check_seeded(T, R, seeds, t0, f64)
    check_labels(lab, T, R, seeds, t0)
    # the unseeded chamber
    open_mid = np.isfinite(cost[:, 17:32, :])
    assert open_mid.any() and np.isinf(T[:, 17:32, :]).all() and (lab[:, 17:32, :] == -1).all()
    assert set(np.unique(lab[:, :16, :])) == {-1, 0} and set(np.unique(lab[:, 33:, :])) == {1}
    # the plateau: finite, one value all along, label -1 inside
    cor = T[CORRIDOR]
    assert np.isfinite(cor).all() and (cor == cor[0]).all() and cor[0] == min(T[12, 1, 12], T[12, 14, 12])
    assert (lab[CORRIDOR] == -1).all()
    # ... and behind it: the cell at the corridor's far end is 12 free cells from the entry instead of a way
    # round the walls, so its chain -- and that of the cells it feeds -- ends in the corridor
    far = (12, 14, 12) if T[12, 1, 12] < T[12, 14, 12] else (12, 1, 12)
    assert T[far] > cor[0] and lab[far] == -1
    assert ((lab[:, :16, :] == -1) & np.isfinite(T[:, :16, :])).sum() > cor.size + 1


@F64
def test_block_of_cost_exactly_zero_is_unlabelled(ctx, f64):
    """see the module docstring: the block's T is the dtype's own (a plateau in fp32, +inf in fp64, where
    the specification has no value); its labels are -1 either way, and all labels follow the rule"""
    cost = raster(FIVE_SHAPE, 13)
    cost[ZERO_BLOCK] = 0.0
    seeds, t0 = [(30, 12, 5), (3, 20, 3)], [0.0, 1.0]
    T, lab = solve(ctx, cost, seeds, t0, f64)
    assert np.array_equal(lab, label_rule3(T, seeds, t0))
    assert (lab[ZERO_BLOCK] == -1).all()
    assert np.isfinite(T[cost > 0]).all() and T[12, 30, 5] == 0.0 and lab[12, 30, 5] == 0
    if f64:  # the reference's arithmetic: the field is the specification's
        close(T, seeded_reference3(cost, seeds, t0), True)


ORACLE_CASES = [((24, 48, 24), (24, 12, 12)), ((20, 40, 41), (3, 3, 3))]


@F64
@pytest.mark.parametrize("shape,goal", ORACLE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_one_seed_at_zero_is_the_single_goal_field(ctx, shape, goal, f64):
    cost = HO.cut_cost3(shape, goal)
    R = HO.oracle_field(("seeds3d", shape, goal), cost, goal)
    T, lab = solve(ctx, cost, [goal], None, f64)
    HO.check_field(T, R, goal, f64)
    assert np.array_equal(lab >= 0, np.isfinite(R)) and set(np.unique(lab)) <= {-1, 0}


# ---------------------------------------------------------------------------------- the entry points
@F64
def test_bad_arguments(ctxs, f64):
    """every EIK_ERR_ARG of the header: the message names the index and nothing is launched (the T buffer
    keeps its NaN fill)"""
    import torch
    from eikonal import _lib as L

    c = ctxs["persistent"]
    dev = torch.device("cuda", 0)
    shape = (8, 9, 7)  # H, W, L
    cd = torch.ones(shape, dtype=torch.float64 if f64 else torch.float32, device=dev)
    Td = torch.full_like(cd, float("nan"))
    lab = torch.full(shape, 77, dtype=torch.int32, device=dev)
    cp, tp, dtype = cd.data_ptr(), Td.data_ptr(), L.EIK_F64 if f64 else L.EIK_F32
    raw = ctypes.CDLL(L.LIB_PATH)  # no argtypes: NULL arrays and K can be passed as they are
    vp, i64 = ctypes.c_void_p, ctypes.c_int64

    def err():
        return L.lib().eik_last_error(c._h).decode()

    def solve_rc(d_cost, d_T, H, W, Lz, seeds, t0, K=None):
        s = None if seeds is None else np.ascontiguousarray(seeds, np.int64).reshape(-1, 3)
        t = None if t0 is None else np.ascontiguousarray(t0, np.float64)
        K = len(s) if K is None else K
        return raw.eik_fim3d_solve_seeds(vp(c._h.value), vp(d_cost), vp(d_T), i64(H), i64(W), i64(Lz), ctypes.c_int(dtype),
                                         vp(None if s is None else s.ctypes.data), vp(None if t is None else t.ctypes.data),
                                         i64(K), vp(None))

    def label_rc(d_T, H, W, Lz, seeds, t0, d_label, K=None):
        s = None if seeds is None else np.ascontiguousarray(seeds, np.int64).reshape(-1, 3)
        t = None if t0 is None else np.ascontiguousarray(t0, np.float64)
        K = len(s) if K is None else K
        return raw.eik_labels3d_dev(vp(c._h.value), vp(d_T), ctypes.c_int(dtype), i64(H), i64(W), i64(Lz),
                                    vp(None if s is None else s.ctypes.data), vp(None if t is None else t.ctypes.data),
                                    i64(K), vp(d_label), vp(None))

    H, W, Lz = shape
    one = [(1, 1, 1)]
    bad = [
        ("K = 0", dict(seeds=one, K=0)),
        ("K = -1", dict(seeds=one, K=-1)),
        ("K = 16777217", dict(seeds=one, K=(1 << 24) + 1)),
        ("seeds is NULL", dict(seeds=None, K=1)),
        (r"seed 1 (9, 3, 3) outside", dict(seeds=[(1, 1, 1), (9, 3, 3)])),
        (r"seed 2 (3, 8, 3) outside", dict(seeds=[(1, 1, 1), (2, 2, 2), (3, 8, 3)])),
        (r"seed 0 (3, 3, 7) outside", dict(seeds=[(3, 3, 7)])),
        (r"seed 1 (3, -1, 3) outside", dict(seeds=[(1, 1, 1), (3, -1, 3)])),
        ("t0[1] = -0.5", dict(seeds=[(1, 1, 1), (2, 2, 2)], t0=[0.0, -0.5])),
        ("t0[0] = nan", dict(seeds=one, t0=[float("nan")])),
        ("t0[2] = inf", dict(seeds=[(1, 1, 1), (2, 2, 2), (3, 3, 3)], t0=[0.0, 1.0, float("inf")])),
        ("bad shape 0 x 9 x 7", dict(seeds=one, H=0)),
        ("bad shape 8 x 0 x 7", dict(seeds=one, W=0)),
        ("bad shape 8 x 9 x -2", dict(seeds=one, Lz=-2)),
    ]
    if not f64:
        bad.append(("t0[1] = 1e+39 rounds to +inf", dict(seeds=[(1, 1, 1), (2, 2, 2)], t0=[0.0, 1e39])))
    for msg, kw in bad:
        a = dict(H=H, W=W, Lz=Lz, t0=None)
        a.update(kw)
        assert solve_rc(cp, tp, **a) == L.EIK_ERR_ARG, msg
        assert msg in err() and "eik_fim3d_solve_seeds" in err(), (msg, err())
        assert label_rc(tp, a["H"], a["W"], a["Lz"], a["seeds"], a["t0"], lab.data_ptr(), a.get("K")) == L.EIK_ERR_ARG, msg
        assert msg in err() and "eik_labels3d_dev" in err(), (msg, err())
    assert solve_rc(None, tp, H, W, Lz, one, None) == L.EIK_ERR_ARG and "d_cost is NULL" in err()
    assert solve_rc(cp, None, H, W, Lz, one, None) == L.EIK_ERR_ARG and "d_T is NULL" in err()
    assert label_rc(None, H, W, Lz, one, None, lab.data_ptr()) == L.EIK_ERR_ARG and "d_T is NULL" in err()
    assert label_rc(tp, H, W, Lz, one, None, None) == L.EIK_ERR_ARG and "d_label is NULL" in err()
    # 2^31 cells: the parents are 32-bit indices (refused before anything is touched)
    assert label_rc(tp, 1 << 11, 1 << 10, 1 << 10, one, None, lab.data_ptr()) == L.EIK_ERR_ARG and "2^31" in err()
    # the host entries check the same list, and their own pointers
    cost = np.ones(shape, dt(f64))
    with pytest.raises(L.EikError, match=r"seed 0 \(1, 1, 9\)") as e:
        c.tmap3d_seeds(cost, [(1, 1, 9)], dtype=dt(f64), labels=True)
    assert e.value.code == L.EIK_ERR_ARG
    with pytest.raises(L.EikError, match=r"t0\[0\] = -1") as e:
        c.tmap3d_seeds(cost, one, [-1.0], dtype=dt(f64))
    assert e.value.code == L.EIK_ERR_ARG
    fn = raw.eik_tmap3d_seeds_f64 if f64 else raw.eik_tmap3d_seeds_f32
    s = np.ascontiguousarray(one, np.int64)
    out = np.empty(shape, dt(f64))
    assert fn(vp(c._h.value), vp(None), i64(H), i64(W), i64(Lz), vp(s.ctypes.data), vp(None), i64(1), vp(out.ctypes.data),
              vp(None)) == L.EIK_ERR_ARG and "cost is NULL" in err()
    assert fn(vp(c._h.value), vp(cost.ctypes.data), i64(H), i64(W), i64(Lz), vp(s.ctypes.data), vp(None), i64(1), vp(None),
              vp(None)) == L.EIK_ERR_ARG and "T is NULL" in err()
    torch.cuda.synchronize()
    assert bool(torch.isnan(Td).all()) and bool((lab == 77).all()), "a refused call launched something"
    # the context is still usable
    assert solve(c, np.ones(shape), one, None, f64, labels=False)[1, 1, 1] == 0


@F64
def test_host_entry_matches_the_device_solver(ctx, f64):
    cost, seeds, t0, R = case("five")
    T, lab = ctx.tmap3d_seeds(cost, seeds, t0, dtype=dt(f64), labels=True)
    assert T.dtype == dt(f64) and lab.dtype == np.int32
    check_seeded(T, R, seeds, t0, f64)
    check_labels(lab, T, R, seeds, t0)
    Td, labd = solve(ctx, cost, seeds, t0, f64)
    close(T, Td.astype(np.float64), f64)
    assert np.array_equal(ctx.labels3d(T, seeds, t0), lab)  # the labels of a host field
    close(ctx.tmap3d_seeds(cost, seeds, t0, dtype=dt(f64)), T.astype(np.float64), f64)


def _smooth():
    """a gentle cost (the 3D walker descends np.gradient of T) with the two walls of the chambers case"""
    ys, xs, zs = np.mgrid[0:FIVE_SHAPE[0], 0:FIVE_SHAPE[1], 0:FIVE_SHAPE[2]]
    cost = (2.0 + 0.5 * np.sin(0.4 * xs) * np.cos(0.3 * ys) + 0.25 * np.sin(0.5 * zs)).astype(np.float32).astype(np.float64)
    cost[:, 16, :] = cost[:, 32, :] = np.inf
    return cost


def test_drop_in_mask_equals_list_and_paths_go_to_the_nearest_goal():
    import FastMarching.FastMarching3D as FM3

    cost = _smooth()
    goals = [(4, 6, 6), (11, 17, 18), (40, 12, 12)]
    offsets = [0.0, 0.5, 4.0]
    R = seeded_reference3(cost, goals, offsets)
    T, lab = FM3.computeTmapMulti(cost, goals, offsets, labels=True)
    assert T.dtype == np.float64 and lab.dtype == np.int32
    check_seeded(T, R, goals, offsets, True)
    check_labels(lab, T, R, goals, offsets)
    close(FM3.computeTmapMulti(cost, goals, offsets), T, True)
    assert np.isinf(T[:, 17:32, :]).all() and (lab[:, 17:32, :] == -1).all()  # the chamber without a goal
    # the mask form: its True cells in row-major order
    mask = np.zeros(cost.shape, bool)
    for x, y, z in goals:
        mask[y, x, z] = True
    order = sorted(range(3), key=lambda k: (goals[k][1], goals[k][0], goals[k][2]))
    assert order != [0, 1, 2]
    Tm, labm = FM3.computeTmapMulti(cost, mask, [offsets[k] for k in order], labels=True)
    close(Tm, T, True)
    assert np.array_equal(labm, label_rule3(Tm, [goals[k] for k in order], [offsets[k] for k in order]))
    for j, k in enumerate(order):
        assert labm[goals[k][1], goals[k][0], goals[k][2]] == j
    starts = [(8.0, 4.0, 10.0), (6.0, 19.0, 14.0), (44.0, 18.0, 8.0), (10.0, 13.0, 16.0)]
    named = [int(lab[int(y), int(x), int(z)]) for x, y, z in starts]
    assert set(named) == {0, 1, 2}  # every goal is somebody's nearest
    paths = FM3.getPathsToNearest(T, lab, goals, starts, 0.5)
    assert len(paths) == 4
    for p, s, k in zip(paths, starts, named):
        assert p.shape[1] == 3 and np.array_equal(p[-1], np.asarray(goals[k], np.float64)), (s, k, p[-1])
        one = FM3.getPathGDM(T, s, goals[k], 0.5)
        assert p.shape == one.shape and np.array_equal(p.view(np.uint8), one.view(np.uint8))
    with pytest.raises(ValueError, match="start 1"):  # a start in the unreached chamber
        FM3.getPathsToNearest(T, lab, goals, [starts[0], (24.0, 12.0, 12.0)], 0.5)
