"""Multi-source 2D solves on the GPU (eik_fim2d_start_seeds / solve_seeds, eik_labels2d_dev,
eik_tmap2d_seeds_*).

The expected field of a seed set is tests/test_seeds_abi.seeded_reference: the fixed point from above
of T = min(T, godunov) from "+inf, the seeds at the min of their T0" -- NOT the minimum of single-source
fields, which lies above it.  Bounds are the suite's (test_gpu_fim2d.check_field): reachability masks
identical, fp32 <= 2e-5 relative, fp64 <= 1e-9 absolute.  Labels are compared for exact equality with
the numpy rule (test_seeds_abi.label_rule) applied to the GPU's own field.

Every case runs in both dtypes on the FIFO, with the priority bands forced, and in list mode.
"""
import functools

import numpy as np
import pytest

import test_gpu_fim2d as F
from test_seeds_abi import (FIVE_SEEDS, FIVE_SHAPE, FIVE_T0, label_rule, raster, seeded_reference, undominated)

pytestmark = pytest.mark.gpu

BANDS = {"PRIO": 0.25, "GRID": 8}  # tiles wait in the bands, as test_gpu_replan.BANDS
MULTI = FIVE_SHAPE  # 3 x 3 tiles, cut on the south and east
DTYPES = [False, True]
MODES = ["fifo", "bands", "list"]


def _context(mode):
    import eikonal
    from eikonal import _lib as L

    opts = {"MODE": L.MODE_LIST} if mode == "list" else {"MODE": L.MODE_PERSISTENT, "QTIMEOUT": 5}
    if mode == "bands":
        opts.update(BANDS)
    return eikonal.Context(0, options=opts)


class Dev:
    """One device-resident solver of B maps with its cost and T tensors"""

    def __init__(self, ctx, cost, f64):
        import torch
        from eikonal import _lib as L

        cost = np.asarray(cost)
        self.torch, self.ctx = torch, ctx
        self.dt = np.float64 if f64 else np.float32
        self.dev = torch.device("cuda", 0)
        self.cd = torch.from_numpy(np.array(cost, self.dt, order="C")).to(self.dev)  # (a copy: the cases are read-only)
        self.Td = torch.full_like(self.cd, float("nan"))
        B = 1 if cost.ndim == 2 else cost.shape[0]
        H, W = cost.shape[-2:]
        self.f = L.Fim2d(ctx, B, H, W, L.EIK_F64 if f64 else L.EIK_F32)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def close(self):
        self.f.close()

    def solve_seeds(self, seeds, t0=None, map_of=None):
        self.f.solve_seeds(self.cd.data_ptr(), self.Td.data_ptr(), seeds, t0, map_of, self.stream)
        return self.T()

    def labels(self, seeds, t0=None, map_of=None):
        return self.ctx.labels2d(self.Td, seeds, t0, map_of).cpu().numpy()

    def T(self):
        self.torch.cuda.synchronize()
        return self.Td.cpu().numpy()


def run(cost, f64, mode, body):
    c = _context(mode)
    try:
        d = Dev(c, cost, f64)
        try:
            return body(d, c)
        finally:
            d.close()
    finally:
        c.close()


def check_seeded(T, R, seeds, t0, f64):
    """test_gpu_fim2d.check_field for a seed set: masks identical, the suite's bounds, and -- in place
    of T[goal] == 0 -- every seed's cell at most its T0, exactly the cell's lowest T0 where the
    reference says no other seed's wave undercut it"""
    assert T.shape == R.shape
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    assert any(undominated(R, seeds, t0))
    for k, (x, y) in enumerate(seeds):
        low = min(v for s, v in zip(seeds, t0) if tuple(s) == (x, y))  # the lowest T0 named for the cell
        if R[y, x] == low:
            assert T[y, x] == T.dtype.type(low), (k, T[y, x])
        else:
            assert T[y, x] < T.dtype.type(low), (k, T[y, x])
    close(T, R, f64)


def close(T, R, f64):
    """the suite's bounds between a field and its expected values"""
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    if not fin.any():
        return
    err = np.abs(T[fin].astype(np.float64) - R[fin])
    print(f"max abs err {err.max():.3e}")
    if f64:
        assert err.max() <= F.ATOL64, err.max()
    else:
        rel = err / np.maximum(np.abs(R[fin]), 1e-30)
        rel[R[fin] == 0] = err[R[fin] == 0]
        print(f"max rel err {rel.max():.3e}")
        assert rel.max() <= F.RTOL32, rel.max()


def check_labels(lab, T, R, seeds, t0):
    """exact equality with the numpy rule on the GPU's own field; every undominated seed's cell carries
    its own k (the lowest k of equal seeds on one cell), a dominated seed's another seed's"""
    assert lab.dtype == np.int32
    want = label_rule(T, seeds, t0)
    assert np.array_equal(lab, want), f"{(lab != want).sum()} labels differ from the rule"
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    und = undominated(R, seeds, t0)
    for k, (x, y) in enumerate(seeds):
        first = min(j for j, s in enumerate(seeds) if tuple(s) == (x, y) and t0[j] == t0[k])
        if und[k]:
            assert lab[y, x] == first, (k, lab[y, x])
        else:
            assert lab[y, x] != k, k
    return want


# ---------------------------------------------------------------------------------- the cases
def _one_sided(col):
    """a seed on a tile's edge column (row) whose in-tile neighbours are all +inf cost: the wave must
    still cross into the neighbour tile (the goal-side hand-off case, with T0 > 0)"""
    cost = raster(MULTI, 21)
    if col:
        s = (63, 100)  # east column of tile (1, 0)
        cost[100, 62] = cost[99, 63] = cost[101, 63] = np.inf
    else:
        s = (100, 64)  # north row of tile (1, 1)
        cost[64, 99] = cost[64, 101] = cost[65, 100] = np.inf
    return cost, [s], [7.5]


def _blocked():
    cost = raster(MULTI, 22)
    cost[99:102, 119:122] = np.inf  # a 3 x 3 block: the seed in its middle spreads nothing
    cost[40, 140] = np.inf          # a lone blocked cell
    return cost, [(20, 30), (120, 100), (140, 40)], [0.0, 6.0, 2.0]


def _chambers():
    cost = raster(MULTI, 11)
    cost[:, 100] = np.inf  # as test_gpu_replan.walled(False)
    return cost, [(20, 30), (150, 100)], [0.0, 4.0]


def _disk():
    ys, xs = np.mgrid[0:MULTI[0], 0:MULTI[1]]
    m = (xs - 64) ** 2 + (ys - 64) ** 2 <= 12 * 12
    return raster(MULTI, 23), [(int(x), int(y)) for y, x in zip(*np.nonzero(m))], None


def _border():
    H, W = MULTI
    s = [(x, y) for y in range(H) for x in range(W) if x in (0, W - 1) or y in (0, H - 1)]
    assert len(s) == 716
    return raster(MULTI, 24), s, [float(x + y) for x, y in s]


def _plateau():
    cost = raster(MULTI, 25)
    cost[60:70, 60:70] = 0.0  # a zero-cost patch across a tile corner: T constant over it
    return cost, [(20, 30), (150, 160)], [0.0, 1.0]


CASES = {
    "five": lambda: (raster(MULTI), FIVE_SEEDS, FIVE_T0),
    "corner4": lambda: (raster(MULTI, 20), [(63, 63), (64, 63), (63, 64), (64, 64)], [0.0, 0.25, 0.5, 0.75]),
    "duplicates": lambda: (raster(MULTI, 26), [(30, 40), (150, 100), (30, 40), (150, 100)], [5.0, 1.0, 2.0, 1.0]),
    "one_sided_col": lambda: _one_sided(True),
    "one_sided_row": lambda: _one_sided(False),
    "blocked": _blocked,
    "chambers": _chambers,
    "disk": _disk,
    "border": _border,
    "plateau": _plateau,
    "tile64": lambda: (raster((64, 64), 27), [(0, 0), (63, 63), (63, 0)], [0.0, 2.0, 30.0]),
    "cut50x40": lambda: (raster((50, 40), 28), [(5, 5), (39, 49)], [1.5, 0.0]),
    "strip1x200": lambda: (raster((1, 200), 29), [(10, 0), (63, 0), (64, 0), (199, 0)], [0.0, 900.0, 3.0, 2.0]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    cost, seeds, t0 = CASES[name]()
    R = seeded_reference(cost, seeds, t0)
    for a in (cost, R):
        a.setflags(write=False)
    return cost, seeds, t0, R


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_field_and_labels(name, mode, f64):
    cost, seeds, t0, R = case(name)

    def body(d, c):
        T = d.solve_seeds(seeds, t0)
        check_seeded(T, R, seeds, t0, f64)
        assert c.stats()["tile_visits"] > 0
        assert c.last_form()["bands"] == (1 if mode == "bands" else 0)
        lab = d.labels(seeds, t0)
        check_labels(lab, T, R, seeds, t0)
        return T, lab

    T, lab = run(cost, f64, mode, body)
    fin = np.isfinite(T)
    if name == "five":
        assert T[5, 100] < 1e4 and T[64, 63] < 40.0  # dominated; (63, 64) undercut from across the tile side
        assert lab[5, 100] in (0, 1, 3) and lab[64, 63] == 3
    elif name == "duplicates":
        assert T[40, 30] == 2.0 and lab[40, 30] == 2 and lab[100, 150] == 1
    elif name.startswith("one_sided"):
        assert fin.sum() == np.isfinite(cost).sum()  # the wave crossed the tile side
        assert (lab[fin] == 0).all()
    elif name == "blocked":
        assert T[100, 120] == 6.0 and np.isinf(T[99:102, 119:122]).sum() == 8  # keeps its T0, spreads nothing
        assert T[40, 140] <= 2.0
    elif name == "chambers":
        assert fin[:, :100].all() and fin[:, 101:].all() and not fin[:, 100].any()
        assert (lab[:, :100] == 0).all() and (lab[:, 101:] == 1).all() and (lab[:, 100] == -1).all()
    elif name == "plateau":
        assert (lab == -1).sum() > 0 and (lab[fin] >= 0).sum() > 0  # the plateau / -1 branch is exercised
    elif name in ("disk", "border"):
        assert (lab[fin] >= 0).all()


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,goal", [(MULTI, (20, 30)), ((64, 64), (5, 5)), ((50, 40), (5, 5)), ((1, 200), (10, 0))])
def test_one_seed_at_zero_is_the_single_goal_solve(shape, goal, mode, f64):
    cost = raster(shape, 30)

    def body(d, c):
        T = d.solve_seeds([goal])
        assert c.stats()["tile_visits"] > 0
        F.check_field(T, F.oracle_field(cost, list(goal)), goal, f64)
        lab = d.labels([goal])
        assert np.array_equal(lab, label_rule(T, [goal])) and (lab[np.isfinite(T)] == 0).all()

    run(cost, f64, mode, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_three_maps_one_without_a_seed(mode, f64):
    costs = np.stack([raster((64, 64), 31 + b) for b in range(3)])
    seeds, t0, map_of = [(5, 5), (60, 50), (63, 0)], [0.0, 3.0, 1.0], [0, 0, 2]

    def body(d, c):
        T = d.solve_seeds(seeds, t0, map_of)
        lab = d.labels(seeds, t0, map_of)
        assert np.isinf(T[1]).all() and (lab[1] == -1).all()
        for b, ks in ((0, [0, 1]), (2, [2])):
            s, v = [seeds[k] for k in ks], [t0[k] for k in ks]
            R = seeded_reference(costs[b], s, v)
            check_seeded(T[b], R, s, v, f64)
            want = np.asarray(ks + [-1], np.int32)[label_rule(T[b], s, v)]  # (local k -> the call's k, -1 stays)
            assert np.array_equal(lab[b], want)

    run(costs, f64, mode, body)


# ---------------------------------------------------------------------------------- device API
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_start_seeds_then_iterate_equals_solve_seeds(mode, f64):
    cost, seeds, t0, R = case("five")

    def body(d, c):
        T = d.solve_seeds(seeds, t0)
        d.Td.fill_(float("nan"))
        d.f.start_seeds(d.cd.data_ptr(), d.Td.data_ptr(), seeds, t0, None, d.stream)
        left = d.f.iterate(1 << 20)
        assert left == 0
        T2 = d.T()
        check_seeded(T2, R, seeds, t0, f64)
        close(T2, T.astype(np.float64), f64)  # (racing sweeps may differ in the last bits between runs)

    run(cost, f64, mode, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("mode", ["fifo", "bands"])
def test_replanning_is_refused_after_a_seeded_solve(mode, f64):
    from eikonal import _lib as L

    cost, seeds, t0, _ = case("five")
    goal = (20, 30)
    new = cost.copy()
    new[60:71, 60:71] = np.inf
    rect = [(60, 60, 71, 71)]

    def body(d, c):
        d.solve_seeds(seeds, t0)
        for fn in (d.f.update, d.f.resolve):
            with pytest.raises(L.EikError, match="seed set") as e:
                fn(rect, None, d.stream)
            assert e.value.code == L.EIK_ERR_ARG
        d.f.solve(d.cd.data_ptr(), d.Td.data_ptr(), [list(goal)], d.stream)  # a single-goal solve clears the mark
        d.cd.copy_(d.torch.from_numpy(np.ascontiguousarray(new, d.dt)))
        d.f.resolve(rect, None, d.stream)
        F.check_field(d.T(), F.oracle_field(new, list(goal)), goal, f64)
        d.solve_seeds(seeds, t0)
        d.f.adopt(d.cd.data_ptr(), d.Td.data_ptr(), [list(goal)], d.stream)  # so does adopt
        d.f.update([], None, d.stream)

    run(cost, f64, mode, body)


def test_host_update_is_refused_on_the_seeded_cached_solver():
    from eikonal import _lib as L

    cost, seeds, t0, R = case("cut50x40")
    c = _context("fifo")
    try:
        T = c.tmap2d_seeds(cost, seeds, t0)
        with pytest.raises(L.EikError, match="seed set") as e:
            c.tmap2d_update(cost, T, seeds[1], [(1, 1, 3, 3)])
        assert e.value.code == L.EIK_ERR_ARG
        T1 = c.tmap2d(cost, seeds[1])  # a single-goal solve on the context
        close(c.tmap2d_update(cost, T1, seeds[1], [(1, 1, 3, 3)]), T1, True)
    finally:
        c.close()


@pytest.mark.parametrize("f64", DTYPES)
def test_bad_arguments(f64):
    from eikonal import _lib as L

    cost = raster((64, 64), 40)
    c = _context("fifo")
    d3 = Dev(c, np.stack([cost, cost]), f64)
    d = Dev(c, cost, f64)
    cp, tp = d.cd.data_ptr(), d.Td.data_ptr()

    def bad(match, fn, *a, **k):
        with pytest.raises(L.EikError, match=match) as e:
            fn(*a, **k)
        assert e.value.code == L.EIK_ERR_ARG

    try:
        for entry in (d.f.start_seeds, d.f.solve_seeds):
            bad("K = 0", entry, cp, tp, np.zeros((0, 2), np.int64))
            bad("K = 16777217", entry, cp, tp, np.zeros(((1 << 24) + 1, 2), np.int64))
            bad("d_cost is NULL", entry, None, tp, [(1, 1)])
            bad("d_T is NULL", entry, cp, None, [(1, 1)])
            bad(r"seed 1 \(64, 3\)", entry, cp, tp, [(1, 1), (64, 3)])
            bad(r"seed 2 \(3, -1\)", entry, cp, tp, [(1, 1), (2, 2), (3, -1)])
            bad(r"map_of\[1\] = 1", entry, cp, tp, [(1, 1), (2, 2)], None, [0, 1])
            bad(r"map_of\[0\] = -1", entry, cp, tp, [(1, 1)], None, [-1])
            bad(r"t0\[1\] = -0.5", entry, cp, tp, [(1, 1), (2, 2)], [0.0, -0.5])
            bad(r"t0\[0\] = nan", entry, cp, tp, [(1, 1)], [float("nan")])
            bad(r"t0\[2\] = inf", entry, cp, tp, [(1, 1), (2, 2), (3, 3)], [0.0, 1.0, float("inf")])
            if not f64:
                bad(r"t0\[1\] = 1e\+39 rounds to \+inf", entry, cp, tp, [(1, 1), (2, 2)], [0.0, 1e39])
        bad("map_of is NULL with B = 2", d3.f.solve_seeds, d3.cd.data_ptr(), d3.Td.data_ptr(), [(1, 1)])
        bad(r"map_of\[0\] = 2", d3.f.solve_seeds, d3.cd.data_ptr(), d3.Td.data_ptr(), [(1, 1)], None, [2])
        # the labels check the same list
        lab = d.torch.empty((64, 64), dtype=d.torch.int32, device=d.dev)
        bad(r"seed 0 \(70, 1\)", c.labels2d, d.cd, [(70, 1)])
        bad(r"t0\[0\] = -1", c.labels2d, d.cd, [(1, 1)], [-1.0])
        bad("map_of is NULL with B = 2", c.labels2d, d3.cd, [(1, 1)])
        bad("K = 0", c.labels2d, d.cd, np.zeros((0, 2), np.int64))
        rc = L.lib().eik_labels2d_dev(c._h, None, L.EIK_F64, 1, 64, 64, np.zeros((1, 2), np.int64), None, None, 1,
                                      lab.data_ptr(), None)
        assert rc == L.EIK_ERR_ARG
        # 2^31 cells: the parents are 32-bit indices (refused before anything is touched)
        rc = L.lib().eik_labels2d_dev(c._h, d.Td.data_ptr(), L.EIK_F64, 1, 65536, 32768, np.zeros((1, 2), np.int64), None,
                                      None, 1, lab.data_ptr(), None)
        assert rc == L.EIK_ERR_ARG and "cells in all" in L.lib().eik_last_error(c._h).decode()
        # a solver with ghost strips bound; a layered block
        g = d.torch.full((64,), float("inf"), dtype=d.cd.dtype, device=d.dev)
        d.f.set_ghosts(g.data_ptr(), None, None, None)
        bad("ghost strips", d.f.solve_seeds, cp, tp, [(1, 1)])
        d.f.set_ghosts(None, None, None, None)
        lay = L.Fim3dLayered(c, 64, 64, 2, 0, 2, L.EIK_F64 if f64 else L.EIK_F32)
        try:
            bad("layered block", lay.solve_seeds, cp, tp, [(1, 1)])
        finally:
            lay.close()
        # nothing was launched: T is as it was
        assert np.isnan(d.T()).all() and np.isnan(d3.T()).all()
        # the host entries check before anything is uploaded
        bad(r"seed 0 \(64, 0\)", c.tmap2d_seeds, cost, [(64, 0)], None, d.dt)
        bad("K = 0", c.tmap2d_seeds, cost, np.zeros((0, 2), np.int64), None, d.dt)
    finally:
        d.close()
        d3.close()
        c.close()


def test_full_band_ring_falls_back_to_the_fifo_with_the_same_seeds():
    """as test_gpu_fim2d.test_priority_band_ring_overflow_falls_back: eik_fim2d_solve_seeds solves again
    on the FIFO and raises nothing.  The rings are forced to 8 slots, and 8 workgroups (BANDS) leave the
    ~230 tiles waiting in the bands: a band a quarter tile of T wide holds the tiles of a whole ring round
    the seed, far more than 8 a few tiles out.  One seed at T0 = 0, so the oracle is the reference at
    this size (bounds as there: 1e-9, or 1e-13 relative)."""
    import eikonal
    from eikonal import _lib as L

    H, W = 777, 1100
    c = np.random.default_rng(77).uniform(1, 10, (H, W))
    goal = (W // 3, H // 2)
    R = F.oracle_field(c, list(goal))
    forms = []
    for ring in (0, 8):
        ctx = eikonal.Context(0, options=dict(BANDS, PRIO_RING=ring))
        try:
            T = ctx.tmap2d_seeds(c, [goal])
            forms.append(ctx.last_form()["bands"])
        finally:
            ctx.close()
        assert np.isfinite(T).all() and T[goal[1], goal[0]] == 0
        assert (np.abs(T - R) <= np.maximum(1e-9, 1e-13 * R)).all()
    assert forms == [1, 0]  # bands when the ring holds; the second attempt's FIFO when it filled


# ---------------------------------------------------------------------------------- host entries, drop-in
@pytest.mark.parametrize("f64", DTYPES)
def test_host_entry_matches_the_device_solver(f64):
    cost, seeds, t0, R = case("five")
    c = _context("fifo")
    try:
        dt = np.float64 if f64 else np.float32
        T, lab = c.tmap2d_seeds(cost, seeds, t0, dtype=dt, labels=True)
        assert T.dtype == dt
        check_seeded(T, R, seeds, t0, f64)
        check_labels(lab, T, R, seeds, t0)
        assert np.array_equal(c.labels2d(T, seeds, t0), lab)  # the labels of a host field
        close(c.tmap2d_seeds(cost, seeds, t0, dtype=dt), T.astype(np.float64), f64)
    finally:
        c.close()


def test_drop_in_mask_equals_list_and_paths_go_to_the_nearest_goal():
    import FastMarching.FastMarching as FM

    cost, seeds, t0, R = case("chambers")
    goals = [(20, 30), (60, 150), (150, 100)]
    offsets = [0.0, 2.0, 4.0]
    T, lab = FM.computeTmapMulti(cost, goals, offsets, labels=True)
    assert T.dtype == np.float64 and lab.dtype == np.int32
    check_seeded(T, seeded_reference(cost, goals, offsets), goals, offsets, True)
    check_labels(lab, T, seeded_reference(cost, goals, offsets), goals, offsets)
    close(FM.computeTmapMulti(cost, goals, offsets), T, True)
    # the mask form: its True cells in row-major order
    mask = np.zeros(cost.shape, bool)
    for x, y in goals:
        mask[y, x] = True
    order = sorted(range(3), key=lambda k: (goals[k][1], goals[k][0]))
    Tm, labm = FM.computeTmapMulti(cost, mask, [offsets[k] for k in order], labels=True)
    close(Tm, T, True)
    assert np.array_equal(labm, label_rule(Tm, [goals[k] for k in order], [offsets[k] for k in order]))
    for j, k in enumerate(order):
        assert labm[goals[k][1], goals[k][0]] == j
    starts = [(30.0, 60.0), (70.0, 170.0), (160.0, 20.0), (120.0, 180.0)]
    assert len({int(lab[int(y), int(x)]) for x, y in starts}) == 3  # every goal is somebody's nearest
    paths = FM.getPathsToNearest(T, lab, goals, starts, 0.5)
    assert len(paths) == 4
    for p, s in zip(paths, starts):
        one = FM.getPathGDM(T, s, goals[lab[int(s[1]), int(s[0])]], 0.5)
        assert p.shape == one.shape and np.array_equal(p.view(np.uint8), one.view(np.uint8))
    # no goal in the east chamber: a start there belongs to no goal
    T2, lab2 = FM.computeTmapMulti(cost, goals[:2], offsets[:2], labels=True)
    assert (lab2[:, 101:] == -1).all()
    with pytest.raises(ValueError, match="start 1"):
        FM.getPathsToNearest(T2, lab2, goals[:2], [starts[0], starts[2]], 0.5)
