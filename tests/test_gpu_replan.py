"""Incremental re-solve after local cost changes (eik_fim2d_update / resolve / adopt)
on the GPU, against from-scratch oracle fields of the new cost.

Bounds are the suite's (test_gpu_fim2d.check_field): reachability masks identical, fp32 <= 2e-5
relative, fp64 <= 1e-9 absolute.  The invalidated set is compared cell for cell with the numpy
closure of tests/test_replan_rule.py.
"""
import numpy as np
import pytest

import test_gpu_fim2d as F
from test_replan_rule import closure, rect_mask

pytestmark = pytest.mark.gpu

ANY, LOWERED = 0, 1
BANDS = {"PRIO": 0.25, "GRID": 8}  # tiles wait in the bands, as in test_wide_c4_schedule
DTYPES = [False, True]
MULTI = (190, 170)  # 3 x 3 tiles, cut on the south and east


def _context(options=None):
    import eikonal
    from eikonal import _lib as L

    return eikonal.Context(0, options=dict(options or {}, MODE=L.MODE_PERSISTENT, QTIMEOUT=5))


def raster(shape, seed=7):
    """U(1, 10) rounded to fp32, so both dtypes solve the same costs"""
    return np.random.default_rng(seed).uniform(1, 10, shape).astype(np.float32).astype(np.float64)


class Dev:
    """One device-resident solver with its cost and T tensors"""

    def __init__(self, ctx, cost, goal, f64):
        import torch
        from eikonal import _lib as L

        self.torch, self.goal, self.f64 = torch, list(goal), f64
        self.dt = np.float64 if f64 else np.float32
        self.dev = torch.device("cuda", 0)
        self.cd = torch.from_numpy(np.ascontiguousarray(cost, self.dt)).to(self.dev)
        self.Td = torch.full_like(self.cd, float("nan"))
        H, W = cost.shape
        self.f = L.Fim2d(ctx, 1, H, W, L.EIK_F64 if f64 else L.EIK_F32)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def close(self):
        self.f.close()

    def solve(self):
        self.f.solve(self.cd.data_ptr(), self.Td.data_ptr(), [self.goal], self.stream)
        return self.T()

    def set_cost(self, cost):
        self.cd.copy_(self.torch.from_numpy(np.ascontiguousarray(cost, self.dt)))

    def resolve(self, cost, rects, kinds=None):
        self.set_cost(cost)
        self.f.resolve(rects, kinds, self.stream)
        return self.T()

    def T(self):
        self.torch.cuda.synchronize()
        return self.Td.cpu().numpy()

    def work(self):
        s = self.f.stats()
        return s["tile_visits"] + s["inplace_passes"]


def run(cost, goal, f64, opts, body):
    c = _context(opts)
    try:
        d = Dev(c, cost, goal, f64)
        try:
            return body(d, c)
        finally:
            d.close()
    finally:
        c.close()


def check(T, cost, goal, f64):
    F.check_field(T, F.oracle_field(cost, list(goal)), goal, f64)


# shape, goal, the new obstacle's rectangle, options
OBSTACLE_CASES = [
    (MULTI, (20, 30), (60, 60, 71, 71), None),  # across a tile corner
    (MULTI, (20, 30), (60, 60, 71, 71), BANDS),
    ((64, 64), (5, 5), (30, 30, 41, 41), None),
    ((50, 40), (5, 5), (20, 25, 28, 33), None),
    ((1, 200), (10, 0), (100, 0, 104, 1), None),
    ((1, 200), (10, 0), (100, 0, 104, 1), BANDS),
]


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("shape,goal,rect,opts", OBSTACLE_CASES)
def test_new_obstacle(shape, goal, rect, opts, f64):
    cost = raster(shape)
    new = cost.copy()
    new[rect[1]:rect[3], rect[0]:rect[2]] = np.inf

    def body(d, c):
        check(d.solve(), cost, goal, f64)
        check(d.resolve(new, [rect]), new, goal, f64)
        info = d.f.update_info()
        assert info["cells"] > 0 and info["tiles_marked"] > 0 and info["fell_back"] == 0

    run(cost, goal, f64, opts, body)


def walled(gap_open):
    cost = raster(MULTI, 11)
    cost[:, 100] = np.inf
    if gap_open:
        cost[80, 100] = 2.0
    return cost


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_closing_the_only_gap_of_a_wall(opts, f64):
    cost, new, goal = walled(True), walled(False), (20, 30)

    def body(d, c):
        d.solve()
        T = d.resolve(new, [(100, 80, 101, 81)])
        check(T, new, goal, f64)
        assert np.isinf(T[:, 101:]).all()

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_opening_a_wall(opts, f64):
    cost, new, goal = walled(False), walled(True), (20, 30)

    def body(d, c):
        T0 = d.solve()
        assert np.isinf(T0[:, 101:]).all()
        T = d.resolve(new, [(100, 80, 101, 81)], [LOWERED])
        check(T, new, goal, f64)
        assert np.isfinite(T[:, 101:]).all()
        assert d.f.update_info()["cells"] == 0  # nothing is reset for a lowered cost

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_mixed_rectangles_in_different_tiles(opts, f64):
    cost, goal = raster(MULTI, 3), (20, 30)
    new = cost.copy()
    new[10:30, 90:110] = np.inf   # raised, tile (0, 1)
    new[140:170, 20:50] = 1.0     # lowered, tile (2, 0)

    def body(d, c):
        d.solve()
        check(d.resolve(new, [(90, 10, 110, 30), (20, 140, 50, 170)], [ANY, LOWERED]), new, goal, f64)

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_lowered_block_declared_any(opts, f64):
    cost, goal = raster(MULTI, 4), (20, 30)
    new = cost.copy()
    new[50:80, 100:140] = 1.0
    rect = [(100, 50, 140, 80)]

    def body(d, c):
        d.solve()
        Tl = d.resolve(new, rect, [LOWERED])
        check(Tl, new, goal, f64)
        d.set_cost(cost)
        d.solve()
        Ta = d.resolve(new, rect, [ANY])
        check(Ta, new, goal, f64)
        F.check_field(Ta, Tl.astype(np.float64), goal, f64)

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_change_on_tile_edge_columns_and_back(opts, f64):
    """a stale edge-column copy (the W / E halo source of the fp64 solve) would show after the revert"""
    cost, goal = raster(MULTI, 5), (20, 30)
    new = cost.copy()
    new[40:60, 63:65] = np.inf
    new[100:120, 127] = np.inf
    rects = [(63, 40, 65, 60), (127, 100, 128, 120)]

    def body(d, c):
        d.solve()
        check(d.resolve(new, rects), new, goal, f64)
        check(d.resolve(cost, rects), cost, goal, f64)  # (the revert lowers costs: ANY is always safe)

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_three_successive_updates(opts, f64):
    cost, goal = raster(MULTI, 6), (20, 30)
    steps = [((130, 20, 150, 45), np.inf, ANY), ((40, 100, 70, 130), 1.0, LOWERED), ((60, 60, 71, 71), np.inf, ANY)]

    def body(d, c):
        d.solve()
        cur = cost.copy()
        for rect, val, kind in steps:
            cur = cur.copy()
            cur[rect[1]:rect[3], rect[0]:rect[2]] = val
            check(d.resolve(cur, [rect], [kind]), cur, goal, f64)

    run(cost, goal, f64, opts, body)


def tie_raster(shape, kind):
    """integer costs 1..3: one-sided updates are exact integer sums, so neighbouring cells often hold
    exactly equal T -- a `<` in place of the flood's `<=` would leave such cells out of the device's set
    (ties ACROSS tile edges: test_zero_cost_patch_round_the_goal, whose fp32 plateau straddles two)"""
    if kind == "integer":
        return np.random.default_rng(8).integers(1, 4, shape).astype(np.float64)
    return raster(shape, 8)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("kind", ["float", "integer"])
@pytest.mark.parametrize("shape,goal,rect,opts", OBSTACLE_CASES)
def test_exact_set(shape, goal, rect, opts, kind, f64):
    """the cells update() turns +inf are exactly the closure of the downloaded T_old, and a raise-only
    re-solve leaves every other cell bit-identical"""
    cost = tie_raster(shape, kind)
    new = cost.copy()
    new[rect[1]:rect[3], rect[0]:rect[2]] = np.inf

    def body(d, c):
        T_old = d.solve()
        cone = closure(T_old, rect_mask(shape, [rect]), goal)
        if kind == "integer" and shape == MULTI:  # the case does hold ties between neighbours
            fin = np.isfinite(T_old)
            tied = ((T_old[:, 1:] == T_old[:, :-1]) & fin[:, 1:]).sum() + ((T_old[1:] == T_old[:-1]) & fin[1:]).sum()
            assert tied > 0
        d.set_cost(new)
        d.f.update([rect], None, d.stream)
        T_mid = d.T()
        assert np.array_equal(np.isfinite(T_old) & np.isinf(T_mid), cone)
        assert np.array_equal(T_mid[~cone].view(np.uint8), T_old[~cone].view(np.uint8))
        info = d.f.update_info()
        assert info["cells"] == int(cone.sum())
        tiles = {(y // 64, x // 64) for y, x in zip(*np.nonzero(cone))}
        assert info["tiles_marked"] == len(tiles)
        assert d.f.iterate(1 << 20) == 0
        T = d.T()
        check(T, new, goal, f64)
        assert np.array_equal(T[~cone].view(np.uint8), T_old[~cone].view(np.uint8))

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_rectangle_containing_the_goal(opts, f64):
    cost, goal = raster(MULTI, 9), (70, 60)
    new = cost.copy()
    new[50:70, 60:80] = 9.5  # the goal's own cost is not used

    def body(d, c):
        d.solve()
        T = d.resolve(new, [(60, 50, 80, 70)])
        check(T, new, goal, f64)
        assert T[goal[1], goal[0]] == 0
        assert d.f.update_info()["cells"] == cost.size - 1  # everything depends on the goal's neighbours

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
@pytest.mark.parametrize("rect", [(66, 58, 69, 63), (60, 50, 80, 70)], ids=["beside_goal", "round_goal"])
def test_zero_cost_patch_round_the_goal(rect, opts, f64):
    """costs of 0 are legal: the cells of a zero-cost patch round the goal have T == 0 (fp32) like the
    goal, so a seed among them -- or a tie flood through them -- reaches the goal's neighbours with
    0 <= 0.  The goal is never invalidated: the set is the numpy closure (p not the goal), T[goal] stays
    0 through the update, and the re-solve is the oracle's field."""
    cost, goal = raster(MULTI, 16), (70, 60)  # the patch straddles the tile edge x = 63 | 64
    cost[52:69, 58:79] = 0.0
    new = cost.copy()
    new[rect[1]:rect[3], rect[0]:rect[2]] = 5.0

    def body(d, c):
        T_old = d.solve()
        check(T_old, cost, goal, f64)
        cone = closure(T_old, rect_mask(MULTI, [rect]), goal)
        assert not cone[goal[1], goal[0]]
        if not f64:  # (fp64 stages a zero cost as 2^-500: T rises by that per cell, no tie with the goal)
            assert (T_old[52:69, 58:79] == 0).all()
            assert cone[goal[1], goal[0] - 1] and cone[goal[1] + 1, goal[0]]  # the ties do reach the goal's side
        d.set_cost(new)
        d.f.update([rect], None, d.stream)
        T_mid = d.T()
        assert T_mid[goal[1], goal[0]] == 0 and not np.signbit(T_mid[goal[1], goal[0]])
        assert np.array_equal(np.isfinite(T_old) & np.isinf(T_mid), cone)
        assert d.f.update_info()["cells"] == int(cone.sum())
        assert d.f.iterate(1 << 20) == 0
        T = d.T()
        check(T, new, goal, f64)
        assert not np.signbit(T).any()

    run(cost, goal, f64, opts, body)


def pocket_raster():
    cost = raster(MULTI, 10)
    cost[120:160, 100] = cost[120:160, 150] = np.inf
    cost[120, 100:151] = cost[159, 100:151] = np.inf
    return cost


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
@pytest.mark.parametrize("rects", [[(110, 130, 140, 150)], []], ids=["pocket", "K0"])
def test_nothing_to_do(rects, opts, f64):
    """a rectangle inside an unreachable pocket, and K == 0: 0 cells invalidated, 0 solve visits, T
    bit-identical, and the solver stays usable"""
    cost, goal = pocket_raster(), (20, 30)
    new = cost.copy()
    if rects:
        new[130:150, 110:140] = 1.5

    def body(d, c):
        T_old = d.solve()
        assert np.isinf(T_old[121:159, 101:150]).all()
        T = d.resolve(new, rects)
        assert np.array_equal(T.view(np.uint8), T_old.view(np.uint8))
        info = d.f.update_info()
        assert info["cells"] == 0 and info["tiles_marked"] == 0 and info["tiles_queued"] == 0
        assert d.work() == 0
        new2 = new.copy()
        new2[60:71, 60:71] = np.inf
        check(d.resolve(new2, [(60, 60, 71, 71)]), new2, goal, f64)

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_work_condition(opts, f64):
    """512 x 512, a 16 x 16 block far from the goal raised to inf: on the CPU the closure is 2.6 % of the
    cells in 4 of 64 tiles -- the flood marks exactly those 4, and the re-solve does less than half
    of the full solve's tile work (visits + in-place passes) on the same solver and new cost"""
    cost = np.random.default_rng(512).uniform(1, 10, (512, 512)).astype(np.float32).astype(np.float64)
    goal = (40, 40)
    new = cost.copy()
    new[400:416, 400:416] = np.inf

    def body(d, c):
        d.solve()
        T = d.resolve(new, [(400, 400, 416, 416)])
        work, info = d.work(), d.f.update_info()
        check(T, new, goal, f64)
        full_T = d.solve()
        full = d.work()
        print(f"f64={f64} {opts}: update {info}, re-solve work {work}, full solve work {full}")
        assert info["tiles_marked"] == 4
        assert work < full / 2, (work, full)
        F.check_field(T, full_T.astype(np.float64), goal, f64)

    run(cost, goal, f64, opts, body)


def test_band_ring_overflow_falls_back_to_a_full_solve():
    """test_gpu_fim2d.test_priority_band_ring_overflow_falls_back's raster; after the first solve the
    band rings are cut to ONE slot and the grid to ONE workgroup, and the whole field is re-solved (a
    rectangle round the goal: only the goal's tile is queued).  The overflow is then certain: the one
    workgroup is busy with the goal's tile when that visit activates its north and east neighbours
    (edges 4 and 17 cells from the goal, T < 160, far below the band width of 64 x the cost's geometric
    mean ~ 300), no workgroup waits, so both entries go to band 0, whose ring holds one.  The launch
    ends on the overflow word and eik_fim2d_resolve solves in full on the FIFO: update_info says so,
    the field is the oracle's, and the solver keeps the FIFO and stays updatable."""
    from eikonal import _lib as L

    H, W = 777, 1100
    cost = np.random.default_rng(77).uniform(1, 10, (H, W))
    goal = (W // 3, H // 2)
    new = cost.copy()
    rect = (goal[0] - 8, goal[1] - 8, goal[0] + 8, goal[1] + 8)
    new[rect[1]:rect[3], rect[0]:rect[2]] = 9.0
    new2 = new.copy()
    new2[600:620, 900:930] = np.inf

    def body(d, c):
        d.solve()
        assert c.last_form()["bands"] == 1
        c.set_option(L.OPT_PRIO_RING, 1)
        c.set_option(L.OPT_GRID, 1)
        check(d.resolve(new, [rect]), new, goal, True)
        info = d.f.update_info()
        assert info["cells"] == cost.size - 1 and info["tiles_queued"] == 1
        assert info["fell_back"] == 1 and c.last_form()["bands"] == 0  # the fall-back's solve ran on the FIFO
        c.set_option(L.OPT_GRID, 0)  # the default grid again
        check(d.resolve(new2, [(900, 600, 930, 620)]), new2, goal, True)
        assert d.f.update_info()["fell_back"] == 0 and c.last_form()["bands"] == 0  # the solver keeps the FIFO

    run(cost, goal, True, {"PRIO": 1.0}, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_adopt_a_field_from_another_context(opts, f64):
    import torch

    cost, goal = raster(MULTI, 12), (20, 30)
    new = cost.copy()
    new[60:71, 60:71] = np.inf
    dt = np.float64 if f64 else np.float32
    other = _context()
    try:
        T0 = other.tmap2d(cost.astype(dt), goal, dtype=dt)
    finally:
        other.close()

    def body(d, c):
        d.Td.copy_(torch.from_numpy(T0))
        d.set_cost(new)
        d.f.adopt(d.cd.data_ptr(), d.Td.data_ptr(), [list(goal)], d.stream)
        d.f.resolve([(60, 60, 71, 71)], None, d.stream)
        check(d.T(), new, goal, f64)
        assert c.last_form()["bands"] == (1 if opts else 0)

    run(cost, goal, f64, opts, body)


def test_host_buffer_forms_leave_inputs_alone():
    import FastMarching.FastMarching as FM

    cost, goal = raster(MULTI, 13), (20, 30)
    new = cost.copy()
    new[60:71, 60:71] = np.inf
    new[140:170, 20:50] = 1.0
    rects = [(60, 60, 71, 71), (20, 140, 50, 170)]
    mask = new != cost
    R = F.oracle_field(new, list(goal))
    c = _context()
    try:
        for f64 in DTYPES:
            dt = np.float64 if f64 else np.float32
            T0 = c.tmap2d(cost.astype(dt), goal, dtype=dt)
            a, b = new.astype(dt), T0.copy()
            T = c.tmap2d_update(a, b, goal, rects, [ANY, LOWERED], dtype=dt)
            assert np.array_equal(a, new.astype(dt)) and np.array_equal(b.view(np.uint8), T0.view(np.uint8))
            F.check_field(T, R, goal, f64)
            with pytest.raises(ValueError):
                c.tmap2d_update(a, b[:, :1], goal, rects, dtype=dt)  # (would broadcast silently)
    finally:
        c.close()
    T0 = FM.computeTmap(cost, goal)
    want = FM.computeTmap(new, goal)
    f64 = FM._DTYPE == np.float64
    for changed in (rects, mask, np.asfortranarray(mask)):
        a, b = np.asfortranarray(new), T0.copy()
        T = FM.updateTmap(a, b, goal, changed)
        assert T.dtype == np.float64 and np.array_equal(a, new) and np.array_equal(b, T0)
        F.check_field(T, R, goal, f64)
        F.check_field(T, want, goal, f64)
    assert np.array_equal(FM.updateTmap(new, want, goal, np.zeros(cost.shape, bool)), want)


def _raises_arg(c, fn):
    import eikonal
    from eikonal import _lib as L

    with pytest.raises(eikonal.EikError) as ei:
        fn()
    assert ei.value.code == L.EIK_ERR_ARG
    assert L.lib().eik_last_error(c._h).decode() != ""


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_argument_errors(opts, f64):
    import torch
    from eikonal import _lib as L

    cost, goal = raster(MULTI, 14), (20, 30)
    new = cost.copy()
    new[60:71, 60:71] = np.inf
    ok = [(60, 60, 71, 71)]

    def body(d, c):
        f, st = d.f, d.stream
        _raises_arg(c, lambda: f.update(ok, None, st))  # never started or adopted
        f.start(d.cd.data_ptr(), d.Td.data_ptr(), [list(goal)], st)
        _raises_arg(c, lambda: f.update(ok, None, st))  # started, not converged
        assert f.iterate(1 << 20) == 0
        T_old = d.T()
        for rects, kinds in (([(71, 60, 60, 71)], None),             # x1 <= x0
                             ([(60, 71, 71, 60)], None),             # y1 <= y0
                             ([(60, 60, 60, 71)], None),             # empty
                             ([(170, 0, 180, 10)], None),            # wholly outside (east)
                             ([(-9, -9, 0, 0)], None),               # wholly outside (north-west)
                             (ok, [2]), (ok, [-1]),                  # kinds other than 0 / 1
                             ([ok[0]] * 1025, None)):                # K > 1024
            _raises_arg(c, lambda: f.update(rects, kinds, st))
            _raises_arg(c, lambda: f.resolve(rects, kinds, st))
        assert np.array_equal(d.T().view(np.uint8), T_old.view(np.uint8))  # nothing was launched
        # an update after the errors works, and so does a solve
        check(d.resolve(new, ok), new, goal, f64)
        d.set_cost(cost)
        check(d.solve(), cost, goal, f64)
        # list mode
        c.set_option(L.OPT_MODE, L.MODE_LIST)
        _raises_arg(c, lambda: f.update(ok, None, st))
        _raises_arg(c, lambda: f.adopt(d.cd.data_ptr(), d.Td.data_ptr(), [list(goal)], st))
        check(d.solve(), cost, goal, f64)                       # a list-mode solve ...
        c.set_option(L.OPT_MODE, L.MODE_PERSISTENT)
        _raises_arg(c, lambda: f.update(ok, None, st))          # ... is not updatable
        d.solve()
        # ghost strips bound
        strip = torch.full((256,), float("inf"), dtype=d.cd.dtype, device=d.dev)
        f.set_ghosts(strip.data_ptr(), None, None, None)
        _raises_arg(c, lambda: f.update(ok, None, st))
        f.set_ghosts(None, None, None, None)
        check(d.resolve(new, ok), new, goal, f64)
        # B = 2, a layered block, a raster past the persistent mode's 32-bit offsets
        dtype = L.EIK_F64 if f64 else L.EIK_F32
        side = 23200 if f64 else 32768
        for g in (L.Fim2d(c, 2, 64, 64, dtype), L.Fim3dLayered(c, 64, 64, 4, 0, 2, dtype), L.Fim2d(c, 1, side, side, dtype)):
            try:
                _raises_arg(c, lambda: g.adopt(d.cd.data_ptr(), d.Td.data_ptr(), [list(goal)], st))
                _raises_arg(c, lambda: g.update(ok, None, st))
            finally:
                g.close()

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_path_after_update(opts, f64):
    # (a uniform cost: on a noisy one the reference's own walk meets a NaN gradient at the wall's corner
    # and returns its truncated fallback path, on a from-scratch field too)
    cost, goal, start = np.full(MULTI, 2.0), (20, 30), (150, 60)
    new = cost.copy()
    new[40:90, 100:106] = np.inf  # a wall between start and goal

    def body(d, c):
        d.solve()
        T = d.resolve(new, [(100, 40, 106, 90)])
        check(T, new, goal, f64)
        path, status = c.path2d(T.astype(np.float64), np.array(start, float), np.array(goal, float))
        from eikonal import _lib as L

        assert status == L.PATH_DONE
        # the walk stops inside the stop radius (1.5 cells) and appends the goal itself
        assert np.array_equal(path[-1], np.array(goal, float))
        assert np.hypot(*(path[-2] - np.array(goal, float))) < 1.5
        # every point lies in a finite-cost cell (cells are unit squares centred on the nodes)
        cells = np.floor(path + 0.5).astype(int)
        assert np.isfinite(new[cells[:, 1], cells[:, 0]]).all()
        assert path[:, 1].min() < 40.5 or path[:, 1].max() > 89.5  # it went round the wall

    run(cost, goal, f64, opts, body)
