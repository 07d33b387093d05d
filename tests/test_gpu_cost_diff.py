"""Rectangle-free replanning on the GPU (eik_cost_diff_dev, eik_fim2d_resolve_cost, eik_tmap2d_update_cost_*,
DESIGN.md §3.15): the device diff against its numpy restatement (tests/cost_diff_np.py) cell for cell and
count for count, and the re-solve it feeds against from-scratch oracle fields of the new cost.

Bounds are the suite's (test_gpu_fim2d.check_field): reachability masks identical, fp32 <= 2e-5 relative,
fp64 <= 1e-9 absolute.  The new cost always goes into a SECOND tensor (two buffers in ping-pong) and no
rectangle is given.
"""
import functools

import numpy as np
import pytest

import cost_diff_np as D
import test_gpu_fim2d as F
import test_gpu_replan as RP
import test_gpu_replan_seeds as RS
from test_gpu_replan import ANY, BANDS, DTYPES, LOWERED, MULTI, OBSTACLE_CASES, check, raster
from test_gpu_seeds import check_seeded
from test_replan_rule import rect_mask
from test_replan_seeds_rule import seeded_closure
from test_seeds_abi import label_rule, seeded_reference

pytestmark = pytest.mark.gpu


class Dev(RP.Dev):
    """test_gpu_replan.Dev with a second cost tensor: resolve_cost writes the new cost there, hands it to the
    solver and swaps the two (the old buffer is the caller's again)"""

    def __init__(self, ctx, cost, goal, f64):
        super().__init__(ctx, cost, goal, f64)
        self.c2 = self.torch.full_like(self.cd, float("nan"))

    def put_second(self, cost):
        self.c2.copy_(self.torch.from_numpy(np.ascontiguousarray(cost, self.dt)))

    def resolve_cost(self, cost):
        self.put_second(cost)
        self.f.resolve_cost(self.c2.data_ptr(), self.stream)
        self.cd, self.c2 = self.c2, self.cd
        return self.T()

    def diff_of_last(self, ctx, cap=1024):
        """the diff between the buffer that was bound before the last resolve_cost and the bound one"""
        from eikonal import _lib as L

        H, W = self.cd.shape
        return ctx.cost_diff(self.c2.data_ptr(), self.cd.data_ptr(), L.EIK_F64 if self.f64 else L.EIK_F32, H, W, cap, self.stream)


def run(cost, goal, f64, opts, body):
    c = RP._context(opts)
    try:
        d = Dev(c, cost, goal, f64)
        try:
            return body(d, c)
        finally:
            d.close()
    finally:
        c.close()


# ------------------------------------------------------------------------------- the diff alone
def block(shape, rng, lo=3, hi=40):
    H, W = shape
    h, w = min(H, int(rng.integers(lo, hi))), min(W, int(rng.integers(lo, hi)))
    y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    return slice(y0, y0 + h), slice(x0, x0 + w)


def diff_pair(shape, seed, invalid):
    """a pair with every kind of change at once: raised to +inf, halved, +inf -> finite, +0 against -0, a
    raised and a lowered cell in the first tile, both sides of a tile corner; invalid: a NaN and a -1"""
    rng = np.random.default_rng(seed)
    H, W = shape
    old = raster(shape, seed)
    b_inf, b_zero, b_up, b_half = (block(shape, rng) for _ in range(4))
    old[b_inf] = np.inf
    old[b_zero] = 0.0
    new = old.copy()
    new[b_inf] = 2.0
    new[b_zero] = -0.0
    new[b_up] = np.inf
    new[b_half] *= 0.5
    new[0, 0] = 11.0
    new[H - 1, W - 1] = 0.25
    new[60:68, 62:66] = np.inf
    if invalid:
        new[H // 2, W // 3] = np.nan
        new[H // 3, W // 2] = -1.0
    return old, new


DIFF_CASES = [(s, f64) for s in [(190, 170), (1, 200), (64, 64), (65, 129)] for f64 in DTYPES] + [((130, 66), False)]


@pytest.mark.parametrize("invalid", [False, True], ids=["valid", "invalid"])
@pytest.mark.parametrize("shape,f64", DIFF_CASES)
def test_cost_diff_matches_the_numpy_rule(shape, f64, invalid):
    import torch
    from eikonal import _lib as L

    dt = np.float64 if f64 else np.float32
    old, new = (a.astype(dt) for a in diff_pair(shape, 31 + shape[1], invalid))
    dev = torch.device("cuda", 0)
    do, dn = torch.from_numpy(old).to(dev), torch.from_numpy(new).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    c = RP._context()
    try:
        for loads in (0, 1):  # plain and non-temporal loads: the same records
            c.set_option(L.OPT_DIFF_LOADS, loads)
            for cap in (1, 2, 1024):
                rects, kinds, info = c.cost_diff(do.data_ptr(), dn.data_ptr(), L.EIK_F64 if f64 else L.EIK_F32, *shape, cap, stream)
                wr, wk, wi = D.cost_diff(old, new, cap)
                print(shape, f64, cap, info, len(rects))
                assert [tuple(int(v) for v in r) for r in rects] == wr
                assert kinds.tolist() == wk
                assert {k: info[k] for k in wi} == wi
                assert info["cells_invalid"] == (2 if invalid else 0)
                assert len(rects) <= cap
        # equal rasters, and the signed zeros alone
        rects, kinds, info = c.cost_diff(dn.data_ptr(), dn.data_ptr(), L.EIK_F64 if f64 else L.EIK_F32, *shape, 1024, stream)
        if not invalid:
            assert len(rects) == 0 and len(kinds) == 0
            assert [info[k] for k in ("cells_changed", "cells_raised", "cells_invalid", "tiles_changed", "block_side")] == [0] * 5
        else:  # an invalid cell counts as changed, whatever the old value
            assert info["cells_changed"] == 2 and info["cells_invalid"] == 2 and info["cells_raised"] == 0
    finally:
        c.close()


def test_cost_diff_argument_errors():
    import torch
    from eikonal import _lib as L

    t = torch.ones((64, 64), dtype=torch.float32, device="cuda:0")
    c = RP._context()
    try:
        for args in ((0, t.data_ptr(), L.EIK_F32, 64, 64, 8), (t.data_ptr(), t.data_ptr(), 7, 64, 64, 8),
                     (t.data_ptr(), t.data_ptr(), L.EIK_F32, 0, 64, 8), (t.data_ptr(), t.data_ptr(), L.EIK_F32, 64, 64, 1025)):
            RP._raises_arg(c, lambda: c.cost_diff(*args))
    finally:
        c.close()


# ------------------------------------------------------------------------------- resolve_cost, single goal
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("shape,goal,rect,opts", OBSTACLE_CASES)
def test_new_obstacle_without_a_rectangle(shape, goal, rect, opts, f64):
    cost = raster(shape)
    new = cost.copy()
    new[rect[1]:rect[3], rect[0]:rect[2]] = np.inf

    def body(d, c):
        check(d.solve(), cost, goal, f64)
        check(d.resolve_cost(new), new, goal, f64)
        info, di = d.f.update_info(), d.f.diff_info()
        assert info["cells"] > 0 and info["tiles_marked"] > 0 and info["fell_back"] == 0
        edit = rect_mask(shape, [rect])
        assert di["cells_changed"] == di["cells_raised"] == int(edit.sum()) and di["cells_invalid"] == 0
        assert di["solved_from_scratch"] == 0 and di["block_side"] == 1 and di["rects"] == di["tiles_changed"] >= 1
        rects, kinds, _ = d.diff_of_last(c)
        assert len(rects) == di["rects"] and (kinds == ANY).all()
        assert not (edit & ~rect_mask(shape, rects.tolist())).any()  # the rectangles cover the edit
        assert c.last_form()["bands"] == (1 if opts else 0)

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_pure_lowering_resets_nothing(opts, f64):
    cost, goal = raster(MULTI, 4), (20, 30)
    new = cost.copy()
    new[50:80, 130:160] *= 0.5  # tiles (0, 2) and (1, 2)

    def body(d, c):
        d.solve()
        check(d.resolve_cost(new), new, goal, f64)
        rects, kinds, info = d.diff_of_last(c)
        assert rects.tolist() == [[130, 50, 160, 64], [130, 64, 160, 80]]
        assert (kinds == LOWERED).all() and info["cells_raised"] == 0 and info["cells_changed"] == 900
        assert d.f.update_info()["cells"] == 0 and d.f.diff_info()["solved_from_scratch"] == 0

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
def test_mixed_edit_in_one_tile_is_any(f64):
    cost, goal = raster(MULTI, 5), (20, 30)
    new = cost.copy()
    new[100, 100] = np.inf       # raised
    new[110:120, 70:90] *= 0.5   # lowered, the same tile (1, 1)

    def body(d, c):
        d.solve()
        check(d.resolve_cost(new), new, goal, f64)
        rects, kinds, info = d.diff_of_last(c)
        assert rects.tolist() == [[70, 100, 101, 120]] and kinds.tolist() == [ANY]
        assert info["cells_raised"] == 1 and info["cells_changed"] == 201
        assert d.f.update_info()["cells"] > 0

    run(cost, goal, f64, None, body)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_equal_rasters_rebind_and_keep_t(opts, f64):
    cost, goal = raster(MULTI, 6), (20, 30)
    new = cost.copy()
    new[60:71, 60:71] = np.inf

    def body(d, c):
        T_old = d.solve()
        T = d.resolve_cost(cost)  # the same values in the second buffer
        assert np.array_equal(T.view(np.uint8), T_old.view(np.uint8))
        info, di = d.f.update_info(), d.f.diff_info()
        assert [info[k] for k in ("cells", "tiles_marked", "flood_visits", "tiles_queued", "fell_back")] == [0] * 5
        assert [di[k] for k in ("cells_changed", "tiles_changed", "block_side", "solved_from_scratch", "rects")] == [0] * 5
        assert d.work() == 0
        # the solver is bound to the second buffer now: the first one is the caller's, and takes the next cost.
        # (Still bound to the first, the solver would diff that buffer against itself and change nothing.)
        check(d.resolve_cost(new), new, goal, f64)
        assert d.f.update_info()["cells"] > 0

    run(cost, goal, f64, opts, body)


@pytest.mark.parametrize("f64", DTYPES)
def test_invalid_new_cost_is_refused_and_nothing_is_rebound(f64):
    import eikonal
    from eikonal import _lib as L

    cost, goal = raster(MULTI, 7), (20, 30)
    rect = (60, 60, 71, 71)
    new = cost.copy()
    new[rect[1]:rect[3], rect[0]:rect[2]] = np.inf
    bad = new.copy()
    bad[150, 100] = np.nan
    bad[30, 140] = -1.0

    def body(d, c):
        T_old = d.solve()
        d.put_second(bad)
        with pytest.raises(eikonal.EikError) as ei:
            d.f.resolve_cost(d.c2.data_ptr(), d.stream)
        assert ei.value.code == L.EIK_ERR_ARG
        msg = L.lib().eik_last_error(c._h).decode()
        assert "2 cells" in msg and "cost[30][140] = -1" in msg, msg  # the lowest changed tile holding one: (0, 2)
        assert d.f.diff_info()["cells_invalid"] == 2
        assert np.array_equal(d.T().view(np.uint8), T_old.view(np.uint8))
        # still bound to the first buffer: an update with a hand-written rectangle reads the new cost there
        check(d.resolve(new, [rect]), new, goal, f64)

    run(cost, goal, f64, None, body)


# ------------------------------------------------------------------------------- a seed set
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", [None, BANDS])
def test_seed_set_goes_through_resolve_seeds(opts, f64):
    shape = MULTI
    seeds, t0 = [(20, 30), (150, 160), (100, 5)], [0.0, 12.5, 3.0]
    cost = raster(shape)
    rect = (60, 60, 71, 71)
    new = cost.copy()
    new[rect[1]:rect[3], rect[0]:rect[2]] = np.inf
    R0, R1 = seeded_reference(cost, seeds, t0), seeded_reference(new, seeds, t0)

    def body(d, c):
        import torch

        T_old = d.solve_seeds(seeds, t0)
        check_seeded(T_old, R0, seeds, t0, f64)
        lab_old = d.labels(seeds, t0)
        c2 = torch.from_numpy(np.ascontiguousarray(new, d.dt)).to(d.dev)
        d.f.resolve_cost(c2.data_ptr(), d.stream)
        T = d.T()
        check_seeded(T, R1, seeds, t0, f64)
        info, di = d.f.update_info(), d.f.diff_info()
        assert info["cells"] > 0 and info["fell_back"] == 0 and di["solved_from_scratch"] == 0 and di["rects"] == 4
        lab = d.labels(seeds, t0)
        assert np.array_equal(lab, label_rule(T, seeds, t0))
        cone, _, _ = seeded_closure(T_old, rect_mask(shape, [rect]), (seeds, t0), (seeds, t0))
        assert info["cells"] == int(cone.sum())
        assert np.array_equal(lab[~cone], lab_old[~cone])
        assert np.array_equal(T[~cone].view(np.uint8), T_old[~cone].view(np.uint8))

    RS.run(cost, f64, opts, body)


WIDE = (190, 370)  # 3 x 6 = 18 tiles, cut on the south and east: more than the share rule's 16-tile floor


@functools.lru_cache(maxsize=None)
def wide_case():
    """the seed set, a cost, its double (every tile changes), a one-tile edit of that, and the two new
    costs' reference fields: made once, shared by both dtypes, left unchanged"""
    seeds, t0 = [(20, 30), (330, 160), (180, 5)], [0.0, 12.5, 3.0]
    cost = raster(WIDE)
    new = 2.0 * cost
    edit = new.copy()
    edit[100:110, 200:210] = np.inf  # inside tile (1, 3)
    made = cost, new, edit, seeded_reference(new, seeds, t0), seeded_reference(edit, seeds, t0)
    for a in made:
        a.setflags(write=False)
    return (seeds, t0, *made)


@pytest.mark.parametrize("f64", DTYPES)
def test_seed_set_whole_raster_change_solves_from_scratch(f64):
    """the share rule on a seeded solver: eik_fim2d_resolve_cost solves from scratch from the bound list"""
    seeds, t0, cost, new, edit, R_new, R_edit = wide_case()

    def body(d, c):
        import torch

        d.solve_seeds(seeds, t0)
        c2 = torch.from_numpy(np.array(new, d.dt, order="C")).to(d.dev)
        d.f.resolve_cost(c2.data_ptr(), d.stream)
        T = d.T()
        info, di = d.f.update_info(), d.f.diff_info()
        print(f64, info, di)
        assert di["tiles_changed"] == 18 and di["cells_raised"] == cost.size
        assert di["solved_from_scratch"] == 1 and di["rects"] == 0 and info["fell_back"] == 0
        check_seeded(T, R_new, seeds, t0, f64)
        assert np.array_equal(d.labels(seeds, t0), label_rule(T, seeds, t0))
        # ... and stays updatable: the solver is bound to c2, the first buffer takes the next cost
        d.set_cost(edit)
        d.f.resolve_cost(d.cd.data_ptr(), d.stream)
        T2 = d.T()
        di = d.f.diff_info()
        assert di["solved_from_scratch"] == 0 and di["tiles_changed"] == 1 and d.f.update_info()["cells"] > 0
        check_seeded(T2, R_edit, seeds, t0, f64)

    RS.run(cost, f64, None, body)


# ------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("f64", DTYPES)
def test_refusals_say_why(f64):
    import torch
    from eikonal import _lib as L

    cost, goal = raster(MULTI, 8), (20, 30)

    def why(c, fn, text):
        RP._raises_arg(c, fn)
        msg = L.lib().eik_last_error(c._h).decode()
        assert text in msg, msg

    def body(d, c):
        f, st = d.f, d.stream
        d.put_second(cost)
        new = d.c2.data_ptr()
        why(c, lambda: f.resolve_cost(new, st), "never started or adopted")
        f.start(d.cd.data_ptr(), d.Td.data_ptr(), [list(goal)], st)
        why(c, lambda: f.resolve_cost(new, st), "did not end converged")
        assert f.iterate(1 << 20) == 0
        why(c, lambda: f.resolve_cost(None, st), "d_cost_new is NULL")
        # list mode: by the option, and a solve that ran in it
        c.set_option(L.OPT_MODE, L.MODE_LIST)
        why(c, lambda: f.resolve_cost(new, st), "persistent mode")
        d.solve()
        c.set_option(L.OPT_MODE, L.MODE_PERSISTENT)
        why(c, lambda: f.resolve_cost(new, st), "did not run in the persistent mode")
        T_old = d.solve()
        # ghost strips bound
        strip = torch.full((256,), float("inf"), dtype=d.cd.dtype, device=d.dev)
        f.set_ghosts(strip.data_ptr(), None, None, None)
        why(c, lambda: f.resolve_cost(new, st), "ghost strips")
        f.set_ghosts(None, None, None, None)
        # B = 2 and a layered block
        dtype = L.EIK_F64 if f64 else L.EIK_F32
        for g, text in ((L.Fim2d(c, 2, 64, 64, dtype), "one map"), (L.Fim3dLayered(c, 64, 64, 4, 0, 2, dtype), "layered")):
            try:
                why(c, lambda: g.resolve_cost(new, st), text)
            finally:
                g.close()
        assert np.array_equal(d.T().view(np.uint8), T_old.view(np.uint8))  # nothing was launched on T
        # and the solver still works
        nw = cost.copy()
        nw[60:71, 60:71] = np.inf
        check(d.resolve_cost(nw), nw, goal, f64)

    run(cost, goal, f64, None, body)


# ------------------------------------------------------------------------------- the share rule, coarsening
BIG = (2112, 2048)  # 33 x 32 = 1056 tiles: the smallest raster with more tiles than eik_fim2d_update takes rectangles


def test_whole_raster_change_solves_from_scratch():
    cost = np.random.default_rng(2112).uniform(1, 10, BIG).astype(np.float32).astype(np.float64)
    goal = (700, 900)
    new = 2.0 * cost  # every tile has raised cells

    def body(d, c):
        d.solve()
        T = d.resolve_cost(new)
        di = d.f.diff_info()
        assert di["tiles_changed"] == 1056 and di["cells_raised"] == cost.size
        assert di["solved_from_scratch"] == 1 and di["rects"] == 0 and di["block_side"] == 0
        check(T, new, goal, False)
        # ... and stays updatable, on the second buffer
        nw = new.copy()
        nw[400:416, 400:416] = np.inf
        T2 = d.resolve_cost(nw)
        assert d.f.diff_info()["solved_from_scratch"] == 0 and d.f.diff_info()["tiles_changed"] == 1
        assert np.isinf(T2[400:416, 400:416]).all() and d.f.update_info()["cells"] > 0

    run(cost, goal, False, None, body)


def test_more_changed_tiles_than_rectangles_are_boxed_per_2x2():
    """one cell lowered in each of 1030 tiles: 1030 > 1024 rectangles, so the boxes are per 2 x 2 tiles.  (The
    measured share, DESIGN.md §3.15, is far below 1030 / 1056: eik_fim2d_resolve_cost would solve this
    from scratch, so the coarsening is checked on eik_cost_diff_dev with cap = 1024.)"""
    import torch
    from eikonal import _lib as L

    rng = np.random.default_rng(1030)
    old = rng.uniform(1, 10, BIG).astype(np.float32)
    new = old.copy()
    tiles = rng.permutation(1056)[:1030]
    ys = tiles // 32 * 64 + rng.integers(0, 64, 1030)
    xs = tiles % 32 * 64 + rng.integers(0, 64, 1030)
    new[ys, xs] *= 0.5
    dev = torch.device("cuda", 0)
    do, dn = torch.from_numpy(old).to(dev), torch.from_numpy(new).to(dev)
    c = RP._context()
    try:
        rects, kinds, info = c.cost_diff(do.data_ptr(), dn.data_ptr(), L.EIK_F32, *BIG, 1024)
        wr, wk, wi = D.cost_diff(old, new, 1024)
        assert info["block_side"] == 2 and info["tiles_changed"] == 1030 and info["cells_changed"] == 1030
        assert len(rects) <= 1024 and (kinds == LOWERED).all()
        assert [tuple(int(v) for v in r) for r in rects] == wr and kinds.tolist() == wk
        assert {k: info[k] for k in wi} == wi
    finally:
        c.close()


# ------------------------------------------------------------------------------- DEM -> cost -> field
def _mesa(n, bx, by, rad=16, h=0.6):
    yy, xx = np.mgrid[0:n, 0:n]
    return h * np.clip((rad - np.hypot(xx - bx, yy - by)) / 3.0, 0, 1)


def test_dem_chain_stays_on_the_device():
    """DEM edit -> eik_costmap_dev into the second buffer -> eik_fim2d_resolve_cost.  The DEM holds a mesa
    at (100, 100), so the largest obstacle-free disc lies to its south-east; the new bump at (45, 45) leaves
    that disc alone and adds no ramp value below the border's, so the ramp's global maximum and minimum stay
    and the costs change in the bump's neighbourhood only (checked with the oracle: 4 of 16 tiles).  A bump
    at (215, 215) would move the maximum and change all 16."""
    import torch
    import costmap_oracle as CO
    import terrain_np
    from eikonal import _lib as L

    n, res = 256, 0.05
    Z0 = terrain_np.dem(n, n, seed=9, rms_slope=0.18) + 3.0 + _mesa(n, 100, 100)
    Z1 = Z0 + _mesa(n, 45, 45)
    goal = (200, 200)
    o0, o1 = (CO.cost_map(Z, res, res * n)[0].T for Z in (Z0, Z1))
    want_tiles = [r["tile"] for r in D.tile_records(o0, o1)]
    assert want_tiles == [0, 1, 4, 5]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    c = RP._context()
    try:
        zd = [torch.from_numpy(Z).to(dev) for Z in (Z0, Z1)]
        cd = [torch.empty((n, n), dtype=torch.float64, device=dev) for _ in range(2)]
        Td = torch.empty((n, n), dtype=torch.float64, device=dev)
        f = L.Fim2d(c, 1, n, n, L.EIK_F64)
        try:
            c._chk(L.lib().eik_costmap_dev(c._h, zd[0].data_ptr(), n, n, res, res * n, None, cd[0].data_ptr(), None, stream))
            f.solve(cd[0].data_ptr(), Td.data_ptr(), [list(goal)], stream)
            c._chk(L.lib().eik_costmap_dev(c._h, zd[1].data_ptr(), n, n, res, res * n, None, cd[1].data_ptr(), None, stream))
            f.resolve_cost(cd[1].data_ptr(), stream)
            torch.cuda.synchronize()
            di, info = f.diff_info(), f.update_info()
            new = cd[1].cpu().numpy()
            assert np.isfinite(new[goal[1], goal[0]])
            check(Td.cpu().numpy(), new, goal, True)
            assert 0 < di["tiles_changed"] < 16 and di["solved_from_scratch"] == 0 and di["cells_invalid"] == 0
            assert di["tiles_changed"] == len(want_tiles) and di["rects"] == len(want_tiles)
            assert info["cells"] > 0 and info["fell_back"] == 0
        finally:
            f.close()
    finally:
        c.close()


# ------------------------------------------------------------------------------- host buffers, the drop-in
def test_host_buffer_forms_leave_inputs_alone():
    import FastMarching.FastMarching as FM

    cost, goal = raster(MULTI, 13), (20, 30)
    new = cost.copy()
    new[60:71, 60:71] = np.inf
    new[140:170, 20:50] = 1.0
    R = F.oracle_field(new, list(goal))
    c = RP._context()
    try:
        for f64 in DTYPES:
            dt = np.float64 if f64 else np.float32
            T0 = c.tmap2d(cost.astype(dt), goal, dtype=dt)
            a, o, b = new.astype(dt), cost.astype(dt), T0.copy()
            T = c.tmap2d_update_cost(o, a, b, goal, dtype=dt)
            assert np.array_equal(a, new.astype(dt)) and np.array_equal(o, cost.astype(dt))
            assert np.array_equal(b.view(np.uint8), T0.view(np.uint8))
            F.check_field(T, R, goal, f64)
            with pytest.raises(ValueError):
                c.tmap2d_update_cost(o, a, b[:, :1], goal, dtype=dt)
            bad = a.copy()
            bad[5, 5] = -2.0
            RP._raises_arg(c, lambda: c.tmap2d_update_cost(o, bad, b, goal, dtype=dt))
    finally:
        c.close()
    T0 = FM.computeTmap(cost, goal)
    want = FM.computeTmap(new, goal)
    f64 = FM._DTYPE == np.float64
    a, o, b = np.asfortranarray(new), np.asfortranarray(cost), T0.copy()
    T = FM.updateTmapFromCost(a, o, b, goal)
    assert T.dtype == np.float64 and np.array_equal(a, new) and np.array_equal(o, cost) and np.array_equal(b, T0)
    F.check_field(T, R, goal, f64)
    F.check_field(T, want, goal, f64)
    assert np.array_equal(FM.updateTmapFromCost(new, new, want, goal), want)
