"""The re-solve of a seeded field after cost and seed-list changes (eik_fim2d_adopt_seeds /
update_seeds / resolve_seeds, eik_tmap2d_update_seeds_*) on the GPU.

The expected field is tests/test_seeds_abi.seeded_reference of the NEW cost and the NEW list; bounds are
the suite's (test_gpu_seeds.check_seeded / close): reachability masks identical, fp32 <= 2e-5 relative,
fp64 <= 1e-9 absolute.  The invalidated set is compared cell for cell with the numpy rule of
tests/test_replan_seeds_rule.py (seeded_closure, restart_state) applied to the device's own T_old.

Every case runs in both dtypes, on the FIFO and with the priority bands forced.  References are computed
once per scenario (functools.lru_cache) and shared by its parametrised runs.
"""
import functools

import numpy as np
import pytest

import test_gpu_fim2d as F
from test_gpu_seeds import BANDS, check_labels, check_seeded, close
from test_replan_rule import rect_mask
from test_replan_seeds_rule import restart_state, seeded_closure
from test_seeds_abi import FIVE_SEEDS, FIVE_SHAPE, FIVE_T0, label_rule, raster, seeded_reference

pytestmark = pytest.mark.gpu

ANY, LOWERED = 0, 1
DTYPES = [False, True]
OPTS = [None, BANDS]
MULTI = FIVE_SHAPE  # 190 x 170: 3 x 3 tiles, cut on the south and east


def _context(options=None):
    import eikonal
    from eikonal import _lib as L

    return eikonal.Context(0, options=dict(options or {}, MODE=L.MODE_PERSISTENT, QTIMEOUT=5))


class Dev:
    """One device-resident solver with its cost and T tensors"""

    def __init__(self, ctx, cost, f64):
        import torch
        from eikonal import _lib as L

        self.torch, self.ctx, self.f64 = torch, ctx, f64
        self.dt = np.float64 if f64 else np.float32
        self.dev = torch.device("cuda", 0)
        self.cd = torch.from_numpy(np.array(cost, self.dt, order="C")).to(self.dev)
        self.Td = torch.full_like(self.cd, float("nan"))
        H, W = cost.shape
        self.f = L.Fim2d(ctx, 1, H, W, L.EIK_F64 if f64 else L.EIK_F32)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def close(self):
        self.f.close()

    def set_cost(self, cost):
        self.cd.copy_(self.torch.from_numpy(np.array(cost, self.dt, order="C")))

    def solve_seeds(self, seeds, t0=None):
        self.f.solve_seeds(self.cd.data_ptr(), self.Td.data_ptr(), seeds, t0, None, self.stream)
        return self.T()

    def resolve_seeds(self, cost, rects, kinds=None, seeds=None, t0=None):
        if cost is not None:
            self.set_cost(cost)
        self.f.resolve_seeds(rects, kinds, seeds, t0, self.stream)
        return self.T()

    def update_seeds(self, cost, rects, kinds=None, seeds=None, t0=None):
        if cost is not None:
            self.set_cost(cost)
        self.f.update_seeds(rects, kinds, seeds, t0, self.stream)
        return self.T()

    def labels(self, seeds, t0=None):
        return self.ctx.labels2d(self.Td, seeds, t0).cpu().numpy()

    def T(self):
        self.torch.cuda.synchronize()
        return self.Td.cpu().numpy()

    def work(self):
        s = self.f.stats()
        return s["tile_visits"] + s["inplace_passes"]


def run(cost, f64, opts, body):
    c = _context(opts)
    try:
        d = Dev(c, cost, f64)
        try:
            return body(d, c)
        finally:
            d.close()
    finally:
        c.close()


def paint(cost, edits):
    """a copy of cost with every ((x0, y0, x1, y1), value) of edits written"""
    new = np.array(cost, np.float64)
    for (x0, y0, x1, y1), v in edits:
        new[y0:y1, x0:x1] = v
    return new


def tiles_of(mask):
    return {(y // 64, x // 64) for y, x in zip(*np.nonzero(mask))}


# Per shape: (shape, seeds, t0, the new obstacle's rectangle).  The last seed of each list is dominated.
SHAPES = {
    "multi": (MULTI, FIVE_SEEDS, FIVE_T0, (60, 60, 71, 71)),  # across a tile corner, over the root (64, 64)
    "tile64": ((64, 64), [(5, 5), (60, 50), (6, 5)], [0.0, 3.0, 50.0], (30, 30, 41, 41)),
    "cut50x40": ((50, 40), [(5, 5), (35, 45), (5, 6)], [1.5, 0.0, 80.0], (20, 25, 28, 33)),
    "strip1x200": ((1, 200), [(10, 0), (199, 0), (11, 0)], [0.0, 2.0, 500.0], (100, 0, 104, 1)),
}
SHAPE_RUNS = [("multi", None), ("multi", BANDS), ("tile64", None), ("cut50x40", None), ("strip1x200", None),
              ("strip1x200", BANDS)]


# ------------------------------------------------------------------------------- scenarios
# A scenario: the first cost and list, then steps (cost edits, rects, kinds, new list or None).  Its
# references -- seeded_reference of every step's cost and list -- are computed once.
def _five(seed=7):
    return raster(MULTI, seed), list(FIVE_SEEDS), list(FIVE_T0)


def _walled(gap_open):
    cost = raster(MULTI, 11)
    cost[:, 100] = np.inf
    if gap_open:
        cost[80, 100] = 2.0
    return cost


WALL_SEEDS, WALL_T0 = [(20, 30), (150, 100), (21, 30)], [0.0, 4.0, 99.0]


def _scenarios():
    S = {}
    for name, (shape, seeds, t0, rect) in SHAPES.items():
        S["obstacle_" + name] = (raster(shape), seeds, t0, [([(rect, np.inf)], [rect], None, None)])
        # a root dropped (seed 1 of every list is one), then the obstacle on top
        keep = [k for k in range(len(seeds)) if k != 1]
        nl = ([seeds[k] for k in keep], [t0[k] for k in keep])
        S["drop_" + name] = (raster(shape), seeds, t0, [([], [], None, nl), ([(rect, np.inf)], [rect], None, None)])
    gap = (100, 80, 101, 81)
    S["close_gap"] = (_walled(True), WALL_SEEDS, WALL_T0, [([(gap, np.inf)], [gap], None, None)])
    S["open_gap"] = (_walled(False), WALL_SEEDS, WALL_T0, [([(gap, 2.0)], [gap], [LOWERED], None)])
    c, s, t = _five(3)
    S["mixed"] = (c, s, t, [([((90, 10, 110, 30), np.inf), ((20, 140, 50, 170), 1.0)],
                            [(90, 10, 110, 30), (20, 140, 50, 170)], [ANY, LOWERED], None)])
    c, s, t = _five(5)
    rects = [(63, 40, 65, 60), (127, 100, 128, 120)]
    back = [(r, None) for r in rects]  # None: the first cost's values again
    S["edge_columns"] = (c, s, t, [([(r, np.inf) for r in rects], rects, None, None), (back, rects, None, None)])
    c, s, t = _five(6)
    S["three_updates"] = (c, s, t, [([((130, 20, 150, 45), np.inf)], [(130, 20, 150, 45)], [ANY], None),
                                    ([((40, 100, 70, 130), 1.0)], [(40, 100, 70, 130)], [LOWERED], None),
                                    ([((60, 60, 71, 71), np.inf)], [(60, 60, 71, 71)], [ANY], None)])
    # cost and list in one call: an obstacle over the root (64, 64), a lowered block, (150, 160) dropped,
    # (20, 30) raised to 6, (100, 5) lowered to 2 (no longer dominated), (100, 100) added
    c, s, t = _five(9)
    nl = ([(20, 30), (63, 64), (64, 64), (100, 5), (100, 100)], [6.0, 40.0, 3.0, 2.0, 1.0])
    S["both"] = (c, s, t, [([((60, 60, 71, 71), np.inf), ((20, 140, 50, 170), 1.0)],
                            [(60, 60, 71, 71), (20, 140, 50, 170)], [ANY, LOWERED], nl)])
    return S


@functools.lru_cache(maxsize=None)
def scenario(name):
    """(cost0, seeds0, t00, R0, [(cost, rects, kinds, list or None, seeds, t0, R), ...])"""
    cost0, seeds0, t00, steps = _scenarios()[name]
    seeds, t0 = seeds0, t00
    R0 = seeded_reference(cost0, seeds0, t00)
    out, cur = [], cost0
    for edits, rects, kinds, nl in steps:
        cur = paint(cur, [(r, v) for r, v in edits if v is not None])
        for r, v in edits:
            if v is None:
                cur[r[1]:r[3], r[0]:r[2]] = cost0[r[1]:r[3], r[0]:r[2]]
        if nl is not None:
            seeds, t0 = nl
        R = seeded_reference(cur, seeds, t0)
        for a in (cur, R):
            a.setflags(write=False)
        out.append((cur, rects, kinds, nl, seeds, t0, R))
    for a in (cost0, R0):
        a.setflags(write=False)
    return cost0, seeds0, t00, R0, out


def play(name, f64, opts, after=None):
    cost0, seeds0, t00, R0, steps = scenario(name)

    def body(d, c):
        check_seeded(d.solve_seeds(seeds0, t00), R0, seeds0, t00, f64)
        for i, (cost, rects, kinds, nl, seeds, t0, R) in enumerate(steps):
            T = d.resolve_seeds(cost, rects, kinds, *(nl or (None, None)))
            check_seeded(T, R, seeds, t0, f64)
            assert not np.signbit(T).any()
            info = d.f.update_info()
            assert info["fell_back"] == 0
            assert c.last_form()["bands"] == (1 if opts else 0)
            if after:
                after(i, d, T, info)

    run(cost0, f64, opts, body)


# ------------------------------------------------------------------------------- 1. cost edits
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("name,opts", SHAPE_RUNS)
def test_new_obstacle_with_the_list_unchanged(name, opts, f64):
    def after(i, d, T, info):
        assert info["cells"] > 0 and info["tiles_marked"] > 0
        if name == "multi":  # the obstacle covers the root (64, 64): spared, it keeps its t0
            assert T[64, 64] == 3.0 and T[64, 63] == 40.0 and np.isinf(T[60:71, 60:71]).sum() == 119

    play("obstacle_" + name, f64, opts, after)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
def test_closing_the_only_gap_of_a_wall(opts, f64):
    def after(i, d, T, info):
        assert np.isfinite(T[:, 101:]).all()  # the east chamber has its own seed

    play("close_gap", f64, opts, after)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
def test_opening_a_wall(opts, f64):
    def after(i, d, T, info):
        assert info["cells"] == 0  # nothing is reset for a lowered cost

    play("open_gap", f64, opts, after)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("name", ["mixed", "edge_columns", "three_updates"])
def test_cost_edits(name, opts, f64):
    """mixed ANY and LOWERED rectangles in different tiles; a change on the tile columns 63 / 64 and back
    (a stale edge-column copy would show after the revert); three successive updates"""
    play(name, f64, opts)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("name,opts", SHAPE_RUNS)
def test_dropping_a_root_then_an_obstacle(name, opts, f64):
    """on every shape: a list edit alone (K == 0), then a cost edit against the list the update bound"""
    def after(i, d, T, info):
        assert info["cells"] > 0

    play("drop_" + name, f64, opts, after)


# ------------------------------------------------------------------------------- 2. the exact set
def tie_raster(shape, kind):
    """integer costs 1..3: neighbouring cells often hold exactly equal T (test_gpu_replan.tie_raster)"""
    if kind == "integer":
        return np.random.default_rng(8).integers(1, 4, shape).astype(np.float64)
    return raster(shape, 8)


@functools.lru_cache(maxsize=None)
def exact_case(name, kind, edit):
    shape, seeds, t0, rect = SHAPES[name]
    if kind == "integer":
        t0 = [float(int(v)) for v in t0]  # integer start values keep the ties
    cost = tie_raster(shape, kind)
    new = paint(cost, [(rect, np.inf)])
    if edit == "cost":
        nl = None
        ns, nt = seeds, t0
    else:  # the root seed 1 dropped, seed 0's t0 raised: raise-only
        keep = [k for k in range(len(seeds)) if k != 1]
        ns, nt = [seeds[k] for k in keep], [t0[k] + (7.0 if k == 0 else 0.0) for k in keep]
        nl = (ns, nt)
    R = seeded_reference(new, ns, nt)
    for a in (cost, new, R):
        a.setflags(write=False)
    return cost, new, seeds, t0, rect, nl, ns, nt, R


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("edit", ["cost", "list"])
@pytest.mark.parametrize("kind", ["float", "integer"])
@pytest.mark.parametrize("name,opts", SHAPE_RUNS)
def test_exact_set(name, opts, kind, edit, f64):
    """after update_seeds and before iterate T is bit for bit the rule's restart state of the downloaded
    T_old: +inf exactly on seeded_closure, the new seeds at min(T, b_new), every other cell untouched;
    after iterate (the edits are raise-only) every cell outside the cone still holds its old bits"""
    cost, new, seeds, t0, rect, nl, ns, nt, R = exact_case(name, kind, edit)
    shape = cost.shape

    def body(d, c):
        T_old = d.solve_seeds(seeds, t0)
        cone, spared, released = seeded_closure(T_old, rect_mask(shape, [rect]), (seeds, t0), (ns, nt))
        assert not (cone & spared).any()
        if edit == "list":
            assert released.sum() == 2
        if kind == "integer" and name == "multi":  # the case does hold ties between neighbours
            fin = np.isfinite(T_old)
            assert ((T_old[:, 1:] == T_old[:, :-1]) & fin[:, 1:]).sum() + ((T_old[1:] == T_old[:-1]) & fin[1:]).sum() > 0
        T_mid = d.update_seeds(new, [rect], None, *(nl or (None, None)))
        want = restart_state(T_old, cone, (ns, nt))
        assert np.array_equal(T_mid.view(np.uint8), want.view(np.uint8))
        gone = np.isfinite(T_old) & np.isinf(T_mid)
        assert np.array_equal(gone | (cone & np.isfinite(want)), cone) and not (gone & ~cone).any()
        for x, y in np.argwhere(spared)[:, ::-1]:
            assert T_mid[y, x] == T_old[y, x]
        info = d.f.update_info()
        assert info["cells"] == int(cone.sum())
        assert info["tiles_marked"] == len(tiles_of(cone))
        assert d.f.iterate(1 << 20) == 0
        T = d.T()
        check_seeded(T, R, ns, nt, f64)
        assert not np.signbit(T).any()
        assert np.array_equal(T[~cone].view(np.uint8), T_old[~cone].view(np.uint8))

    run(cost, f64, opts, body)


# ------------------------------------------------------------------------------- 3. list edits
DUP_SEEDS, DUP_T0 = [(30, 40), (150, 100), (30, 40), (150, 100)], [5.0, 1.0, 2.0, 1.0]


def _without(seeds, t0, k):
    return [s for j, s in enumerate(seeds) if j != k], [v for j, v in enumerate(t0) if j != k]


def _with_t0(k, v):
    t = list(FIVE_T0)
    t[k] = v
    return list(FIVE_SEEDS), t


# name: (cost seed, old list, new list, what is expected of the invalidation)
LIST_EDITS = {
    "drop_root": (7, (FIVE_SEEDS, FIVE_T0), _without(FIVE_SEEDS, FIVE_T0, 1), "region"),
    "raise_t0": (7, (FIVE_SEEDS, FIVE_T0), _with_t0(1, 60.0), "region"),
    "lower_t0": (7, (FIVE_SEEDS, FIVE_T0), _with_t0(1, 2.0), "none"),
    "add_seed": (7, (FIVE_SEEDS, FIVE_T0), (FIVE_SEEDS + [(100, 100)], FIVE_T0 + [1.0]), "none"),
    "drop_lower_of_two": (26, (DUP_SEEDS, DUP_T0), _without(DUP_SEEDS, DUP_T0, 2), "region"),
    "drop_dominated": (7, (FIVE_SEEDS, FIVE_T0), _without(FIVE_SEEDS, FIVE_T0, 4), "identical"),
    "drop_dominating": (7, (FIVE_SEEDS, FIVE_T0), _without(FIVE_SEEDS, FIVE_T0, 3), "region"),
    "disjoint": (7, (FIVE_SEEDS, FIVE_T0), ([(10, 180), (160, 10), (85, 95)], [0.0, 2.0, 1.0]), "all"),
}


@functools.lru_cache(maxsize=None)
def list_case(name):
    seed, old, new, expect = LIST_EDITS[name]
    cost = raster(MULTI, seed)
    R0, R = seeded_reference(cost, *old), seeded_reference(cost, *new)
    for a in (cost, R0, R):
        a.setflags(write=False)
    return cost, old, new, expect, R0, R


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("name", list(LIST_EDITS))
def test_list_edit_at_an_unchanged_cost(name, opts, f64):
    cost, old, new, expect, R0, R = list_case(name)

    def body(d, c):
        T_old = d.solve_seeds(*old)
        check_seeded(T_old, R0, old[0], old[1], f64)
        cone, spared, released = seeded_closure(T_old, np.zeros(MULTI, bool), old, new)
        T = d.resolve_seeds(None, [], None, *new)
        info, work = d.f.update_info(), d.work()
        check_seeded(T, R, new[0], new[1], f64)
        assert info["cells"] == int(cone.sum()) and info["tiles_marked"] == len(tiles_of(cone)) and info["fell_back"] == 0
        if expect == "none":
            assert info["cells"] == 0 and not released.any() and work > 0  # lowering edits reset nothing
        elif expect == "identical":
            assert info["cells"] == 0 and info["tiles_queued"] == 0 and work == 0
            assert np.array_equal(T.view(np.uint8), T_old.view(np.uint8))
        elif expect == "region":
            assert released.sum() == 1 and 0 < info["cells"] < cost.size
            assert np.array_equal(T[~cone].view(np.uint8), T_old[~cone].view(np.uint8))  # (raise-only edits)
        else:
            assert released.sum() == 3 and info["cells"] == cost.size  # every root released: the whole field
            close(T, d.solve_seeds(*new).astype(np.float64), f64)       # ... equals a fresh solve
        if name == "drop_lower_of_two":
            assert T_old[40, 30] == 2.0 and T[40, 30] == 5.0  # released, re-seeded at the higher t0
        if name == "drop_dominating":
            assert T_old[64, 63] < 40.0 and T[64, 63] == 40.0  # (63, 64) is a root now
        # the updated list is the bound one: a further update of the cost alone spares its roots
        new_cost = paint(cost, [((130, 20, 150, 45), np.inf)])
        T2 = d.resolve_seeds(new_cost, [(130, 20, 150, 45)])
        for (x, y), v in zip(*new):
            assert T2[y, x] <= T.dtype.type(v)
        assert not np.signbit(T2).any() and np.isinf(T2[20:45, 130:150]).all()

    run(cost, f64, opts, body)


# ------------------------------------------------------------------------------- 4. both, labels
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
def test_cost_and_list_edits_in_one_call_and_labels(opts, f64):
    def after(i, d, T, info):
        _, _, _, _, steps = scenario("both")
        seeds, t0, R = steps[0][4], steps[0][5], steps[0][6]
        lab = d.labels(seeds, t0)
        check_labels(lab, T, R, seeds, t0)
        assert np.array_equal(lab, label_rule(T, seeds, t0))
        assert T[5, 100] == 2.0 and lab[5, 100] == 3 and T[100, 100] == 1.0 and lab[100, 100] == 4
        assert info["cells"] > 0

    play("both", f64, opts, after)


# ------------------------------------------------------------------------------- 5. zero costs round a root
ZERO_SEEDS, ZERO_T0 = [(70, 60), (150, 160)], [0.0, 5.0]


@functools.lru_cache(maxsize=None)
def zero_case(rect):
    cost = raster(MULTI, 16)
    cost[52:69, 58:79] = 0.0  # the patch straddles the tile edge x = 63 | 64
    new = paint(cost, [(rect, 5.0)])
    R0, R = seeded_reference(cost, ZERO_SEEDS, ZERO_T0), seeded_reference(new, ZERO_SEEDS, ZERO_T0)
    for a in (cost, new, R0, R):
        a.setflags(write=False)
    return cost, new, R0, R


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("rect", [(66, 58, 69, 63), (60, 50, 80, 70)], ids=["beside_root", "round_root"])
def test_zero_cost_patch_round_a_root(rect, opts, f64):
    """test_gpu_replan.test_zero_cost_patch_round_the_goal with a root in the goal's place: the cells of the
    zero-cost patch hold T == 0 (fp32) like the root, so the flood's 0 <= 0 ties reach the root's
    neighbours -- and the spared root is never invalidated"""
    cost, new, R0, R = zero_case(rect)
    gx, gy = ZERO_SEEDS[0]
    lst = (ZERO_SEEDS, ZERO_T0)

    def body(d, c):
        T_old = d.solve_seeds(*lst)
        check_seeded(T_old, R0, ZERO_SEEDS, ZERO_T0, f64)
        cone, spared, released = seeded_closure(T_old, rect_mask(MULTI, [rect]), lst, lst)
        assert spared[gy, gx] and not cone[gy, gx] and not released.any()
        if not f64:  # (fp64 stages a zero cost as 2^-500: T rises by that per cell, no tie with the root)
            assert (T_old[52:69, 58:79] == 0).all()
            assert cone[gy, gx - 1] and cone[gy + 1, gx]  # the ties do reach the root's side
        T_mid = d.update_seeds(new, [rect])
        assert T_mid[gy, gx] == 0 and not np.signbit(T_mid[gy, gx])
        assert np.array_equal(np.isfinite(T_old) & np.isinf(T_mid), cone)
        assert d.f.update_info()["cells"] == int(cone.sum())
        assert d.f.iterate(1 << 20) == 0
        T = d.T()
        check_seeded(T, R, ZERO_SEEDS, ZERO_T0, f64)
        assert not np.signbit(T).any()

    run(cost, f64, opts, body)


# ------------------------------------------------------------------------------- 6. nothing to do
POCKET_SEEDS, POCKET_T0 = [(20, 30), (60, 150), (21, 30)], [0.0, 3.0, 77.0]


@functools.lru_cache(maxsize=None)
def pocket_case():
    cost = raster(MULTI, 10)
    cost[120:160, 100] = cost[120:160, 150] = np.inf
    cost[120, 100:151] = cost[159, 100:151] = np.inf
    new2 = paint(cost, [((110, 130, 140, 150), 1.5), ((60, 60, 71, 71), np.inf)])
    R2 = seeded_reference(new2, POCKET_SEEDS, POCKET_T0)
    for a in (cost, new2, R2):
        a.setflags(write=False)
    return cost, new2, R2


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("what", ["K0", "pocket", "same_list"])
def test_nothing_to_do(what, opts, f64):
    """K == 0 with seeds=None, a rectangle inside an unreachable pocket, an identical list passed
    explicitly: 0 cells invalidated, 0 tiles queued, 0 solve visits, T bit-identical, the solver usable"""
    cost, new2, R2 = pocket_case()
    new = paint(cost, [((110, 130, 140, 150), 1.5)]) if what == "pocket" else cost
    rects = [(110, 130, 140, 150)] if what == "pocket" else []
    lst = (POCKET_SEEDS, POCKET_T0) if what == "same_list" else (None, None)

    def body(d, c):
        T_old = d.solve_seeds(POCKET_SEEDS, POCKET_T0)
        assert np.isinf(T_old[121:159, 101:150]).all()
        T = d.resolve_seeds(new, rects, None, *lst)
        assert np.array_equal(T.view(np.uint8), T_old.view(np.uint8))
        info = d.f.update_info()
        assert info["cells"] == 0 and info["tiles_marked"] == 0 and info["tiles_queued"] == 0
        assert d.work() == 0
        if what != "pocket":  # a no-op leaves the solver converged: an update without an iterate in between
            d.f.update_seeds([], None, None, None, d.stream)
            d.f.update_seeds([], None, *lst, d.stream)
        check_seeded(d.resolve_seeds(new2, [(60, 60, 71, 71), (110, 130, 140, 150)]), R2, POCKET_SEEDS, POCKET_T0, f64)

    run(cost, f64, opts, body)


# ------------------------------------------------------------------------------- 7. work
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
def test_work_condition(opts, f64):
    """512 x 512, three seeds, a 16 x 16 block raised to inf: the flood marks exactly the tiles of the
    numpy cone of the device's T_old (on the CPU 822 cells in one tile, 0.3 %), and the re-solve does less
    than half of the full seeded solve's tile work (visits + in-place passes) on the same solver and
    cost -- test_gpu_replan.test_work_condition's bound.  The field is compared with that full solve."""
    cost = np.random.default_rng(512).uniform(1, 10, (512, 512)).astype(np.float32).astype(np.float64)
    seeds, t0 = [(40, 40), (470, 60), (60, 470)], [0.0, 5.0, 0.0]
    rect = (400, 400, 416, 416)
    new = paint(cost, [(rect, np.inf)])

    def body(d, c):
        T_old = d.solve_seeds(seeds, t0)
        cone, _, _ = seeded_closure(T_old, rect_mask(cost.shape, [rect]), (seeds, t0), (seeds, t0))
        T = d.resolve_seeds(new, [rect])
        work, info = d.work(), d.f.update_info()
        full_T = d.solve_seeds(seeds, t0)
        full = d.work()
        print(f"f64={f64} {opts}: update {info}, cone {int(cone.sum())} cells, re-solve work {work}, full solve work {full}")
        assert info["cells"] == int(cone.sum()) and info["tiles_marked"] == len(tiles_of(cone))
        assert work < full / 2, (work, full)
        close(T, full_T.astype(np.float64), f64)
        for (x, y), v in zip(seeds, t0):
            assert T[y, x] == v

    run(cost, f64, opts, body)


# ------------------------------------------------------------------------------- 8. band-ring overflow
def test_band_ring_overflow_falls_back_to_a_full_seeded_solve():
    """test_gpu_replan.test_band_ring_overflow_falls_back_to_a_full_solve with a seed list: the root where
    the goal was, and a dominated seed beside it in the same tile.  After the first solve the band rings
    are cut to ONE slot and the grid to ONE workgroup; a rectangle round the root resets the whole field,
    and only the root's tile is queued (the dominated seed's push finds it queued).  That tile's visit
    activates two neighbours into band 0, whose ring holds one: the launch ends on the overflow word and
    eik_fim2d_resolve_seeds solves in full on the FIFO with the bound list."""
    from eikonal import _lib as L

    H, W = 777, 1100
    cost = np.random.default_rng(77).uniform(1, 10, (H, W))
    goal = (W // 3, H // 2)
    seeds, t0 = [goal, (goal[0] + 1, goal[1])], [0.0, 500.0]
    rect = (goal[0] - 8, goal[1] - 8, goal[0] + 8, goal[1] + 8)
    new = paint(cost, [(rect, 9.0)])
    new2 = paint(new, [((900, 600, 930, 620), np.inf)])

    def check(T, cost):
        F.check_field(T, F.oracle_field(cost, list(goal)), goal, True)  # (the dominated seed changes nothing)

    def body(d, c):
        check(d.solve_seeds(seeds, t0), cost)
        assert c.last_form()["bands"] == 1
        c.set_option(L.OPT_PRIO_RING, 1)
        c.set_option(L.OPT_GRID, 1)
        check(d.resolve_seeds(new, [rect]), new)
        info = d.f.update_info()
        assert info["cells"] == cost.size - 1 and info["tiles_queued"] == 1
        assert info["fell_back"] == 1 and c.last_form()["bands"] == 0  # the fall-back's solve ran on the FIFO
        c.set_option(L.OPT_GRID, 0)  # the default grid again
        check(d.resolve_seeds(new2, [(900, 600, 930, 620)]), new2)
        assert d.f.update_info()["fell_back"] == 0 and c.last_form()["bands"] == 0  # the solver keeps the FIFO

    run(cost, True, {"PRIO": 1.0}, body)


# ------------------------------------------------------------------------------- 9. adopt, host forms
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
def test_adopt_a_seeded_field_from_another_context(opts, f64):
    import torch

    cost0, seeds0, t00, R0, steps = scenario("both")
    cost, rects, kinds, nl, seeds, t0, R = steps[0]
    dt = np.float64 if f64 else np.float32
    other = _context()
    try:
        T0 = other.tmap2d_seeds(cost0.astype(dt), seeds0, t00, dtype=dt)
    finally:
        other.close()

    def body(d, c):
        d.Td.copy_(torch.from_numpy(T0))
        d.set_cost(cost)
        d.f.adopt_seeds(d.cd.data_ptr(), d.Td.data_ptr(), seeds0, t00, d.stream)
        d.f.resolve_seeds(rects, kinds, *nl, d.stream)
        check_seeded(d.T(), R, seeds, t0, f64)
        assert c.last_form()["bands"] == (1 if opts else 0)

    run(cost0, f64, opts, body)


def test_host_buffer_forms_leave_inputs_alone_and_paths_follow():
    import FastMarching.FastMarching as FM

    cost0, seeds0, t00, R0, steps = scenario("both")
    cost, rects, kinds, nl, seeds, t0, R = steps[0]
    c = _context()
    try:
        for f64 in DTYPES:
            dt = np.float64 if f64 else np.float32
            T0 = c.tmap2d_seeds(cost0.astype(dt), seeds0, t00, dtype=dt)
            a, b = cost.astype(dt), T0.copy()
            T, lab = c.tmap2d_update_seeds(a, b, seeds0, t00, rects, kinds, nl[0], nl[1], dtype=dt, labels=True)
            assert np.array_equal(a, cost.astype(dt)) and np.array_equal(b.view(np.uint8), T0.view(np.uint8))
            assert T.dtype == dt
            check_seeded(T, R, seeds, t0, f64)
            check_labels(lab, T, R, seeds, t0)
            # the list kept: the cost edit alone
            Tk = c.tmap2d_update_seeds(a, b, seeds0, t00, rects, kinds, dtype=dt)
            Rk = seeded_reference(cost, seeds0, t00)
            check_seeded(Tk, Rk, seeds0, t00, f64)
            with pytest.raises(ValueError):
                c.tmap2d_update_seeds(a, b[:, :1], seeds0, t00, rects, dtype=dt)  # (would broadcast silently)
    finally:
        c.close()
    f64 = FM._DTYPE == np.float64
    T0 = FM.computeTmapMulti(cost0, seeds0, t00)
    mask = cost != cost0
    for changed in (rects, mask, np.asfortranarray(mask)):
        a, b = np.asfortranarray(cost), T0.copy()
        T, lab = FM.updateTmapMulti(a, b, seeds0, changed, t00, nl[0], nl[1], labels=True)
        assert T.dtype == np.float64 and lab.dtype == np.int32
        assert np.array_equal(a, cost) and np.array_equal(b, T0)
        check_seeded(T, R, seeds, t0, f64)
        assert np.array_equal(lab, label_rule(T.astype(FM._DTYPE), seeds, t0))
    close(FM.updateTmapMulti(cost, T0, seeds0, rects, t00, nl[0], nl[1]), T, f64)
    # no rectangle, no list change: a copy, and the old list's labels with it
    Tc, labc = FM.updateTmapMulti(cost0, T0, seeds0, [], t00, labels=True)
    assert np.array_equal(Tc, T0) and np.array_equal(labc, label_rule(T0.astype(FM._DTYPE), seeds0, t00))
    # paths on the updated (T, labels) go to the nearest NEW goal: each is getPathGDM's to that goal
    starts = [(30.0, 60.0), (150.0, 150.0), (110.0, 110.0), (100.0, 20.0)]
    assert len({int(lab[int(y), int(x)]) for x, y in starts}) >= 3
    paths = FM.getPathsToNearest(T, lab, seeds, starts, 0.5)
    assert len(paths) == len(starts)
    for p, s in zip(paths, starts):
        one = FM.getPathGDM(T, s, seeds[lab[int(s[1]), int(s[0])]], 0.5)
        assert p.shape == one.shape and np.array_equal(p.view(np.uint8), one.view(np.uint8))


# ------------------------------------------------------------------------------- 10. gates, 11. old calls
def _raises_arg(c, fn, match=None):
    import eikonal
    from eikonal import _lib as L

    with pytest.raises(eikonal.EikError, match=match) as ei:
        fn()
    assert ei.value.code == L.EIK_ERR_ARG
    assert L.lib().eik_last_error(c._h).decode() != ""


@functools.lru_cache(maxsize=None)
def gate_case():
    cost = raster(MULTI, 14)
    new = paint(cost, [((60, 60, 71, 71), np.inf)])
    R, O1 = seeded_reference(new, FIVE_SEEDS, FIVE_T0), F.oracle_field(new, [20, 30])
    for a in (cost, new, R, O1):
        a.setflags(write=False)
    return cost, new, R, O1


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("opts", OPTS)
def test_gates_and_argument_errors(opts, f64):
    from eikonal import _lib as L

    cost, new, R, O1 = gate_case()
    seeds, t0 = list(FIVE_SEEDS), list(FIVE_T0)
    goal = (20, 30)
    ok = [(60, 60, 71, 71)]

    def body(d, c):
        f, st = d.f, d.stream
        cp, tp = d.cd.data_ptr(), d.Td.data_ptr()
        up = lambda *a: f.update_seeds(*a, st)  # noqa: E731
        _raises_arg(c, lambda: up(ok, None, None, None), "never started")
        f.start_seeds(cp, tp, seeds, t0, None, st)
        _raises_arg(c, lambda: up(ok, None, None, None), "did not end converged")
        assert f.iterate(1 << 20) == 0
        T_old = d.T()
        # bad rectangles and kinds, as eik_fim2d_update
        for rects, kinds in (([(71, 60, 60, 71)], None), ([(60, 71, 71, 60)], None), ([(60, 60, 60, 71)], None),
                             ([(170, 0, 180, 10)], None), ([(-9, -9, 0, 0)], None), (ok, [2]), (ok, [-1]),
                             ([ok[0]] * 1025, None)):
            _raises_arg(c, lambda: up(rects, kinds, None, None), "eik_fim2d_update_seeds")
            _raises_arg(c, lambda: f.resolve_seeds(rects, kinds, None, None, st))
        # bad seed lists: the shared check names the index
        _raises_arg(c, lambda: up(ok, None, [(1, 1), (170, 3)], None), r"seed 1 \(170, 3\)")
        _raises_arg(c, lambda: up(ok, None, [(1, 1), (3, -1)], None), r"seed 1 \(3, -1\)")
        _raises_arg(c, lambda: up(ok, None, [(1, 1), (2, 2)], [0.0, -0.5]), r"t0\[1\] = -0.5")
        _raises_arg(c, lambda: up(ok, None, [(1, 1)], [float("nan")]), r"t0\[0\] = nan")
        _raises_arg(c, lambda: up(ok, None, [(1, 1)], [float("inf")]), r"t0\[0\] = inf")
        _raises_arg(c, lambda: up(ok, None, np.zeros((0, 2), np.int64), None), "K = 0")  # Ks < 1 with seeds
        _raises_arg(c, lambda: f.adopt_seeds(cp, tp, [(170, 3)], None, st), r"seed 0 \(170, 3\)")
        _raises_arg(c, lambda: f.adopt_seeds(None, tp, seeds, t0, st), "d_cost is NULL")
        assert np.array_equal(d.T().view(np.uint8), T_old.view(np.uint8))  # nothing was launched
        # 11. the single-goal calls keep refusing the seeded solver, before and after a seeded update
        for fn in (f.update, f.resolve):
            _raises_arg(c, lambda: fn(ok, None, st), "seed set")
        d.set_cost(new)
        f.resolve_seeds(ok, None, None, None, st)
        for fn in (f.update, f.resolve):
            _raises_arg(c, lambda: fn(ok, None, st), "seed set")
        assert d.T()[64, 64] == 3.0
        # a single-goal-bound solver: solve, and adopt
        d.set_cost(cost)
        f.solve(cp, tp, [list(goal)], st)
        T1 = d.T()
        _raises_arg(c, lambda: up(ok, None, None, None), "single goal")
        _raises_arg(c, lambda: up(ok, None, seeds, t0), "single goal")
        f.adopt(cp, tp, [list(goal)], st)
        _raises_arg(c, lambda: f.resolve_seeds(ok, None, None, None, st), "single goal")
        assert np.array_equal(d.T().view(np.uint8), T1.view(np.uint8))
        f.adopt_seeds(cp, tp, [goal], None, st)  # ... until adopt_seeds binds the field to a list
        d.set_cost(new)
        f.resolve_seeds(ok, None, None, None, st)
        F.check_field(d.T(), O1, goal, f64)
        # list mode
        d.set_cost(cost)
        c.set_option(L.OPT_MODE, L.MODE_LIST)
        _raises_arg(c, lambda: up(ok, None, None, None), "persistent mode")
        _raises_arg(c, lambda: f.adopt_seeds(cp, tp, seeds, t0, st), "persistent mode")
        d.solve_seeds(seeds, t0)                                   # a list-mode seeded solve ...
        c.set_option(L.OPT_MODE, L.MODE_PERSISTENT)
        _raises_arg(c, lambda: up(ok, None, None, None), "persistent mode")  # ... is not updatable
        T2 = d.solve_seeds(seeds, t0)
        # B = 2
        g = L.Fim2d(c, 2, 64, 64, L.EIK_F64 if f64 else L.EIK_F32)
        try:
            _raises_arg(c, lambda: g.adopt_seeds(cp, tp, [(1, 1)], None, st), "one map")
            _raises_arg(c, lambda: g.update_seeds(ok, None, None, None, st), "one map")
        finally:
            g.close()
        assert np.array_equal(d.T().view(np.uint8), T2.view(np.uint8))
        check_seeded(d.resolve_seeds(new, ok), R, seeds, t0, f64)

    run(cost, f64, opts, body)
