"""Hand-offs, cut tiles and the pass cap of the two 3D solvers -- fim3d.hip (general: six face flags,
three tile shapes, the self re-queue at the pass cap, the visit budget, batches) and fim2dl.hip
(layered: per-layer side flags raised by the row waves, layer groups that meet only in LDS) -- on
the volumes of tests/handoff3d.py, built so that one lost store, flag or z neighbour shows in the
field (tests/test_handoff3d_cases.py checks the constructions on the oracle alone).

Everything is checked against the oracle (O.fmm3d, non-strict) with test_gpu_fim3d.py's tolerances:
masks identical, T[goal] == 0, fp64 <= 1e-9 absolute, fp32 <= 2e-5 relative.

Which solver a volume reaches (eikonal_api.cpp fim3d_solve_one): on the persistent driver fp32 with
L <= 4 and fp64 with L <= 3 go to the layered solver, as do that many layers between two all-+inf
pad layers; everything else -- list mode, fp64 with L = 4, every batch, every fp64 solve with a
`start` -- goes to fim3d.hip.  The tests assert the route through eik_stats::fresh_visits, which only
the layered solver counts.
"""
import numpy as np
import pytest

import handoff3d as H3
import oracle as O

pytestmark = pytest.mark.gpu

DRIVERS = ("persistent", "list")


def _context(driver, options=()):
    import eikonal
    from eikonal import _lib as L

    c = eikonal.Context(0)
    c.set_option(L.OPT_MODE, L.MODE_PERSISTENT if driver == "persistent" else L.MODE_LIST)
    for k, v in options:
        c.set_option(getattr(L, k), v)
    return c


@pytest.fixture(scope="module")
def ctxs():
    cs = {d: _context(d) for d in DRIVERS}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module", params=DRIVERS)
def ctx(request, ctxs):
    return ctxs[request.param]


def dt(f64):
    return np.float64 if f64 else np.float32


def solve(c, cost, goal, f64, layered):
    """tmap3d plus the route check: layered = the volume must have gone to fim2dl.hip."""
    T = c.tmap3d(cost, goal, dtype=dt(f64))
    assert (c.stats()["fresh_visits"] > 0) == layered, "the volume went to the other 3D solver"
    return T


F64 = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])


# ------------------------------------------------------ A. general solver: six-face hand-offs
@pytest.mark.parametrize("gaps", H3.SHELL_CASES, ids=H3.shell_id)
@F64
def test_shell_handoff(ctx, gaps, f64):
    """fim3d.hip (L = 24), both drivers: 3 x 3 x 3 tiles of 16 x 8 x 8, the centre tile walled in but
    for one gap cell (a face's centre, an edge cell or a corner, the latter two linked to the interior
    by a chain off the named face), or all six face centres: the other 26 tiles are reachable only
    through the face flag the gap cell raises (process_tile3) and the neighbour face_neighbour3 names."""
    cost = H3.shell_cost(gaps)
    R = H3.oracle_field(("shell", gaps), cost, H3.SHELL_GOAL)
    assert H3.corners_finite(R)
    H3.check_field(solve(ctx, cost, H3.SHELL_GOAL, f64, layered=False), R, H3.SHELL_GOAL, f64)


def flat_runs():
    out = []
    for shape, side, z in H3.FLAT_CASES:
        combos = [("list", False), ("list", True)]
        if shape[2] == 4:
            combos.append(("persistent", True))  # (persistent fp32 with 4 layers is the layered solver's)
        elif shape[2] > 4:
            combos += [("persistent", False), ("persistent", True)]
        out += [(shape, side, z, d, f) for d, f in combos]
    return out


@pytest.mark.parametrize("shape,side,z,driver,f64", flat_runs(),
                         ids=lambda v: H3.flat_id(v) if not isinstance(v, bool) else ("f64" if v else "f32"))
def test_flat_handoff(ctxs, shape, side, z, driver, f64):
    """fim3d.hip's few-layer tile shapes, one tile layer (x and y faces only): 48 x 48 x 3 and
    48 x 48 x 4 with 16 x 16 x L tiles (list mode; 4 layers also persistent fp64), 24 x 48 x 6 with
    16 x 8 x 6 tiles (both drivers).  The centre tile's ring is +inf in every layer, the gap one cell
    of one layer: the flag must come from that layer's cell."""
    goal = H3.flat_goal(shape)
    cost = H3.flat_cost(shape, ((side, z),))
    R = H3.oracle_field(("flat", shape, side, z), cost, goal)
    assert H3.corners_finite(R)
    H3.check_field(solve(ctxs[driver], cost, goal, f64, layered=False), R, goal, f64)


# ------------------------------------------- B. layered solver: one cell of one layer of one side
@pytest.mark.parametrize("f64,nl,gaps", H3.ring_cases(), ids=H3.ring_id)
def test_ring_handoff(ctxs, f64, nl, gaps):
    """fim2dl.hip (persistent, fp32 NL <= 4 / fp64 NL <= 3): 3 x 3 tiles, the centre tile's ring +inf
    in every layer but one cell of one layer -- every side x layer at the middle lane, the corner
    lanes in the last layer (fp64 NL = 3 side S: row 39, the partial last row of row wave 3)."""
    th = H3.layered_rows(f64)
    goal = H3.ring_goal(th)
    cost = H3.ring_cost(th, nl, gaps)
    R = H3.oracle_field(("ring", th, nl, gaps, False), cost, goal)
    assert H3.corners_finite(R)
    H3.check_field(solve(ctxs["persistent"], cost, goal, f64, layered=True), R, goal, f64)


@pytest.mark.parametrize("f64,nl,gaps", H3.ring_pad_cases(), ids=H3.ring_id)
def test_ring_handoff_padded(ctxs, f64, nl, gaps):
    """fim2dl.hip through the z-padded form (two all-+inf pad layers: z0 = 1, L = NL + 2): one side
    per layer; the pad layers of T stay +inf."""
    th = H3.layered_rows(f64)
    goal = H3.ring_goal(th, 1)
    cost = H3.ring_cost(th, nl, gaps, pad=True)
    R = H3.oracle_field(("ring", th, nl, gaps, True), cost, goal)
    T = solve(ctxs["persistent"], cost, goal, f64, layered=True)
    H3.check_field(T, R, goal, f64)
    assert np.all(np.isinf(T[:, :, 0])) and np.all(np.isinf(T[:, :, -1]))


# (option, value) lists by the names of eikonal._lib
SCHEDULES = {
    "passes1": [("OPT_PASSES", 1)],
    "passes2": [("OPT_PASSES", 2)],
    "passes24": [("OPT_PASSES", 24)],
    "prio0": [("OPT_PRIO", 0.0)],
    "prio0.05": [("OPT_PRIO", 0.05)],
    "prio1": [("OPT_PRIO", 1.0)],
    "volume_layout": [("OPT_LAYER_PLANAR", 0)],
    "sched0": [("OPT_SCHED", 0)],
    "sched3": [("OPT_SCHED", 3)],
}


@pytest.mark.parametrize("case", list(SCHEDULES))
@F64
def test_ring_schedules(case, f64):
    """fim2dl.hip (persistent): the four-gap ring volume (one gap per side, each in another layer:
    fp32 4 layers, fp64 3) under every pass cap, band width, the volume's own layout and the 2D
    in-place schedules: a different visit order, the same field.  A pass cap of 1 leaves no in-place
    pass."""
    th = H3.layered_rows(f64)
    nl, gaps = H3.four_gaps(f64)
    goal = H3.ring_goal(th)
    cost = H3.ring_cost(th, nl, gaps)
    R = H3.oracle_field(("ring", th, nl, gaps, False), cost, goal)
    c = _context("persistent", SCHEDULES[case])
    try:
        H3.check_field(solve(c, cost, goal, f64, layered=True), R, goal, f64)
        if case == "passes1":
            assert c.stats()["inplace_passes"] == 0
    finally:
        c.close()


# ---------------------------------------------------------------------------- C. z pinholes
@pytest.mark.parametrize("f64,nl,name,shape,pin", H3.PIN_CASES,
                         ids=[f"{'f64' if c[0] else 'f32'}-nl{c[1]}-{c[2]}" for c in H3.PIN_CASES])
def test_z_pinhole(ctxs, f64, nl, name, shape, pin):
    """fim2dl.hip (persistent; NL = 3 both dtypes, NL = 4 fp32) -- and fim3d.hip for NL = 4 in fp64:
    layers 0 and NL - 1 open, between them +inf but one z column, the goal in layer 0: layer NL - 1 is
    reachable only up that column, across the layer groups (fp32 {0, 1} | {2[, 3]}, fp64 one layer
    each).  Columns inside a tile, at its lane 0 / row 0, in its last row (fp64: rows 39 and 79) and
    in the cut last tile row / column."""
    cost = H3.pinhole_cost(shape, pin)
    R = H3.oracle_field(("pin", shape, pin), cost, H3.PIN_GOAL)
    assert np.isfinite(R[:, :, nl - 1]).all()
    layered = nl <= (H3.L64_MAX_LAYERS if f64 else H3.L32_MAX_LAYERS)
    H3.check_field(solve(ctxs["persistent"], cost, H3.PIN_GOAL, f64, layered), R, H3.PIN_GOAL, f64)


# -------------------------------------------------- D. general solver: cut volumes, corner goals
CUT_SHAPES = [(8, 16, 8), (7, 15, 7), (9, 17, 9), (17, 33, 17), (1, 1, 9), (1, 40, 9), (20, 1, 12), (9, 17, 5),
              (17, 17, 4)]


def cut_goals(shape):
    """The first and the last cell; where they exist, the last cell of the first tile and the first
    cell of the tile diagonal to it."""
    H, W, L = shape
    tx, ty, tz = H3.tile_shape3(L)
    goals = [(0, 0, 0), (W - 1, H - 1, L - 1)]
    goals += [g for g in ((tx - 1, ty - 1, tz - 1), (tx, ty, tz)) if g[0] < W and g[1] < H and g[2] < L]
    return list(dict.fromkeys(goals))


def cut_runs():
    out = []
    for shape in CUT_SHAPES:
        for goal in cut_goals(shape):
            for driver in DRIVERS:
                for f64 in (False, True):
                    if shape[2] <= 4 and driver == "persistent" and not f64:
                        continue  # 4 layers in persistent fp32: the layered solver's, not this one's
                    out.append((shape, goal, driver, f64))
    return out


@pytest.mark.parametrize("shape,goal,driver,f64", cut_runs(),
                         ids=lambda v: H3.flat_id(v) if not isinstance(v, bool) else ("f64" if v else "f32"))
def test_cut_volumes(ctxs, shape, goal, driver, f64):
    """fim3d.hip, both drivers: exactly one tile, a tile short on every axis, one cell past one / two
    tiles on every axis, a line, two sheets, 16 x 8 x 5 tiles and 16 x 16 x 4 tiles (list mode and
    fp64), goals in the volume's and the tiles' corners: the cells beyond the volume stage as +inf and
    are neither stored nor flagged."""
    cost = H3.cut_cost3(shape, goal)
    R = H3.oracle_field(("cut", shape, goal), cost, goal)
    H3.check_field(solve(ctxs[driver], cost, goal, f64, layered=False), R, goal, f64)


# ---------------------------------------------- E. general solver: pass cap and self re-queue
ONE_TILE = (8, 16, 8)


@pytest.mark.parametrize("passes", [1, 2, 64])
@pytest.mark.parametrize("driver", DRIVERS)
@F64
def test_pass_cap_one_tile(driver, passes, f64):
    """fim3d.hip: one open 16 x 8 x 8 tile, goal in a corner, under a pass cap of 1, 2 and 64.  At a
    cap of 1 the first visit's only pass lowers the goal's neighbours and ends with flag 128; a single
    tile has no neighbour to re-activate it, so only the self re-queue (list: enqueue3 on the tile;
    persistent: kPending | kSelf on its state word) brings the visits that finish the field.  On the
    persistent driver every visit then reports exactly one relaxation pass."""
    goal = (0, 0, 0)
    cost = np.ones(ONE_TILE)
    R = H3.oracle_field(("open", ONE_TILE), cost, goal)
    c = _context(driver, [("OPT_PASSES", passes)])
    try:
        H3.check_field(solve(c, cost, goal, f64, layered=False), R, goal, f64)
        s = c.stats()
        if passes == 1:
            assert s["tile_visits"] >= 2, s
            if driver == "persistent":
                assert s["inplace_passes"] == s["tile_visits"], s
    finally:
        c.close()


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("driver", DRIVERS)
@F64
def test_pass_cap_six_gaps(driver, passes, f64):
    """fim3d.hip: the six-gap shell volume at a pass cap of 1 and 2 -- face flags and the self
    re-queue (flag 128) raised by the same visits."""
    cost = H3.shell_cost(H3.SIX_GAPS)
    R = H3.oracle_field(("shell", H3.SIX_GAPS), cost, H3.SHELL_GOAL)
    c = _context(driver, [("OPT_PASSES", passes)])
    try:
        H3.check_field(solve(c, cost, H3.SHELL_GOAL, f64, layered=False), R, H3.SHELL_GOAL, f64)
    finally:
        c.close()


# ----------------------------------------------------------- the goal's own hand-off
# A write-back flags a side only for cells the visit lowered, and the goal is never lowered: the
# seeding has to hand a goal on a tile side to the neighbour across it.  (test_cut_volumes' goals in a
# cut tile one cell wide, (16, 8, 8) of 9 x 17 x 9, found this: nothing but the goal was reached.)
@pytest.mark.parametrize("face", H3.FACES)
@F64
def test_goal_lone_exit(ctx, face, f64):
    """fim3d.hip, both drivers: 2 x 2 x 2 tiles, the goal in a tile corner with every neighbour +inf
    but the one across the named face."""
    goal = H3.lone3_goal(face)
    cost = H3.lone_exit_cost(H3.LONE3_SHAPE, goal, face)
    R = H3.oracle_field(("lone", H3.LONE3_SHAPE, goal, face), cost, goal)
    assert H3.corners_finite(R)
    H3.check_field(solve(ctx, cost, goal, f64, layered=False), R, goal, f64)


@pytest.mark.parametrize("side", "NSWE")
@pytest.mark.parametrize("nl", [1, 3])
@F64
def test_goal_lone_exit_layered(ctxs, side, nl, f64):
    """fim2dl.hip (persistent): 2 x 2 tiles, the goal in a tile corner of layer 0, its z neighbour
    and every other neighbour +inf but the one across the named side."""
    th = H3.layered_rows(f64)
    shape, goal, face = H3.lone2_shape(th, nl), H3.lone2_goal(th, side), H3.LONE_SIDES[side]
    cost = H3.lone_exit_cost(shape, goal, face)
    R = H3.oracle_field(("lone", shape, goal, face), cost, goal)
    assert H3.corners_finite(R)
    H3.check_field(solve(ctxs["persistent"], cost, goal, f64, layered=True), R, goal, f64)


@F64
def test_goal_in_one_cell_tile_layered(ctxs, f64):
    """fim2dl.hip (persistent), one layer: the goal alone in the cut corner tile of a (TH + 1) x 65
    volume (it has no in-tile neighbour at all)."""
    th = H3.layered_rows(f64)
    cost, goal = np.ones((th + 1, H3.LCOLS + 1, 1)), (H3.LCOLS, th, 0)
    R = H3.oracle_field(("open", cost.shape, goal), cost, goal)
    T = ctxs["persistent"].tmap3d(cost, goal, dtype=dt(f64))
    H3.check_field(T, R, goal, f64)


_oracle2d = {}


def oracle_field2d(key, cost, goal):
    if key not in _oracle2d:
        O.set_strict(False)
        try:
            _oracle2d[key] = O.fmm2d(cost, goal)
        finally:
            O.set_strict(True)
    return _oracle2d[key]


@pytest.mark.parametrize("case", ["N", "S", "W", "E", "one_cell_tile"])
@F64
def test_goal_lone_exit_2d(ctx, case, f64):
    """fim2d.hip, both drivers (the same seeding, the same write-back rule): 128 x 128 with the goal in
    a tile corner and one open neighbour across the named side, and 65 x 65 with the goal alone in
    the cut corner tile.  Tolerances of tests/test_gpu_writeback.py."""
    if case == "one_cell_tile":
        cost, goal = np.ones((65, 65)), (64, 64)
    else:
        g3 = H3.lone2_goal(H3.LCOLS, case)
        cost, goal = H3.lone_exit_cost(H3.lone2_shape(H3.LCOLS, 1), g3, H3.LONE_SIDES[case])[:, :, 0], g3[:2]
    R = oracle_field2d(case, cost, goal)
    assert np.isfinite(R[0, 0]) and np.isfinite(R[-1, -1])
    T = ctx.tmap2d(cost, goal, dtype=dt(f64))
    H3.check_field(T[:, :, None], R[:, :, None], goal + (0,), f64)


# ------------------------------------- F. general solver: batch, NaN, budget, pruned solve
BATCH_SHAPE = (17, 33, 9)
BOXED = 2  # the volume of the batch whose goal sits in a closed +inf box


def batch_case():
    goals = cut_goals(BATCH_SHAPE)
    assert len(goals) == 4
    goals = [goals[b % 4] for b in range(6)]
    costs = np.stack([H3.cut_cost3(BATCH_SHAPE, g, salt=b + 1) for b, g in enumerate(goals)])
    gx, gy, gz = goals[BOXED]  # (15, 7, 7): the box spans the 8 tiles that meet at (16, 8, 8)
    H, W, L = BATCH_SHAPE
    y, x, z = np.ogrid[:H, :W, :L]
    d = np.maximum(np.maximum(abs(x - gx), abs(y - gy)), abs(z - gz))
    c = costs[BOXED]
    c[d <= 1] = np.where(np.isinf(c[d <= 1]), 2.0, c[d <= 1])
    c[d == 2] = np.inf
    c[gy, gx, gz] = 1.0
    return costs, goals, d <= 1


def test_batch(ctx):
    """fim3d.hip (every batch), both drivers, fp64: 6 volumes of 17 x 33 x 9 with their own costs and
    corner goals share the tile lists / the FIFO; one volume's goal is boxed in, and its field
    outside the box stays +inf while the others solve (no activation crosses to another volume's
    tiles)."""
    costs, goals, inside = batch_case()
    T = ctx.tmap3d_batch(costs, goals)
    assert ctx.stats()["fresh_visits"] == 0
    for b, g in enumerate(goals):
        R = H3.oracle_field(("batch6", b), costs[b], g)
        H3.check_field(T[b], R, g, True)
    assert np.all(np.isinf(T[BOXED][~inside])) and np.isfinite(T[BOXED][inside]).all()


def test_batch_of_one(ctx):
    """fim3d.hip: a batch of one 17 x 33 x 9 volume."""
    g = (16, 8, 8)
    cost = H3.cut_cost3(BATCH_SHAPE, g)
    R = H3.oracle_field(("cut", BATCH_SHAPE, g), cost, g)
    H3.check_field(ctx.tmap3d_batch(cost[None], [g])[0], R, g, True)


def test_batch_seed_spans_blocks(ctx):
    """fim3d.hip: 300 volumes of 3 x 3 x 5 (one tile each): the seed kernels run 256 volumes per
    block, so the last 44 goals are seeded by a second block."""
    B, shape = 300, (3, 3, 5)
    rng = np.random.default_rng(300)
    costs = rng.uniform(1, 10, (B,) + shape)
    costs[rng.random(costs.shape) < 0.05] = np.inf
    costs = costs.astype(np.float32).astype(np.float64)
    goals = np.stack([rng.integers(0, 3, B), rng.integers(0, 3, B), rng.integers(0, 5, B)], axis=1)
    for b, (gx, gy, gz) in enumerate(goals):
        costs[b, gy, gx, gz] = 1.0
    T = ctx.tmap3d_batch(costs, goals)
    for b in range(B):
        R = H3.oracle_field(("batch300", b), costs[b], goals[b])
        H3.check_field(T[b], R, goals[b], True)


def nan_case():
    shape = (40, 44, 12)
    rng = np.random.default_rng(4044)
    c = rng.uniform(1, 4, shape)
    c[rng.random(shape) < 0.08] = np.inf
    goal = (30, 5, 6)
    c[goal[1], goal[0], goal[2]] = 1.0
    cn = c.copy()
    cn[18:22, 6:, :] = np.nan  # a wall across the volume in every layer, open at columns 0..5
    return cn, goal


@F64
def test_nan_cost_blocks(ctx, f64):
    """fim3d.hip (L = 12) on the device-buffer entry (no host cost check), both drivers: a NaN cost is
    a blocked cell -- neither lowered itself nor a source for its neighbours.  Field = the oracle's
    with those cells at +inf."""
    import torch
    from eikonal import _lib as L

    cn, goal = nan_case()
    dev = torch.device("cuda", 0)
    cd = torch.from_numpy(cn.astype(dt(f64))).to(dev)
    Td = torch.empty_like(cd)
    H, W, Lz = cn.shape
    ctx._chk(L.lib().eik_fim3d_solve(ctx._h, cd.data_ptr(), Td.data_ptr(), H, W, Lz, L.EIK_F64 if f64 else L.EIK_F32,
                                     np.ascontiguousarray(goal, np.int64), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert ctx.stats()["fresh_visits"] == 0
    T = Td.cpu().numpy()
    R = H3.oracle_field("nan", np.where(np.isnan(cn), np.inf, cn), goal)
    assert np.isfinite(R[-1, -1, :]).any()  # the far side is reached round the wall
    assert np.all(np.isinf(T[np.isnan(cn)]))
    H3.check_field(T, R, goal, f64)


@F64
def test_visit_budget(f64):
    """fim3d.hip, persistent driver, ONE workgroup (EIK_OPT_GRID 1) and EIK_OPT_MAX_VISITS 64: a
    64 x 64 x 40 volume has 4 x 8 x 5 = 160 tiles, so the workgroup makes at least 160 visits, charges
    its first 64 and the solve ends with EIK_ERR_NOCONVERGE.  The grid of 1 is the point: a workgroup
    charges the budget only every 64 visits of its own, so with the default grid no workgroup of a
    160-tile volume ever charges.  With the budget back at its default the same context solves the
    volume: a failed solve leaves it usable."""
    from eikonal import _lib as L
    from eikonal import EikError

    shape = (64, 64, 40)
    rng = np.random.default_rng(646440)
    cost = rng.uniform(1, 4, shape).astype(np.float32).astype(np.float64)
    goal = (31, 33, 17)
    R = H3.oracle_field("budget", cost, goal)
    c = _context("persistent", [("OPT_GRID", 1), ("OPT_MAX_VISITS", 64)])
    try:
        with pytest.raises(EikError) as e:
            c.tmap3d(cost, goal, dtype=dt(f64))
        assert e.value.code == L.EIK_ERR_NOCONVERGE
        c.set_option(L.OPT_MAX_VISITS, 0)
        H3.check_field(solve(c, cost, goal, f64, layered=False), R, goal, f64)
        assert c.stats()["tile_visits"] >= 160
    finally:
        c.close()


PRUNE_GAP = (("x+", "centre"),)
PRUNE_STARTS = [(27, 12, 12), (32, 12, 12), (0, 0, 0)]  # 3 steps from the goal, just outside the gap, far


def prune_cost():
    """The x+ single-gap shell volume with cut_cost values (no exact ties) in the open cells; the
    goal, the gap, the starts and the goal-to-gap line are kept open."""
    rng = np.random.default_rng(31)
    u = rng.uniform(1, 10, H3.SHELL_SHAPE)
    fill = np.where(rng.random(H3.SHELL_SHAPE) < 0.05, np.inf, u).astype(np.float32).astype(np.float64)
    u = u.astype(np.float32).astype(np.float64)
    fill[12, 24:33, 12] = u[12, 24:33, 12]
    fill[0, 0, 0] = u[0, 0, 0]
    return H3.shell_cost(PRUNE_GAP, fill)


@pytest.mark.parametrize("start", PRUNE_STARTS, ids=lambda s: "-".join(map(str, s)))
def test_pruned_early_exit(ctx, start):
    """fim3d.hip (every fp64 solve with a `start`), both drivers: the solve only lowers cells up to
    (T[start] + max cost) x 1.000001 (early_bound), here with the bound inside the walled-in tile,
    just past its only gap, and at the far corner.  The result equals the early-exit restatement
    applied to the GPU's own full field (test_early_exit_kernel_restatement's criterion)."""
    cost = prune_cost()
    Tf = ctx.tmap3d(cost, H3.SHELL_GOAL)
    assert np.isfinite(Tf[start[1], start[0], start[2]])
    H3.check_field(Tf, H3.oracle_field("prune", cost, H3.SHELL_GOAL), H3.SHELL_GOAL, True)
    T = ctx.tmap3d(cost, H3.SHELL_GOAL, start=start)
    E = O.fm3d_early_from_full(cost, Tf, H3.SHELL_GOAL, start)
    fin = np.isfinite(E)
    assert np.array_equal(np.isfinite(T), fin)
    assert np.all(np.abs(T[fin] - E[fin]) <= 1e-12 * np.maximum(1.0, E[fin]))
