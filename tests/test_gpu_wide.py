"""Solver paths that the raster's size alone selects, at sizes where the oracle is cheap.

* The 4-waves-per-SIMD form of the fp32 persistent kernel (fim2d_persist_kernel<float, 4>, by
  default only on maps of >= 16384 tiles) forced with EIK_OPT_WIDE = 1 and run over the suite's small
  hostile rasters: the golden fields, test_gpu_fim2d.py's oracle shapes, test_gpu_writeback.py's
  hand-off / cut-tile / schedule matrix, C4's own schedule (bands, 128-entry dispatches, 16
  passes), a batch, decomposition blocks with ghost strips (the relaunch schedule; the multi-process
  live schedule of test_gpu_dd_live.py is out of scope here) and the visit budget.  Tolerances are
  the suite's: masks identical, T[goal] == 0, <= 2e-5 relative to O.fmm2d (non-strict).
* The size gates themselves, with no switch: what a 1048576 x 3 raster (16384 tiles) takes in fp32
  and in fp64, the pass-cap defaults, and the fp64 band gate on a 1030 x 16300 raster with obstacles.
* Priority bands shared by two maps (biComputeTmap's two fronts and a B = 2 batch), forced with
  EIK_OPT_PRIO at sizes below the 4096^2 where they are the default.

Every solve asserts through Context.last_form() that it took the form it was meant to take.  The
cases and their checks are those of the files named above, imported, not restated.
"""
import numpy as np
import pytest

import test_gpu_bidir_exact as E
import test_gpu_bidir_join as J
import test_gpu_dd as D
import test_gpu_fim2d as F
import test_gpu_fullsize as FS
import test_gpu_path as P
import test_gpu_writeback as W

pytestmark = pytest.mark.gpu


class FormChecked:
    """A Context whose solves each assert the entries `want` of last_form() (fp64 tmap2d calls
    pass unchecked: EIK_OPT_WIDE is fp32's)."""

    def __init__(self, ctx, want):
        self.ctx, self.want = ctx, want

    def _check(self):
        form = self.ctx.last_form()
        assert {k: form[k] for k in self.want} == self.want, form

    def tmap2d(self, cost, goal, dtype=np.float64):
        T = self.ctx.tmap2d(cost, goal, dtype=dtype)
        if np.dtype(dtype) == np.float32:
            self._check()
        return T

    def tmap2d_batch(self, costs, goals):
        T = self.ctx.tmap2d_batch(costs, goals)
        self._check()
        return T

    def tmap2d_bidir(self, cost, goal, start):
        out = self.ctx.tmap2d_bidir(cost, goal, start)
        self._check()
        return out

    def __getattr__(self, name):
        return getattr(self.ctx, name)


def _context(options):
    import eikonal
    from eikonal import _lib as L

    return eikonal.Context(0, options=dict(options, MODE=L.MODE_PERSISTENT))


@pytest.fixture(scope="module")
def wide():
    c = _context({"WIDE": 1})
    yield FormChecked(c, {"wide": 1})
    c.close()


# ----------------------------------------------------- B. the wide form against the oracle
@pytest.mark.parametrize("i", range(13))
def test_wide_golden_fields(wide, golden, i):
    F.test_golden_fields(wide, golden, i, False)


@pytest.mark.parametrize("name", ["uniform", "random"])
def test_wide_c1_config(wide, golden, name):
    F.test_c1_config(wide, golden, name, False)


@pytest.mark.parametrize("shape,kind,seed", [((517, 1031), "obst", 1), ((1024, 1024), "random", 2),
                                             ((300, 70), "maze", 3), ((64, 64), "random", 4),
                                             ((1, 200), "random", 5), ((37, 1), "random", 6)])
def test_wide_vs_oracle(wide, shape, kind, seed):
    c, goal = F.vs_oracle_case(shape, kind, seed)
    F.check_field(wide.tmap2d(c, goal, dtype=np.float32), F.oracle_field(c, goal), goal, False)


def test_wide_enclosed_goal_and_unreachable(wide):
    F.test_enclosed_goal_and_unreachable(wide)


def test_wide_non_inf_border(wide):
    F.test_non_inf_border_matches_oob_as_inf(wide)


@pytest.mark.parametrize("gaps", W.HANDOFFS, ids=lambda g: "+".join(f"{s}{l}" for s, l in g))
def test_wide_single_cell_handoff(wide, gaps):
    W.test_single_cell_handoff(wide, gaps, False)


@pytest.mark.parametrize("shape,goal", W.cut_cases(), ids=lambda v: "x".join(map(str, v)))
def test_wide_cut_tiles(wide, shape, goal):
    W.test_cut_tiles(wide, shape, goal, False)


@pytest.mark.parametrize("case", ["passes1", "passes40", "sched0", "sched1", "sched3"])
def test_wide_inplace_passes_and_deferral(case):
    """The fp32 members of test_gpu_writeback.py's SCHEDULES on the four-gap raster (ordered_list is
    list mode: no persistent kernel, so no form)."""
    options, dtypes = W.SCHEDULES[case]
    assert False in dtypes
    cost = W.ring_cost(W.FOUR_GAPS)
    R = W.oracle_field(("ring", W.FOUR_GAPS), cost, W.GOAL)
    c = _context({"WIDE": 1, **{k[4:]: v for k, v in options}})
    try:
        T = c.tmap2d(cost, W.GOAL, dtype=np.float32)
        form = c.last_form()
    finally:
        c.close()
    assert form["wide"] == 1 and form["bands"] == 0, form
    if case.startswith("passes"):
        assert form["passes"] == int(case[6:]), form
    W.check_field(T, R, W.GOAL, False)


_sched = {}


def _schedule_case():
    if not _sched:
        cost, goal = F.schedule_raster(np.random.default_rng(12))
        R = F.oracle_field(cost, goal)
        R.setflags(write=False)
        _sched["case"] = (cost, goal, R)
    return _sched["case"]


@pytest.mark.parametrize("prio", [0.1, 1])
@pytest.mark.parametrize("ring", [0, 8])
@pytest.mark.parametrize("grid", [0, 8])
def test_wide_c4_schedule(prio, ring, grid):
    """What a 16384^2 fp32 solve runs -- the wide form, priority bands, 128-entry dispatches, 16
    passes -- on test_schedule_options' 640 x 770 raster with 15 % obstacles.  ring = 8: bands of 8
    slots for 110 tiles; a band that fills stops the launch and the solve runs again on the FIFO,
    still on the wide form, without an error (a ring that happened not to fill keeps the bands).
    grid = 8: eight workgroups instead of every co-resident one -- a push goes to the bands only
    while no workgroup waits for a tile (fim_engine.hpp qgrab_prio), which at 110 tiles and a full
    grid is rare; with eight the tiles queue in the bands as they do at full size.  (Observed: ring 8
    fills at grid 8 at both widths, the solve ending on the FIFO, and never at the full grid.)"""
    cost, goal, R = _schedule_case()
    c = _context({"WIDE": 1, "PRIO": prio, "PRIO_DISPATCH": 128, "PASSES": 16, "PRIO_RING": ring, "GRID": grid,
                  "QTIMEOUT": 5})
    try:
        T = c.tmap2d(cost, goal, dtype=np.float32)
        form = c.last_form()
        T2 = c.tmap2d(cost, goal, dtype=np.float32)  # the same solver again (after an overflow: FIFO from the start)
        form2 = c.last_form()
    finally:
        c.close()
    print(f"prio {prio} ring {ring} grid {grid}: {form} then {form2}")
    want = {"wide": 1, "bands": 1, "passes": 16, "dispatch": 128}
    if ring == 0:
        assert form == want and form2 == want, (form, form2)
    else:
        fifo = {"wide": 1, "bands": 0, "passes": 16, "dispatch": 0}
        assert form in (want, fifo) and form2 in (want, fifo), (form, form2)
        assert form2 == fifo or form == want, (form, form2)  # a solver that fell back keeps the FIFO
    F.check_field(T, R, goal, False)
    F.check_field(T2, R, goal, False)


def test_wide_batch_matches_single(wide):
    F.test_batch_matches_single(wide)
    assert wide.last_form()["passes"] == 2


def test_wide_dd_block_with_ghosts():
    form = W.dd_block_with_ghosts("persistent", False, options={"WIDE": 1})
    assert form["wide"] == 1, form


@pytest.mark.parametrize("px,py", [(2, 1), (2, 2)])
def test_wide_dd_blocks_match_single_domain(px, py):
    from eikonal import _lib as L

    cost, goal = D.dd_case(px, py, False)
    forms = []
    T, rounds = D.solve_blocks(cost, goal, px, py, False, L.MODE_PERSISTENT, options={"WIDE": 1}, forms=forms)
    assert len(forms) == px * py and all(f["wide"] == 1 for f in forms), forms
    R = D.oracle_field(cost, goal)
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin)
    assert (np.abs(T[fin] - R[fin]) / np.maximum(R[fin], 1e-30)).max() <= 2e-5
    assert rounds >= 2


def test_wide_visit_budget_device_buffers():
    """EIK_OPT_MAX_VISITS = 128 on the wide form: EIK_ERR_NOCONVERGE, and the context and the solver
    solve the same raster correctly afterwards."""
    import torch
    import eikonal
    from eikonal import _lib as L

    cost, goal = F.visit_budget_raster(False)
    c = _context({"WIDE": 1, "MAX_VISITS": 128})
    try:
        dev = torch.device("cuda", 0)
        cd = torch.from_numpy(cost).to(dev)
        Td = torch.empty_like(cd)
        f = L.Fim2d(c, 1, 1024, 1024, L.EIK_F32)
        try:
            with pytest.raises(eikonal.EikError) as ei:
                f.solve(cd.data_ptr(), Td.data_ptr(), goal, torch.cuda.current_stream(dev).cuda_stream)
            assert ei.value.code == L.EIK_ERR_NOCONVERGE
            assert c.last_form()["wide"] == 1
            c.set_option(L.OPT_MAX_VISITS, 0)
            f.solve(cd.data_ptr(), Td.data_ptr(), goal, torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
            assert c.last_form()["wide"] == 1
            F.check_field(Td.cpu().numpy(), F.oracle_field(cost, goal[0]), goal[0], False)
        finally:
            f.close()
    finally:
        c.close()


def test_wide_switch_both_ways_on_one_solver():
    """EIK_OPT_WIDE changed between two solves of the same cached solver: each launch takes the form
    asked for (the co-resident workgroup count is kept per form), 0 forces the narrow form, < 0 gives
    the choice back to the size."""
    from eikonal import _lib as L

    cost, goal, R = _schedule_case()
    c = _context({})
    try:
        for v, want in ((1, 1), (0, 0), (1, 1), (-1, 0)):
            c.set_option(L.OPT_WIDE, v)
            T = c.tmap2d(cost, goal, dtype=np.float32)
            assert c.last_form() == {"wide": want, "bands": 0, "passes": 40, "dispatch": 0}
            F.check_field(T, R, goal, False)
    finally:
        c.close()


# ----------------------------------------------------------------------- C. the size gates
THIN = (1048576, 3)  # 16384 tiles of 64 x 3 cells, 3.1 M cells


def _thin_cost():
    rng = np.random.default_rng(16384)
    return rng.uniform(1, 10, THIN).astype(np.float32)  # no obstacles: one blocks a 3-wide raster at once


def test_gate_fp32_thin_raster():
    """16384 tiles select the wide form, the bands, 16 passes and 128-entry dispatches by default.
    The field is checked by its local properties (test_gpu_fullsize.py check_properties: residual of
    the reference's local solve <= 2e-5, descent, closure), not against the fp64 oracle: T is carried
    along a path of ~5e5 cells here, over which fp32 rounding alone adds up to the order of 2e-5."""
    import torch

    cost = _thin_cost()
    goal = (1, THIN[0] // 2)
    c = _context({})
    try:
        T = c.tmap2d(cost, goal, dtype=np.float32)
        form = c.last_form()
    finally:
        c.close()
    assert form == {"wide": 1, "bands": 1, "passes": 16, "dispatch": 128}, form
    assert np.isfinite(T).all()
    dev = torch.device("cuda", 0)
    worst = FS.check_properties(torch, torch.from_numpy(T).to(dev), torch.from_numpy(cost).to(dev), goal, rows=32768)
    print(f"thin fp32 raster: worst local residual {worst:.3g}")


def test_gate_fp64_thin_raster():
    """fp64 has the one form, and below a side of sqrt(H W) = 1774 < 4096 the FIFO.  (This strip and
    the fp32 one take 1590 / 2350 visits + in-place passes per tile: a default visit budget of a flat
    1024 per tile reported both as EIK_ERR_NOCONVERGE; it grows with the raster's elongation now.)"""
    cost = _thin_cost().astype(np.float64)
    goal = (1, THIN[0] // 2)
    c = _context({})
    try:
        T = c.tmap2d(cost, goal, dtype=np.float64)
        form = c.last_form()
    finally:
        c.close()
    assert form == {"wide": 0, "bands": 0, "passes": 40, "dispatch": 0}, form
    assert T[goal[1], goal[0]] == 0 and np.isfinite(T).all()


def test_gate_pass_cap_defaults():
    c = _context({})
    try:
        c.tmap2d(np.ones((512, 512), np.float32), (256, 256), dtype=np.float32)
        assert c.last_form() == {"wide": 0, "bands": 0, "passes": 40, "dispatch": 0}
        c.tmap2d_batch(np.ones((6, 100, 130), np.float32), np.full((6, 2), 50, np.int64))
        assert c.last_form() == {"wide": 0, "bands": 0, "passes": 2, "dispatch": 0}
    finally:
        c.close()


def test_gate_fp64_default_bands_hostile_raster():
    """1030 x 16300 = 16.79 M cells >= 4096^2, both sides ragged, 15 % obstacles: the fp64 default is
    the priority bands with 16-entry dispatches (4335 tiles).  The field against the oracle at
    test_priority_bands_fp64's bound, |T - R| <= max(1e-9, 1e-13 R)."""
    H, W = 1030, 16300
    rng = np.random.default_rng(1030)
    cost = rng.uniform(1, 10, (H, W))
    cost[rng.random((H, W)) < 0.15] = np.inf
    cost = cost.astype(np.float32).astype(np.float64)
    goal = (W // 3, H // 2)
    cost[goal[1], goal[0]] = 1.0
    c = _context({})
    try:
        T = c.tmap2d(cost, goal, dtype=np.float64)
        form = c.last_form()
    finally:
        c.close()
    assert form["bands"] == 1 and form["dispatch"] == 16 and form["wide"] == 0, form
    R = F.oracle_field(cost, goal)
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin) and T[goal[1], goal[0]] == 0
    e = np.abs(T[fin] - R[fin])
    print(f"fp64 default bands: {fin.mean():.2f} reached, T up to {R[fin].max():.3g}, max abs err {e.max():.3g}")
    assert (e <= np.maximum(1e-9, 1e-13 * R[fin])).all(), (e.max(), (e / np.maximum(R[fin], 1)).max())


# ------------------------------------------------------------- D. bands over two maps
# (prio, grid); grid = 8: few workgroups, so that the tiles wait in the bands (test_wide_c4_schedule)
@pytest.fixture(scope="module", params=[(0.25, 0), (0.02, 0), (0.25, 8)], ids=lambda p: f"prio{p[0]}-grid{p[1]}")
def exact_bands(request):
    prio, grid = request.param
    c = _context({"EXACT_BAND": 1, "PRIO": prio, "GRID": grid})
    yield FormChecked(c, {"bands": 1})
    c.close()


@pytest.mark.parametrize("i", range(6))
def test_bands_exact_vs_reference(exact_bands, golden, i):
    E.test_bidirectional_exact_vs_reference(exact_bands, golden, i)


@pytest.mark.parametrize("kind,H,W,seed", [("random", 97, 131, 1), ("obst", 257, 190, 4), ("integer", 200, 160, 16),
                                           ("plateaus", 300, 280, 12)])
def test_bands_exact_vs_oracle(exact_bands, kind, H, W, seed):
    E.test_bidirectional_exact_vs_oracle(exact_bands, kind, H, W, seed)


def test_bands_exact_capped_fronts(exact_bands):
    E.test_bidirectional_exact_capped_fronts(exact_bands)


@pytest.fixture(scope="module")
def bands():
    c = _context({"PRIO": 0.25})
    yield FormChecked(c, {"bands": 1})
    c.close()


@pytest.fixture(scope="module")
def full_fronts():
    import eikonal

    c = eikonal.Context(0, options="FRONTS_CAP=0")
    yield c
    c.close()


@pytest.mark.parametrize("i", range(6))
def test_bands_bidirectional(bands, golden, i):
    P.test_bidirectional(bands, golden, i)


@pytest.mark.parametrize("kind,goal,start", J.FRONT_CASES, ids=[c[0] for c in J.FRONT_CASES])
def test_bands_capped_fronts_equal_full_fronts(bands, full_fronts, kind, goal, start):
    J.test_capped_fronts_equal_full_fronts(bands, full_fronts, kind, goal, start)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("grid", [0, 4])
def test_bands_two_map_batch(swap, grid):
    """B = 2 maps on one set of bands whose width is sampled from map 0 only: the second map is the
    first x 1e4, so with map 0 at U(1, 8) every key of map 1 lands in the open-ended last band, and
    the other way round map 1's keys all fall into band 0.  grid = 4: four workgroups, so that the
    70 tiles wait in the bands (test_wide_c4_schedule)."""
    rng = np.random.default_rng(300420)
    H, Wd = 300, 420
    base = rng.uniform(1, 8, (H, Wd)).astype(np.float32)
    base[rng.random((H, Wd)) < 0.1] = np.inf
    goals = np.array([[60, 50], [350, 260]], np.int64)
    for g in goals:
        base[g[1], g[0]] = 1.0
    costs = np.stack([base, base * np.float32(1e4)])
    if swap:
        costs = np.ascontiguousarray(costs[::-1])
    c = _context({"PRIO": 1, "GRID": grid})
    try:
        T = c.tmap2d_batch(costs, goals)
        form = c.last_form()
    finally:
        c.close()
    assert form["bands"] == 1 and form["wide"] == 0, form
    for b in range(2):
        F.check_field(T[b], F.oracle_field(costs[b], goals[b]), goals[b], False)
