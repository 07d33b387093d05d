"""The tile visit's write-back (fim2d.hip process_tile): which cells are stored, which sides are
flagged for activation, the entering keys and the subdomain edge bits -- on rasters built so that a
lost store or a lost flag shows in the field.

Everything is checked against the oracle (O.fmm2d, non-strict) with test_gpu_fim2d.py's tolerances:
masks identical, T[goal] == 0, fp64 <= 1e-9 absolute, fp32 <= 2e-5 relative; on both solver drivers
and in both dtypes unless a case says otherwise.
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

RTOL32 = 2e-5
ATOL64 = 1e-9
TILE = 64


@pytest.fixture(scope="module", params=["persistent", "list"])
def ctx(request):
    import eikonal
    from eikonal import _lib as L

    c = eikonal.Context(0)
    c.set_option(L.OPT_MODE, L.MODE_PERSISTENT if request.param == "persistent" else L.MODE_LIST)
    yield c
    c.close()


_oracle_cache = {}


def oracle_field(key, cost, goal):
    """The oracle's field of (cost, goal), computed once per key and shared read-only."""
    if key not in _oracle_cache:
        O.set_strict(False)
        try:
            R = O.fmm2d(np.asarray(cost, np.float64), goal)
        finally:
            O.set_strict(True)
        R.setflags(write=False)
        _oracle_cache[key] = R
    return _oracle_cache[key]


def check_field(T, R, goal, f64):
    assert T.shape == R.shape
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    assert T[goal[1], goal[0]] == 0
    err = np.abs(T[fin].astype(np.float64) - R[fin])
    if f64:
        assert err.max() <= ATOL64, err.max()
    else:
        rel = err / np.maximum(np.abs(R[fin]), 1e-30)
        rel[R[fin] == 0] = err[R[fin] == 0]
        assert rel.max() <= RTOL32, rel.max()


# ------------------------------------------------------------------ single-cell hand-offs
# 192 x 192, unit cost, goal in the centre tile, whose own border ring (rows and columns 64 and
# 127) is +inf except the gap cells: the eight outer tiles are reachable only through an edge flag
# raised by a gap cell (lanes 0 and 63 of a side are the ring's corners, on two sides at once; see
# ring_cost for how a corner is reached).
GOAL = (96, 96)


def gap_cell(side, lane):
    lo, hi = TILE, 2 * TILE - 1
    return {"N": (lo, lo + lane), "S": (hi, lo + lane), "W": (lo + lane, lo), "E": (lo + lane, hi)}[side]  # (row, col)


def ring_cost(gaps):
    c = np.ones((3 * TILE, 3 * TILE))
    lo, hi = TILE, 2 * TILE - 1
    c[lo, lo:hi + 1] = c[hi, lo:hi + 1] = c[lo:hi + 1, lo] = c[lo:hi + 1, hi] = np.inf
    for side, lane in gaps:
        r, q = gap_cell(side, lane)
        c[r, q] = 1.0
        if lane in (0, TILE - 1):
            # a corner's two neighbours inside the tile are ring cells (the stencil is 4-connected):
            # the one on the adjoining side is opened too, so that on the named side the corner
            # lane alone raises the flag
            if side in "NS":
                c[r + (1 if side == "N" else -1), q] = 1.0
            else:
                c[r, q + (1 if side == "W" else -1)] = 1.0
    return c


FOUR_GAPS = (("N", 31), ("S", 31), ("W", 31), ("E", 31))
HANDOFFS = [((s, l),) for s in "NSWE" for l in (0, 31, 63)] + [FOUR_GAPS]


@pytest.mark.parametrize("gaps", HANDOFFS, ids=lambda g: "+".join(f"{s}{l}" for s, l in g))
@pytest.mark.parametrize("f64", [False, True])
def test_single_cell_handoff(ctx, gaps, f64):
    cost = ring_cost(gaps)
    R = oracle_field(("ring", gaps), cost, GOAL)
    assert np.isfinite(R[0, 0]) and np.isfinite(R[-1, -1]) and np.isfinite(R[0, -1]) and np.isfinite(R[-1, 0])
    T = ctx.tmap2d(cost, GOAL, dtype=np.float64 if f64 else np.float32)
    check_field(T, R, GOAL, f64)


# ------------------------------------------------------------------------------ cut tiles
def cut_cost(shape, goal):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    c = rng.uniform(1, 10, shape)
    c[rng.random(shape) < 0.05] = np.inf
    c = c.astype(np.float32).astype(np.float64)
    c[goal[1], goal[0]] = 1.0
    return c


def cut_cases():
    out = []
    for H, W in [(130, 67), (67, 130), (128, 128), (64, 64)]:
        goals = [(0, 0), (W - 1, H - 1), (63, 63)]
        if H > 64 and W > 64:
            goals.append((64, 64))
        out += [((H, W), g) for g in dict.fromkeys(goals)]  # (64^2: its last cell is (63, 63))
    return out


@pytest.mark.parametrize("shape,goal", cut_cases(), ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("f64", [False, True])
def test_cut_tiles(ctx, shape, goal, f64):
    """W & 3 != 0 takes the per-cell store path; the partial last tile row / column keeps ghost
    cells out of the changed set; 128^2 is a full 2 x 2 and 64^2 one tile with every side a border."""
    cost = cut_cost(shape, goal)
    R = oracle_field(("cut", shape, goal), cost, goal)
    T = ctx.tmap2d(cost, goal, dtype=np.float64 if f64 else np.float32)
    check_field(T, R, goal, f64)


# ---------------------------------------------------------------- in-place passes and deferral
def _solve_with(options, cost, goal, f64):
    import eikonal
    from eikonal import _lib as L

    c = eikonal.Context(0)
    try:
        for k, v in options:
            c.set_option(getattr(L, k), getattr(L, v) if isinstance(v, str) else v)
        return c.tmap2d(cost, goal, dtype=np.float64 if f64 else np.float32)
    finally:
        c.close()


# (option name, value) lists by the names of eikonal._lib, and the dtypes each runs in
SCHEDULES = {
    "passes1": ([("OPT_PASSES", 1)], (False, True)),
    "passes40": ([("OPT_PASSES", 40)], (False, True)),
    "sched0": ([("OPT_SCHED", 0)], (False, True)),
    "sched1": ([("OPT_SCHED", 1)], (False, True)),
    "sched3": ([("OPT_SCHED", 3)], (False, True)),
    "prio": ([("OPT_PRIO", 0.25)], (True,)),  # priority bands forced on: the entering keys, fp64
    "ordered_list": ([("OPT_MODE", "MODE_LIST"), ("OPT_DELTA", 16.0)], (False, True)),  # the keys in list mode
}


@pytest.mark.parametrize("case,f64", [(k, f) for k, (_, fs) in SCHEDULES.items() for f in fs])
def test_inplace_passes_and_deferral(case, f64):
    """The four-gap raster under every in-place / deferral schedule of the persistent driver (and the
    ordered list mode, the other user of the keys): the same field within tolerance."""
    cost = ring_cost(FOUR_GAPS)
    R = oracle_field(("ring", FOUR_GAPS), cost, GOAL)
    check_field(_solve_with(SCHEDULES[case][0], cost, GOAL, f64), R, GOAL, f64)


# ------------------------------------------------------------------ domain-decomposition bits
@pytest.mark.parametrize("mode", ["persistent", "list"])
@pytest.mark.parametrize("f64", [False, True])
def test_dd_block_with_ghosts(mode, f64):
    """A 96 x 96 block (cut tiles on S and E, where the subdomain's edge row / column lies inside a
    tile) with +inf ghost strips bound on all four sides, through the relaunch API of a
    decomposition block (eikonal.dd.GpuLocal, world 1): its field equals the oracle's and the edges
    it packs are its last row / column.  (The per-side "edge changed" word the write-back's bits 32 /
    64 feed has no reader in the C ABI or the Python API, so it is exercised here -- the ghosts bind
    it -- but not read; tests/test_gpu_dd_live.py covers its effect at larger size.)"""
    dd_block_with_ghosts(mode, f64)


def dd_block_with_ghosts(mode, f64, options=None):
    """test_dd_block_with_ghosts' body; options: further Context options -> the context's last_form()."""
    import eikonal
    import torch
    from eikonal import _lib as L
    from eikonal import dd

    H = W = 96
    goal = (10, 20)
    cost = cut_cost((H, W), goal)
    R = oracle_field(("cut", (H, W), goal), cost, goal)
    dev = torch.device("cuda", 0)
    dt = torch.float64 if f64 else torch.float32
    ctx = eikonal.Context(0, options=options)
    try:
        ctx.set_option(L.OPT_MODE, L.MODE_PERSISTENT if mode == "persistent" else L.MODE_LIST)
        ctx.set_option(L.OPT_QTIMEOUT, 5.0)
        c = torch.from_numpy(cost).to(dev, dt)
        T = torch.empty_like(c)
        ghosts = [torch.full((n,), float("inf"), dtype=dt, device=dev) for n in (W, W, H, H)]
        send = [torch.full((n,), -1.0, dtype=dt, device=dev) for n in (W, W, H, H)]
        fim = eikonal.Fim2d(ctx, 1, H, W, L.EIK_F64 if f64 else L.EIK_F32)
        loc = dd.GpuLocal(fim, ghosts)
        loc.start(c, T, goal, torch.cuda.current_stream(dev).cuda_stream)
        for _ in range(1000):
            loc.iterate(4)
            if loc.active() == 0:
                break
        else:
            raise AssertionError("block did not converge")
        loc.pack_edges(*send)
        torch.cuda.synchronize()
        Tg = T.cpu().numpy()
        edges = [s.cpu().numpy() for s in send]
        form = ctx.last_form()
        fim.close()
    finally:
        ctx.close()
    check_field(Tg, R, goal, f64)
    for got, want in zip(edges, (Tg[0, :], Tg[-1, :], Tg[:, 0], Tg[:, -1])):
        assert np.array_equal(got, want)
    return form
