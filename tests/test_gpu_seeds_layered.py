"""Goal sets on the layered 3D solver (EIK_OPT_SEEDS_LAYERED, eik_fim3d_last_solver).

With the option on, eik_fim3d_solve_seeds gives a few-layer volume to the layered solver (fim2dl.hip) by
eik_fim3d_solve's own rule, when every seed's z lies among the solved layers; otherwise -- and always with
the option off -- the general solver runs as before.  Which solver ran is read from eik_fim3d_last_solver
and asserted in every test: the field must not tell.

The expected field is the specification of the general solver's tests, tests/seeds3d_np.seeded_reference3,
at the suite's bounds (handoff3d.ATOL64 / RTOL32): reachability masks identical, fp64 <= 1e-9 absolute, fp32
<= 2e-5 relative; every seed cell exactly its lowest t0 where undominated, strictly below it otherwise.
Labels are compared for exact equality with the numpy rule (seeds3d_np.label_rule3) on the GPU's own field.
No cell is exempt from either check.  The cases are tests/seeds_layered_cases.py's, built per dtype (tiles of
64 rows in fp32, 40 in fp64) and solved on the specification once per module.

Every context carries EIK_OPT_QTIMEOUT 5, so a lost activation is an error and not a hang.
"""
import ctypes

import numpy as np
import pytest

import handoff3d as HO
import seeds_layered_cases as SC
from seeds3d_np import label_rule3, undominated3

pytestmark = pytest.mark.gpu

F64 = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
GENERAL = {"layered": 0, "z0": 0, "nl": 0, "bands": 0}


def _context(**options):
    import eikonal

    opts = {"QTIMEOUT": 5, "SEEDS_LAYERED": 1}
    opts.update(options)
    return eikonal.Context(0, options=opts)


@pytest.fixture(scope="module")
def ctxs():
    from eikonal import _lib as L

    cs = {
        "on": _context(),
        "off": _context(SEEDS_LAYERED=0),
        "list": _context(MODE=L.MODE_LIST),
        "rounds2": _context(MAX_ROUNDS=2),
    }
    # corners' four forms: the layer-planar copies or the volume's own layout, the FIFO or priority bands
    for planar in (1, 0):
        for prio in (0, 0.25):
            cs[planar, prio] = _context(LAYER_PLANAR=planar, PRIO=prio)
    yield cs
    for c in cs.values():
        c.close()


def dt(f64):
    return np.float64 if f64 else np.float32


def solve(c, cost, seeds, t0, f64, expect, labels=True):
    """eik_fim3d_solve_seeds on device buffers, eik_fim3d_last_solver == expect, then eik_labels3d_dev on the
    field where it lies"""
    import torch
    from eikonal import _lib as L

    dev = torch.device("cuda", 0)
    cd = torch.from_numpy(np.array(cost, dt(f64), order="C")).to(dev)
    Td = torch.full_like(cd, float("nan"))
    H, W, Lz = cost.shape
    c.fim3d_solve_seeds(cd.data_ptr(), Td.data_ptr(), H, W, Lz, L.EIK_F64 if f64 else L.EIK_F32, seeds, t0,
                        torch.cuda.current_stream(dev).cuda_stream)
    s, which = c.stats(), c.last_solver3d()
    assert which == expect, (which, expect)
    assert s["tile_visits"] > 0 and s["host_syncs"] <= 1
    T = Td.cpu().numpy()
    if not labels:
        return T
    lab = c.labels3d(Td, seeds, t0)
    assert lab.dtype == torch.int32 and lab.shape == Td.shape
    return T, lab.cpu().numpy()


def layered(name, f64, bands=0):
    on, z0, nl = SC.expect_layered(name, f64)
    return {"layered": on, "z0": z0, "nl": nl, "bands": bands if on else 0}


# ------------------------------------------------ the checks of tests/test_gpu_seeds3d.py, copied
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


def run(c, name, f64, expect):
    cost, seeds, t0, R = SC.case(name, f64)
    T, lab = solve(c, cost, seeds, t0, f64, expect)
    check_seeded(T, R, seeds, t0, f64)
    check_labels(lab, T, R, seeds, t0)
    return T, lab


# ---------------------------------------------------------------------------------- 1. corners
@F64
@pytest.mark.parametrize("prio", [0, 0.25], ids=["fifo", "bands"])
@pytest.mark.parametrize("planar", [1, 0], ids=["planar", "volume"])
def test_corners(ctxs, planar, prio, f64):
    """seeds on the last cell of a tile and the first cell of its diagonal neighbour, in different layers, in
    a cut corner tile, one of them dominated: layered, layers 0 .. 2, the bands as asked for"""
    T, lab = run(ctxs[planar, prio], "corners", f64, {"layered": 1, "z0": 0, "nl": 3, "bands": int(prio > 0)})
    assert set(np.unique(lab)) == {-1, 0, 1, 2, 4}  # (-1: the +inf cells) the 1e4 seed owns nothing


# ---------------------------------------------------------------------------------- 2. padded
@F64
def test_padded(ctxs, f64):
    T, lab = run(ctxs["on"], "padded", f64, {"layered": 1, "z0": 1, "nl": 3, "bands": 0})
    assert np.isinf(T[:, :, 0]).all() and np.isinf(T[:, :, 4]).all()
    assert (lab[:, :, 0] == -1).all() and (lab[:, :, 4] == -1).all()


# ---------------------------------------------------------------------------------- 3. fall-backs
@F64
@pytest.mark.parametrize("which,name", [("on", "pad_seed"), ("on", "open4"), ("list", "corners"), ("rounds2", "corners")])
def test_falls_back_to_the_general_solver(ctxs, which, name, f64):
    """a seed in a padding layer; four open layers (fp64: one more than the layered solver takes -- fp32 takes
    them, and says so); a list-mode context; EIK_OPT_MAX_ROUNDS = 2: the general solver, the field still right"""
    expect = layered(name, f64) if which == "on" else GENERAL
    if name == "pad_seed" or (name == "open4" and f64) or which != "on":
        assert expect == GENERAL
    T, lab = run(ctxs[which], name, f64, expect)
    if name == "pad_seed":
        x, y, z = SC.PAD_SEED
        assert T[y, x, 0] == SC.PAD_SEED_T0 and lab[y, x, 1] == len(SC.case(name, f64)[1]) - 1  # fed from the padding


# ---------------------------------------------------------------------------------- 4. small cases
@F64
@pytest.mark.parametrize("name", ["inf_seed", "column", "pair"] + list(SC.TINY))
def test_small_cases(ctxs, name, f64):
    T, lab = run(ctxs["on"], name, f64, layered(name, f64))
    if name == "inf_seed":  # the seed on a +inf cell of a solved layer keeps its t0 and feeds its neighbour
        (x, y, z), (nx, ny, nz) = SC.INF_SEED, SC.INF_NEXT
        assert T[y, x, z] == 2.0 and lab[y, x, z] == 1 and T[ny, nx, nz] == 3.0 and lab[ny, nx, nz] == 1
    if name == "column":
        x, y = SC.COLUMN
        assert T[y, x, 0] == 0.0 and T[y, x, 2] == 0.75 and np.isinf(T[y, x, 1]) and set(np.unique(lab)) == {-1, 0, 1}
    if name == "pair":  # two seeds on one cell: the lower value holds and the label is 1
        x, y, z = SC.case(name, f64)[1][0]
        assert T[y, x, z] == 3.0 and lab[y, x, z] == 1 and set(np.unique(lab)) <= {-1, 1}


# ---------------------------------------------------------------------------------- 5. one seed at 0
@F64
def test_one_seed_at_zero_is_the_single_goal_field(ctxs, f64):
    """... against the oracle at the suite's bounds; the single-goal entry on the same volume and context
    reports the layered solver too (both entries set eik_fim3d_last_solver)"""
    import torch
    from eikonal import _lib as L

    c = ctxs["on"]
    cost, seeds, _, _ = SC.case("corners", f64)
    goal = seeds[0]
    R = HO.oracle_field(("seeds_layered", cost.shape, goal), cost, goal)
    T, lab = solve(c, cost, [goal], None, f64, {"layered": 1, "z0": 0, "nl": 3, "bands": 0})
    HO.check_field(T, R, goal, f64)
    assert np.array_equal(lab >= 0, np.isfinite(R)) and set(np.unique(lab)) <= {-1, 0}
    # a general-solver solve in between (fp64, four open layers), so that the next answer is the single-goal
    # solve's own
    solve(c, SC.case("open4", True)[0], [(4, 4, 0)], None, True, GENERAL, labels=False)
    dev = torch.device("cuda", 0)
    cd = torch.from_numpy(np.array(cost, dt(f64), order="C")).to(dev)
    Td = torch.full_like(cd, float("nan"))
    H, W, Lz = cost.shape
    c._chk(L.lib().eik_fim3d_solve(c._h, cd.data_ptr(), Td.data_ptr(), H, W, Lz, L.EIK_F64 if f64 else L.EIK_F32,
                                   np.asarray(goal, np.int64), torch.cuda.current_stream(dev).cuda_stream))
    assert c.last_solver3d() == {"layered": 1, "z0": 0, "nl": 3, "bands": 0}
    Tg = Td.cpu().numpy()
    HO.check_field(Tg, R, goal, f64)


# ---------------------------------------------------------------------------------- 6. the option off
@F64
@pytest.mark.parametrize("name", ["corners", "padded"])
def test_option_off_is_the_general_solver(ctxs, name, f64):
    """no behaviour change: the same call on a context without the option runs the general solver, as a
    context that never heard of the option does, and passes the same checks"""
    import eikonal

    run(ctxs["off"], name, f64, GENERAL)
    if name == "corners":
        c = eikonal.Context(0, options={"QTIMEOUT": 5})  # the default
        try:
            run(c, name, f64, GENERAL)
            assert c.stats()["fresh_visits"] == 0
        finally:
            c.close()


# ---------------------------------------------------------------------------------- 7. bad arguments
@F64
def test_bad_arguments(ctxs, f64):
    """the EIK_ERR_ARG list of tests/test_gpu_seeds3d.py with the option on: the same messages, d_T untouched
    (it keeps its NaN fill), nothing launched"""
    import torch
    from eikonal import _lib as L

    c = ctxs["on"]
    dev = torch.device("cuda", 0)
    shape = (8, 9, 3)  # H, W, L: a volume the layered solver would take
    cd = torch.ones(shape, dtype=torch.float64 if f64 else torch.float32, device=dev)
    Td = torch.full_like(cd, float("nan"))
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

    H, W, Lz = shape
    one = [(1, 1, 1)]
    solve(c, np.ones(shape), one, None, f64, {"layered": 1, "z0": 0, "nl": 3, "bands": 0}, labels=False)
    before = c.last_solver3d()
    bad = [
        ("K = 0", dict(seeds=one, K=0)),
        ("K = -1", dict(seeds=one, K=-1)),
        ("K = 16777217", dict(seeds=one, K=(1 << 24) + 1)),
        ("seeds is NULL", dict(seeds=None, K=1)),
        (r"seed 1 (9, 3, 2) outside", dict(seeds=[(1, 1, 1), (9, 3, 2)])),
        (r"seed 2 (3, 8, 2) outside", dict(seeds=[(1, 1, 1), (2, 2, 2), (3, 8, 2)])),
        (r"seed 0 (3, 3, 3) outside", dict(seeds=[(3, 3, 3)])),
        (r"seed 1 (3, -1, 2) outside", dict(seeds=[(1, 1, 1), (3, -1, 2)])),
        ("t0[1] = -0.5", dict(seeds=[(1, 1, 1), (2, 2, 2)], t0=[0.0, -0.5])),
        ("t0[0] = nan", dict(seeds=one, t0=[float("nan")])),
        ("t0[2] = inf", dict(seeds=[(1, 1, 1), (2, 2, 2), (3, 3, 2)], t0=[0.0, 1.0, float("inf")])),
        ("bad shape 0 x 9 x 3", dict(seeds=one, H=0)),
        ("bad shape 8 x 0 x 3", dict(seeds=one, W=0)),
        ("bad shape 8 x 9 x -2", dict(seeds=one, Lz=-2)),
    ]
    if not f64:
        bad.append(("t0[1] = 1e+39 rounds to +inf", dict(seeds=[(1, 1, 1), (2, 2, 2)], t0=[0.0, 1e39])))
    for msg, kw in bad:
        a = dict(H=H, W=W, Lz=Lz, t0=None)
        a.update(kw)
        assert solve_rc(cp, tp, **a) == L.EIK_ERR_ARG, msg
        assert msg in err() and "eik_fim3d_solve_seeds" in err(), (msg, err())
    assert solve_rc(None, tp, H, W, Lz, one, None) == L.EIK_ERR_ARG and "d_cost is NULL" in err()
    assert solve_rc(cp, None, H, W, Lz, one, None) == L.EIK_ERR_ARG and "d_T is NULL" in err()
    # the host entries check the same list
    cost = np.ones(shape, dt(f64))
    with pytest.raises(L.EikError, match=r"seed 0 \(1, 1, 9\)") as e:
        c.tmap3d_seeds(cost, [(1, 1, 9)], dtype=dt(f64), labels=True)
    assert e.value.code == L.EIK_ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(Td).all()), "a refused call launched something"
    assert c.last_solver3d() == before  # ... and decided nothing
    # the query's own arguments
    assert raw.eik_fim3d_last_solver(vp(None), vp(np.zeros(4, np.int64).ctypes.data)) == L.EIK_ERR_ARG
    assert raw.eik_fim3d_last_solver(vp(c._h.value), vp(None)) == L.EIK_ERR_ARG
    # the context is still usable
    assert solve(c, np.ones(shape), one, None, f64, before, labels=False)[1, 1, 1] == 0


# ---------------------------------------------------------------------------------- the host entry
@F64
def test_host_entry_follows_the_same_rule(ctxs, f64):
    c = ctxs["on"]
    cost, seeds, t0, R = SC.case("corners", f64)
    T, lab = c.tmap3d_seeds(cost, seeds, t0, dtype=dt(f64), labels=True)
    assert c.last_solver3d() == {"layered": 1, "z0": 0, "nl": 3, "bands": 0}
    assert T.dtype == dt(f64) and lab.dtype == np.int32
    check_seeded(T, R, seeds, t0, f64)
    check_labels(lab, T, R, seeds, t0)
    cost, seeds, t0, R = SC.case("pad_seed", f64)
    T = c.tmap3d_seeds(cost, seeds, t0, dtype=dt(f64))
    assert c.last_solver3d() == GENERAL
    check_seeded(T, R, seeds, t0, f64)


# ---------------------------------------------------------------------------------- 8. the drop-in
def _smooth_padded(shape):
    """H x W x 5: one gentle open raster in layers 1 .. 3, layers 0 and 4 all +inf"""
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    flat = (2.0 + 0.5 * np.sin(0.4 * xs) * np.cos(0.3 * ys)).astype(np.float32).astype(np.float64)
    inf = np.full(flat.shape, np.inf)
    return np.stack([inf, flat, flat, flat, inf], axis=-1)


@F64
def test_drop_in(f64, monkeypatch):
    import FastMarching.FastMarching3D as FM3
    from eikonal import _lib as L

    monkeypatch.setattr(FM3, "_DTYPE", dt(f64))
    monkeypatch.delenv("EIKONAL_SEEDS_LAYERED", raising=False)
    dc = FM3._ctx()
    cost, goals, offsets, R = SC.case("corners", f64)
    # the list form, then the mask form: its True cells in row-major order
    T, lab = FM3.computeTmapMulti(cost, goals, offsets, labels=True, layered=True)
    assert dc.last_solver3d() == {"layered": 1, "z0": 0, "nl": 3, "bands": 0}
    assert dc.get_option(L.OPT_SEEDS_LAYERED) == 0  # put back
    assert T.dtype == np.float64 and lab.dtype == np.int32
    Tn = T.astype(dt(f64))
    check_seeded(Tn, R, goals, offsets, f64)
    check_labels(lab, Tn, R, goals, offsets)
    mask = np.zeros(cost.shape, bool)
    for x, y, z in goals:
        mask[y, x, z] = True
    order = sorted(range(len(goals)), key=lambda k: (goals[k][1], goals[k][0], goals[k][2]))
    assert order != list(range(len(goals)))
    Tm, labm = FM3.computeTmapMulti(cost, mask, [offsets[k] for k in order], labels=True, layered=True)
    assert dc.last_solver3d()["layered"] == 1
    close(Tm.astype(dt(f64)), T, f64)
    assert np.array_equal(labm, label_rule3(Tm.astype(dt(f64)), [goals[k] for k in order], [offsets[k] for k in order]))
    und = undominated3(R, goals, offsets)
    for j, k in enumerate(order):
        assert (labm[goals[k][1], goals[k][0], goals[k][2]] == j) == und[k], (j, k)
    # without the switch: the environment on every call, else off -- and the general solver, as before
    T0 = FM3.computeTmapMulti(cost, goals, offsets)
    assert dc.last_solver3d() == GENERAL
    close(T0.astype(dt(f64)), R, f64)
    monkeypatch.setenv("EIKONAL_SEEDS_LAYERED", "1")
    FM3.computeTmapMulti(cost, goals, offsets)
    assert dc.last_solver3d()["layered"] == 1 and dc.get_option(L.OPT_SEEDS_LAYERED) == 0
    FM3.computeTmapMulti(cost, goals, offsets, layered=False)
    assert dc.last_solver3d() == GENERAL
    monkeypatch.setenv("EIKONAL_SEEDS_LAYERED", "0")
    FM3.computeTmapMulti(cost, goals, offsets)
    assert dc.last_solver3d() == GENERAL
    # a call that raises puts the option back too
    with pytest.raises(L.EikError):
        FM3.computeTmapMulti(cost, goals, [-1.0] * len(goals), layered=True)
    assert dc.get_option(L.OPT_SEEDS_LAYERED) == 0
    # afterwards the default context's own seeded solves are the general solver's again
    dc.tmap3d_seeds(cost, goals, offsets, dtype=dt(f64))
    assert dc.last_solver3d() == GENERAL

    # paths to the nearest goal: the planner's form of the volume -- three layers between two +inf padding
    # layers -- with a gentle cost (the 3D walker descends np.gradient of T), the same in every layer, and the
    # corners' cells as goals in the middle layer, so that the descent has no z component to leave the volume by
    smooth, goals = _smooth_padded(cost.shape), [(x, y, 2) for x, y, _ in goals]
    Ts, labs = FM3.computeTmapMulti(smooth, goals, [0.0, 0.0, 0.0, 1e4, 0.0], labels=True, layered=True)
    assert dc.last_solver3d() == {"layered": 1, "z0": 1, "nl": 3, "bands": 0}
    starts = [(20.0, 20.0, 2.0), (100.0, 30.0, 2.0), (30.0, 110.0, 2.0), (110.0, 115.0, 2.0), (75.0, 70.0, 2.0)]
    named = [int(labs[int(y), int(x), int(z)]) for x, y, z in starts]
    assert set(named) == {0, 1, 2, 4}  # every goal but the one at 1e4 is somebody's nearest
    paths = FM3.getPathsToNearest(Ts, labs, goals, starts, 0.5)
    assert len(paths) == len(starts)
    for p, s, k in zip(paths, starts, named):
        assert p.shape[1] == 3 and np.array_equal(p[-1], np.asarray(goals[k], np.float64)), (s, k, p[-1])
