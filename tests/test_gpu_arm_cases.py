"""The end-effector volume on the GPU, branch by branch (arm.hip, eik_arm_*), against the
reference's own outputs on crafted inputs (tests/golden/arm_cases.npz; the cases and the branch
each one pins are listed in tests/arm_cases.py):

* every case the reference returns: planner.TunnelCost / planner.GetObstMap bit for bit;
* every case the reference raises on (NaN / inf heights, base points, headings; an index below
  -sZ): EikError, and the same context then reproduces a returning case;
* the existing error returns (non-square volume, waypoint outside, too many tunnel events);
* one context across the largest and smallest tables (the scratch layout moves between calls);
* eik_arm_path_f64 on two crafted volumes: cost bit-exact, field and path against the oracle;
* eik_tmap3d_batch_f64 at cut tiles, corner goals and a walled-in goal for B in {1, 3, 16}."""
import numpy as np
import pytest

import arm_cases as AC
import oracle as O
from band import BAND_BRACKET, band_ratio
import planner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import eikonal

    c = eikonal.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(golden):
    return golden("arm_cases")


def _volume(c):
    if "xy_m" in c:
        return planner.volume(*c["shape"], *c["res"], *c["xy_m"])
    return planner.volume(*c["shape"], *c["res"], 0.0, 0.0, *c["radii"], c["finalWP"], c["initWP"])


def _tunnel(ctx, c):
    return ctx.arm_tunnel_cost(c["base"], c["heading"], _volume(c))


# ---------------------------------------------------------------- parity with the reference
@pytest.mark.parametrize("name", AC.T_OK)
def test_tunnel_cost_case(cases, name):
    c = AC.case(cases, name)
    got = planner.TunnelCost(*AC.tunnel_args(c))
    assert got.shape == c["tunnel"].shape
    assert np.array_equal(got, c["tunnel"]), int((got != c["tunnel"]).sum())


@pytest.mark.parametrize("name", AC.G_OK)
def test_obst_map_case(ctx, cases, name):
    c = AC.case(cases, name)
    f, o, g = planner.GetObstMap(*AC.obst_args(c))
    assert np.array_equal(f, c["finalMap"]), int((f != c["finalMap"]).sum())
    assert np.array_equal(o, c["obstMap"]) and np.array_equal(g, c["groundMap"])
    f1, o1, g1 = ctx.arm_obst_map(c["Z"], c["obst"], _volume(c), all_maps=False)
    assert o1 is None and g1 is None and np.array_equal(f1, c["finalMap"])


# ---------------------------------------------------------------- where the reference raises
@pytest.mark.parametrize("name", AC.T_RAISE)
def test_tunnel_cost_raises(ctx, cases, name):
    import eikonal

    c = AC.case(cases, name)
    got = None
    with pytest.raises(eikonal.EikError):
        got = _tunnel(ctx, c)
    assert got is None
    ok = AC.case(cases, "T6")  # the context is still usable
    assert np.array_equal(_tunnel(ctx, ok), ok["tunnel"])


@pytest.mark.parametrize("name", AC.G_RAISE)
def test_obst_map_raises(ctx, cases, name):
    import eikonal

    c = AC.case(cases, name)
    got = None
    with pytest.raises(eikonal.EikError):
        got = ctx.arm_obst_map(c["Z"], c["obst"], _volume(c))
    assert got is None
    ok = AC.case(cases, "G1")
    f, o, g = ctx.arm_obst_map(ok["Z"], ok["obst"], _volume(ok))
    assert np.array_equal(f, ok["finalMap"]) and np.array_equal(o, ok["obstMap"]) and np.array_equal(g, ok["groundMap"])


def test_arm_path_raises_on_bad_input(ctx, cases):
    """The chain takes the same decisions: a NaN height, a NaN base point, then a clean run."""
    import eikonal

    t, g = AC.case(cases, "T1"), AC.case(cases, "C1")
    vol = planner.volume(*t["shape"], *t["res"], *g["xy_m"], *t["radii"], t["finalWP"], t["initWP"])
    Z = g["Z"].copy()
    Z[3, 4] = np.nan
    with pytest.raises(eikonal.EikError, match="GetObstMap"):
        ctx.arm_path(Z, g["obst"], t["base"], t["heading"], vol, 0.5)
    base = t["base"].copy()
    base[0, 2] = np.nan
    with pytest.raises(eikonal.EikError, match="TunnelCost"):
        ctx.arm_path(g["Z"], g["obst"], base, t["heading"], vol, 0.5)
    path, st, cost, _ = ctx.arm_path(g["Z"], g["obst"], t["base"], t["heading"], vol, 0.5, want_fields=True)
    assert np.array_equal(cost, g["finalMap"] * t["tunnel"])


def test_non_square_volume(ctx, cases):
    import eikonal

    c = AC.case(cases, "T6")
    vol = planner.volume(12, 10, 12, *c["res"], 0.0, 0.0, *c["radii"], c["finalWP"], c["initWP"])
    with pytest.raises(eikonal.EikError, match="square"):
        ctx.arm_tunnel_cost(c["base"], c["heading"], vol)
    g = AC.case(cases, "G1")
    with pytest.raises(eikonal.EikError, match="square"):
        ctx.arm_obst_map(g["Z"], g["obst"], planner.volume(12, 10, 12, *g["res"], *g["xy_m"]))
    assert np.array_equal(_tunnel(ctx, c), c["tunnel"])


@pytest.mark.parametrize("which", ["final", "initial"])
def test_arm_path_waypoint_outside(ctx, cases, which):
    import eikonal

    t, g = AC.case(cases, "T1"), AC.case(cases, "C1")
    out = (t["shape"][0], 3, 3)  # x == sX: one past the last column
    fw, iw = (out, t["initWP"]) if which == "final" else (t["finalWP"], out)
    vol = planner.volume(*t["shape"], *t["res"], *g["xy_m"], *t["radii"], fw, iw)
    with pytest.raises(eikonal.EikError, match="waypoint outside"):
        ctx.arm_path(g["Z"], g["obst"], t["base"], t["heading"], vol, 0.5)


def test_too_many_tunnel_events(ctx, cases):
    """Event numbers are 32 bit.  res = 0.5 / 2395 with rlim = 0.25 gives nX = nZ = 2400, so 400 base
    points make 2 . 400 . 2400^2 = 4.6e9 >= 2^32 events; the host tables stay at 2 . 2400^2 doubles
    (92 MB) and the call returns before any launch."""
    import eikonal

    res = 0.5 / 2395
    npts = 400
    base = np.full((npts, 3), 2 * res)
    heading = np.zeros((npts, 3))
    vol = planner.volume(4, 4, 4, res, res, res, 0.0, 0.0, 0.25, 0.12, 0.04, (1, 1, 1), (2, 2, 2))
    with pytest.raises(eikonal.EikError, match="too many tunnel events"):
        ctx.arm_tunnel_cost(base, heading, vol)
    ok = AC.case(cases, "T6")
    assert np.array_equal(_tunnel(ctx, ok), ok["tunnel"])


# ---------------------------------------------------------------- one context, moving scratch layout
def test_stale_state_across_table_sizes(ctx, cases):
    """tables | first | closed share one scratch buffer whose split moves with the table size (nZ,
    base points) and the cell count: largest, smallest, largest, with a GetObstMap in between."""
    big, small, one = AC.case(cases, "T2a"), AC.case(cases, "T6"), AC.case(cases, "T1")
    g = AC.case(cases, "G5a")
    for c in (big, small, big, g, one, small, g, big):
        if "tunnel" in c:
            got = _tunnel(ctx, c)
            assert np.array_equal(got, c["tunnel"]), int((got != c["tunnel"]).sum())
        else:
            f, o, gm = ctx.arm_obst_map(c["Z"], c["obst"], _volume(c))
            assert np.array_equal(f, c["finalMap"]) and np.array_equal(o, c["obstMap"]) and np.array_equal(gm, c["groundMap"])


# ---------------------------------------------------------------- volume -> field -> path
@pytest.mark.parametrize("t,g", [("T1", "C1"), ("T2b", "C2")])
def test_arm_path_chain(ctx, cases, t, g):
    t, g = AC.case(cases, t), AC.case(cases, g)
    fw, iw = t["finalWP"], t["initWP"]
    vol = planner.volume(*t["shape"], *t["res"], *g["xy_m"], *t["radii"], fw, iw)
    path, st, cost, T = ctx.arm_path(g["Z"], g["obst"], t["base"], t["heading"], vol, 0.5, want_fields=True)
    ref_cost = g["finalMap"] * t["tunnel"]  # :1580, both factors the reference's own
    assert np.array_equal(cost, ref_cost)
    R = O.fmm3d(ref_cost, [int(v) for v in fw], [int(v) for v in iw])
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin)
    ts = R[iw[1], iw[0], iw[2]]
    closed = fin & (R < ts)
    assert np.abs(T[closed] - R[closed]).max() <= 1e-9
    band = fin & ~closed
    assert np.all(T[band] <= R[band] + 1e-9)
    r = band_ratio(T, R, band)
    assert r <= BAND_BRACKET, f"band: reference / GPU up to {r:.4f} (bracket {BAND_BRACKET})"
    ref_path, ref_st = O.gdm3d(R, [float(v) for v in iw], [float(v) for v in fw], 0.5)
    assert st == ref_st and path.shape == ref_path.shape and np.abs(path - ref_path).max() <= 1e-9
    assert len(path) >= 2 and np.array_equal(path[-1], fw.astype(float))


# ---------------------------------------------------------------- eik_tmap3d_batch_f64
def _batch(B, H, W, Lz):
    """Volume b: b % 3 == 0 goal in the last cell, 1 goal in the first cell (of the next volume),
    2 goal inside a block that +inf walls in."""
    rng = np.random.default_rng(100 * B + H)
    cost = rng.uniform(1, 5, (B, H, W, Lz))
    cost[:, H // 2, 2:W - 1, : max(1, Lz - 1)] = np.inf  # a wall with gaps, crossing tile cuts
    goals = np.zeros((B, 3), np.int64)
    for b in range(B):
        if b % 3 == 0:
            goals[b] = (W - 1, H - 1, Lz - 1)
        elif b % 3 == 2:
            y, x, z = H // 4 + 1, W // 2, Lz // 2
            blk = cost[b, y - 1:y + 2, x - 1:x + 2, max(0, z - 1):z + 2].copy()
            cost[b] = np.inf
            cost[b, y - 1:y + 2, x - 1:x + 2, max(0, z - 1):z + 2] = blk
            goals[b] = (x, y, z)
        cost[b, goals[b, 1], goals[b, 0], goals[b, 2]] = 1.0
    return cost, goals


@pytest.fixture(scope="module")
def batch_refs():
    """cost, goals and the oracle field of each volume, computed once per (B, shape)."""
    out = {}
    for shape in ((17, 9, 9), (18, 17, 3)):
        for B in (1, 3, 16):
            cost, goals = _batch(B, *shape)
            R = np.stack([O.fmm3d(cost[b], [int(v) for v in goals[b]]) for b in range(B)])
            cost.setflags(write=False)
            R.setflags(write=False)
            out[B, shape] = (cost, goals, R)
    return out


@pytest.mark.parametrize("shape", [(17, 9, 9), (18, 17, 3)])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_tmap3d_batch_cut_tiles(ctx, batch_refs, B, shape):
    cost, goals, R = batch_refs[B, shape]
    T = ctx.tmap3d_batch(cost, goals)
    for b in range(B):
        fin = np.isfinite(R[b])
        assert fin.any() and (b % 3 != 2 or fin.sum() <= 27)
        assert np.array_equal(np.isfinite(T[b]), fin), b
        assert np.abs(T[b][fin] - R[b][fin]).max() <= 1e-9, b
