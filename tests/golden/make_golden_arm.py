"""Golden fixtures for the planner's end-effector volume:
GetObstMap (Coupled_motion_planner.py:319-358) and TunnelCost (:505-725).

Run ONCE in the build container, where the reference sources are readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_arm.py          # arm.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_arm.py cases    # arm_cases.npz

The second form writes the crafted per-branch cases (crafted_cases() below, listed in
tests/arm_cases.py) and leaves arm.npz alone.

The reference module cannot be imported here (its top-level `import cv2` fails: OpenCV is not
installed), so this script reads /root/reference/src/Coupled_motion_planner.py as text, compiles
ONLY the two function definitions (found with `ast`, unmodified) and runs them in a namespace
holding what they use (numpy as np, math, numpy.dot as dot -- the module's own imports, :1-16).
Nothing else of the planner runs.  Inputs are shaped as main() builds them (:1462-1575): a square
area of 2h x 2h DEM cells with resX = res (2h - 1) / (2h), resZ = 0.02, sZ = round(aZ / 0.02), the
arm base path and heading inside it, waypoints rounded to uint32 nodes.  Outputs are stored next to
this script as arm.npz; nothing under tests/ reads /root/reference at test time.
"""
import ast
import math
import os
import sys

import numpy as np

REF = "/root/reference/src/Coupled_motion_planner.py"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def load_reference_functions(names):
    src = open(REF).read()
    tree = ast.parse(src)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(d.name for d in defs) == sorted(names)
    ns = {"np": np, "math": math, "dot": np.dot}
    exec(compile(ast.Module(body=defs, type_ignores=[]), REF, "exec"), ns)
    return [ns[n] for n in names]


GetObstMap, TunnelCost = load_reference_functions(["GetObstMap", "TunnelCost"])

Rm, rm = 0.4241, 0.1105          # :1121-1122
rO = (Rm + rm) / 2               # :1123
Rlim = 0.527                     # :1124


def case(seed, half, res=0.05, m=12, sample_on_grid=False):
    rng = np.random.default_rng(seed)
    n = 2 * half
    ixmin, ixmax = 100, 100 + n  # :1487-1509 (an interior area)
    aX = res * (ixmax - 1) - res * ixmin  # :1523
    # smooth heights >= 0 (ZsMap - Zmin, :1537-1545)
    yy, xx = np.mgrid[0:n, 0:n] * res
    Z = 0.08 * np.sin(1.7 * xx + seed) * np.cos(1.3 * yy) + 0.05 * np.sin(3.1 * yy + 0.4 * xx)
    Z = Z + 0.02 * rng.standard_normal((n, n))
    Z = Z - Z.min()
    aZ = Z.max() - Z.min() + 0.5  # :1525
    sX, sY = Z.shape  # :1528
    sZ = int(round(aZ / 0.02))  # :1529
    resX, resY, resZ = aX / sX, aX / sY, 0.02  # :1532-1534
    obst = (rng.random((n, n)) < 0.08).astype(np.float64)
    # arm base path towards the sample, heading (roll, pitch, yaw) along it
    p0 = np.array([0.25 * n * resX, 0.3 * n * resY])
    p1 = np.array([0.55 * n * resX, 0.6 * n * resY])
    t = np.linspace(0, 1, m)[:, None]
    xy = p0 + t * (p1 - p0) + 0.02 * rng.standard_normal((m, 2))
    base = np.zeros((m, 3))
    base[:, :2] = xy
    base[:, 2] = 0.23 + 0.1 * rng.random(m)
    yaw = math.atan2(p1[1] - p0[1], p1[0] - p0[0]) + 0.1 * rng.standard_normal(m)
    heading = np.stack([0.05 * rng.standard_normal(m), 0.05 * rng.standard_normal(m), yaw], 1)
    xmNew, ymNew, zmNew = p1[0] + 0.25, p1[1] + 0.2, Z.max() * 0.5 + 0.1
    finalWP = np.uint32(np.round([xmNew / resX, ymNew / resY, zmNew / resZ]))  # :1574
    initWP = np.uint32(np.round([(p0[0] + 0.2) / resX, (p0[1] + 0.1) / resY, 0.4 / resZ]))  # :1573
    # GetObstMap's sample test compares resX * i with the GLOBAL xm (:329); one case puts the
    # sample exactly on a grid column/row to exercise the skip
    xm, ym = (resX * 7, resY * 9) if sample_on_grid else (12.3456, 7.891)
    fm, om, gm = GetObstMap(Z, resX, resY, resZ, sX, sY, sZ, obst, xm, ym)
    cm = TunnelCost(Rlim, rO, rm, base, sX, sY, sZ, resX, resY, resZ, heading, finalWP, initWP)
    return dict(Z=Z, obst=obst, res=np.array([resX, resY, resZ]), shape=np.array([sX, sY, sZ]),
                xy_m=np.array([xm, ym]), base=base, heading=heading, finalWP=finalWP, initWP=initWP,
                finalMap=fm, obstMap=om, groundMap=gm, tunnel=cm, radii=np.array([Rlim, rO, rm]))


# ------------------------------------------------------------------ crafted per-branch cases
# A second fixture file, arm_cases.npz: small volumes (<= 24 x 24 x 30) that each drive one branch
# of the two functions, with the reference's output or, where it raises, the exception's class name
# (`err`, "" where it returns).  Written by `make_golden_arm.py cases`; arm.npz is not touched.
RAD = (0.25, 0.12, 0.04)  # rlim, rO, rm: not the planner's, so nX / nZ / nK change parity with resZ


def _run(fn, *a):
    try:
        return fn(*a), ""
    except Exception as e:  # the class name is the fixture
        return None, type(e).__name__


def _sizes(rlim, resX, resZ):
    tr = rlim + 2 * resX
    nX, nZ = int(round(2 * tr / resX) + 1), int(round(2 * tr / resZ) + 1)
    return tr, nX, nZ, round(nZ / 2) + 1


def _event_nodes(radii, shape, res, base, heading):
    """Nodes of the close events by kind (wall :579, back :641, cap :722) and the extent of all
    events, formed as the reference forms them; only the generator's own assertions use this."""
    sys.path.insert(0, os.path.join(OUT, "..", "..", "oracle"))
    import arm_oracle as AO

    rlim, rO, rm = radii
    resX, resY, resZ = res
    tr, nX, nZ, nK = _sizes(rlim, resX, resZ)
    I, K = np.meshgrid(np.linspace(-tr, tr, nX), np.linspace(-tr, tr, nZ), indexing="ij")
    I, K = I.ravel(), K.ravel()
    norm = np.sqrt(I ** 2 + K ** 2)
    ins = norm < rlim
    vA = 15 * (norm[ins] - (rO + rm) / 2) ** 2 + 2 + 4 * (I[ins] + rlim + 2 * resZ)
    ks = np.linspace(0, tr, nK)
    vC = 15 * (ks - (rO + rm) / 2) ** 2 + 2
    assert not (vA == 10).any() and not (vC == 10).any(), "an assign of exactly 10 is not modelled"
    m = len(base)
    wall, alln = [], []
    for j in range(m):
        T = AO._toa(heading[j], base[j], math.pi / 2)
        n0 = np.stack(AO._nodes(T, I, np.zeros_like(I), K, res), 1)
        n1 = np.stack(AO._nodes(T, I, np.full_like(I, resY), K, res), 1)
        wall.append(n0[~ins])
        alln += [n0, n1[ins]]
    T = AO._toa(heading[0], base[0], math.pi / 2)
    back = np.stack(AO._nodes(T, I, np.full_like(I, -resY), K, res), 1)[ins]
    T = AO._toa(heading[m - 1], base[m - 1], 0.0)
    th = np.array([math.pi * t / 180 for t in range(-100, 100, 2)])[:, None]
    sg = np.array([math.pi * s / 180 for s in range(-90, 90, 2)])[None, :]
    rad = rlim + 2 * resZ
    X, Y, Zc = rad * np.cos(th) * np.cos(sg), rad * np.cos(th) * np.sin(sg), rad * np.sin(th) * np.ones_like(sg)
    cap = np.stack(AO._nodes(T, X.ravel(), Y.ravel(), Zc.ravel(), res), 1)
    alln += [back, cap]
    return dict(wall=np.concatenate(wall), back=back, cap=cap, all=np.concatenate(alln))


def tcase(shape, res, base, heading, fw, iw):
    base = np.asarray(base, np.float64).reshape(-1, 3)
    heading = np.asarray(heading, np.float64).reshape(-1, 3)
    fw, iw = np.uint32(fw), np.uint32(iw)
    cm, err = _run(TunnelCost, *RAD, base, *shape, *res, heading, fw, iw)  # RAD: stored once, as t_radii
    c = dict(vol=np.array([*shape, *res], np.float64), base=base, heading=heading, finalWP=fw, initWP=iw, err=err)
    if cm is not None:
        c["tunnel"] = cm
    return c


def gcase(Z, obst, res, shape, xm=12.3456, ym=7.891):
    Z, obst = np.asarray(Z, np.float64), np.asarray(obst, np.float64)
    r, err = _run(GetObstMap, Z, *res, *shape, obst, xm, ym)
    c = dict(Z=Z, obst=obst, vol=np.array([*shape, *res, xm, ym], np.float64), err=err)
    if r is not None:
        c["finalMap"], c["obstMap"], c["groundMap"] = r
    return c


def dem(m, n, lo, hi, seed=0):
    """(m, n) heights in [lo, hi] and a 0/1 obstacle raster, both deterministic."""
    jj, ii = np.mgrid[0:m, 0:n]
    w = 0.5 + 0.25 * np.sin(0.9 * ii + 0.4 * jj + seed) + 0.25 * np.cos(1.3 * jj - 0.7 * ii)
    Z = np.round((lo + (hi - lo) * np.clip(w, 0, 1)) * 4096) / 4096  # dyadic: the file stays small
    obst = (((3 * ii + 5 * jj + seed) % 7) == 0).astype(np.float64)
    return Z, obst


def crafted_cases():
    T, G = {}, {}
    far = lambda shape: (shape[0] - 1, shape[1] - 1, shape[2] - 1)  # noqa: E731

    # T1: one base point -- back closure and half sphere from the same transform's point.  Its
    # waypoints are the ones the chain test solves between (tests/test_gpu_arm_cases.py).
    sh1, res1 = (24, 24, 30), (0.05, 0.05, 0.02)
    b1, h1 = [[0.55, 0.5, 0.3]], [[0.02, -0.03, 0.4]]
    d = np.array([math.cos(0.4), math.sin(0.4)])
    fw1 = np.round([(0.55 + 0.2 * d[0]) / 0.05, (0.5 + 0.2 * d[1]) / 0.05, 0.4 / 0.02])
    iw1 = np.round([(0.55 + 0.05 * d[0]) / 0.05, (0.5 + 0.05 * d[1]) / 0.05, 0.2 / 0.02])
    T["T1"] = tcase(sh1, res1, b1, h1, fw1, iw1)

    # T2a-d: resX != resY and four resZ; nX / nZ / nK printed below
    b2 = [[0.3, 0.35, 0.3], [0.4, 0.52, 0.31], [0.5, 0.7, 0.3]]
    yaw = math.atan2(0.35, 0.2)
    h2 = [[0.03, 0.02, yaw - 0.1], [-0.02, 0.04, yaw], [0.01, -0.03, yaw + 0.1]]
    dd = np.array([math.cos(yaw), math.sin(yaw)])
    for tag, resZ, sZ in (("a", 0.02, 30), ("b", 0.025, 24), ("c", 0.03, 20), ("d", 0.04, 15)):
        res = (0.04, 0.05, resZ)
        fw = np.round([(0.5 + 0.15 * dd[0]) / 0.04, (0.7 + 0.15 * dd[1]) / 0.05, 0.34 / resZ])
        iw = np.round([(0.3 + 0.04 * dd[0]) / 0.04, (0.35 + 0.04 * dd[1]) / 0.05, 0.27 / resZ])
        T["T2" + tag] = tcase((24, 24, sZ), res, b2, h2, fw, iw)
        tr, nX, nZ, nK = _sizes(RAD[0], 0.04, resZ)
        print(f"T2{tag}: resZ {resZ} nX {nX} nZ {nZ} (nZ/2 = {nZ / 2}) nK {nK}", flush=True)
    nzs = [_sizes(RAD[0], 0.04, rz)[2] for rz in (0.02, 0.025, 0.03, 0.04)]
    assert any(z % 2 for z in nzs) and any(z % 2 == 0 for z in nzs)  # odd nZ: nZ / 2 on a half (:678)

    # T3: strong roll and pitch, yaws beyond +-pi/2
    T["T3"] = tcase((24, 24, 24), (0.04, 0.05, 0.025), [[0.6, 0.8, 0.3], [0.45, 0.6, 0.28], [0.4, 0.4, 0.33]],
                    [[0.5, -0.4, 2.9], [-0.7, 0.3, -1.9], [0.3, 0.6, -2.0]], (3, 3, 3), (20, 20, 20))

    # T4: a waypoint on a cell that only the exemption keeps open
    sh4, res4 = (24, 24, 24), (0.04, 0.05, 0.025)
    b4, h4 = np.array(b2[:2]), np.array(h2[:2])
    free = tcase(sh4, res4, b4, h4, far(sh4), far(sh4))["tunnel"]
    assert free[far(sh4)[1], far(sh4)[0], far(sh4)[2]] == 10
    ev = _event_nodes(RAD, sh4, res4, b4, h4)
    key = lambda a: {tuple(int(x) for x in r) for r in a  # noqa: E731
                     if all(1 <= r[k] < sh4[k] - 1 for k in range(3))}
    sets = {k: key(ev[k]) for k in ("wall", "back", "cap")}
    for kind, which in (("cap", "fw"), ("back", "iw"), ("wall", "fw")):
        only = sorted(sets[kind] - set().union(*(sets[o] for o in sets if o != kind)))
        cell = only[len(only) // 2]
        assert np.isinf(free[cell[1], cell[0], cell[2]])
        c = tcase(sh4, res4, b4, h4, cell if which == "fw" else far(sh4), cell if which == "iw" else far(sh4))
        got = c["tunnel"][cell[1], cell[0], cell[2]]
        assert got != free[cell[1], cell[0], cell[2]], (kind, cell)  # the exemption decided this value
        assert (c["tunnel"] != free).sum() == 1
        print(f"T4{kind}: {which} = {cell}: free inf -> {got}", flush=True)
        T["T4" + kind] = c

    # T5: wholly outside; T7: beyond int64 (Python ints do not overflow: all 10)
    T["T5"] = tcase(sh4, res4, b4 + 10.0, h4, (5, 5, 5), (6, 6, 6))
    for tag, v in (("a", 1e300), ("b", -1e300)):
        b = b4.copy()
        b[:, 0] = v
        T["T7" + tag] = tcase(sh4, res4, b, h4, (5, 5, 5), (6, 6, 6))
    for k in ("T5", "T7a", "T7b"):
        assert (T[k]["tunnel"] == 10).all()
    b = b4.copy()
    b[1, 1] = 1e300  # the last point alone: the first point's events and the back closure remain
    T["T7c"] = tcase(sh4, res4, b, h4, (5, 5, 5), (6, 6, 6))
    assert T["T7c"]["err"] == "" and not (T["T7c"]["tunnel"] == 10).all()

    # T6: a volume smaller than the tunnel: events fall off every face
    sh6, res6 = (12, 12, 12), (0.04, 0.05, 0.04)
    b6, h6 = np.array([[0.24, -0.03, 0.24], [0.24, 0.55, 0.24]]), np.array([[0.0, 0.0, math.pi / 2]] * 2)
    e6 = _event_nodes(RAD, sh6, res6, b6, h6)["all"]
    assert all(e6[:, k].min() < 0 and e6[:, k].max() >= sh6[k] for k in range(3))
    T["T6"] = tcase(sh6, res6, b6, h6, (5, 5, 5), (6, 6, 6))

    # T8: non-finite base points and headings
    for tag, (arr, idx, v) in (("a", ("b", (0, 1), np.nan)), ("b", ("b", (1, 2), np.inf)), ("c", ("h", (1, 2), np.nan))):
        b, h = b4.copy(), h4.copy()
        (b if arr == "b" else h)[idx] = v
        T["T8" + tag] = tcase(sh4, res4, b, h, (5, 5, 5), (6, 6, 6))
        assert T["T8" + tag]["err"] != ""
    b = b4.copy()
    b[1, 1] = 1e308  # finite, but 1e308 / resY is not: OverflowError from a finite input
    T["T8d"] = tcase(sh4, res4, b, h4, (5, 5, 5), (6, 6, 6))
    assert T["T8d"]["err"] == "OverflowError"

    # ---- GetObstMap
    shG, resG = (12, 12, 12), (0.05, 0.05, 0.04)
    Z, ob = dem(12, 12, -0.1, 0.3)
    G["G1"] = gcase(Z, ob, resG, shG)  # negative indices wrap
    assert np.rint(Z / 0.04).min() < 0
    G["G2"] = gcase(Z - 1.0, ob, resG, shG)  # below -sZ: IndexError
    G["G3"] = gcase(Z + 0.3, ob, resG, shG)  # some iz >= sZ: skipped
    assert (np.rint((Z + 0.3) / 0.04) >= 12).any() and (np.rint((Z + 0.3) / 0.04) < 12).any()
    G["G4a"] = gcase(Z, ob, resG, shG, xm=0.05 * 3, ym=7.891)
    G["G4b"] = gcase(Z, ob, resG, shG, xm=12.3456, ym=0.05 * 7)
    G["G4c"] = gcase(Z, ob, resG, shG, xm=0.05 * 3, ym=0.05 * 7)
    G["G4d"] = gcase(Z, ob, resG, shG)
    G["G5a"] = gcase(*dem(16, 20, -0.05, 0.3, 1), resG, shG)
    G["G5b"] = gcase(*dem(7, 5, -0.05, 0.3, 2), resG, shG)
    ob6 = ob.copy()
    ob6[2, :] = 2.0
    ob6[5, :] = np.nan
    ob6[8, :] = 0.9999999
    ob6[9, :] = 1.0
    G["G6"] = gcase(Z, ob6, resG, shG)
    Z7 = np.empty((12, 12))
    Z7[:] = (np.arange(-3, 9) + 0.5)[None, :] * 0.03125  # exact halves: round half to even
    G["G7"] = gcase(Z7, ob, (0.05, 0.05, 0.03125), shG)
    G["G8a"] = gcase([[0.0]], [[1.0]], resG, (1, 1, 1))
    G["G8b"] = gcase(*dem(3, 3, 0.0, 0.04, 3), resG, (3, 3, 2))
    for tag, (j, i, v) in (("a", (4, 6, np.nan)), ("b", (7, 2, np.inf))):
        Z9 = Z.copy()
        Z9[j, i] = v
        G["G9" + tag] = gcase(Z9, ob, resG, shG)
    Z9, ob9 = dem(16, 20, -0.05, 0.3, 1)
    Z9[14, 18] = np.nan  # outside the volume's extent: converted before the bounds test (:334-335)
    G["G9c"] = gcase(Z9, ob9, resG, shG)
    Z9 = Z.copy()
    Z9[5, 3] = np.nan  # in the column the xm test skips
    G["G9d"] = gcase(Z9, ob, resG, shG, xm=0.05 * 3, ym=7.891)
    Z9 = Z.copy()
    Z9[7, 4] = np.inf  # in the row the ym test skips
    G["G9e"] = gcase(Z9, ob, resG, shG, xm=12.3456, ym=0.05 * 7)
    Z9 = Z.copy()
    Z9[2, 9] = -1e308  # finite, but the quotient by resZ is -inf
    G["G9f"] = gcase(Z9, ob, resG, shG)
    assert G["G9f"]["err"] == "OverflowError"
    for tag, v in (("a", 1e300), ("b", -1e300)):
        Z10 = Z.copy()
        Z10[6, 6] = v
        G["G10" + tag] = gcase(Z10, ob, resG, shG)
    for k in ("G2", "G9a", "G9b", "G9c", "G10b"):
        assert G[k]["err"] != "", k
    for k in ("G1", "G3", "G9d", "G9e", "G10a"):
        assert G[k]["err"] == "", k

    # the chain test's DEMs on T1's and T2b's volumes (waypoints: those cases' own)
    for k, t, seed in (("C1", "T1", 4), ("C2", "T2b", 5)):
        Zc, oc = dem(24, 24, 0.0, 0.1, seed)
        G[k] = gcase(Zc, oc, tuple(T[t]["vol"][3:6]), tuple(int(v) for v in T[t]["vol"][:3]))
    return T, G


def write_cases():
    T, G = crafted_cases()
    # vol: (sX, sY, sZ, resX, resY, resZ[, xm, ym]); err: the class the reference raised, "" if none
    out = {"t_names": np.array(sorted(T)), "g_names": np.array(sorted(G)), "t_radii": np.array(RAD)}
    out["t_err"] = np.array([T[k].pop("err") for k in sorted(T)])
    out["g_err"] = np.array([G[k].pop("err") for k in sorted(G)])
    print(dict(zip(sorted(T), out["t_err"])), dict(zip(sorted(G), out["g_err"])), sep="\n", flush=True)
    for cases in (T, G):
        for name, c in cases.items():
            for k, v in c.items():
                out[f"{name}_{k}"] = v
    path = os.path.join(OUT, "arm_cases.npz")
    np.savez_compressed(path, **out)
    with np.load(path, allow_pickle=False) as d:  # data only
        assert all(d[k].dtype.kind in "fuU" for k in d.files)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if sys.argv[1:] == ["cases"]:
        write_cases()
        sys.exit(0)
    out = {}
    for i, (seed, half, grid) in enumerate([(1, 16, False), (2, 20, True), (3, 24, False)]):
        c = case(seed, half, sample_on_grid=grid)
        for k, v in c.items():
            out[f"a{i}_{k}"] = v
        print(i, c["shape"], "tunnel finite/inf/10:", int(np.isfinite(c["tunnel"]).sum()),
              int(np.isinf(c["tunnel"]).sum()), int((c["tunnel"] == 10).sum()), flush=True)
    np.savez_compressed(os.path.join(OUT, "arm.npz"), **out)
