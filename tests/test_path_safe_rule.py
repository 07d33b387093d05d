"""The obstacle-safe 2D path rule on the host (tests/path_safe_np.py, the specification gdm_safe.hip is
tested against in tests/test_gpu_path_safe.py) and its entry points at the C-ABI boundary.  No GPU.

Rasters as the rule's issue built them, 64 x 64 from np.random.default_rng(seed): the cost of one kind
(uniform 1, U(1, 10), exp(N(0, 1.5))), obstacles cost[rng.random((64, 64)) < d] = inf, an inf border,
cost[7:10, 7:10] = 1; goal (8, 8); seven starts, those with finite T.  Seeds 0-7, d in {0, 0.1, 0.2,
0.3}, tau 0.5 and 0.25: 1160 walks (the count is asserted).
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle as O
import path_safe_np as S
from eikonal import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOAL = (8, 8)
STARTS = [(56, 56), (33, 30), (50, 12), (12, 55), (36, 31), (29, 40), (61, 3)]
KINDS = ("uniform", "u1_10", "lognormal")


def POW(v):  # the reference's numpy-scalar x**2 goes through libm pow()
    return math.pow(v, 2)


def _fmm(cost, goal):
    O.set_strict(False)  # uniform rasters tie
    try:
        return O.fmm2d(cost, goal)
    finally:
        O.set_strict(True)


def _raster(kind, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        cost = np.ones((64, 64))
    elif kind == "u1_10":
        cost = rng.uniform(1, 10, (64, 64))
    else:
        cost = np.exp(rng.normal(0, 1.5, (64, 64)))
    cost[rng.random((64, 64)) < d] = np.inf
    cost[0, :] = cost[-1, :] = cost[:, 0] = cost[:, -1] = np.inf
    cost[7:10, 7:10] = 1
    return cost


@pytest.fixture(scope="module")
def fields():
    """(kind, d, seed) -> (T, SafeField on the oracle's gradient), computed once"""
    out = {}
    for kind in KINDS:
        for d in (0, 0.1, 0.2, 0.3):
            for seed in range(8):
                T = _fmm(_raster(kind, d, seed), GOAL)
                out[kind, d, seed] = (T, S.SafeField(T, O.gradient2d(T)))
    return out


def _length(p):
    return float(np.hypot(*(p[1:] - p[:-1]).T).sum())


def test_reaches_the_goal(fields):
    walks = 0
    bad = []
    for key, (T, f) in fields.items():
        for tau in (0.5, 0.25):
            for s in STARTS:
                if not np.isfinite(T[s[1], s[0]]):
                    continue
                walks += 1
                p, st, info = S.safe_path(f, s, GOAL, tau, sq=POW)
                body = p[:-1]  # without the final jump to `end`
                mids = (body[:-1] + body[1:]) / 2
                seg = np.hypot(*(body[1:] - body[:-1]).T)
                if (st != S.DONE or S.nearest_is_inf(T, p).any() or S.nearest_is_inf(T, mids).any()
                        or (len(seg) and seg.max() > 1.5)):
                    bad.append((key, s, tau, st, info.tolist()))
    assert walks == 1160
    assert not bad, bad[:5]


def test_stall_rule_is_what_ends_rough_walks(fields):
    """without the rule the log-normal walks run out their budget; with it they end DONE in integer mode"""
    T, f = fields["lognormal", 0, 0]
    p, st, info = S.safe_path(f, (56, 56), GOAL, 0.5)
    assert st == S.DONE and info[2] >= 0 and info[3] < 2000
    _, st0, info0 = S.safe_path(f, (56, 56), GOAL, 0.5, stall=False)
    assert st0 == S.STUCK and info0[2] == -1 and info0[3] == 30000


def _wall(x0, x1):
    cost = np.ones((64, 64))
    cost[12:52, x0:x1] = np.inf
    cost[0, :] = cost[-1, :] = cost[:, 0] = cost[:, -1] = np.inf
    return _fmm(cost, GOAL)


def test_thin_wall():
    T = _wall(30, 31)
    start = (33, 30)
    r, rst = O.gdm2d(T, np.array(start, float), np.array(GOAL, float), 0.5)
    assert rst == S.DONE and S.nearest_is_inf(T, r).sum() >= 1 and np.isinf(T[np.rint(r[:, 1]).astype(int), np.rint(r[:, 0]).astype(int)]).any()
    assert _length(r) < T[start[1], start[0]] * 0.95  # the reference's walk tunnels
    p, st, _ = S.safe_path(S.SafeField(T, O.gradient2d(T)), start, GOAL, 0.5, sq=POW)
    assert st == S.DONE and not S.nearest_is_inf(T, p).any()
    assert _length(p) >= T[start[1], start[0]] * 0.95


def test_thick_wall():
    T = _wall(29, 32)
    start = (36, 31)
    _, rst = O.gdm2d(T, np.array(start, float), np.array(GOAL, float), 0.5)
    assert rst == S.FALLBACK
    p, st, info = S.safe_path(S.SafeField(T, O.gradient2d(T)), start, GOAL, 0.5, sq=POW)
    assert st == S.DONE and info[0] >= 1 and not S.nearest_is_inf(T, p).any()


def test_identity_to_the_reference(fields):
    """no obstacles (beyond the border): the safe walk is oracle.gdm2d's, bit for bit, wherever that walk
    is DONE with fewer than 4000 points"""
    compared = 0
    for kind in ("uniform", "u1_10"):
        for seed in range(8):
            T, f = fields[kind, 0, seed]
            for s in STARTS:
                r, rst = O.gdm2d(T, np.array(s, float), np.array(GOAL, float), 0.5)
                if rst != S.DONE or len(r) >= 4000:
                    continue
                compared += 1
                p, st, info = S.safe_path(f, s, GOAL, 0.5, sq=POW)
                assert st == S.DONE and p.shape == r.shape and np.array_equal(p, r), (kind, seed, s, info.tolist())
    assert compared >= 100


def test_default_squares_stay_within_the_walkers_tolerance(fields):
    """the kernel's exact products against the reference's pow(): the 1e-9 cells the 2D walker is held to"""
    T, f = fields["u1_10", 0.1, 3]
    g = S.SafeField(T)  # path_safe_np's own gradient, exact products
    for s in STARTS:
        if np.isfinite(T[s[1], s[0]]):
            a, sa, ia = S.safe_path(f, s, GOAL, 0.5, sq=POW)
            b, sb, ib = S.safe_path(g, s, GOAL, 0.5)
            assert sa == sb and a.shape == b.shape and np.array_equal(ia, ib) and np.abs(a - b).max() <= 1e-9


def test_unit_cases():
    T = _wall(29, 32)
    # a start on an impassable node: the fallback drops it and nothing is left
    p, st, info = S.safe_path(T, (30.0, 30.0), GOAL, 0.5)
    assert st == S.ERROR and len(p) == 0 and info.tolist() == [1, 1, -1, 1]
    # a plateau pit away from the goal: the walk sinks into it and no neighbour is lower
    yy, xx = np.mgrid[0:48, 0:48]
    pit = 10.0 + np.hypot(xx - 30.0, yy - 30.0)
    pit[29:32, 29:32] = 10.0
    p, st, info = S.safe_path(pit, (38.0, 30.0), (5.0, 5.0), 0.5)
    assert st == S.STUCK and 29 <= p[-1, 0] <= 31 and 29 <= p[-1, 1] <= 31 and info[3] < 200
    p, st, info = S.safe_path(pit, (30.0, 30.0), (5.0, 5.0), 0.5)  # 0/0 gradient on the plateau
    assert st == S.STUCK and p.tolist() == [[30.0, 30.0]] and info.tolist() == [1, 1, -1, 1]
    with pytest.raises(ValueError):
        S.safe_path(T, (36.0, 31.0), GOAL, 1.01)
    import FastMarching.FastMarching as FM

    for fn in (lambda: FM.getPathSafe(T, (36.0, 31.0), GOAL, 1.01), lambda: FM.getPathsSafe(T, [(36.0, 31.0)], GOAL, 1.01)):
        with pytest.raises(ValueError):  # before any GPU call
            fn()
    assert S.stall_limit(0.5) == 16 and S.stall_limit(0.25) == 32 and S.stall_limit(1.0) == 16


# ------------------------------------------------------------------ the C-ABI boundary, no GPU
NARGS = {"eik_path2d_safe_dev": 14, "eik_path2d_safe_f64": 12, "eik_path2d_safe_batch_dev": 17,
         "eik_path2d_safe_batch_f64": 15}


def test_declared_in_header():
    raw = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in NARGS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    assert re.search(r"\bEIK_PATH_STUCK\s*=\s*3\b", src)
    # what the header's comment has to tell a caller
    for words in ("tau <= 0.5", "NOT swept", "up to the first blocked step or stall"):
        assert words in raw, words


def test_exported_and_bound():
    cdll = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    for name, nargs in NARGS.items():
        assert hasattr(cdll, name), name
        assert name in L.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    assert L.PATH_STUCK == 3


def test_methods_present():
    import inspect

    import FastMarching.FastMarching as FM

    for m in ("path2d_safe", "path2d_safe_batch"):
        assert callable(getattr(L.Context, m)), m
    assert callable(FM.getPathSafe) and callable(FM.getPathsSafe)
    assert inspect.signature(FM.getPathsToNearest).parameters["safe"].default is False
