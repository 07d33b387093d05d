"""Multi-source solves at the C-ABI boundary and their CPU references, no GPU.

The five entry points are declared in include/eikonal.h, exported by the built library and bound by
eikonal._lib.  `seeded_reference` (the expected field of a seed set: the fixed point from above of
T = min(T, godunov), tests/test_replan_rule.jacobi) and `label_rule` (the label rule of eikonal.h in
numpy) are what tests/test_gpu_seeds.py compares the device with; here they are checked against each
other.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from eikonal import _lib as L
from test_replan_rule import jacobi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eik_fim2d_start_seeds", "eik_fim2d_solve_seeds", "eik_labels2d_dev", "eik_tmap2d_seeds_f32",
         "eik_tmap2d_seeds_f64"]
# parameters per function, from the issue's prototypes
NARGS = {"eik_fim2d_start_seeds": 8, "eik_fim2d_solve_seeds": 8, "eik_labels2d_dev": 12, "eik_tmap2d_seeds_f32": 9,
         "eik_tmap2d_seeds_f64": 9}


# ------------------------------------------------------------------------------- references
def raster(shape, seed=7):
    """U(1, 10) rounded to fp32, so both dtypes solve the same costs (as tests/test_gpu_replan.raster)"""
    return np.random.default_rng(seed).uniform(1, 10, shape).astype(np.float32).astype(np.float64)


def seeded_reference(cost, seeds, t0=None):
    """The field of the seed set: jacobi from T_init = +inf with the seeds at the min of their T0"""
    T = np.full(cost.shape, np.inf)
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    for (x, y), v in zip(seeds, t0):
        T[y, x] = min(T[y, x], v)
    return jacobi(T, np.asarray(cost, np.float64))


def label_rule(T, seeds, t0=None):
    """The label rule of include/eikonal.h on one field T (H x W, any float dtype), in numpy: roots
    first, then every cell in ascending T takes the label of its strictly lowest 4-neighbour, ties in
    the order x-1, x+1, y-1, y+1 (a parent is strictly lower, so it is labelled before its child)."""
    H, W = T.shape
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    t0 = t0.astype(T.dtype)  # (R)t0
    lab = np.full(H * W, -1, np.int32)
    root = np.zeros(H * W, bool)
    for k in reversed(range(len(seeds))):  # of several roots on a cell the lowest k wins
        x, y = seeds[k]
        if T[y, x] == t0[k]:  # (non-negative, never NaN: == is equality of the bit patterns)
            lab[y * W + x] = k
            root[y * W + x] = True
    P = np.full((H + 2, W + 2), np.inf, T.dtype)
    P[1:-1, 1:-1] = T
    nb = np.stack([P[1:-1, :-2], P[1:-1, 2:], P[:-2, 1:-1], P[2:, 1:-1]])  # x-1, x+1, y-1, y+1
    best = nb.argmin(axis=0)  # the first of equal minima
    has = (np.isfinite(T) & (nb.min(axis=0) < T)).ravel() & ~root
    par = np.arange(H * W) + np.array([-1, 1, -W, W])[best.ravel()]
    for i in np.argsort(T.ravel(), kind="stable"):
        if has[i]:
            lab[i] = lab[par[i]]
    return lab.reshape(H, W)


def undominated(R, seeds, t0=None):
    """per seed: the reference field holds the lowest T0 named for its cell, and it is this seed's"""
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    return [bool(R[y, x] == v) for (x, y), v in zip(seeds, t0)]


FIVE_SHAPE = (190, 170)
FIVE_SEEDS = [(20, 30), (150, 160), (63, 64), (64, 64), (100, 5)]
FIVE_T0 = [0.0, 12.5, 40.0, 3.0, 1e4]


# ------------------------------------------------------------------------------- the ABI
def _header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_declared_in_header():
    src = _header()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == NARGS[name], name


def test_label_rule_is_in_the_header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("T[c] == (R)t0_k bit for bit", "the lowest wins", "smallest T strictly below T[c]",
                   "x-1, x+1, y-1, y+1", "label = -1"):
        assert phrase in flat, phrase


def test_exported_by_library():
    lib = ctypes.CDLL(L.LIB_PATH)
    missing = [n for n in NAMES if not hasattr(lib, n)]
    assert not missing, missing


def test_bound_with_argtypes():
    lib = L.lib()
    for name in NAMES:
        assert name in L.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == NARGS[name], name


def test_methods_present():
    import FastMarching.FastMarching as FM

    for m in ("tmap2d_seeds", "labels2d"):
        assert callable(getattr(L.Context, m)), m
    for m in ("start_seeds", "solve_seeds"):
        assert callable(getattr(L.Fim2d, m)), m
    assert callable(FM.computeTmapMulti) and callable(FM.getPathsToNearest)


def test_seed_arrays_are_checked_on_the_host():
    s, t, m, K = L._seeds([(1, 2), (3, 4)], None)
    assert K == 2 and t is None and m is None and s.dtype == np.int64 and s.tolist() == [[1, 2], [3, 4]]
    s, t, m, K = L._seeds(np.array([[1, 2]]), [0.5], [0])
    assert t.dtype == np.float64 and m.dtype == np.int32
    with pytest.raises(ValueError):
        L._seeds([(1, 2), (3, 4)], [0.0])
    with pytest.raises(ValueError):
        L._seeds([(1, 2), (3, 4)], None, [0])


# ------------------------------------------------------------------------------- the drop-in's mask form
def test_mask_to_goal_list_is_row_major_and_checks_the_shape_first():
    import FastMarching.FastMarching as FM

    m = np.zeros((5, 7), bool)
    m[3, 1] = m[0, 6] = m[0, 2] = m[4, 0] = True
    g = FM._goal_list(m, (5, 7))
    assert g.dtype == np.int64 and g.tolist() == [[2, 0], [6, 0], [1, 3], [0, 4]]  # (x, y), rows first
    assert FM._goal_list([(3, 4), (1, 2)], (5, 7)).tolist() == [[3, 4], [1, 2]]
    assert FM._goal_list(np.array([[3.0, 4.0, 9.0]]), (5, 7)).tolist() == [[3, 4]]
    cost = np.ones((5, 7))
    with pytest.raises(ValueError):
        FM.computeTmapMulti(cost, np.zeros((7, 5), bool))  # before anything runs
    with pytest.raises(ValueError):
        FM.computeTmapMulti(cost, np.zeros((5, 7), bool))  # no goal
    with pytest.raises(ValueError):
        FM.computeTmapMulti(cost, [1, 2])
    with pytest.raises(ValueError):
        FM.getPathsToNearest(np.zeros((5, 7)), np.zeros((7, 5), np.int32), [(1, 1)], [(2, 2)], 0.5)
    with pytest.raises(ValueError, match="start 1"):  # an unlabelled start, before anything runs
        FM.getPathsToNearest(np.zeros((5, 7)), np.array([[0] * 7] * 4 + [[-1] * 7]), [(1, 1)], [(2, 2), (3, 4)], 0.5)


# ------------------------------------------------------------------------------- the references
def test_five_seed_reference_and_label_rule_agree():
    cost = raster(FIVE_SHAPE)
    R = seeded_reference(cost, FIVE_SEEDS, FIVE_T0)
    assert np.isfinite(R).all()
    und = undominated(R, FIVE_SEEDS, FIVE_T0)
    assert und == [True, True, False, True, False]
    assert R[5, 100] < 1e4 and R[64, 63] < 40.0  # (100, 5) and (63, 64) are dominated
    lab = label_rule(R, FIVE_SEEDS, FIVE_T0)
    assert (lab >= 0).all(), "every finite cell is labelled"
    for k, (x, y) in enumerate(FIVE_SEEDS):
        assert (lab[y, x] == k) == und[k], k
    assert lab[64, 63] == 3  # undercut from across the tile boundary
    assert set(np.unique(lab)) == {0, 1, 3}
    # a label's cells hold no less than the seed's own field would allow: T >= t0 of the label
    assert (R >= np.asarray(FIVE_T0)[lab]).all()


def test_joint_field_lies_below_the_minimum_of_the_single_fields():
    """why the seeds are solved as one problem"""
    cost = raster(FIVE_SHAPE)
    R = seeded_reference(cost, FIVE_SEEDS, FIVE_T0)
    singles = np.minimum.reduce([seeded_reference(cost, [s], [v]) for s, v in zip(FIVE_SEEDS, FIVE_T0)])
    assert (R <= singles + 1e-9).all()
    assert ((singles - R) > 1e-9).mean() > 0.01


def test_label_rule_branches():
    T = np.array([[2.0, 1.0, 2.0, np.inf, 7.0],
                  [3.0, 2.0, 2.0, np.inf, 7.0]])
    # seed 0 on (1, 0) holds its T0; seed 1 on (2, 0) was undercut (T = 2 < 5); seeds 2 and 3 share (4, 0)
    lab = label_rule(T, [(1, 0), (2, 0), (4, 0), (4, 0)], [1.0, 5.0, 7.0, 7.0])
    # (2, 1): neighbours x-1 = 2, y-1 = 2, none strictly lower -> -1; (4, 1): a plateau beside a root -> -1
    assert lab.tolist() == [[0, 0, 0, -1, 2], [0, 0, -1, -1, -1]]
