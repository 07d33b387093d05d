"""Goal sets for 3D solves at the C-ABI boundary and their CPU references, no GPU.

The four entry points are declared in include/eikonal.h, exported by the built library and bound by
eikonal._lib.  tests/seeds3d_np.py holds the specification in numpy (`jacobi3`, `seeded_reference3`,
`label_rule3`, `undominated3`); here it is checked against the oracle and against itself.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import handoff3d as HO
from eikonal import _lib as L
from seeds3d_np import (FIVE_SEEDS, FIVE_SHAPE, FIVE_T0, FIVE_UNDOMINATED, jacobi3, label_rule3, seeded_reference3,
                        undominated3)
from test_seeds_abi import raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# parameters per function, from the issue's prototypes
NARGS = {"eik_fim3d_solve_seeds": 11, "eik_labels3d_dev": 11, "eik_tmap3d_seeds_f32": 10, "eik_tmap3d_seeds_f64": 10}
NAMES = list(NARGS)


# ------------------------------------------------------------------------------- the ABI
def test_declared_in_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eikonal.h")).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == NARGS[name], name


def test_label_rule_is_in_the_header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    flat = " ".join(src.replace("*", " ").split())
    at = flat.index("Goal sets for 3D solves")
    text = flat[at:flat.index("int eik_fim3d_solve_seeds", at)]
    for phrase in ("T[c] == (R)t0_k bit for bit", "the lowest wins", "6-neighbour with the smallest T strictly below T[c]",
                   "x-1, x+1, y-1, y+1, z-1, z+1", "label = -1", "3D replanning", "B > 1", "the layered solver",
                   "early exit with a seed set"):
        assert phrase in text, phrase


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
    import FastMarching.FastMarching3D as FM3

    for m in ("tmap3d_seeds", "fim3d_solve_seeds", "labels3d"):
        assert callable(getattr(L.Context, m)), m
    assert callable(FM3.computeTmapMulti) and callable(FM3.getPathsToNearest)
    assert "computeTmapMulti" in FM3.__doc__ and "getPathsToNearest" in FM3.__doc__


def test_seed_arrays_are_checked_on_the_host():
    s, t, K = L._seeds3([(1, 2, 3), (4, 5, 6)], None)
    assert K == 2 and t is None and s.dtype == np.int64 and s.tolist() == [[1, 2, 3], [4, 5, 6]]
    assert s.flags["C_CONTIGUOUS"]
    s, t, K = L._seeds3(np.array([[1, 2, 3]], np.int32), [0.5])
    assert K == 1 and s.dtype == np.int64 and t.dtype == np.float64 and t.tolist() == [0.5]
    for bad in ([(1, 2), (3, 4)], [1, 2, 3], [[(1, 2, 3)]], [(1, 2, 3, 4)], []):
        with pytest.raises(ValueError):
            L._seeds3(bad, None)
    with pytest.raises(ValueError):
        L._seeds3([(1, 2, 3), (4, 5, 6)], [0.0])
    with pytest.raises(ValueError):
        L._seeds3([(1, 2, 3)], [0.0, 1.0])


# ------------------------------------------------------------------------------- the drop-in's mask form
def test_mask_to_goal_list_is_row_major_and_checks_the_shape_first():
    import FastMarching.FastMarching3D as FM3

    m = np.zeros((4, 5, 3), bool)
    m[3, 1, 0] = m[0, 4, 2] = m[0, 4, 1] = m[0, 2, 2] = m[2, 0, 1] = True
    g = FM3._goal_list(m, (4, 5, 3))
    # (x, y, z): rows (y) first, then x, then z
    assert g.dtype == np.int64 and g.tolist() == [[2, 0, 2], [4, 0, 1], [4, 0, 2], [0, 2, 1], [1, 3, 0]]
    assert FM3._goal_list([(3, 2, 1), (1, 2, 0)], (4, 5, 3)).tolist() == [[3, 2, 1], [1, 2, 0]]
    assert FM3._goal_list(np.array([[3.0, 2.0, 1.0, 9.0]]), (4, 5, 3)).tolist() == [[3, 2, 1]]
    cost = np.ones((4, 5, 3))
    with pytest.raises(ValueError):
        FM3.computeTmapMulti(cost, np.zeros((5, 4, 3), bool))  # before anything runs
    with pytest.raises(ValueError):
        FM3.computeTmapMulti(cost, np.zeros((4, 5, 3), bool))  # no goal
    with pytest.raises(ValueError):
        FM3.computeTmapMulti(cost, [1, 2, 3])
    with pytest.raises(ValueError):
        FM3.computeTmapMulti(cost, [(1, 2)])
    with pytest.raises(ValueError):
        FM3.getPathsToNearest(np.zeros((4, 5, 3)), np.zeros((5, 4, 3), np.int32), [(1, 1, 1)], [(2, 2, 2)], 0.5)
    lab = np.zeros((4, 5, 3), np.int32)
    lab[3] = -1
    with pytest.raises(ValueError, match="start 1"):  # an unlabelled start, before anything runs
        FM3.getPathsToNearest(np.zeros((4, 5, 3)), lab, [(1, 1, 1)], [(2, 2, 2), (3, 3, 1)], 0.5)


# ------------------------------------------------------------------------------- jacobi3 against the oracle
ORACLE_CASES = [((24, 48, 24), (24, 12, 12)), ((17, 33, 9), (5, 5, 4)), ((33, 35, 3), (16, 16, 1)), ((20, 40, 41), (3, 3, 3))]


@pytest.mark.parametrize("shape,goal", ORACLE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_jacobi3_with_one_seed_is_the_oracle_field(shape, goal):
    cost = HO.cut_cost3(shape, goal)
    R = HO.oracle_field(("seeds3d", shape, goal), cost, goal)
    n = []
    T0 = np.full(shape, np.inf)
    T0[goal[1], goal[0], goal[2]] = 0.0
    T = jacobi3(T0, cost, n)
    assert np.array_equal(T, seeded_reference3(cost, [goal], [0.0]))
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    err = np.abs(T[fin] - R[fin]).max()
    print(f"{shape}: {n[0]} iterations, max abs err {err:.3e}")
    assert err <= 1e-9, err


# ------------------------------------------------------------------------------- the five seeds
@functools.lru_cache(maxsize=None)
def five():
    cost = raster(FIVE_SHAPE)
    R = seeded_reference3(cost, FIVE_SEEDS, FIVE_T0)
    R.setflags(write=False)
    return cost, R


def test_five_seed_reference_and_label_rule_agree():
    cost, R = five()
    assert np.isfinite(R).all()
    und = undominated3(R, FIVE_SEEDS, FIVE_T0)
    assert und == FIVE_UNDOMINATED == [True, True, False, True, False]
    assert R[2, 30, 12] < 1e4 and R[7, 15, 7] < 40.0  # (30, 2, 12) and (15, 7, 7) are dominated
    lab = label_rule3(R, FIVE_SEEDS, FIVE_T0)
    assert (lab >= 0).all(), "every finite cell is labelled"
    for k, (x, y, z) in enumerate(FIVE_SEEDS):
        assert (lab[y, x, z] == k) == und[k], k
    assert set(np.unique(lab)) == {0, 1, 3}
    # a label's cells hold no less than the seed's own start value
    assert (R >= np.asarray(FIVE_T0)[lab]).all()


def test_joint_field_lies_below_the_minimum_of_the_single_fields():
    """why the seeds are solved as one problem: the issue's prototype found 8.4 % of the
    cells more than 1e-9 below the minimum of the five single-seed fields, by up to 1.89"""
    cost, R = five()
    singles = np.minimum.reduce([seeded_reference3(cost, [s], [v]) for s, v in zip(FIVE_SEEDS, FIVE_T0)])
    assert (R <= singles + 1e-9).all()
    gap = singles - R
    print(f"{(gap > 1e-9).mean():.4f} of the cells below, by up to {gap.max():.3f}")
    assert (gap > 1e-9).mean() > 0.01


# ------------------------------------------------------------------------------- the label rule's branches
def test_label_rule_branches():
    T = np.empty((2, 5, 2))
    T[:, :, 0] = [[2.0, 1.0, 2.0, np.inf, 7.0],
                  [3.0, 2.0, 2.0, np.inf, 7.0]]
    T[:, :, 1] = [[3.0, 2.0, 2.5, np.inf, 7.0],
                  [3.0, 3.0, 2.5, 9.0, 8.0]]
    # seed 0 on (1, 0, 0) holds its t0; seed 1 on (2, 0, 0) was undercut (T = 2 < 5: no root); seeds 2 and 3
    # share (4, 0, 0) at one t0: the lowest k wins
    lab = label_rule3(T, [(1, 0, 0), (2, 0, 0), (4, 0, 0), (4, 0, 0)], [1.0, 5.0, 7.0, 7.0])
    # layer 0 -- (2, 1, 0): neighbours x-1 = 2, y-1 = 2, z+1 = 2.5, none strictly lower -> -1; (4, 1, 0): a
    # plateau beside a root -> -1; +inf -> -1
    assert lab[:, :, 0].tolist() == [[0, 0, 0, -1, 2], [0, 0, -1, -1, -1]]
    # layer 1 -- (0, 1, 1) = 3: x+1 = 3, y-1 = 3, z-1 = 3: a plateau -> -1; (1, 1, 1) = 3: y-1 = 2 and z-1 = 2
    # tie, y-1 is first in the order -> (1, 0, 1) -> 0; (2, 0, 1) = 2.5: x-1 = 2 and z-1 = 2 tie, x-1 is
    # first -> (1, 0, 1) -> 0; (2, 1, 1) = 2.5: z-1 = (2, 1, 0), unlabelled -> -1; (3, 1, 1) = 9: x-1 = 2.5
    # is the lowest -> (2, 1, 1) -> -1 (a chain that ends in a plateau); (4, 1, 1) = 8: y-1 = 7 and z-1 = 7
    # tie, y-1 first -> (4, 0, 1) = 7, itself a plateau beside the root -> -1
    assert lab[:, :, 1].tolist() == [[0, 0, 0, -1, -1], [-1, 0, -1, -1, -1]]
    # the tie order decides the label: two roots, the cell between them equally far from both
    T = np.array([[[1.0], [2.0], [1.0]]])  # H = 1, W = 3, L = 1
    assert label_rule3(T, [(0, 0, 0), (2, 0, 0)], [1.0, 1.0])[0, :, 0].tolist() == [0, 0, 1]  # x-1 before x+1
    T = np.array([[[1.0, 2.0, 1.0]]])      # along z
    assert label_rule3(T, [(0, 0, 0), (0, 0, 2)], [1.0, 1.0])[0, 0].tolist() == [0, 0, 1]     # z-1 before z+1
    T = np.array([[[5.0, 1.0]], [[2.0, 9.0]], [[1.0, 9.0]]])  # (0, 1, 0) = 2: y+1 = 1 beats y-1 = 5
    assert label_rule3(T, [(0, 0, 1), (0, 2, 0)], [1.0, 1.0])[:, 0, 0].tolist() == [0, 1, 1]
    # float32 fields take (R)t0
    T32 = np.array([[[np.float32(0.1), np.float32(0.3)]]], np.float32)
    assert label_rule3(T32, [(0, 0, 0)], [0.1]).tolist() == [[[0, 0]]]
