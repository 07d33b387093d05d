"""The seeded re-solve at the C-ABI boundary, no GPU: the five entry points are
declared in include/eikonal.h with the issue's parameter counts, exported by the built library and bound
by eikonal._lib; the rule stands in the header; the drop-in checks its arguments before any device work.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from eikonal import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"eik_fim2d_adopt_seeds": 7, "eik_fim2d_update_seeds": 8, "eik_fim2d_resolve_seeds": 8,
         "eik_tmap2d_update_seeds_f32": 15, "eik_tmap2d_update_seeds_f64": 15}


def test_declared_in_header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n in NARGS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n, name


def test_the_rule_is_in_the_header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("T_old[c] == b_old(c) bit for bit", "An old root with b_new(c) <= b_old(c)",
                   "An old root with b_new(c) > b_old(c), where removal means +inf", "p not a spared root",
                   "T[c] = min(T[c], b_new(c)) at every new seed", "supersolution of the new problem",
                   "added seeds and lowered t0 need no reset", "the list stays as it is",
                   "the bound solve has a single goal: eik_fim2d_update, or eik_fim2d_adopt_seeds first",
                   "may read +inf", "the bound solve has a seed set"):
        assert phrase in flat, phrase
    assert "knows one goal" not in flat


def test_exported_by_library():
    lib = ctypes.CDLL(L.LIB_PATH)
    missing = [n for n in NARGS if not hasattr(lib, n)]
    assert not missing, missing


def test_bound_with_argtypes():
    lib = L.lib()
    for name, n in NARGS.items():
        assert name in L.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name


def test_methods_present():
    import FastMarching.FastMarching as FM

    assert callable(L.Context.tmap2d_update_seeds)
    for m in ("adopt_seeds", "update_seeds", "resolve_seeds"):
        assert callable(getattr(L.Fim2d, m)), m
    assert callable(FM.updateTmapMulti)


def test_update_tmap_multi_checks_its_arguments_before_anything_runs():
    import FastMarching.FastMarching as FM

    cost = np.ones((20, 30))
    T = np.zeros((20, 30))
    goals = [(3, 3), (20, 10)]
    ok = [(1, 1, 2, 2)]
    with pytest.raises(ValueError, match="Tmap has shape"):
        FM.updateTmapMulti(cost, np.zeros((20, 1)), goals, ok)  # would broadcast silently
    with pytest.raises(ValueError, match="mask has shape"):
        FM.updateTmapMulti(cost, T, goals, np.zeros((30, 20), bool))
    with pytest.raises(ValueError, match="mask has shape"):
        FM.updateTmapMulti(cost, T, np.zeros((30, 20), bool), ok)  # the goals' mask
    with pytest.raises(ValueError, match="no goal"):
        FM.updateTmapMulti(cost, T, np.zeros((20, 30), bool), ok)
    with pytest.raises(ValueError, match="goals must be"):
        FM.updateTmapMulti(cost, T, [1, 2], ok)
    with pytest.raises(ValueError, match="2 goals but 1 offsets"):
        FM.updateTmapMulti(cost, T, goals, ok, offsets=[0.0])
    with pytest.raises(ValueError, match="no new goal"):
        FM.updateTmapMulti(cost, T, goals, ok, newGoals=np.zeros((20, 30), bool))
    with pytest.raises(ValueError, match="1 new goals but 2 new offsets"):
        FM.updateTmapMulti(cost, T, goals, ok, newGoals=[(5, 5)], newOffsets=[0.0, 1.0])
    with pytest.raises(ValueError, match="newOffsets without newGoals"):
        FM.updateTmapMulti(cost, T, goals, ok, newOffsets=[0.0, 1.0])
    # no rectangle and no list change: a float64 copy, no device
    a = np.arange(600, dtype=np.float32).reshape(20, 30)
    out = FM.updateTmapMulti(cost, a, goals, np.zeros((20, 30), bool))
    assert out.dtype == np.float64 and out is not a and np.array_equal(out, a)
    assert np.array_equal(FM.updateTmapMulti(cost, a, goals, []), a)
