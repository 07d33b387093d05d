"""Rectangle-free replanning at the C-ABI boundary, no GPU: the five entry points are
declared in include/eikonal.h, exported by the built library and bound by eikonal._lib with matching
argument counts; the Python and drop-in forms exist and check their shapes before anything runs.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from eikonal import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# parameters per function, from the issue's prototypes
NARGS = {"eik_cost_diff_dev": 12, "eik_fim2d_resolve_cost": 3, "eik_fim2d_diff_info": 2, "eik_tmap2d_update_cost_f32": 8,
         "eik_tmap2d_update_cost_f64": 8}
NAMES = list(NARGS)


def _header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_declared_in_header():
    src = _header()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == NARGS[name], name


def test_rule_and_contract_are_in_the_header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("+0 equals -0", "finite -> +inf is raised", "new is NaN or < 0", "block of 2 x 2 tiles",
                   "ascending (block row, block column)", "nothing is rebound", "T keeps its bits",
                   "INVALID until a solve from scratch", "EIK_OPT_DIFF_SHARE"):
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


def test_options_are_bound():
    src = _header()
    for name, val in (("DIFF_LOADS", 21), ("DIFF_SHARE", 22)):
        assert getattr(L, "OPT_" + name) == val
        assert re.search(r"\bEIK_OPT_" + name + r"\s*=\s*%d\b" % val, src), name
    assert L.parse_options("DIFF_SHARE=2,DIFF_LOADS=1") == {"DIFF_SHARE": 2.0, "DIFF_LOADS": 1.0}


def test_methods_present_and_check_shapes_first():
    import FastMarching.FastMarching as FM

    for m in ("cost_diff", "tmap2d_update_cost"):
        assert callable(getattr(L.Context, m)), m
    for m in ("resolve_cost", "diff_info"):
        assert callable(getattr(L.Fim2d, m)), m
    cost = np.ones((20, 30))
    with pytest.raises(ValueError):
        FM.updateTmapFromCost(cost, np.ones((30, 20)), np.zeros((20, 30)), (3, 3))
    with pytest.raises(ValueError):
        FM.updateTmapFromCost(cost, cost, np.zeros((20, 1)), (3, 3))  # would broadcast silently
