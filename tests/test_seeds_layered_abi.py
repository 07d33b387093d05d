"""Goal sets on the layered 3D solver at the C-ABI boundary, no GPU: the option and the
query are declared in include/eikonal.h, exported by the built library and bound by eikonal._lib, and the
drop-in takes the switch."""
import ctypes
import inspect
import os
import re

import pytest

from eikonal import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "eikonal.h")).read()


def test_option_and_prototype_in_header():
    src = header()
    assert re.search(r"\bEIK_OPT_SEEDS_LAYERED\s*=\s*23\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+eik_fim3d_last_solver\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m and len(m.group(1).split(",")) == 2
    assert re.search(r"const\s+eik_ctx\s*\*", m.group(1)) and re.search(r"int64_t\s+\w+\[4\]", m.group(1))
    # no two options share a value
    vals = re.findall(r"\bEIK_OPT_\w+\s*=\s*(\d+)", code)
    assert len(vals) == len(set(vals)) and max(map(int, vals)) == 23


def test_header_text():
    flat = " ".join(header().replace("*", " ").split())
    at = flat.index("Goal sets for 3D solves")
    text = flat[at:flat.index("int eik_fim3d_solve_seeds", at)]
    assert "EIK_OPT_SEEDS_LAYERED" in text and "eik_fim3d_last_solver" in text
    not_covered = text[text.rindex("Not covered:"):]
    for phrase in ("eik_fim3dl_", "3D replanning", "B > 1", "early exit with a seed set"):
        assert phrase in not_covered, phrase
    assert "the layered solver" not in not_covered and "the layered solver" in text


def test_exported_by_library():
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "eik_fim3d_last_solver")


def test_bound():
    assert L.OPT_SEEDS_LAYERED == 23
    assert "eik_fim3d_last_solver" in L.EXPORTED
    fn = L.lib().eik_fim3d_last_solver
    assert fn.argtypes is not None and len(fn.argtypes) == 2
    assert callable(L.Context.last_solver3d) and callable(L.Context.get_option)
    assert L.parse_options("SEEDS_LAYERED=1") == {"SEEDS_LAYERED": 1.0}
    assert L.parse_options({"SEEDS_LAYERED": 0}) == {"SEEDS_LAYERED": 0.0}
    with pytest.raises(ValueError):
        L.parse_options("SEEDS_LAYERD=1")


def test_drop_in_takes_the_switch():
    import FastMarching.FastMarching3D as FM3

    p = inspect.signature(FM3.computeTmapMulti).parameters
    assert list(p) == ["costMap", "goals", "offsets", "labels", "layered"] and p["layered"].default is None
    assert "EIKONAL_SEEDS_LAYERED" in FM3.computeTmapMulti.__doc__
