"""The batched path entry points at the C-ABI boundary, no GPU: declared in include/eikonal.h,
exported by the built library, bound (argtypes set) by eikonal._lib."""
import ctypes
import os
import re

from eikonal import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eik_path2d_batch_dev", "eik_path2d_batch_f64", "eik_path3d_batch_dev", "eik_path3d_batch_f64",
         "eik_plan2d_batch_f32"]
# parameters per function, from the issue's prototypes
NARGS = {"eik_path2d_batch_dev": 16, "eik_path2d_batch_f64": 14, "eik_path3d_batch_dev": 17,
         "eik_path3d_batch_f64": 15, "eik_plan2d_batch_f32": 13}


def _header():
    src = open(os.path.join(ROOT, "include", "eikonal.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_declared_in_header():
    src = _header()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == NARGS[name], name


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
    import FastMarching.FastMarching3D as FM3D

    for m in ("path2d_batch", "path3d_batch", "plan2d_batch"):
        assert callable(getattr(L.Context, m)), m
    assert callable(FM.getPathsGDM) and callable(FM3D.getPathsGDM)
