#!/usr/bin/env python3
"""What the obstacle-safe 2D walker costs per step, hipEvents around each kernel.

  default   eik_path2d_dev on bench.py's C2 field (4096^2 DEM-derived cost, seed 42, goal at the
            centre, fp64, start (256, 256)): us per path step of this tree's default walker
  parent    the same call through a second library, --parent-lib (the parent commit's libeikonal.so),
            on the same device field in the same run, alternating with the others
  safe      eik_path2d_safe_dev on that field: no +inf beyond the border, so the walk is the gradient
            phase (the tool says how many fallbacks and whether integer mode began)
  integer   eik_path2d_safe_dev on a rough raster (exp(N(0, 1.5)), 2048^2), where the stall rule puts
            the walk in integer mode after a few dozen iterations: us per iteration of the run loop

Appends its lines to --log (default profiles/path_safe_ab.log) and prints one JSON line.
  python tools/path_safe_ab.py [--parent-lib PATH] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-motion_planning_amd"))
import eikonal  # noqa: E402
from eikonal import _lib as L  # noqa: E402
from eikonal import terrain  # noqa: E402

CAP, TAU = 30004, 0.5


class ParentLib:
    """eik_create / eik_path2d_dev / eik_destroy of another build of the library"""

    def __init__(self, path, device):
        vp, i64 = C.c_void_p, C.c_int64
        f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
        self.lib = C.CDLL(os.path.abspath(path))
        self.lib.eik_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.lib.eik_destroy.argtypes = [vp]
        self.lib.eik_destroy.restype = None
        self.lib.eik_path2d_dev.argtypes = [vp, vp, C.c_int, i64, i64, f64p, f64p, C.c_double, vp, i64, vp, vp, vp]
        self.h = vp()
        rc = self.lib.eik_create(device, C.byref(self.h))
        if rc:
            raise RuntimeError(f"{path}: eik_create returned {rc}")

    def close(self):
        self.lib.eik_destroy(self.h)


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def line(name, what, v):
    return f"{name:8s}{what:22s}runs {[round(x, 4) for x in v]}  median {np.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rough-size", type=int, default=2048)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "path_safe_ab.log"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = eikonal.Context(0)
    stream = torch.cuda.current_stream(dev)
    lib = L.lib()
    parent = ParentLib(a.parent_lib, 0) if a.parent_lib else None
    out = torch.empty((CAP, 2), dtype=torch.float64, device=dev)
    n_d = torch.zeros(1, dtype=torch.int64, device=dev)
    st_d = torch.zeros(1, dtype=torch.int32, device=dev)
    info_d = torch.zeros(4, dtype=torch.int64, device=dev)

    def solve(cost, goal):
        N = cost.shape[0]
        T = torch.empty_like(cost)
        fim = eikonal.Fim2d(ctx, 1, N, N, L.EIK_F64)
        fim.solve(cost.data_ptr(), T.data_ptr(), [goal], stream.cuda_stream)
        torch.cuda.synchronize()
        fim.close()
        return T

    def default(T, N, s, g, h=None):
        fn, hh = (lib.eik_path2d_dev, ctx._h) if h is None else (h.lib.eik_path2d_dev, h.h)
        rc = fn(hh, T.data_ptr(), L.EIK_F64, N, N, s, g, TAU, out.data_ptr(), CAP, n_d.data_ptr(), st_d.data_ptr(),
                stream.cuda_stream)
        assert rc == 0, rc

    def safe(T, N, s, g):
        ctx._chk(lib.eik_path2d_safe_dev(ctx._h, T.data_ptr(), L.EIK_F64, N, N, s, g, TAU, out.data_ptr(), CAP,
                                         n_d.data_ptr(), st_d.data_ptr(), info_d.data_ptr(), stream.cuda_stream))

    # ---- C2: default (this tree, parent) and the safe walker's gradient phase, alternating
    N = a.size
    cost = terrain.cost_block(0, 0, N, N, N, N, seed=42, device=dev).double().contiguous()
    goal = (N // 2, N // 2)
    T = solve(cost, goal)
    s, g = np.array((N / 16.0, N / 16.0)), np.array(goal, np.float64)
    res = {"tool": "path_safe_ab", "device": torch.cuda.get_device_name(0), "tau": TAU, "field": f"C2 {N}^2 fp64"}
    default(T, N, s, g)
    torch.cuda.synchronize()
    n_def, st_def = int(n_d.item()), int(st_d.item())
    ref = out[:n_def].clone()
    safe(T, N, s, g)
    torch.cuda.synchronize()
    n_safe, st_safe, info = int(n_d.item()), int(st_d.item()), info_d.cpu().numpy().copy()
    same = n_safe == n_def and bool(torch.equal(out[:n_safe], ref))
    ms = {"new": [], "parent": [], "safe": []}
    for _ in range(a.reps):
        ms["new"].append(timed(stream, lambda: default(T, N, s, g)))
        if parent:
            ms["parent"].append(timed(stream, lambda: default(T, N, s, g, parent)))
        ms["safe"].append(timed(stream, lambda: safe(T, N, s, g)))
    steps_def, iters = max(n_def - 2, 1), max(int(info[3]), 1)
    lines = [f"# tools/path_safe_ab.py on {res['device']}: C2 {N}^2 fp64 field, start {s.tolist()}, tau {TAU}, {a.reps} runs each, "
             "alternating; us per step = kernel ms (hipEvents) / steps",
             f"# default walk: {n_def} points, status {st_def}; safe walk: {n_safe} points, status {st_safe}, info {info.tolist()}"
             f" (fallbacks, dropped, integer from, iterations); safe path == default path bit for bit: {same}"]
    us = {k: [1e3 * x / (iters if k == "safe" else steps_def) for x in v] for k, v in ms.items() if v}
    for k, name in (("parent", "parent"), ("new", "new"), ("safe", "safe")):
        if k in us:
            lines.append(line(name, "default_us_per_step" if k != "safe" else "gradient_us_per_step", us[k]))
            res[f"{k}_us_per_step"] = round(float(np.median(us[k])), 4)
    res.update({"default_points": n_def, "safe_points": n_safe, "safe_info": info.tolist(), "safe_equals_default": same})
    del cost, T
    torch.cuda.empty_cache()
    # ---- integer mode: a rough raster, the stall rule fires early and the run loop does the rest
    M = a.rough_size
    rng = np.random.default_rng(13)
    rough = np.exp(rng.normal(0, 1.5, (M, M)))
    rough[0, :] = rough[-1, :] = rough[:, 0] = rough[:, -1] = np.inf
    goal = (M // 2, M // 2)
    rough[goal[1] - 1:goal[1] + 2, goal[0] - 1:goal[0] + 2] = 1.0
    Tr = solve(torch.from_numpy(rough).to(dev), goal)
    s, g = np.array((M / 16.0, M / 16.0)), np.array(goal, np.float64)
    safe(Tr, M, s, g)
    torch.cuda.synchronize()
    info = info_d.cpu().numpy().copy()
    st_r, n_r = int(st_d.item()), int(n_d.item())
    run = max(int(info[3] - info[2]), 1)
    msi = [timed(stream, lambda: safe(Tr, M, s, g)) for _ in range(a.reps)]
    usi = [1e3 * x / run for x in msi]
    lines.append(f"# integer mode: exp(N(0, 1.5)) {M}^2 fp64, start {s.tolist()}: {n_r} points, status {st_r}, info {info.tolist()}; "
                 f"us per step = kernel ms / the {run} iterations from info[2] on (the {int(info[2])} before them are in the ms)")
    lines.append(line("safe", "integer_us_per_step", usi))
    res.update({"integer_us_per_step": round(float(np.median(usi)), 4), "integer_info": info.tolist(), "integer_status": st_r})
    if parent:
        parent.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
