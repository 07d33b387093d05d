#!/usr/bin/env python3
"""Timing of the 3D goal-set solve and its label pass (eik_fim3d_solve_seeds, eik_labels3d_dev, DESIGN.md
§3.16) beside the single-goal solve, on the end-effector volume's size.

A 60 x 60 x 41 fp64 volume (the planner's arm volume, cost[y][x][z]) with a synthetic cost -- exp of a
smooth field, 1 .. ~20, fixed generator -- and a +inf border, same process, alternating:

  (a) parent   eik_fim3d_solve of another build of the library, --parent-lib (the parent commit's
               libeikonal.so, loaded beside this tree's as tools/path_safe_ab.py does)
  (b) single   eik_fim3d_solve of this tree, the same goal
  (c) K=1      eik_fim3d_solve_seeds with that goal as the only seed, t0 = 0
  (d) K=8      eight seeds scattered over the open cells (fixed generator), t0 = 0
  (e) labels   eik_labels3d_dev on the field of (c) and of (d)

Times are hipEvents on the stream around each call (init, seeding and solve together; the calls are
synchronous, so the events bracket the whole device work), one warm-up alternation, then --reps
alternations; min / median / max per case, so the same-build run-to-run spread stands beside every
difference.  The log says whether (b) - (a) and (c) - (b) lie inside that spread.

    python tools/seeds3d_ab.py [--parent-lib PATH] [--reps 9] [--out profiles/seeds3d_ab.log]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-motion_planning_amd"))

import eikonal  # noqa: E402
from eikonal import _lib as L  # noqa: E402

SHAPE = (60, 60, 41)


class ParentLib:
    """eik_create / eik_fim3d_solve / eik_destroy of another build of the library"""

    def __init__(self, path, device):
        vp, i64 = C.c_void_p, C.c_int64
        self.lib = C.CDLL(os.path.abspath(path))
        self.lib.eik_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.lib.eik_destroy.argtypes = [vp]
        self.lib.eik_destroy.restype = None
        self.lib.eik_fim3d_solve.argtypes = [vp, vp, vp, i64, i64, i64, C.c_int,
                                             np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), vp]
        self.h = vp()
        rc = self.lib.eik_create(device, C.byref(self.h))
        if rc:
            raise RuntimeError(f"{path}: eik_create returned {rc}")

    def close(self):
        self.lib.eik_destroy(self.h)


def volume():
    rng = np.random.default_rng(41)
    H, W, Lz = SHAPE
    ys, xs, zs = np.mgrid[0:H, 0:W, 0:Lz]
    f = sum(a * np.sin(kx * xs + ky * ys + kz * zs + p)
            for a, kx, ky, kz, p in zip(rng.uniform(0.3, 0.8, 6), rng.uniform(0.05, 0.5, 6), rng.uniform(0.05, 0.5, 6),
                                        rng.uniform(0.05, 0.5, 6), rng.uniform(0, 6.28, 6)))
    cost = np.exp(f + 1.0).clip(1.0, 20.0)
    cost[0, :, :] = cost[-1, :, :] = cost[:, 0, :] = cost[:, -1, :] = cost[:, :, 0] = cost[:, :, -1] = np.inf
    return cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeds3d_ab.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = eikonal.Context(0, options=L.options_from_env())
    parent = ParentLib(args.parent_lib, 0) if args.parent_lib else None
    H, W, Lz = SHAPE
    cost_h = volume()
    cost = torch.from_numpy(cost_h).to(dev)
    T = torch.empty_like(cost)
    goal = (45, 40, 30)  # (x, y, z)
    g = np.ascontiguousarray(goal, np.int64)
    rng = np.random.default_rng(5)
    scattered = []
    while len(scattered) < 8:
        x, y, z = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, Lz))
        if np.isfinite(cost_h[y, x, z]) and (x, y, z) not in scattered:
            scattered.append((x, y, z))
    say(f"# seeds3d_ab: {torch.cuda.get_device_name(dev)}, {eikonal.lib().eik_version().decode()}, "
        f"{H} x {W} x {Lz} fp64, goal {goal}, reps {args.reps}" + ("" if parent else ", NO parent library"))
    say("# ms between hipEvents on the stream around each call; one warm-up alternation, then min / median / max")

    def single(h=None):
        if h is None:
            ctx._chk(L.lib().eik_fim3d_solve(ctx._h, cost.data_ptr(), T.data_ptr(), H, W, Lz, L.EIK_F64, g, stream.cuda_stream))
        else:
            rc = h.lib.eik_fim3d_solve(h.h, cost.data_ptr(), T.data_ptr(), H, W, Lz, L.EIK_F64, g, stream.cuda_stream)
            assert rc == 0, rc

    def seeded(seeds):
        ctx.fim3d_solve_seeds(cost.data_ptr(), T.data_ptr(), H, W, Lz, L.EIK_F64, seeds, None, stream.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    cases = (["parent"] if parent else []) + ["single", "K=1", "K=8"]
    ms = {k: [] for k in cases + ["labels K=1", "labels K=8"]}
    info = {}
    ref = None
    for rep in range(args.reps + 1):  # the first alternation warms every path up
        for name in cases:
            if name == "parent":
                t, _ = timed(lambda: single(parent))
            elif name == "single":
                t, _ = timed(single)
            else:
                seeds = [goal] if name == "K=1" else scattered
                t, _ = timed(lambda: seeded(seeds))
            if rep == 0:
                if name in ("parent", "single", "K=1"):
                    ref = T.clone() if ref is None else ref
                    info[name] = f"max |T - first| = {float((T - ref)[torch.isfinite(ref)].abs().max()):.3e}, " \
                                 f"masks equal {bool(torch.equal(torch.isfinite(T), torch.isfinite(ref)))}"
                if name != "parent":
                    s = ctx.stats()
                    info[name] = info.get(name, "") + f" visits {s['tile_visits']} passes {s['inplace_passes']}"
            else:
                ms[name].append(t)
            if name.startswith("K="):
                tl, lab = timed(lambda: ctx.labels3d(T, seeds))
                if rep == 0:
                    reach = torch.isfinite(T)
                    info["labels " + name] = f"labelled {int((lab[reach] >= 0).sum())} of {int(reach.sum())} reachable, " \
                                             f"{labels_passes(H * W * Lz)} jump passes launched"
                else:
                    ms["labels " + name].append(tl)
    say(f"\n{'case':12s} | {'min':>7s} {'median':>7s} {'max':>7s} | notes")
    for name in ms:
        if ms[name]:
            a = np.array(ms[name])
            say(f"{name:12s} | {a.min():7.3f} {np.median(a):7.3f} {a.max():7.3f} | {info.get(name, '')}")
    med = {k: float(np.median(v)) for k, v in ms.items() if v}
    spread = {k: float(max(v) - min(v)) for k, v in ms.items() if v}

    def verdict(a, b):
        d, sp = med[b] - med[a], max(spread[a], spread[b])
        return f"{b} - {a}: {d:+.3f} ms (medians), same-build spread {sp:.3f} ms -> {'inside' if abs(d) <= sp else 'OUTSIDE'}"

    say()
    if parent:
        say(verdict("parent", "single"))
    say(verdict("single", "K=1"))
    say(verdict("K=1", "K=8"))
    if parent:
        parent.close()
    ctx.close()
    log.close()


def labels_passes(n):
    p = 1
    while p < 32 and (1 << p) < n:
        p += 1
    return p


if __name__ == "__main__":
    main()
