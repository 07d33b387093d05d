#!/usr/bin/env python3
"""Batched path extraction against loops of single-path calls (DESIGN.md "Batched paths").

  c3      128 paths over 128 x 1024^2 fp32 fields resident on the device (bench.py's C3 maps and
          goals): one eik_path2d_batch_dev against 128 eik_path2d_dev calls, hipEvents on the stream
  fleet   P = 1024 starts on one 4096^2 fp32 field (four rounds of workgroups on 256 CUs): the
          batch against the same 1024 single calls, hipEvents
  plan    host cost rasters of C3 -> paths: plan2d_batch against tmap2d_batch + one path2d per map
          (wall clock: the difference is the 512 MiB field download and the serial walks)

Prints one JSON line; every batch result is also checked bit for bit against the single calls.
  python tools/path_batch_ab.py [--maps 128] [--fleet 1024] [--skip plan]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-motion_planning_amd"))
import eikonal  # noqa: E402
from eikonal import _lib as L  # noqa: E402
from eikonal import terrain  # noqa: E402

CAP, TAU = 30004, 0.5


def c3_goal(cost_b, b, N):  # bench.py's
    rng = np.random.default_rng(1000 + b)
    while True:
        gx, gy = (int(v) for v in rng.integers(N // 8, N - N // 8, 2))
        if float(cost_b[gy, gx]) < 50:
            return gx, gy


def far_start(T_b, goal, rng):
    """A reached low-T-gradient cell at least a third of the raster away from the goal."""
    N = T_b.shape[0]
    while True:
        x, y = (int(v) for v in rng.integers(N // 16, N - N // 16, 2))
        if abs(x - goal[0]) + abs(y - goal[1]) >= N // 3 and bool(torch.isfinite(T_b[y, x])):
            return x + 0.25, y + 0.5


def events(stream, fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def spread(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def batch_vs_loop(ctx, dev, stream, T, B, N, map_of, starts, goals, reps):
    """T: [B][N][N] fp32 on the device; path p: map_of[p], starts[p] -> goals[p]."""
    P = len(starts)
    out_b = torch.empty((P, CAP, 2), dtype=torch.float64, device=dev)
    n_b = torch.zeros(P, dtype=torch.int64, device=dev)
    st_b = torch.zeros(P, dtype=torch.int32, device=dev)
    out_s = torch.empty_like(out_b)
    n_s, st_s = torch.zeros_like(n_b), torch.zeros_like(st_b)
    m = np.ascontiguousarray(map_of, np.int32)
    lib = L.lib()

    def batch():
        ctx._chk(lib.eik_path2d_batch_dev(ctx._h, T.data_ptr(), L.EIK_F32, B, N, N, P, m.ctypes.data, starts, goals, TAU,
                                          out_b.data_ptr(), CAP, n_b.data_ptr(), st_b.data_ptr(), stream.cuda_stream))

    def loop():
        for p in range(P):
            ctx._chk(lib.eik_path2d_dev(ctx._h, T.data_ptr() + 4 * int(m[p]) * N * N, L.EIK_F32, N, N, starts[p].copy(),
                                        goals[p].copy(), TAU, out_s.data_ptr() + 16 * CAP * p, CAP,
                                        n_s.data_ptr() + 8 * p, st_s.data_ptr() + 4 * p, stream.cuda_stream))

    batch()
    loop()
    torch.cuda.synchronize()
    n = n_s.cpu().numpy()
    equal = bool(torch.equal(n_b, n_s) and torch.equal(st_b, st_s)) and all(
        torch.equal(out_b[p, : n[p]], out_s[p, : n[p]]) for p in range(P))
    tb, tl = events(stream, batch, reps), events(stream, loop, reps)
    # each walk alone: the batch's floor is the longest one
    longest = max(range(P), key=lambda p: n[p])
    one = events(stream, lambda: ctx._chk(lib.eik_path2d_dev(
        ctx._h, T.data_ptr() + 4 * int(m[longest]) * N * N, L.EIK_F32, N, N, starts[longest].copy(), goals[longest].copy(),
        TAU, out_s.data_ptr(), CAP, n_s.data_ptr(), st_s.data_ptr(), stream.cuda_stream)), reps)
    return {"paths": P, "equal_bits": equal, "points_total": int(n.sum()), "points_longest": int(n.max()),
            "status_counts": np.bincount(st_s.cpu().numpy(), minlength=3).tolist(),
            "batch_ms": spread(tb), "loop_ms": spread(tl), "longest_alone_ms": spread(one),
            "loop_over_batch": round(float(np.median(tl) / np.median(tb)), 2),
            "batch_over_longest": round(float(np.median(tb) / np.median(one)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=128)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--fleet", type=int, default=1024)
    ap.add_argument("--fleet-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated: c3, fleet, plan")
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))
    dev = torch.device("cuda", 0)
    ctx = eikonal.Context(0)
    stream = torch.cuda.Stream(dev)
    res = {"tool": "path_batch_ab", "device": torch.cuda.get_device_name(0), "tau": TAU, "cap": CAP}
    rng = np.random.default_rng(5)
    B, N = a.maps, a.size
    if "c3" not in skip or "plan" not in skip:
        cost = torch.empty((B, N, N), dtype=torch.float32, device=dev)
        goals = []
        for b in range(B):
            cost[b] = terrain.cost_block(0, 0, N, N, N, N, seed=1000 + b, device=dev)
            goals.append(c3_goal(cost[b], b, N))
        T = torch.empty_like(cost)
        fim = eikonal.Fim2d(ctx, B, N, N, L.EIK_F32)
        with torch.cuda.stream(stream):
            fim.solve(cost.data_ptr(), T.data_ptr(), goals, stream.cuda_stream)
            torch.cuda.synchronize()
            starts = np.array([far_start(T[b], goals[b], rng) for b in range(B)], np.float64)
            g = np.array(goals, np.float64)
            if "c3" not in skip:
                res["c3"] = {"maps": f"{B} x {N}^2 fp32", **batch_vs_loop(ctx, dev, stream, T, B, N, np.arange(B), starts, g,
                                                                          a.reps)}
        fim.close()
        if "plan" not in skip:
            hc = cost.cpu().numpy()
            hg = np.array(goals, np.int64)
            del cost, T
            torch.cuda.empty_cache()
            tp, tl = [], []
            for rep in range(a.reps + 1):  # the first: buffers
                t0 = time.perf_counter()
                got = ctx.plan2d_batch(hc, hg, starts, TAU)
                t1 = time.perf_counter()
                Th = ctx.tmap2d_batch(hc, hg)
                t2 = time.perf_counter()
                ref = [ctx.path2d(Th[b], starts[b], g[b], TAU) for b in range(B)]
                t3 = time.perf_counter()
                if rep:
                    tp.append((t1 - t0) * 1e3)
                    tl.append((t3 - t1) * 1e3)
                    last = ((t2 - t1) * 1e3, (t3 - t2) * 1e3)
            # (the loop's walks read the fp32 field widened to fp64, the same values: equal bits expected)
            same = sum(int(x[1] == y[1] and x[0].shape == y[0].shape and np.array_equal(x[0], y[0])) for x, y in zip(got, ref))
            res["plan"] = {"plan2d_batch_ms": spread(tp), "tmap2d_batch_plus_path2d_loop_ms": spread(tl),
                           "loop_split_ms": {"tmap2d_batch": round(last[0], 1), "path2d_x_maps": round(last[1], 1)},
                           "paths_equal": f"{same}/{B}", "clock": "host wall clock"}
            del hc, Th
        else:
            del cost, T
        torch.cuda.empty_cache()
    if "fleet" not in skip:
        M, P = a.fleet_size, a.fleet
        cost = terrain.cost_block(0, 0, M, M, M, M, seed=42, device=dev).reshape(1, M, M).contiguous()
        goal = c3_goal(cost[0], 0, M)
        T = torch.empty_like(cost)
        fim = eikonal.Fim2d(ctx, 1, M, M, L.EIK_F32)
        with torch.cuda.stream(stream):
            fim.solve(cost.data_ptr(), T.data_ptr(), [goal], stream.cuda_stream)
            torch.cuda.synchronize()
            starts = np.array([far_start(T[0], goal, rng) for _ in range(P)], np.float64)
            g = np.repeat(np.array([goal], np.float64), P, axis=0)
            res["fleet"] = {"field": f"{M}^2 fp32", **batch_vs_loop(ctx, dev, stream, T, 1, M, np.zeros(P, np.int32), starts, g,
                                                                    a.reps)}
        fim.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
