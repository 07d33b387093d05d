#!/usr/bin/env python3
"""A/B of goal sets on the layered 3D solver (EIK_OPT_SEEDS_LAYERED).

The bench's C5 volume (bench.c5_volume of the 4096^2 terrain raster, seed 42: three locomotion modes between
two +inf padding layers, 5 layers in memory, 3 solved), in fp32 and fp64.  Per dtype, in one process on one
context, after one warm-up round, three solves alternated --reps (3) times, in the order (c) (a) (c) (b):

  (a) single   eik_fim3d_solve, the bench's goal (N/2, N/2, mode 0): the layered solver
  (b) K=1 on   eik_fim3d_solve_seeds with that goal as the only seed, t0 = 0, the option on: the layered solver
  (c) K=1 off  the same call with the option off: the general solver

((c) before each of the two, so that (a) and (b) start from the same state of caches and clocks: in the order
(a) (b) (c), (a) alone followed the general solver's pass over the whole volume and read 0.1 ms slower than
(b) in both dtypes), and the same with K = 16 seeds on a 4 x 4 grid over the raster, the modes in turn, t0 = 0:
(b16), (c16).
Times are eik_get_stats' solve_ms (stream events around init, seeding, solve and the planar copies).  The
line says for each dtype: the layered gain (c)/(b) at K = 1 and K = 16, (b) - (a) beside the spread (max -
min) that (a) itself shows over its alternations, the visits and in-place passes of (a) and (b), which solver
eik_fim3d_last_solver named, and how far the fields of (a), (b) and (c) lie apart.

Every dtype is a GPU step of its own: a child process under `timeout -k 10`, started only when the step
before it ended well.  One JSON line on stdout (and in --out).

    python tools/seeds_layered_ab.py [--n 4096] [--reps 3] [--limit 240] [--out profiles/seeds_layered_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(dtype, N, reps):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench  # noqa: E402  (c5_volume; puts the package on the path)
    from bench import eikonal, terrain  # noqa: E402
    from eikonal import _lib as L  # noqa: E402

    f64 = dtype == "f64"
    tdt, edt = (torch.float64, L.EIK_F64) if f64 else (torch.float32, L.EIK_F32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cost = bench.c5_volume(terrain.cost_block(0, 0, N, N, N, N, seed=42, device=dev).to(tdt), dev)
    H, W, Lm = cost.shape
    Ta, Tb, Tc = (torch.empty_like(cost) for _ in range(3))
    goal = (N // 2, N // 2, 1)
    g3 = np.asarray(goal, np.int64)
    grid = [(int((i + 0.5) * N / 4), int((j + 0.5) * N / 4), 1 + (4 * j + i) % 3) for j in range(4) for i in range(4)]
    ctx = eikonal.Context(0, options=L.options_from_env())
    ctx.set_option(L.OPT_QTIMEOUT, 20)

    def single():
        ctx._chk(L.lib().eik_fim3d_solve(ctx._h, cost.data_ptr(), Ta.data_ptr(), H, W, Lm, edt, g3, stream))

    def seeded(T, seeds, on):
        ctx.set_option(L.OPT_SEEDS_LAYERED, on)
        ctx.fim3d_solve_seeds(cost.data_ptr(), T.data_ptr(), H, W, Lm, edt, seeds, None, stream)

    runs = {"a": single, "b": lambda: seeded(Tb, [goal], 1), "c": lambda: seeded(Tc, [goal], 0),
            "b16": lambda: seeded(Tb, grid, 1), "c16": lambda: seeded(Tc, grid, 0)}
    ms = {k: [] for k in runs}
    info = {}
    out = {"dtype": dtype, "shape": [H, W, Lm], "reps": reps}

    def far(X, Y):
        """(masks equal, max |X - Y|, max relative) over the cells finite in both"""
        both = torch.isfinite(X) & torch.isfinite(Y)
        same = bool((torch.isfinite(X) == torch.isfinite(Y)).all())
        d = (X[both] - Y[both]).abs()
        return [same, float(d.max()), float((d / Y[both].abs().clamp_min(1e-30)).max())]

    # (c) runs before (a) AND before (b): whatever a 0.3 s general solve of the whole volume leaves behind in
    # the caches and clocks, the two layered solves that are compared with each other both start from it
    for group in (("c", "a", "c", "b"), ("b16", "c16")):
        for rep in range(reps + 1):  # round 0: warm-up
            for k in group:
                runs[k]()
                s = ctx.stats()
                if rep:
                    ms[k].append(s["solve_ms"])
                info[k] = {"solver": ctx.last_solver3d(), "tile_visits": s["tile_visits"],
                           "inplace_passes": s["inplace_passes"], "fresh_visits": s["fresh_visits"]}
        torch.cuda.synchronize()
        if "a" in group:
            out["fields_K1"] = {"b_vs_a": far(Tb, Ta), "c_vs_b": far(Tc, Tb)}
            out["reached_fraction"] = round(float(torch.isfinite(Ta[:, :, 1:4]).float().mean()), 4)
        else:
            out["fields_K16"] = {"c_vs_b": far(Tc, Tb)}
    ctx.set_option(L.OPT_SEEDS_LAYERED, 0)
    ctx.close()
    cells = H * W * 3
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out["solve_ms"] = {k: [round(x, 4) for x in v] for k, v in ms.items()}
    out["median_ms"] = {k: round(v, 4) for k, v in med.items()}
    out["gcells_per_s"] = {k: round(cells / (v * 1e-3) / 1e9, 3) for k, v in med.items()}
    out["gain_layered_K1"] = round(med["c"] / med["b"], 3)
    out["gain_layered_K16"] = round(med["c16"] / med["b16"], 3)
    out["b_minus_a_ms"] = round(med["b"] - med["a"], 4)
    out["a_spread_ms"] = round(max(ms["a"]) - min(ms["a"]), 4)
    out["b_within_a_spread"] = bool(abs(med["b"] - med["a"]) <= max(ms["a"]) - min(ms["a"]))
    out["info"] = info
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeds_layered_ab.json"))
    ap.add_argument("--worker", choices=["f32", "f64"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.n, args.reps)
        return 0
    res = {"tool": "seeds_layered_ab", "n": args.n, "steps": []}
    rc = 0
    for dtype in ("f32", "f64"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", dtype,
               "--n", str(args.n), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        line = next((ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            # a step that failed, faulted or ran out of time: nothing more is started on the GPU
            res["steps"].append({"dtype": dtype, "exit": p.returncode, "stderr": p.stderr[-2000:]})
            rc = p.returncode or 1
            break
        res["steps"].append(json.loads(line))
    text = json.dumps(res)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
