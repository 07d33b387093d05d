#!/usr/bin/env python3
"""A/B of the incremental re-solve (eik_fim2d_resolve) against the full solve.

On the bench's C2 raster (4096^2, eikonal/terrain.py seed 42, goal at the centre) in fp64 and fp32,
and on a 16384^2 fp64 raster (seed 7, the C4 raster), a 32 x 32 block is raised to +inf centred on
the cells at the 0.05 / 0.25 / 0.5 / 0.9 / 0.99 quantiles of the finite T (0.05: close to the goal, where
a block shadows most of the raster), and one block at the 0.5 quantile
is lowered (its costs halved, declared EIK_CHANGE_LOWERED).  Per case, alternating on one solver:

  full     eik_fim2d_solve of the new cost from scratch -- the yardstick (its code is unchanged)
  update   the old field put back (eik_fim2d_adopt, not timed: a planner loop's solver simply stays
           converged), then eik_fim2d_resolve: invalidation flood + reset + the partial solve

Times are device times between events on the solver's stream (eik_stats.solve_ms: for the update it
spans the flood, the reset and the solve; update_info's device_us is the flood + reset share) and the
host's wall time around each synchronous call.  The two fields are compared cell for cell.

    python tools/replan_ab.py [--sizes 4096,16384] [--reps 5] [--out profiles/replan_ab.log]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replan_ab.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx = eikonal.Context(0, options=L.options_from_env())
    say(f"# replan_ab: {torch.cuda.get_device_name(dev)}, {eikonal.lib().eik_version().decode()}, reps {args.reps}, "
        f"block {args.block}")
    say("# times: min / median over the alternations, ms; dev = events on the stream, wall = host clock around the call")
    for N in (int(s) for s in args.sizes.split(",")):
        for tdt, edt, name in ((torch.float64, L.EIK_F64, "fp64"), (torch.float32, L.EIK_F32, "fp32")):
            if N > 4096 and name == "fp32":
                continue
            cost = terrain.cost_block(0, 0, N, N, N, N, seed=42 if N == 4096 else 7, device=dev).to(tdt).contiguous()
            goal = [[N // 2, N // 2]]
            T = torch.empty_like(cost)
            fim = L.Fim2d(ctx, 1, N, N, edt)
            fim.solve(cost.data_ptr(), T.data_ptr(), goal, stream)  # warm-up
            fim.solve(cost.data_ptr(), T.data_ptr(), goal, stream)
            T_old = T.clone()
            st0 = fim.stats()
            fin = torch.isfinite(T_old)
            nfin = int(fin.sum())
            order = torch.argsort(T_old.flatten())  # +inf last
            say(f"\n## {N}^2 {name}: full solve of the unchanged raster {st0['solve_ms']:.3f} ms, "
                f"{st0['tile_visits']} visits + {st0['inplace_passes']} passes; {nfin} of {N * N} cells reachable")
            say("case              cells_inval  frac_reach  tiles  flood_vis  queued | flood+reset  update_dev    update_wall  |"
                " full_dev      full_wall    | upd/full  visits upd/full  max|dT|")
            cases = [("raise q=%.2f" % q, q, L.CHANGE_ANY) for q in (0.05, 0.25, 0.5, 0.9, 0.99)] + [("lower q=0.50", 0.5, L.CHANGE_LOWERED)]
            for label, q, kind in cases:
                cell = int(order[int(q * (nfin - 1))])
                cy, cx = divmod(cell, N)
                h = args.block // 2
                x0, y0 = max(cx - h, 0), max(cy - h, 0)
                x1, y1 = min(cx + h, N), min(cy + h, N)
                new = cost.clone()
                if kind == L.CHANGE_ANY:
                    new[y0:y1, x0:x1] = float("inf")
                    new[N // 2, N // 2] = cost[N // 2, N // 2]
                else:
                    new[y0:y1, x0:x1] *= 0.5
                rect = [(x0, y0, x1, y1)]
                Tu = torch.empty_like(cost)
                rows = {"full": [], "upd": []}
                info = work_u = work_f = None
                for rep in range(args.reps + 1):  # the first alternation warms both paths up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fim.solve(new.data_ptr(), T.data_ptr(), goal, stream)
                    wall = (time.perf_counter() - t0) * 1e3
                    s = fim.stats()
                    work_f = s["tile_visits"] + s["inplace_passes"]
                    if rep:
                        rows["full"].append((s["solve_ms"], wall))
                    Tu.copy_(T_old)
                    fim.adopt(new.data_ptr(), Tu.data_ptr(), goal, stream)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fim.resolve(rect, [kind], stream)
                    wall = (time.perf_counter() - t0) * 1e3
                    s = fim.stats()
                    info = fim.update_info()
                    work_u = s["tile_visits"] + s["inplace_passes"]
                    if rep:
                        rows["upd"].append((s["solve_ms"], wall, info["device_us"] / 1e3))
                torch.cuda.synchronize()
                same_mask = bool((torch.isfinite(T) == torch.isfinite(Tu)).all())
                both = torch.isfinite(T) & torch.isfinite(Tu)
                dmax = float((T[both] - Tu[both]).abs().max()) if bool(both.any()) else 0.0
                f = np.array(rows["full"])
                u = np.array(rows["upd"])

                def mm(a):
                    return f"{a.min():6.3f}/{np.median(a):6.3f}"

                say(f"{label:16s} {info['cells']:11d}  {info['cells'] / max(nfin, 1):9.4f}  {info['tiles_marked']:5d}  "
                    f"{info['flood_visits']:9d}  {info['tiles_queued']:6d} | {mm(u[:, 2])}  {mm(u[:, 0])}  {mm(u[:, 1])} | "
                    f"{mm(f[:, 0])}  {mm(f[:, 1])} | {np.median(u[:, 0]) / np.median(f[:, 0]):7.3f}  "
                    f"{work_u:7d}/{work_f:<7d}  {dmax:.2e}{'' if same_mask else '  MASKS DIFFER'}"
                    f"{'  FELL BACK' if info['fell_back'] else ''}")
            fim.close()
            del cost, T, T_old, order, fin
            torch.cuda.empty_cache()
    ctx.close()
    log.close()


if __name__ == "__main__":
    main()
