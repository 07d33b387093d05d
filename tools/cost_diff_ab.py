#!/usr/bin/env python3
"""A/B of the rectangle-free re-solve (eik_cost_diff_dev / eik_fim2d_resolve_cost).

On the bench's C2 raster (4096^2, eikonal/terrain.py seed 42, goal at the centre) in fp64 and fp32, and on
a 16384^2 fp64 raster (seed 7), as tools/replan_ab.py.  Variants alternate in one process on one solver:
one warm-up round, then --reps rounds; medians, minima and the spread (max - min) are logged.

  1. the diff alone   eik_cost_diff_dev, plain and non-temporal loads, on three cases -- a 32 x 32 block at
                      the median T raised to +inf, the same block halved, no change -- against a
                      hipMemcpyAsync device-to-device copy of one raster in the same rounds (the diff reads
                      2N bytes, the copy reads N and writes N).  dev: the two kernels between stream
                      events (info[5]); wall: the whole synchronous call, so wall - dev is the launch,
                      the read-back of the list and the synchronisation.
  2. end to end       the raised and the halved block: eik_fim2d_resolve_cost (diff + update) against
                      eik_fim2d_resolve with the hand-written rectangle and kind, and against the full
                      solve (its code is unchanged: the yardstick).  The old field is put back with
                      eik_fim2d_adopt before each update (not timed).
  3. the share        changed tiles of kind ANY scattered over 1/64, 1/16, 1/4, 1/2 and all of the tiles
                      (one cell doubled per tile, seeded positions), eik_fim2d_resolve_cost with the
                      share rule switched off (EIK_OPT_DIFF_SHARE = 2) against the full solve.

    python tools/cost_diff_ab.py [--sizes 4096,16384] [--reps 5] [--out profiles/cost_diff_ab.log]
"""
import argparse
import ctypes
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


def stat(a):
    a = np.asarray(a, float)
    return f"{np.median(a):8.3f} (min {a.min():7.3f}, spread {a.max() - a.min():6.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_diff_ab.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    hip_path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")  # the one runtime of the process
    hip = ctypes.CDLL(hip_path if os.path.exists(hip_path) else "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    ctx = eikonal.Context(0, options=L.options_from_env())
    say(f"# cost_diff_ab: {torch.cuda.get_device_name(dev)}, {eikonal.lib().eik_version().decode()}, reps {args.reps}, "
        f"block {args.block}; all times in ms: median (min, spread = max - min) over the rounds")
    for N in (int(s) for s in args.sizes.split(",")):
        for tdt, edt, name in ((torch.float64, L.EIK_F64, "fp64"), (torch.float32, L.EIK_F32, "fp32")):
            if N > 4096 and name == "fp32":
                continue
            cost = terrain.cost_block(0, 0, N, N, N, N, seed=42 if N == 4096 else 7, device=dev).to(tdt).contiguous()
            goal = [[N // 2, N // 2]]
            T = torch.empty_like(cost)
            Tu = torch.empty_like(cost)
            spare = torch.empty_like(cost)
            fim = L.Fim2d(ctx, 1, N, N, edt)
            fim.solve(cost.data_ptr(), T.data_ptr(), goal, stream)  # warm-up
            fim.solve(cost.data_ptr(), T.data_ptr(), goal, stream)
            T_old = T.clone()
            fin = torch.isfinite(T_old)
            nfin = int(fin.sum())
            order = torch.argsort(T_old.flatten())
            cy, cx = divmod(int(order[int(0.5 * (nfin - 1))]), N)
            del order
            h = args.block // 2
            x0, y0, x1, y1 = max(cx - h, 0), max(cy - h, 0), min(cx + h, N), min(cy + h, N)
            rect = [(x0, y0, x1, y1)]
            raised = cost.clone()
            raised[y0:y1, x0:x1] = float("inf")
            raised[N // 2, N // 2] = cost[N // 2, N // 2]
            lowered = cost.clone()
            lowered[y0:y1, x0:x1] *= 0.5
            nbytes = cost.numel() * cost.element_size()
            tiles = ((N + 63) // 64) ** 2
            say(f"\n## {N}^2 {name}: {tiles} tiles, {nbytes / 2**20:.0f} MiB per raster, block {rect[0]}")

            # ---- 1. the diff alone
            say("# 1. the diff alone")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            rows = {}
            for rep in range(args.reps + 1):
                torch.cuda.synchronize()
                ev[0].record()
                hip.hipMemcpyAsync(spare.data_ptr(), cost.data_ptr(), nbytes, 3, stream)  # hipMemcpyDeviceToDevice
                ev[1].record()
                torch.cuda.synchronize()
                if rep:
                    rows.setdefault(("copy", ""), []).append((ev[0].elapsed_time(ev[1]), 0.0))
                # (no change: the copy just made, a second buffer -- the diff always reads two rasters)
                for case, new in (("raised", raised), ("lowered", lowered), ("no change", spare)):
                    for loads in (0, 1):
                        ctx.set_option(L.OPT_DIFF_LOADS, loads)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        r, k, info = ctx.cost_diff(cost.data_ptr(), new.data_ptr(), edt, N, N, 1024, stream)
                        wall = (time.perf_counter() - t0) * 1e3
                        if rep:
                            rows.setdefault((case, "nt" if loads else "plain"), []).append((info["device_us"] / 1e3, wall))
                        want = {"raised": (1, L.CHANGE_ANY), "lowered": (1, L.CHANGE_LOWERED), "no change": (0, None)}[case]
                        assert len(r) >= want[0] and (want[1] is None or all(int(v) == want[1] for v in k)), (case, r, k, info)
            ctx.set_option(L.OPT_DIFF_LOADS, 1)  # the default
            cp = np.array(rows[("copy", "")])[:, 0]
            say(f"d2d copy of one raster           dev {stat(cp)}   {2 * nbytes / np.median(cp) / 1e9:6.2f} TB/s moved")
            for key, v in rows.items():
                if key[0] == "copy":
                    continue
                v = np.array(v)
                say(f"diff {key[0]:10s} {key[1]:6s}          dev {stat(v[:, 0])}   {2 * nbytes / np.median(v[:, 0]) / 1e9:6.2f} TB/s read   "
                    f"wall {stat(v[:, 1])}   dev/copy {np.median(v[:, 0]) / np.median(cp):5.3f}")

            # ---- 2. end to end
            say("# 2. end to end: resolve_cost (diff + update) vs resolve with the hand-written rectangle vs the full solve")
            for case, new, kind in (("raised", raised, L.CHANGE_ANY), ("lowered", lowered, L.CHANGE_LOWERED)):
                rows = {"full": [], "hand": [], "auto": []}
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fim.solve(new.data_ptr(), T.data_ptr(), goal, stream)
                    wall = (time.perf_counter() - t0) * 1e3
                    if rep:
                        rows["full"].append((fim.stats()["solve_ms"], wall))
                    Tu.copy_(T_old)
                    fim.adopt(new.data_ptr(), Tu.data_ptr(), goal, stream)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fim.resolve(rect, [kind], stream)
                    wall = (time.perf_counter() - t0) * 1e3
                    if rep:
                        rows["hand"].append((fim.stats()["solve_ms"], wall))
                    Tu.copy_(T_old)
                    fim.adopt(cost.data_ptr(), Tu.data_ptr(), goal, stream)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fim.resolve_cost(new.data_ptr(), stream)
                    wall = (time.perf_counter() - t0) * 1e3
                    di = fim.diff_info()
                    if rep:
                        rows["auto"].append((fim.stats()["solve_ms"] + di["device_us"] / 1e3, wall))
                    assert di["solved_from_scratch"] == 0 and di["rects"] >= 1, di
                torch.cuda.synchronize()
                both = torch.isfinite(T) & torch.isfinite(Tu)
                same = bool((torch.isfinite(T) == torch.isfinite(Tu)).all())
                dmax = float((T[both] - Tu[both]).abs().max()) if bool(both.any()) else 0.0
                f, hd, au = (np.array(rows[k]) for k in ("full", "hand", "auto"))
                say(f"{case:8s} full solve        dev {stat(f[:, 0])}   wall {stat(f[:, 1])}")
                say(f"{case:8s} resolve(rect)     dev {stat(hd[:, 0])}   wall {stat(hd[:, 1])}")
                say(f"{case:8s} resolve_cost      dev {stat(au[:, 0])}   wall {stat(au[:, 1])}   over the rectangle: dev "
                    f"{np.median(au[:, 0]) - np.median(hd[:, 0]):+.3f}, wall {np.median(au[:, 1]) - np.median(hd[:, 1]):+.3f}; "
                    f"/ full solve: dev {np.median(au[:, 0]) / np.median(f[:, 0]):.3f}, wall {np.median(au[:, 1]) / np.median(f[:, 1]):.3f}; "
                    f"max|dT| {dmax:.2e}{'' if same else '  MASKS DIFFER'}")

            # ---- 3. the share
            say("# 3. the share: ANY tiles scattered (one cell doubled per tile), resolve_cost with the rule off vs the full solve")
            ctx.set_option(L.OPT_DIFF_SHARE, 2.0)
            ntx = (N + 63) // 64
            rng = np.random.default_rng(N)
            for share in (1 / 64, 1 / 16, 1 / 4, 1 / 2, 1.0):
                pick = rng.permutation(tiles)[: max(1, int(round(share * tiles)))]
                ys = torch.from_numpy(np.minimum(pick // ntx * 64 + rng.integers(0, 64, len(pick)), N - 1)).to(dev)
                xs = torch.from_numpy(np.minimum(pick % ntx * 64 + rng.integers(0, 64, len(pick)), N - 1)).to(dev)
                new = cost.clone()
                new[ys, xs] *= 2.0  # (a +inf cell stays +inf: the tile then counts as unchanged, see `tiles` below)
                new[N // 2, N // 2] = cost[N // 2, N // 2]
                rows = {"full": [], "auto": []}
                di = info = None
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fim.solve(new.data_ptr(), T.data_ptr(), goal, stream)
                    wall = (time.perf_counter() - t0) * 1e3
                    if rep:
                        rows["full"].append((fim.stats()["solve_ms"], wall))
                    Tu.copy_(T_old)
                    fim.adopt(cost.data_ptr(), Tu.data_ptr(), goal, stream)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fim.resolve_cost(new.data_ptr(), stream)
                    wall = (time.perf_counter() - t0) * 1e3
                    di, info = fim.diff_info(), fim.update_info()
                    if rep:
                        rows["auto"].append((fim.stats()["solve_ms"] + di["device_us"] / 1e3, wall))
                torch.cuda.synchronize()
                both = torch.isfinite(T) & torch.isfinite(Tu)
                same = bool((torch.isfinite(T) == torch.isfinite(Tu)).all())
                dmax = float((T[both] - Tu[both]).abs().max()) if bool(both.any()) else 0.0
                f, au = np.array(rows["full"]), np.array(rows["auto"])
                gain = np.median(f[:, 1]) - np.median(au[:, 1])
                say(f"share {share:6.4f}: tiles {di['tiles_changed']:6d} rects {di['rects']:5d} side {di['block_side']} cells reset "
                    f"{info['cells']:10d} | update dev {stat(au[:, 0])} wall {stat(au[:, 1])} | full dev {stat(f[:, 0])} wall "
                    f"{stat(f[:, 1])} | full - update (wall) {gain:+8.3f} vs the full solve's spread {f[:, 1].max() - f[:, 1].min():.3f}"
                    f"{'  FELL BACK' if info['fell_back'] else ''}; max|dT| {dmax:.2e}{'' if same else '  MASKS DIFFER'}")
                del new
            ctx.set_option(L.OPT_DIFF_SHARE, -1.0)
            fim.close()
            del cost, T, Tu, spare, T_old, fin, raised, lowered
            torch.cuda.empty_cache()
    ctx.close()
    log.close()


if __name__ == "__main__":
    main()
