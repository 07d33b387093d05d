"""Drop-in ``FastMarching.FastMarching`` (reference: src/FastMarching/FastMarching.py).

Same function names, argument meaning and return types as the reference; the Eikonal solves,
the gradient and the path extraction run on the GPU (libeikonal.so via ctypes):

  computeTmap(costMap, goal, start)      FastMarching.py:92-112   -> GPU block-FIM, full field
  biComputeTmap(costMap, goal, start)    FastMarching.py:114-162  -> GPU fields + GPU join
  getPathGDM(T, init, end, tau)          FastMarching.py:164-236  -> GPU path kernel
  computeGradient(cost, point=[])        FastMarching.py:242-300  -> GPU gradient kernel

Additions with no reference counterpart:
  getPathsGDM(T, inits, end, tau)        many getPathGDM walks on one field in one GPU launch
  updateTmap(costMap, Tmap, goal, changed)  computeTmap's field after local cost changes, from the old field
  computeTmapMulti(costMap, goals, offsets, labels)  the field of a goal set with start values (+ nearest-goal labels)
  getPathsToNearest(T, labels, goals, inits, tau, safe=False)  each start's path to the goal its cell belongs to, one launch
  getPathSafe(T, init, end, tau)         the obstacle-safe walk: a step blocked by a +inf cell or a stalled walk
                                         descends node to node instead; 0 < tau <= 1
  getPathsSafe(T, inits, end, tau)       many getPathSafe walks on one field in one GPU launch

getPathGDM, getPathsGDM and getPathsToNearest's default keep the reference's behaviour beside +inf cells,
the truncated path of its NaN fallback included; the safe walks are a mode of their own.

Scalar/list helpers that the reference exposes at module level keep their reference
semantics on the host (they operate on Python scalars and lists the caller owns):
  getEikonal :17-29, getNeighbours :31-42, updateNode :44-80, getMinNB :82-89,
  interpolatePoint :305-338.

Differences from the reference, by design:
  * computeTmap returns the full converged field (the reference raises ValueError at :107);
    with a `start` the values of every cell the reference would have closed are identical.
  * biComputeTmap returns the reference's PARTIAL goal/start fields (closed cells at their
    final values, the band at its final value where the reference holds a tentative one, the
    rest inf) and the join read from the two fronts' pop ranks.
  * the reference raises StopIteration on some tied decrease-keys (:72-73); the GPU solver has
    no narrow band and returns the intended field.  The host helper updateNode keeps that
    behaviour (and the IndexError of a search that runs past the band's end).
  * dtype: fields are computed in float64 by default (EIKONAL_DTYPE=float32 for fp32 speed).
"""
import bisect
import math
import os

import numpy as np

from eikonal import default_context, PATH_ERROR, PATH_STUCK
from eikonal._lib import OPT_EXACT_BAND

_DTYPE = np.float32 if os.environ.get("EIKONAL_DTYPE", "float64") in ("float32", "f32") else np.float64


def _ctx():
    return default_context(int(os.environ.get("EIKONAL_DEVICE", "0")))


# ------------------------------------------------------------------ scalar / list helpers
def getEikonal(Thor, Tver, cost):
    """FastMarching.py:17-29 (scalar 2D Godunov update)."""
    if np.isinf(Thor):
        if np.isinf(Tver):
            return np.inf
        return Tver + cost
    if np.isinf(Tver):
        return Thor + cost
    if cost < np.abs(Thor - Tver):
        return np.minimum(Thor, Tver) + cost
    return .5 * (Thor + Tver + math.sqrt(2 * np.power(cost, 2) - np.power(Thor - Tver, 2)))


def getNeighbours(nodeTarget, closedMap):
    """FastMarching.py:31-42 (unused by the reference planner)."""
    out = []
    for d in ([-1, 0], [1, 0], [0, -1], [0, 1]):
        n = np.add(nodeTarget[0:2], d)
        if closedMap[n[1], n[0]] == 0:
            out.append(n)
    return out


def _band_index(nbNodes, lo, c):
    """The band search of FastMarching.py:73: enumerate(nbNodes[lo-1:], lo) visits the indices
    lo .. lo + len(nbNodes[lo-1:]) - 1.  For lo >= 1 that is lo .. len(nbNodes) (the last one is
    past the end: IndexError if c was not found before it); for lo == 0 the slice [-1:] holds one
    entry, so only index 0 is tested (StopIteration if c is not first)."""
    count = min(1, len(nbNodes)) if lo == 0 else len(nbNodes) - lo + 1
    for k in range(lo, lo + count):
        if np.array_equal(c, nbNodes[k]):
            return k
    raise StopIteration


def updateNode(nodeTarget, costMap, Tmap, nbT, nbNodes, closedMap):
    """FastMarching.py:44-80: narrow-band update of the four children of nodeTarget.
    Host bookkeeping on the caller's lists; the GPU solver does not use a narrow band."""
    for d in ([0, -1], [0, 1], [-1, 0], [1, 0]):
        c = np.add(nodeTarget, d)
        if closedMap[c[1], c[0]] != 0:
            continue
        Thor = np.minimum(Tmap[c[1], c[0] + 1], Tmap[c[1], c[0] - 1])
        Tver = np.minimum(Tmap[c[1] + 1, c[0]], Tmap[c[1] - 1, c[0]])
        T = getEikonal(Thor, Tver, costMap[c[1], c[0]])
        if np.isinf(Tmap[c[1], c[0]]):
            i = bisect.bisect_left(nbT, T)
            nbT.insert(i, T)
            nbNodes.insert(i, c)
            Tmap[c[1], c[0]] = T
        elif T < Tmap[c[1], c[0]]:
            i = _band_index(nbNodes, bisect.bisect_left(nbT, Tmap[c[1], c[0]]), c)
            del nbT[i]
            del nbNodes[i]
            i = bisect.bisect_left(nbT, T)
            nbT.insert(i, T)
            nbNodes.insert(i, c)
            Tmap[c[1], c[0]] = T
    return Tmap, nbT, nbNodes


def getMinNB(nbT, nbNodes):
    """FastMarching.py:82-89: pop the smallest entry of the sorted narrow band."""
    node = nbNodes.pop(0)
    del nbT[0]
    return node, nbT, nbNodes


def interpolatePoint(point, mapI):
    """FastMarching.py:305-338 (scalar bilinear interpolation with the reference's branches)."""
    i = np.uint32(np.fix(point[0]))
    j = np.uint32(np.fix(point[1]))
    a = point[0] - i
    b = point[1] - j
    m, n = np.uint32(mapI.shape)
    if i == n:
        if j == m:
            return mapI[j, i]
        return b * mapI[j + 1, i] + (1 - b) * mapI[j, i]
    if j == m:
        return a * mapI[j, i + 1] + (1 - a) * mapI[j, i]
    a00 = mapI[j, i]
    a10 = mapI[j, i + 1] - mapI[j, i]
    a01 = mapI[j + 1, i] - mapI[j, i]
    a11 = mapI[j + 1, i + 1] + mapI[j, i] - mapI[j, i + 1] - mapI[j + 1, i]
    if a == 0:
        return a00 if b == 0 else a00 + a01 * b
    return a00 + a10 * a if b == 0 else a00 + a10 * a + a01 * b + a11 * a * b


# ---------------------------------------------------------------------------- GPU paths
def _node(p):
    return int(p[0]), int(p[1])


def computeTmap(costMap, goal, start=None):
    """FastMarching.py:92-112 -> arrival-time field T (float64, inf = unreached)."""
    cost = np.ascontiguousarray(costMap, dtype=_DTYPE)
    T = _ctx().tmap2d(cost, _node(goal), dtype=_DTYPE)
    return T.astype(np.float64, copy=False)


_MAX_RECTS = 1024  # eik_fim2d_update's limit


def _mask_rects(mask, block=64, limit=_MAX_RECTS):
    """The bounding box of a boolean (H, W) mask's True cells per block x block cells -> (x0, y0, x1, y1).
    A mask that touches more than `limit` blocks is boxed per block of twice the side, and so on: fewer,
    larger rectangles, which only invalidate more (every changed cell stays covered)."""
    mask = np.asarray(mask, dtype=bool)
    while True:
        rects = []
        for y0 in range(0, mask.shape[0], block):
            rows = mask[y0:y0 + block]
            if not rows.any():
                continue
            for x0 in range(0, mask.shape[1], block):
                ys, xs = np.nonzero(rows[:, x0:x0 + block])
                if len(ys):
                    rects.append((x0 + int(xs.min()), y0 + int(ys.min()), x0 + int(xs.max()) + 1, y0 + int(ys.max()) + 1))
        if len(rects) <= limit:
            return rects
        block *= 2


def updateTmap(costMap, Tmap, goal, changed):
    """No reference counterpart: the field computeTmap(costMap, goal) would return, from Tmap -- the
    field computeTmap returned for an earlier costMap that differs from this one only inside `changed`,
    a list of at most 1024 (x0, y0, x1, y1) rectangles (half-open) or a boolean (H, W) mask of the
    changed cells (boxed per 64 x 64 block, per larger blocks if that gives more than 1024 rectangles).
    Only the cells whose old value depended on a changed cell are solved again.
    The inputs are not modified; the result is float64."""
    cost = np.ascontiguousarray(costMap, dtype=_DTYPE)
    if np.shape(Tmap) != cost.shape:
        raise ValueError(f"updateTmap: Tmap has shape {np.shape(Tmap)}, costMap {cost.shape}")
    ch = np.asarray(changed)
    if ch.dtype == bool and ch.shape != cost.shape:
        raise ValueError(f"updateTmap: the mask has shape {ch.shape}, costMap {cost.shape}")
    rects = _mask_rects(ch) if ch.dtype == bool and ch.shape == cost.shape else [tuple(int(v) for v in r) for r in changed]
    if not rects:
        return np.array(Tmap, dtype=np.float64, order="C")
    T = _ctx().tmap2d_update(cost, np.ascontiguousarray(Tmap, dtype=_DTYPE), _node(goal), rects, dtype=_DTYPE)
    return T.astype(np.float64, copy=False)


def updateTmapFromCost(costMap, oldCostMap, Tmap, goal):
    """No reference counterpart: the field computeTmap(costMap, goal) would return, from Tmap -- the
    field computeTmap returned for oldCostMap.  The two cost maps are compared on the device, so no mask
    or rectangle is needed; only the cells whose old value depended on a raised cell are solved again
    (DESIGN.md §3.15).  The inputs are not modified; the result is float64."""
    cost = np.ascontiguousarray(costMap, dtype=_DTYPE)
    old = np.ascontiguousarray(oldCostMap, dtype=_DTYPE)
    if old.shape != cost.shape or np.shape(Tmap) != cost.shape:
        raise ValueError(f"updateTmapFromCost: costMap {cost.shape}, oldCostMap {old.shape}, Tmap {np.shape(Tmap)}")
    T = _ctx().tmap2d_update_cost(old, cost, np.ascontiguousarray(Tmap, dtype=_DTYPE), _node(goal), dtype=_DTYPE)
    return T.astype(np.float64, copy=False)


def biComputeTmap(costMap, goal, start):
    """FastMarching.py:114-162 -> (TmapG, TmapS, nodeJoin uint32[2]).  EIKONAL_EXACT_BAND=1: the
    reference's own band values and LIFO ties, bit for bit (EIK_OPT_EXACT_BAND, csrc/bidir_exact.hip;
    ~6x the default's time on a 4096^2 raster)."""
    cost = np.ascontiguousarray(costMap, dtype=np.float64)
    c = _ctx()
    c.set_option(OPT_EXACT_BAND, 1 if os.environ.get("EIKONAL_EXACT_BAND", "0") not in ("", "0") else 0)
    TG, TS, join = c.tmap2d_bidir(cost, _node(goal), _node(start))
    return TG, TS, np.uint32(join)


def getPathGDM(totalCostMap, initWaypoint, endWaypoint, tau):
    """FastMarching.py:164-236 -> (K, 2) float64 path, first row init, last row end
    (a NaN-gradient fallback returns the reference's truncated path, :217-218)."""
    init = np.asarray(initWaypoint, dtype=np.float64).reshape(-1)[:2]
    end = np.asarray(endWaypoint, dtype=np.float64).reshape(-1)[:2]
    path, status = _ctx().path2d(np.ascontiguousarray(totalCostMap, dtype=np.float64), init, end, float(tau))
    if status == PATH_ERROR:
        raise IndexError("getPathGDM: the descent left the field (the reference raises here too)")
    return path


def getPathsGDM(totalCostMap, initWaypoints, endWaypoint, tau):
    """No reference counterpart: getPathGDM from every row of initWaypoints (P, 2) to endWaypoint on
    one field, in one launch -> a list of P (K, 2) float64 paths, each equal to getPathGDM's for
    that start; IndexError if any of them raises there."""
    inits = np.asarray(initWaypoints, dtype=np.float64)
    inits = inits.reshape(-1, inits.shape[-1])[:, :2]
    end = np.asarray(endWaypoint, dtype=np.float64).reshape(-1)[:2]
    res = _ctx().path2d_batch(np.ascontiguousarray(totalCostMap, dtype=np.float64), inits, end, float(tau))
    bad = [p for p, (_, status) in enumerate(res) if status == PATH_ERROR]
    if bad:
        raise IndexError(f"getPathsGDM: the descent of path {bad[0]} left the field (getPathGDM raises here too)")
    return [path for path, _ in res]


def _safe_paths(who, res):
    """the paths of Context.path2d_safe* results; IndexError / RuntimeError naming the first bad path"""
    for p, (path, status, _) in enumerate(res):
        if status == PATH_ERROR:
            raise IndexError(f"{who}: the descent of path {p} left the field or started on an impassable cell")
        if status == PATH_STUCK:
            last = tuple(int(round(v)) for v in path[-1])
            raise RuntimeError(f"{who}: path {p} is stuck at node {last}: no lower neighbour, or out of iterations")
    return [path for path, _, _ in res]


def getPathSafe(totalCostMap, initWaypoint, endWaypoint, tau):
    """No reference counterpart: getPathGDM's walk made safe beside +inf cells -> (K, 2)
    float64 path from init to end.  A step whose interpolation would use an impassable node, and a walk
    whose arrival time stops falling, descend node to node instead; no returned point lies nearest an
    impassable node (tau <= 0.5, converged field).  Equal to getPathGDM's path up to the first such step.
    0 < tau <= 1 (ValueError).  RuntimeError: stuck (names the last node); IndexError as getPathGDM."""
    if not 0 < tau <= 1:
        raise ValueError(f"getPathSafe: tau = {tau} (0 < tau <= 1 needed)")
    init = np.asarray(initWaypoint, dtype=np.float64).reshape(-1)[:2]
    end = np.asarray(endWaypoint, dtype=np.float64).reshape(-1)[:2]
    res = _ctx().path2d_safe(np.ascontiguousarray(totalCostMap, dtype=np.float64), init, end, float(tau))
    return _safe_paths("getPathSafe", [res])[0]


def getPathsSafe(totalCostMap, initWaypoints, endWaypoint, tau):
    """No reference counterpart: getPathSafe from every row of initWaypoints (P, 2) to endWaypoint on one
    field, in one launch -> a list of P (K, 2) float64 paths, each equal to getPathSafe's for that start."""
    if not 0 < tau <= 1:
        raise ValueError(f"getPathsSafe: tau = {tau} (0 < tau <= 1 needed)")
    inits = np.asarray(initWaypoints, dtype=np.float64)
    inits = inits.reshape(-1, inits.shape[-1])[:, :2]
    end = np.asarray(endWaypoint, dtype=np.float64).reshape(-1)[:2]
    res = _ctx().path2d_safe_batch(np.ascontiguousarray(totalCostMap, dtype=np.float64), inits, end, float(tau))
    return _safe_paths("getPathsSafe", res)


def _goal_list(goals, shape):
    """goals as a (K, 2) int64 array of nodes (x, y): a list of nodes, or a boolean mask of `shape` whose
    True cells are the seeds in row-major order"""
    g = np.asarray(goals)
    if g.dtype == bool:
        if g.shape != tuple(shape):
            raise ValueError(f"computeTmapMulti: the mask has shape {g.shape}, costMap {tuple(shape)}")
        ys, xs = np.nonzero(g)  # row-major
        return np.stack([xs, ys], axis=1).astype(np.int64)
    if g.ndim != 2 or g.shape[1] < 2:
        raise ValueError(f"computeTmapMulti: goals must be K nodes (x, y) or a boolean mask, not shape {g.shape}")
    return np.ascontiguousarray(g[:, :2], dtype=np.int64)


def computeTmapMulti(costMap, goals, offsets=None, labels=False):
    """No reference counterpart: the arrival-time field of a goal SET, min over the goals of (offset +
    cost-to-go), solved as one problem.  goals: K nodes (x, y), or a boolean mask of
    costMap's shape (its True cells, row-major); offsets: K start values >= 0 (None: all 0).  Returns T
    (float64), or with labels=True (T, labels): int32, the index into goals of the goal each cell
    belongs to, -1 for unreached cells."""
    cost = np.ascontiguousarray(costMap, dtype=_DTYPE)
    g = _goal_list(goals, cost.shape)
    if len(g) == 0:
        raise ValueError("computeTmapMulti: no goal")
    res = _ctx().tmap2d_seeds(cost, g, offsets, dtype=_DTYPE, labels=labels)
    if labels:
        return res[0].astype(np.float64, copy=False), res[1]
    return res.astype(np.float64, copy=False)


def updateTmapMulti(costMap, Tmap, goals, changed, offsets=None, newGoals=None, newOffsets=None, labels=False):
    """No reference counterpart: the field computeTmapMulti(costMap, newGoals, newOffsets) would return,
    from Tmap -- the field computeTmapMulti returned for `goals` / `offsets` and an earlier costMap that
    differs from this one only inside `changed` (rectangles or a boolean mask, as in updateTmap).
    newGoals=None: the goal set is unchanged (newOffsets then needs newGoals).  Only the cells whose old
    value depended on a changed cell, or on a goal that was dropped or whose offset went up, are solved
    again.  The inputs are not modified; the result is float64, or with labels=True
    (T, labels) with labels indexing the new goals."""
    cost = np.ascontiguousarray(costMap, dtype=_DTYPE)
    if np.shape(Tmap) != cost.shape:
        raise ValueError(f"updateTmapMulti: Tmap has shape {np.shape(Tmap)}, costMap {cost.shape}")
    ch = np.asarray(changed)
    if ch.dtype == bool and ch.shape != cost.shape:
        raise ValueError(f"updateTmapMulti: the mask has shape {ch.shape}, costMap {cost.shape}")
    g = _goal_list(goals, cost.shape)
    if len(g) == 0:
        raise ValueError("updateTmapMulti: no goal")
    if offsets is not None and len(np.ravel(offsets)) != len(g):
        raise ValueError(f"updateTmapMulti: {len(g)} goals but {len(np.ravel(offsets))} offsets")
    gn = None
    if newGoals is not None:
        gn = _goal_list(newGoals, cost.shape)
        if len(gn) == 0:
            raise ValueError("updateTmapMulti: no new goal (None keeps the goals)")
        if newOffsets is not None and len(np.ravel(newOffsets)) != len(gn):
            raise ValueError(f"updateTmapMulti: {len(gn)} new goals but {len(np.ravel(newOffsets))} new offsets")
    elif newOffsets is not None:
        raise ValueError("updateTmapMulti: newOffsets without newGoals")
    rects = _mask_rects(ch) if ch.dtype == bool and ch.shape == cost.shape else [tuple(int(v) for v in r) for r in changed]
    if not rects and gn is None:
        T = np.array(Tmap, dtype=np.float64, order="C")
        return (T, _ctx().labels2d(np.ascontiguousarray(Tmap, dtype=_DTYPE), g, offsets)) if labels else T
    res = _ctx().tmap2d_update_seeds(cost, np.ascontiguousarray(Tmap, dtype=_DTYPE), g, offsets, rects, seeds_new=gn,
                                     t0_new=newOffsets, dtype=_DTYPE, labels=labels)
    if labels:
        return res[0].astype(np.float64, copy=False), res[1]
    return res.astype(np.float64, copy=False)


def getPathsToNearest(totalCostMap, labels, goals, initWaypoints, tau, safe=False):
    """No reference counterpart: from every row of initWaypoints (P, 2), getPathGDM to the goal its cell
    belongs to -- goals[labels[node(start)]], with (totalCostMap, labels) from computeTmapMulti(...,
    labels=True) and the same goals -- in one launch -> a list of P (K, 2) float64 paths.  ValueError
    names a start whose cell has no label (-1: unreached); IndexError as getPathsGDM.  safe=True walks
    as getPathSafe does (0 < tau <= 1; RuntimeError names a stuck path) instead of as getPathGDM."""
    T = np.ascontiguousarray(totalCostMap, dtype=np.float64)
    lab = np.asarray(labels)
    if lab.shape != T.shape:
        raise ValueError(f"getPathsToNearest: labels have shape {lab.shape}, the field {T.shape}")
    g = _goal_list(goals, T.shape)
    inits = np.asarray(initWaypoints, dtype=np.float64)
    inits = inits.reshape(-1, inits.shape[-1])[:, :2]
    ends = np.empty_like(inits)
    for p, s in enumerate(inits):
        x, y = _node(s)
        k = int(lab[y, x]) if 0 <= x < T.shape[1] and 0 <= y < T.shape[0] else -1
        if k < 0 or k >= len(g):
            raise ValueError(f"getPathsToNearest: start {p} ({x}, {y}) belongs to no goal (label {k})")
        ends[p] = g[k]
    if safe:
        if not 0 < tau <= 1:
            raise ValueError(f"getPathsToNearest: tau = {tau} (0 < tau <= 1 needed with safe=True)")
        return _safe_paths("getPathsToNearest", _ctx().path2d_safe_batch(T, inits, ends, float(tau)))
    res = _ctx().path2d_batch(T, inits, ends, float(tau))
    bad = [p for p, (_, status) in enumerate(res) if status == PATH_ERROR]
    if bad:
        raise IndexError(f"getPathsToNearest: the descent of path {bad[0]} left the field (getPathGDM raises here too)")
    return [path for path, _ in res]


def computeGradient(cost, point=[]):
    """FastMarching.py:242-300 -> (Gnx, Gny): inf-aware normalised gradient; with a point only
    the window [int(p)-3, int(p)+3) is filled (zeros elsewhere), as in the reference."""
    T = np.ascontiguousarray(cost, dtype=np.float64)
    gx, gy = _ctx().gradient2d(T)
    if len(point) != 0:
        m, n = T.shape
        jmax, imax = min(m, int(point[1]) + 3), min(n, int(point[0]) + 3)
        jmin, imin = max(0, int(point[1] - 3)), max(0, int(point[0] - 3))
        mask = np.zeros_like(T, dtype=bool)
        mask[jmin:jmax, imin:imax] = True
        gx = np.where(mask, gx, 0.0)
        gy = np.where(mask, gy, 0.0)
    return gx, gy
