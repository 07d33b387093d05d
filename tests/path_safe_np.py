"""The obstacle-safe 2D path rule (eik_path2d_safe_*, csrc/gdm_safe.hip) restated on the host: the
specification the kernel is tested against.  Host only, numpy + plain Python.

The walk is getPathGDM's (FastMarching.py:164-236) with three changes:
  * the gradient field G' is computeGradient's (Gnx, Gny) with NaN at every node whose T is +inf, so
    a step whose interpolation uses an impassable corner is blocked (as is the reference's own NaN);
  * a blocked step takes the fallback of :178-218 as it was intended (and as FastMarching3D.py:212-264
    runs it): snap to the nearest node, back out of +inf nodes, step to the lowest 4-neighbour;
  * a walk whose T has not fallen for S = max(16, ceil(8 / tau)) iterations goes to that integer
    descent for good (the stall rule).

`sq` is how the step squares a component: the default is the exact product, the kernel's form; the
reference squares numpy scalars through libm pow(), `sq=lambda v: math.pow(v, 2)` with the oracle's
gradient as `grad` gives oracle.gdm2d's bits.
"""
import math

import numpy as np

DONE, FALLBACK, ERROR, STUCK = 0, 1, 2, 3
INF = math.inf


def stall_limit(tau):
    return max(16, math.ceil(8 / tau))


def gradient(T):
    """computeGradient (FastMarching.py:242-300) on the whole field with exact-product squares."""
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(all="ignore"):
        def axis(c, lo, hi):  # interior rule of :268-277 on three shifted views
            return np.where(np.isinf(hi), np.where(np.isinf(lo), 0.0, c - lo), np.where(np.isinf(lo), hi - c, (hi - lo) / 2))

        Gy = np.empty_like(T)
        Gx = np.empty_like(T)
        Gy[0] = T[1] - T[0]
        Gy[-1] = T[-1] - T[-2]
        Gy[1:-1] = axis(T[1:-1], T[:-2], T[2:])
        Gx[:, 0] = T[:, 1] - T[:, 0]
        Gx[:, -1] = T[:, -1] - T[:, -2]
        Gx[:, 1:-1] = axis(T[:, 1:-1], T[:, :-2], T[:, 2:])
        den = np.sqrt(Gx * Gx + Gy * Gy)
        return Gx / den, Gy / den


class SafeField:
    """T and G' as nested lists (fast scalar access), shared by the walks on one field."""

    def __init__(self, T, grad=None):
        T = np.asarray(T, dtype=np.float64)
        gx, gy = gradient(T) if grad is None else grad
        blocked = np.isinf(T)
        self.H, self.W = T.shape
        self.T = T.tolist()
        self.gx = np.where(blocked, np.nan, gx).tolist()
        self.gy = np.where(blocked, np.nan, gy).tolist()


def _interp(a, b, g00, g01, g10, g11):  # interpolatePoint :323-336
    a00 = g00
    a10 = g01 - g00
    a01 = g10 - g00
    a11 = g11 + g00 - g01 - g10
    if a == 0:
        return a00 if b == 0 else a00 + a01 * b
    return a00 + a10 * a if b == 0 else a00 + a10 * a + a01 * b + a11 * a * b


def safe_path(field, init, end, tau, cap=None, sq=None, stall=True, trace=None):
    """-> (path (K, 2) float64, status, info int64[4]): fallbacks taken, points dropped, the first
    iteration run in integer mode (-1: never), iterations run.  `field`: a SafeField or an (H, W)
    array.  stall=False switches the stall rule off (what the rule is measured against).  `trace`: a
    list that gets one (iteration, the points a fallback dropped) entry per fallback."""
    if not (0 < tau <= 1):
        raise ValueError(f"safe path: tau = {tau} (0 < tau <= 1 needed)")
    f = field if isinstance(field, SafeField) else SafeField(field)
    T, H, W = f.T, f.H, f.W
    sq = sq or (lambda v: v * v)
    steps = int(round(15000 / tau))
    cap = steps + 4 if cap is None else cap
    kmax = min(steps, cap - 1)
    S = stall_limit(tau)
    ex, ey = float(end[0]), float(end[1])
    pts = [(float(init[0]), float(init[1]))]
    status = DONE
    fallbacks = dropped = 0
    int_from = -1

    def bad(x, y):  # NaN point, or its interpolation cell leaves the raster
        return x != x or y != y or x < 0 or y < 0 or int(x) + 1 >= W or int(y) + 1 >= H

    def near(x, y):  # nearest node, Python round: half to even
        return min(max(round(x), 0), W - 1), min(max(round(y), 0), H - 1)

    stale = 0
    tlow = INF
    if not bad(*pts[0]):
        nx, ny = near(*pts[0])
        tlow = T[ny][nx]
    integer = False
    reached = False
    k = 0
    while k < kmax:
        px, py = pts[-1]
        k += 1
        if bad(px, py):
            status = ERROR
            break
        dx = dy = math.nan
        if not integer:
            i, j = int(px), int(py)
            a, b = px - i, py - j
            dx = _interp(a, b, f.gx[j][i], f.gx[j][i + 1], f.gx[j + 1][i], f.gx[j + 1][i + 1])
            dy = _interp(a, b, f.gy[j][i], f.gy[j][i + 1], f.gy[j + 1][i], f.gy[j + 1][i + 1])
        if dx != dx or dy != dy:
            fallbacks += 1
            gone = []
            if trace is not None:
                trace.append((k, gone))
            nx, ny = near(px, py)
            while T[ny][nx] == INF:
                gone.append(pts.pop())
                dropped += 1
                if not pts:
                    break
                nx, ny = near(*pts[-1])
            if not pts:
                status = ERROR
                break
            while pts and math.sqrt((pts[-1][0] - nx) * (pts[-1][0] - nx) + (pts[-1][1] - ny) * (pts[-1][1] - ny)) < 1:
                gone.append(pts.pop())
                dropped += 1
            pts.append((float(nx), float(ny)))
            best, child = T[ny][nx], None
            for cx, cy in ((nx, ny - 1), (nx, ny + 1), (nx - 1, ny), (nx + 1, ny)):
                if 0 <= cx < W and 0 <= cy < H and T[cy][cx] < best:
                    best, child = T[cy][cx], (cx, cy)
            if child is None:
                status = STUCK
                break
            pts.append((float(child[0]), float(child[1])))
        else:  # :220-229
            nrm = math.sqrt(dx * dx + dy * dy)
            if nrm < 0.01:
                den = math.sqrt(sq(dx) + sq(dy))
                dxn, dyn = dx / den, dy / den
            else:
                dxn = dx / math.sqrt(sq(dx) + sq(dy))
                dyn = dy / math.sqrt(sq(dxn) + sq(dy))
            pts.append((px - tau * dxn, py - tau * dyn))
        lx, ly = pts[-1]
        if math.sqrt((lx - ex) * (lx - ex) + (ly - ey) * (ly - ey)) < 1.5:  # :231
            reached = True
            break
        if stall and not integer and not bad(lx, ly):
            nx, ny = near(lx, ly)
            t = T[ny][nx]
            if t < tlow:
                tlow, stale = t, 0
            else:
                stale += 1
                if stale >= S:
                    integer = True
                    int_from = k
    if status == DONE and not reached:
        status = STUCK if kmax == steps else ERROR  # out of iterations / out of rows
    if status == DONE:
        pts.append((ex, ey))  # :234
    path = np.array(pts, dtype=np.float64).reshape(-1, 2)
    return path, status, np.array([fallbacks, dropped, int_from, k], dtype=np.int64)


def nearest_is_inf(T, pts):
    """per point: is its nearest node (half to even, clamped into the raster) a +inf node of T"""
    T = np.asarray(T)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    x = np.clip(np.rint(pts[:, 0]).astype(np.int64), 0, T.shape[1] - 1)
    y = np.clip(np.rint(pts[:, 1]).astype(np.int64), 0, T.shape[0] - 1)
    return np.isinf(T[y, x])
