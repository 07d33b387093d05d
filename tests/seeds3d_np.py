"""Goal sets for 3D solves: the specification in numpy, host only.

`seeded_reference3` is the expected field of a seed set in a volume: the fixed point from above of
T = min(T, update) from "+inf, the seeds at the min of their t0", with the update of
FastMarching3D.py:59-75.  `label_rule3` is the label rule of include/eikonal.h (eik_labels3d_dev).
tests/test_seeds3d_abi.py checks them against the oracle and against each other, tests/test_gpu_seeds3d.py
compares the device with them.

Layout as everywhere: cost[y][x][z], nodes and seeds (x, y, z).
"""
import numpy as np

# the five seeds of the issue on raster((24, 48, 24)): 3 x 3 x 3 tiles of 16 x 8 x 8; (15, 7, 7) and
# (16, 8, 8) are the last cell of one tile and the first cell of its diagonal neighbour
FIVE_SHAPE = (24, 48, 24)
FIVE_SEEDS = [(3, 3, 3), (40, 20, 20), (15, 7, 7), (16, 8, 8), (30, 2, 12)]
FIVE_T0 = [0.0, 12.5, 40.0, 3.0, 1e4]
FIVE_UNDOMINATED = [True, True, False, True, False]


def update3(T, cost):
    """FastMarching3D.py:59-75 on every cell at once: the three axis minima (+inf outside the volume),
    sorted; the n-axis solution (S + sqrt(n C^2 + S^2 - n Q)) / n is taken for the largest n whose
    acceptance test C^2 > sum (Tmax - Ti)^2 holds, dropping the largest value each time it fails.  A cell
    where no n is accepted (no finite neighbour, +inf cost, or C = 0, where the reference raises) gets +inf."""
    H, W, L = T.shape
    P = np.full((H + 2, W + 2, L + 2), np.inf)
    P[1:-1, 1:-1, 1:-1] = T
    s = np.sort(np.stack([np.minimum(P[1:-1, :-2, 1:-1], P[1:-1, 2:, 1:-1]),      # x-1, x+1
                          np.minimum(P[:-2, 1:-1, 1:-1], P[2:, 1:-1, 1:-1]),      # y-1, y+1
                          np.minimum(P[1:-1, 1:-1, :-2], P[1:-1, 1:-1, 2:])]), axis=0)  # z-1, z+1
    C2 = cost * cost
    out = np.full(T.shape, np.inf)
    done = ~np.isfinite(cost)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in (3, 2, 1):
            t = s[:n]
            sumT = ((t[n - 1] - t) ** 2).sum(axis=0)  # NaN where Tmax = +inf: the test fails
            S, Q = t.sum(axis=0), (t * t).sum(axis=0)
            ok = (C2 > sumT) & ~done
            tr = (S + np.sqrt(n * C2 + S * S - n * Q)) / n
            out[ok] = tr[ok]
            done |= ok
    return out


def jacobi3(T, cost, count=None):
    """T = min(T, update3(T, cost)) to its fixed point (count: a one-element list that receives the
    number of iterations)"""
    T = np.array(T, np.float64)
    cost = np.asarray(cost, np.float64)
    it = 0
    while True:
        nv = np.minimum(T, update3(T, cost))
        it += 1
        if np.array_equal(nv, T):
            if count is not None:
                count.append(it)
            return T
        T = nv


def _t0(seeds, t0):
    return np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)


def seeded_reference3(cost, seeds, t0=None):
    """The field of the seed set: jacobi3 from T = +inf with the seeds at the min of their t0"""
    T = np.full(np.shape(cost), np.inf)
    for (x, y, z), v in zip(seeds, _t0(seeds, t0)):
        T[y, x, z] = min(T[y, x, z], v)
    return jacobi3(T, cost)


def label_rule3(T, seeds, t0=None):
    """The label rule of include/eikonal.h on one volume T (H x W x L, any float dtype): roots first,
    then every cell in ascending T takes the label of its strictly lowest 6-neighbour, ties in the order
    x-1, x+1, y-1, y+1, z-1, z+1 (a parent is strictly lower, so it is labelled before its child)."""
    H, W, L = T.shape
    t0 = _t0(seeds, t0).astype(T.dtype)  # (R)t0
    n = H * W * L
    lab = np.full(n, -1, np.int32)
    root = np.zeros(n, bool)
    for k in reversed(range(len(seeds))):  # of several roots on a cell the lowest k wins
        x, y, z = seeds[k]
        if T[y, x, z] == t0[k]:  # (non-negative, never NaN: == is equality of the bit patterns)
            lab[(y * W + x) * L + z] = k
            root[(y * W + x) * L + z] = True
    P = np.full((H + 2, W + 2, L + 2), np.inf, T.dtype)
    P[1:-1, 1:-1, 1:-1] = T
    nb = np.stack([P[1:-1, :-2, 1:-1], P[1:-1, 2:, 1:-1], P[:-2, 1:-1, 1:-1], P[2:, 1:-1, 1:-1],
                   P[1:-1, 1:-1, :-2], P[1:-1, 1:-1, 2:]])
    best = nb.argmin(axis=0)  # the first of equal minima
    has = (np.isfinite(T) & (nb.min(axis=0) < T)).ravel() & ~root
    par = np.arange(n) + np.array([-L, L, -W * L, W * L, -1, 1])[best.ravel()]
    for i in np.argsort(T.ravel(), kind="stable"):
        if has[i]:
            lab[i] = lab[par[i]]
    return lab.reshape(H, W, L)


def undominated3(R, seeds, t0=None):
    """per seed: the reference field holds this seed's t0 at its cell (no other seed's wave, and no lower
    seed on the same cell, undercut it)"""
    return [bool(R[y, x, z] == v) for (x, y, z), v in zip(seeds, _t0(seeds, t0))]
