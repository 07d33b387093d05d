"""The invalidation rule of the incremental re-solve, on the CPU against the oracle.

After the cost changed inside some rectangles, the CONE is the closure of "p joins if a 4-neighbour q
in the cone has T_old(q) <= T_old(p), p finite, p not the goal", seeded with the finite-T_old cells of
the rectangles whose cost may have gone up.  Setting the cone to +inf, keeping T_old elsewhere and
iterating T = min(T, godunov) on the new cost must reach the field of the new cost: masks equal,
values within 1e-9 of the oracle's.  `closure` is the helper the GPU tests compare the device's
invalidated set with, cell for cell.
"""
import numpy as np
import pytest

import oracle as O
from dd_cpu import godunov


def closure(T, seeds, goal):
    """The cone of the boolean (H, W) mask `seeds` in the field T (any float dtype; non-negative
    values compare like their bit patterns)."""
    H, W = T.shape
    fin = np.isfinite(T).ravel()
    Tf = T.ravel()
    gidx = goal[1] * W + goal[0]
    M = (np.asarray(seeds, bool).ravel() & fin).copy()
    M[gidx] = False
    front = np.flatnonzero(M)
    while front.size:
        y, x = np.divmod(front, W)
        nxt = []
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            yy, xx = y + dy, x + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            p, q = yy[ok] * W + xx[ok], front[ok]
            take = fin[p] & ~M[p] & (Tf[q] <= Tf[p]) & (p != gidx)
            p = np.unique(p[take])
            M[p] = True
            nxt.append(p)
        front = np.unique(np.concatenate(nxt))
    return M.reshape(H, W)


def rect_mask(shape, rects):
    m = np.zeros(shape, bool)
    for x0, y0, x1, y1 in rects:
        m[max(y0, 0):y1, max(x0, 0):x1] = True
    return m


def jacobi(T, cost):
    """T = min(T, godunov(neighbour minima, cost)) to its fixed point"""
    T = T.copy()
    while True:
        P = np.full((T.shape[0] + 2, T.shape[1] + 2), np.inf)
        P[1:-1, 1:-1] = T
        a = np.minimum(P[1:-1, :-2], P[1:-1, 2:])
        b = np.minimum(P[:-2, 1:-1], P[2:, 1:-1])
        with np.errstate(invalid="ignore"):
            nv = np.minimum(T, godunov(a, b, cost))
        if np.array_equal(nv, T):
            return T
        T = nv


def oracle_field(cost, goal):
    O.set_strict(False)
    try:
        return O.fmm2d(np.asarray(cost, np.float64), list(goal))
    finally:
        O.set_strict(True)


def make_case(kind, change, seed):
    rng = np.random.default_rng(seed)
    H, W = (int(v) for v in rng.integers(60, 161, 2))
    if kind == "uniform":
        c = np.full((H, W), 2.0)
    elif kind == "integer":
        c = rng.integers(1, 10, (H, W)).astype(np.float64)
    else:
        c = rng.uniform(1, 10, (H, W))
    if kind == "obst":
        c[rng.random((H, W)) < 0.2] = np.inf
    goal = (W // 3, H // 2)
    c[goal[1], goal[0]] = 1.0
    new = c.copy()
    raised, lowered = [], []
    for k in range(int(rng.integers(1, 4))):
        while True:
            w, h = (int(v) for v in rng.integers(3, 25, 2))
            x0, y0 = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            if not (x0 <= goal[0] < x0 + w and y0 <= goal[1] < y0 + h):
                break
        up = change == "raised" or (change == "mixed" and k % 2 == 0)
        # (every cost is >= 1, so 1.0 never raises one; rectangles may overlap: a raised rectangle
        # seeds all of its cells whatever a later one wrote over them, which is always safe)
        new[y0:y0 + h, x0:x0 + w] = np.inf if up else 1.0
        (raised if up else lowered).append((x0, y0, x0 + w, y0 + h))
    outside_raised = ~rect_mask(c.shape, raised)
    assert not (outside_raised & (new > c)).any()  # no cost went up outside the raised rectangles
    return c, new, goal, raised, lowered


CASES = [(k, ch, s) for k in ("uniform", "integer", "obst", "float") for ch in ("raised", "lowered", "mixed")
         for s in (0, 1)]


@pytest.mark.parametrize("kind,change,seed", CASES)
def test_cone_restart_reaches_the_new_field(kind, change, seed):
    c, new, goal, raised, lowered = make_case(kind, change, 1000 * CASES.index((kind, change, seed)) + seed)
    T_old = oracle_field(c, goal)
    R = oracle_field(new, goal)
    cone = closure(T_old, rect_mask(c.shape, raised), goal)
    start = np.where(cone, np.inf, T_old)
    # the restart state is a supersolution of the new problem, up to the sequential FMM's last ulp
    fin = np.isfinite(R)
    assert (start[fin] >= R[fin] - 4 * np.spacing(R[fin])).all()
    T = jacobi(start, new)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    assert T[goal[1], goal[0]] == 0
    if fin.any():
        assert np.abs(T[fin] - R[fin]).max() <= 1e-9
    if change == "raised":
        # a raise-only change leaves every cell outside the cone at its old value: the oracle's two
        # fields agree there to 1 ulp (its pop order may differ between the two runs)
        keep = ~cone & np.isfinite(T_old)
        assert np.array_equal(np.isfinite(R[~cone]), np.isfinite(T_old[~cone]))
        assert (np.abs(R[keep] - T_old[keep]) <= np.spacing(T_old[keep])).all()


def test_closure_floods_ties_both_ways_and_spares_the_goal():
    T = np.array([[2.0, 1.0, 2.0, 3.0],
                  [1.0, 0.0, 1.0, np.inf],
                  [2.0, 1.0, 2.0, 5.0]])
    goal = (1, 1)
    seeds = np.zeros(T.shape, bool)
    seeds[0, 1] = True  # T = 1: reaches the 2s beside it, the 3 behind them, never the goal or the other 1s
    M = closure(T, seeds, goal)
    want = np.zeros(T.shape, bool)
    want[0, :] = True
    want[0, 1] = True
    assert np.array_equal(M, want), M
    seeds[:] = False
    seeds[1, 3] = True  # an unreached cell seeds nothing
    assert not closure(T, seeds, goal).any()
    Tt = np.array([[0.0, 1.0, 1.0, 1.0]])  # ties flood both ways
    seeds = np.array([[False, False, True, False]])
    assert np.array_equal(closure(Tt, seeds, (0, 0)), np.array([[False, True, True, True]]))


def test_mask_rectangles_cover_the_mask_and_stay_within_the_update_limit():
    """FastMarching.updateTmap's mask form: one box per 64 x 64 block, per larger blocks when that would
    be more rectangles than eik_fim2d_update takes (1024); every True cell stays covered"""
    import FastMarching.FastMarching as FM

    m = np.zeros((190, 170), bool)
    m[60:71, 60:71] = True
    assert FM._mask_rects(m) == [(60, 60, 64, 64), (64, 60, 71, 64), (60, 64, 64, 71), (64, 64, 71, 71)]
    big = np.zeros((4096, 4096), bool)
    big[5::64, 9::64] = True  # 4096 blocks touched
    rects = FM._mask_rects(big)
    assert 0 < len(rects) <= 1024
    assert not (big & ~rect_mask(big.shape, rects)).any()
    assert FM._mask_rects(np.zeros((10, 10), bool)) == []


def test_update_tmap_checks_shapes_before_anything_runs():
    import FastMarching.FastMarching as FM

    cost = np.ones((20, 30))
    with pytest.raises(ValueError):
        FM.updateTmap(cost, np.zeros((20, 1)), (3, 3), [(1, 1, 2, 2)])  # would broadcast silently
    with pytest.raises(ValueError):
        FM.updateTmap(cost, np.zeros((20, 30)), (3, 3), np.zeros((30, 20), bool))
