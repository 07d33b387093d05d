"""The invalidation rule of the seeded re-solve (include/eikonal.h), on the CPU.

One map; the OLD seed list produced the converged field T_old, the NEW list may be the same.  Roots
take the goal's place in the rule of tests/test_replan_rule.py: an old root (T_old[c] == b_old(c) bit
for bit) is SPARED when b_new(c) <= b_old(c) -- never in the cone, handing no mark on -- and RELEASED,
a cone seed, otherwise.  The restart state is +inf on the cone, T_old elsewhere, then min(T, b_new) at
every new seed; iterating T = min(T, godunov) on the new cost from it must reach the field of the new
cost and new list (tests/test_seeds_abi.seeded_reference): masks equal, values within 1e-9.
`seeded_closure` and `restart_state` are what the GPU tests compare the device with, cell for cell.
"""
import numpy as np
import pytest

from test_replan_rule import closure, jacobi, rect_mask
from test_seeds_abi import seeded_reference


def cell_min(shape, seeds, t0, dtype):
    """b(c): the smallest (R)t0 of the seeds on c, +inf where there is none"""
    b = np.full(shape, np.inf, dtype)
    t0 = np.zeros(len(seeds)) if t0 is None else np.asarray(t0, np.float64)
    for (x, y), v in zip(seeds, t0.astype(dtype)):
        b[y, x] = min(b[y, x], v)
    return b


def seeded_closure(T_old, raised_mask, old, new):
    """(cone, spared, released) boolean (H, W) masks of the rule.  T_old: the converged field of the
    list old = (seeds, t0), any float dtype (non-negative values compare like their bit patterns);
    raised_mask: the cells of the EIK_CHANGE_ANY rectangles; new = (seeds, t0): the new list."""
    H, W = T_old.shape
    b_old = cell_min(T_old.shape, old[0], old[1], T_old.dtype)
    b_new = cell_min(T_old.shape, new[0], new[1], T_old.dtype)
    root = np.isfinite(b_old) & (T_old == b_old)
    spared = root & (b_new <= b_old)
    released = root & ~spared
    fin = np.isfinite(T_old).ravel()
    Tf = T_old.ravel()
    sp = spared.ravel()
    M = ((np.asarray(raised_mask, bool) & np.isfinite(T_old)) | released).ravel() & ~sp
    front = np.flatnonzero(M)
    while front.size:
        y, x = np.divmod(front, W)
        nxt = []
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            yy, xx = y + dy, x + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            p, q = yy[ok] * W + xx[ok], front[ok]
            take = fin[p] & ~M[p] & (Tf[q] <= Tf[p]) & ~sp[p]
            p = np.unique(p[take])
            M[p] = True
            nxt.append(p)
        front = np.unique(np.concatenate(nxt))
    return M.reshape(H, W), spared, released


def restart_state(T_old, cone, new):
    """+inf on the cone, T_old elsewhere, then T[c] = min(T[c], b_new(c)) at every new seed"""
    return np.minimum(np.where(cone, np.inf, T_old).astype(T_old.dtype), cell_min(T_old.shape, new[0], new[1], T_old.dtype))


def make_case(kind, edit, seed):
    """A raster of 60..140 cells a side with six seeds -- s4 and s5 on one cell, s3 dominated (beside s0,
    t0 far above) -- and an edit of the cost (1-3 rectangles raised to +inf or lowered to 1), of the list
    (s1 and the dominated s3 dropped, s0's t0 raised, s2's lowered, s6 added, s4 -- the lower of the two
    on the shared cell -- dropped), or of both."""
    rng = np.random.default_rng(seed)
    H, W = (int(v) for v in rng.integers(60, 141, 2))
    if kind == "uniform":
        c = np.full((H, W), 2.0)
    elif kind == "integer":
        c = rng.integers(1, 10, (H, W)).astype(np.float64)
    else:
        c = rng.uniform(1, 10, (H, W))
    if kind == "obst":
        c[rng.random((H, W)) < 0.2] = np.inf
    s0 = (W // 4, H // 4)
    seeds = [s0, (3 * W // 4, H // 4), (W // 4, 3 * H // 4), (s0[0] + 1, s0[1]), (3 * W // 4, 3 * H // 4),
             (3 * W // 4, 3 * H // 4)]
    t0 = [0.0, 5.0, 9.0, 1000.0, 2.0, 7.0]
    added = (W // 2, H // 2)
    for x, y in seeds + [added]:
        c[y, x] = 1.0
    new = c.copy()
    raised, lowered = [], []
    if edit in ("cost", "both"):
        for k in range(int(rng.integers(1, 4))):
            w, h = (int(v) for v in rng.integers(3, 25, 2))
            x0, y0 = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            up = k % 2 == 0
            new[y0:y0 + h, x0:x0 + w] = np.inf if up else 1.0  # (every cost is >= 1: 1.0 never raises one)
            (raised if up else lowered).append((x0, y0, x0 + w, y0 + h))
        assert not (~rect_mask(c.shape, raised) & (new > c)).any()
    nseeds, nt0 = seeds, t0
    if edit in ("seeds", "both"):
        nseeds = [seeds[0], seeds[2], seeds[5], added]
        nt0 = [30.0, 4.0, 7.0, 1.0]
    return c, new, (seeds, t0), (nseeds, nt0), raised, lowered


CASES = [(k, e, s) for k in ("uniform", "integer", "obst", "float") for e in ("cost", "seeds", "both") for s in (0, 1)]


@pytest.mark.parametrize("kind,edit,seed", CASES)
def test_cone_restart_reaches_the_new_seeded_field(kind, edit, seed):
    c, new, old, nw, raised, lowered = make_case(kind, edit, 1000 * CASES.index((kind, edit, seed)) + seed)
    T_old = seeded_reference(c, *old)
    assert T_old[old[0][3][1], old[0][3][0]] < 1000.0  # s3 is dominated
    R = seeded_reference(new, *nw)
    cone, spared, released = seeded_closure(T_old, rect_mask(c.shape, raised), old, nw)
    assert not (cone & spared).any(), "a spared root is in the cone"
    assert (released & ~cone).sum() == 0
    if edit == "cost":
        assert not released.any() and spared.sum() == 4  # s0, s1, s2 and the shared cell (s4's t0)
    else:
        # s0 (t0 raised), s1 (dropped) and the shared cell (its lower seed dropped) are released; s2 is spared
        assert released.sum() == 3 and spared.sum() == 1
    start = restart_state(T_old, cone, nw)
    fin = np.isfinite(R)
    assert (start[fin] >= R[fin] - 4 * np.spacing(R[fin])).all()  # a supersolution of the new problem
    T = jacobi(start, new)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    if fin.any():
        assert np.abs(T[fin] - R[fin]).max() <= 1e-9


@pytest.mark.parametrize("seed", [0, 1])
def test_one_seed_at_zero_is_the_single_goal_rule(seed):
    rng = np.random.default_rng(40 + seed)
    c = rng.integers(1, 4, (70, 90)).astype(np.float64)  # ties
    goal = (30, 35)
    T_old = seeded_reference(c, [goal], [0.0])
    rects = [(50, 10, 62, 30), (25, 30, 36, 41)]  # the second covers the goal
    m = rect_mask(c.shape, rects)
    cone, spared, released = seeded_closure(T_old, m, ([goal], [0.0]), ([goal], [0.0]))
    assert np.array_equal(cone, closure(T_old, m, goal))
    assert spared.sum() == 1 and spared[goal[1], goal[0]] and not released.any()


def test_classes_on_a_crafted_field():
    T = np.array([[2.0, 1.0, 2.0, 3.0, 9.0],
                  [1.0, 0.0, 1.0, np.inf, 8.0],
                  [2.0, 1.0, 2.0, 5.0, 7.0]])
    old = ([(1, 1), (4, 2), (2, 1)], [0.0, 7.0, 4.0])  # (2, 1) is dominated: T = 1 < 4
    none = np.zeros(T.shape, bool)
    # the same list: every root spared, no cone
    cone, spared, released = seeded_closure(T, none, old, old)
    assert not cone.any() and spared.sum() == 2 and not released.any() and not spared[1, 2]
    # (4, 2) dropped: released, and the cells its wave fed (8 and 9 behind it; the 5 beside it is lower) follow
    cone, spared, released = seeded_closure(T, none, old, ([(1, 1)], [0.0]))
    assert released[2, 4] and released.sum() == 1 and spared[1, 1]
    want = np.zeros(T.shape, bool)
    want[2, 4] = want[1, 4] = want[0, 4] = True
    assert np.array_equal(cone, want), cone
    # t0 lowered and a seed added: nothing is released, no cone
    cone, spared, released = seeded_closure(T, none, old, ([(1, 1), (4, 2), (0, 0)], [0.0, 6.0, 0.5]))
    assert not cone.any() and not released.any()
    # the dominated seed dropped: an ordinary cell, nothing happens
    cone, spared, released = seeded_closure(T, none, old, ([(1, 1), (4, 2)], [0.0, 7.0]))
    assert not cone.any() and not released.any() and spared.sum() == 2
    # a spared root inside a raised rectangle hands no mark on: ties 0 <= ... never start at it
    m = np.zeros(T.shape, bool)
    m[1, 1] = True
    cone, _, _ = seeded_closure(T, m, old, old)
    assert not cone.any()
    # the restart state puts the new seeds in
    S = restart_state(T, want, ([(1, 1), (4, 0)], [0.0, 3.5]))
    assert S[0, 4] == 3.5 and np.isinf(S[1, 4]) and np.isinf(S[2, 4]) and S[1, 1] == 0.0
