"""The obstacle-safe 2D walker (eik_path2d_safe_*, csrc/gdm_safe.hip) against its specification,
tests/path_safe_np.py, on fields the GPU solver produced: equal point count, status and info words,
points within 1e-9 cells (the bound the 2D walker is held to; path_safe_np's default
arithmetic is the kernel's, so the paths agree far closer than that).

Fields: A 96 x 96 fp64, U(1, 10) with 20 % single-cell dust; B 72 x 200 fp64 (more than one 64-node
window in x, a prefetch edge in y), uniform with a three-cell wall, a one-cell wall and sparse dust;
C 96 x 96 fp32, exp(N(0, 1.5)) without obstacles, where the stall rule fires.
"""
import numpy as np
import pytest

import oracle as O
import path_safe_np as S

pytestmark = pytest.mark.gpu
PATH_ATOL = 1e-9
GOAL_A, GOAL_B, GOAL_C = (8, 8), (10, 36), (8, 8)
STARTS_A = [(88.0, 88.0), (50.5, 80.25), (86.0, 10.0), (12.0, 85.0), (60.3, 47.6), (40.0, 70.0)]
STARTS_B = [(190.0, 36.0), (170.5, 60.25), (125.0, 30.0), (104.3, 36.4), (153.0, 40.0), (60.0, 30.0)]
STARTS_C = [(88.0, 88.0), (50.0, 80.0), (86.0, 10.0), (12.0, 85.0), (60.0, 47.0)]
CROSS_B, TAU_CROSS = (66.0, 36.0), 0.1  # the walk whose fallback drops points on both sides of x = 34


def _border(cost):
    cost[0, :] = cost[-1, :] = cost[:, 0] = cost[:, -1] = np.inf
    return cost


def cost_a():
    rng = np.random.default_rng(11)
    cost = rng.uniform(1, 10, (96, 96))
    cost[rng.random((96, 96)) < 0.2] = np.inf
    _border(cost)
    cost[7:10, 7:10] = 1
    for x, y in STARTS_A:
        cost[int(y):int(y) + 2, int(x):int(x) + 2] = 2.0
    cost[47, 61] = np.inf  # (60.3, 47.6)'s cell has an impassable corner: its first step is blocked
    return cost


def cost_b():
    rng = np.random.default_rng(12)
    cost = np.ones((72, 200))
    cost[8:60, 100:103] = np.inf   # thick wall
    cost[12:64, 150] = np.inf      # thin wall
    dust = rng.random((72, 200)) < 0.08
    dust[:, :20] = dust[:, 96:] = False
    dust[:22] = dust[50:] = False
    cost[dust] = np.inf
    _border(cost)
    for x, y in STARTS_B + [CROSS_B]:
        cost[int(y), int(x)] = 1.0
    return cost


def cost_c():
    rng = np.random.default_rng(13)
    cost = np.exp(rng.normal(0, 1.5, (96, 96)))
    _border(cost)
    cost[7:10, 7:10] = 1
    return cost


@pytest.fixture(scope="module")
def ctx():
    import eikonal

    c = eikonal.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fields(ctx):
    """name -> (T as float64, SafeField, starts, goal); the fields come from the GPU solver"""
    out = {}
    for name, cost, dtype, starts, goal in (("A", cost_a(), np.float64, STARTS_A, GOAL_A),
                                            ("B", cost_b(), np.float64, STARTS_B, GOAL_B),
                                            ("C", cost_c(), np.float32, STARTS_C, GOAL_C)):
        T = ctx.tmap2d(cost.astype(dtype), goal, dtype=dtype).astype(np.float64)
        starts = [s for s in starts if np.isfinite(T[int(s[1]), int(s[0])])]
        out[name] = (T, S.SafeField(T), starts, goal)
    return out


def _check(got, ref, what):
    (p, st, info), (q, rst, rinfo) = got, ref
    assert st == rst and len(p) == len(q) and np.array_equal(info, rinfo), (what, st, rst, len(p), len(q), info, rinfo)
    if len(p):
        assert np.abs(p - q).max() <= PATH_ATOL, (what, np.abs(p - q).max())


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("tau", [0.5, 0.25])
def test_matches_the_rule(ctx, fields, name, tau):
    T, f, starts, goal = fields[name]
    assert len(starts) >= 4
    for s in starts:
        ref = S.safe_path(f, s, goal, tau)
        got = ctx.path2d_safe(T, s, goal, tau)
        _check(got, ref, (name, s, tau))
        assert got[1] == S.DONE and not S.nearest_is_inf(T, got[0]).any(), (name, s, tau)
        if name == "C":
            assert got[2][2] >= 0, (s, tau)  # the stall rule fired
        else:
            assert got[2][0] > 0 and got[2][2] == -1, (name, s, tau)  # blocked steps, no stall


def test_fp32_field_on_the_device(ctx, fields):
    """the fp32 instantiation: the field stays float on the device (eik_path2d_safe_dev)"""
    import ctypes as C

    import torch
    from eikonal import _lib as L

    T, f, starts, goal = fields["C"]
    dev = torch.device("cuda:0")
    dT = torch.from_numpy(T.astype(np.float32)).to(dev)
    cap = 30004
    d_out = torch.empty((cap, 2), dtype=torch.float64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    d_info = torch.zeros(4, dtype=torch.int64, device=dev)
    s = starts[0]
    rc = L.lib().eik_path2d_safe_dev(ctx._h, dT.data_ptr(), L.EIK_F32, 96, 96, np.array(s, np.float64),
                                     np.array(goal, np.float64), 0.5, d_out.data_ptr(), cap, d_n.data_ptr(),
                                     d_st.data_ptr(), d_info.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    n = int(d_n.item())
    got = (d_out[:n].cpu().numpy(), int(d_st.item()), d_info.cpu().numpy())
    _check(got, S.safe_path(f, s, goal, 0.5), ("C fp32", s))


def test_first_step_blocked(ctx, fields):
    T, f, _, goal = fields["A"]
    s = (60.3, 47.6)
    assert np.isinf(T[47, 61]) and np.isfinite(T[48, 60])
    trace = []
    ref = S.safe_path(f, s, goal, 0.5, trace=trace)
    assert trace[0][0] == 1 and ref[1] == S.DONE  # the fallback of iteration 1 dropped the start itself
    assert tuple(ref[0][0]) != s
    _check(ctx.path2d_safe(T, s, goal, 0.5), ref, "first step blocked")


def test_drop_across_a_window_boundary(ctx, fields):
    """The start's window spans x in [34, 98); walking left (rows 34-37: no prefetch in y) the walker
    prefetches a window 17 nodes on and switches to it when its cell's x falls below 34.  This walk takes
    a fallback in the new window whose drop loop removes points computed in the old one."""
    T, f, _, goal = fields["B"]
    trace = []
    ref = S.safe_path(f, CROSS_B, goal, TAU_CROSS, trace=trace)
    edge = int(CROSS_B[0]) - 32
    assert any(gone and gone[0][0] < edge and max(g[0] for g in gone) >= edge for _, gone in trace), "no such fallback"
    _check(ctx.path2d_safe(T, CROSS_B, goal, TAU_CROSS), ref, "drop across a window boundary")


def test_batch(ctx, fields):
    """P = 5 paths over B = 2 fields with map_of: each as the single call; an ERROR and a STUCK path do not
    fail the call"""
    TA, _, sa, ga = fields["A"]
    TC, _, sc, gc = fields["C"]
    pit = TC.copy()
    pit[40:43, 60:63] = pit[40:43, 60:63].min() - 1.0  # a plateau lower than everything around it
    stack = np.stack([TA, pit])
    wall = np.argwhere(np.isinf(TA[20:70, 20:70]))[0] + 20
    inits = [sa[0], (61.0, 41.0), sa[1], (float(wall[1]), float(wall[0])), sc[0]]
    map_of = [0, 1, 0, 0, 1]
    ends = [ga, gc, ga, ga, gc]
    got = ctx.path2d_safe_batch(stack, inits, ends, 0.5, map_of=map_of)
    assert [g[1] for g in got][1] == S.STUCK and got[3][1] == S.ERROR and got[0][1] == S.DONE
    for p in range(5):
        one = ctx.path2d_safe(stack[map_of[p]], inits[p], ends[p], 0.5)
        assert got[p][1] == one[1] and np.array_equal(got[p][0], one[0]) and np.array_equal(got[p][2], one[2]), p
        _check(got[p], S.safe_path(stack[map_of[p]], inits[p], ends[p], 0.5), ("batch", p))


def test_tau_above_one_is_an_argument_error(ctx, fields):
    import eikonal

    T, _, starts, goal = fields["A"]
    with pytest.raises(eikonal.EikError):
        ctx.path2d_safe(T, starts[0], goal, 1.01)
    with pytest.raises(eikonal.EikError):
        ctx.path2d_safe_batch(T, starts[:2], goal, 1.5)


def test_drop_in(ctx):
    """getPathsToNearest(safe=True) walks round an impassable block to the start's goal; the default
    returns the reference's truncated walk"""
    import FastMarching.FastMarching as FM

    cost = _border(np.ones((64, 64)))
    cost[26:39, 30:34] = np.inf
    goals = [(8, 32), (61, 61)]
    T, lab = FM.computeTmapMulti(cost, goals, labels=True)
    start = (36.0, 32.0)
    assert lab[32, 36] == 0
    safe = FM.getPathsToNearest(T, lab, goals, [start], 0.5, safe=True)[0]
    assert tuple(safe[0]) == start and tuple(safe[-1]) == (8.0, 32.0) and not S.nearest_is_inf(T, safe).any()
    assert np.hypot(*(safe[1:-1] - safe[:-2]).T).max() <= 1.5
    assert np.hypot(*(safe[-1] - safe[-2])) < 1.5  # it did reach that goal's stop radius
    plain = FM.getPathsToNearest(T, lab, goals, [start], 0.5)[0]
    assert tuple(plain[-1]) != (8.0, 32.0)  # truncated beside the block
    assert np.array_equal(FM.getPathSafe(T, start, goals[0], 0.5), safe)
    assert np.array_equal(FM.getPathsSafe(T, [start, (20.0, 40.0)], goals[0], 0.5)[0], safe)
    pit = T.copy()
    pit[50:53, 50:53] = -1.0
    with pytest.raises(RuntimeError, match=r"stuck at node \(5[0-2], 5[0-2]\)"):
        FM.getPathSafe(pit, (53.0, 51.0), goals[0], 0.5)
    with pytest.raises(IndexError):
        FM.getPathSafe(T, (31.0, 30.0), goals[0], 0.5)  # starts on the block


def _window_switches(pts, H, W):
    """The walkers' window rule (csrc/gdm_walk.hpp Walk2Win::cross) on the points a step starts from:
    per switch of the 64-node window, the axis along which the point's cell left it."""
    PW, PRE = 64, 16
    xmax, ymax = max(W - PW, 0), max(H - PW, 0)

    def origin(i, j):
        return min(max(i - PW // 2, 0), xmax), min(max(j - PW // 2, 0), ymax)

    def inside(w, i, j):
        return w is not None and w[0] <= i and i + 1 < w[0] + PW and w[1] <= j and j + 1 < w[1] + PW

    cur = ahead = None
    axes = []
    for x, y in pts:
        i, j = int(x), int(y)
        if not inside(cur, i, j):
            if cur is not None:
                axes.append("y" if cur[0] <= i < cur[0] + PW - 1 else "x")
            cur = ahead if inside(ahead, i, j) else origin(i, j)
            ahead = None
        if ahead is None and ((i - cur[0] < PRE and cur[0] > 0) or (cur[0] + PW - 2 - i < PRE and cur[0] < xmax) or
                              (j - cur[1] < PRE and cur[1] > 0) or (cur[1] + PW - 2 - j < PRE and cur[1] < ymax)):
            ahead = origin(i, j)
    return axes


def test_safe_walk_is_the_default_walk_without_obstacles(ctx):
    """The two walkers run one copy of the window state and of the step's arithmetic: on a smooth finite
    field without obstacles, across several window switches in both axes, eik_path2d_safe_f64's rows are
    eik_path2d_f64's bit for bit (loop forms 0 and 4), with the same n and status, and no fallback."""
    from eikonal import _lib as L

    H, W, tau = 200, 160, 0.5
    start, goal = (150.25, 190.5), (8, 8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    T = np.sqrt((x - goal[0]) ** 2 + 3.0 * (y - goal[1]) ** 2) + 0.5 * np.sin(x / 9.0) * np.sin(y / 11.0)
    assert np.isfinite(T).all()
    # the precondition, on the host: a plain gradient walk (the rule's restatement takes no fallback, drops
    # nothing, never stalls, ends at the goal) that switches windows along x and along y
    ref, rst, rinfo = S.safe_path(T, start, goal, tau)
    assert rst == S.DONE and rinfo[0] == 0 and rinfo[1] == 0 and rinfo[2] == -1, (rst, rinfo)
    axes = _window_switches(ref[:-2], H, W)  # (the last walked point and the appended goal start no step)
    assert len(axes) >= 3 and "x" in axes and "y" in axes, axes
    safe, sst, info = ctx.path2d_safe(T, start, goal, tau)
    assert sst == S.DONE and np.array_equal(info, [0, 0, -1, rinfo[3]]), (sst, info, rinfo)
    try:
        for form in (0, 4):
            ctx.set_option(L.OPT_PATH_LOOP, form)
            p, st = ctx.path2d(T, start, goal, tau)
            assert st == sst and p.shape == safe.shape, (form, st, sst, p.shape, safe.shape)
            assert np.array_equal(p.view(np.uint64), safe.view(np.uint64)), (form, np.abs(p - safe).max())
    finally:
        ctx.set_option(L.OPT_PATH_LOOP, 4)  # the default (include/eikonal.h)


@pytest.mark.parametrize("name", ["A", "B"])
def test_default_mode_untouched(ctx, fields, name):
    """eik_path2d_f64 on the same fields is still oracle.gdm2d's walk, truncation included"""
    T, _, starts, goal = fields[name]
    statuses = set()
    for s in starts:
        p, st = ctx.path2d(T, s, goal, 0.5)
        r, rst = O.gdm2d(T, np.array(s, float), np.array(goal, float), 0.5)
        assert st == rst and p.shape == r.shape and (len(p) == 0 or np.abs(p - r).max() <= PATH_ATOL), (name, s)
        statuses.add(st)
    assert S.FALLBACK in statuses  # the fields do make the reference's walk truncate
