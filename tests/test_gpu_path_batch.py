"""Batched path extraction (eik_path2d_batch_*, eik_path3d_batch_*, eik_plan2d_batch_f32; gdm.hip's
grid form: one workgroup per path) against the single-path entries, whose parity with the oracle
tests/test_gpu_path.py and tests/test_gpu_fim3d.py pin.  Equality is bit for bit: np.array_equal on
the rows (NaN rows of an error start compare equal), the same point count, the same status.  A few
paths also go to the oracle directly (<= 1e-9 cells, the single entry's own tolerance: the reference
squares with pow(), the kernel with exact products).
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
PATH_ATOL = 1e-9
FILL = -7.0


@pytest.fixture(scope="module")
def ctx():
    import eikonal

    c = eikonal.Context(0)
    yield c
    c.close()


def _relaxed(fn, *a):
    O.set_strict(False)
    try:
        return fn(*a)
    finally:
        O.set_strict(True)


def _same(got, ref):
    (pa, sa), (pb, sb) = got, ref
    return sa == sb and pa.shape == pb.shape and np.array_equal(pa, pb, equal_nan=True)


def _assert_all_same(got, ref, what=""):
    assert len(got) == len(ref)
    bad = [p for p in range(len(ref)) if not _same(got[p], ref[p])]
    assert not bad, (what, bad, [(got[p][1], len(got[p][0]), ref[p][1], len(ref[p][0])) for p in bad[:4]])


# ------------------------------------------------------------------ case 1's field and starts
H1, W1 = 150, 170  # more than one 64-node window on both axes: walks switch and prefetch windows
GOAL1 = (W1 - 30, H1 - 25)
POCKET = (63.3, 43.6)  # inside a walled-off block: T = +inf there, the walk takes the NaN fallback


@pytest.fixture(scope="module")
def field1():
    rng = np.random.default_rng(31)
    cost = rng.uniform(1, 6, (H1, W1))
    cost[rng.random((H1, W1)) < 0.08] = np.inf
    cost[0, :] = cost[-1, :] = cost[:, 0] = cost[:, -1] = np.inf
    gx, gy = GOAL1
    cost[gy - 3:gy + 4, gx - 3:gx + 4] = 1.0
    cost[40:47, 60:67] = np.inf  # the pocket's wall ...
    cost[41:46, 61:66] = 2.0     # ... and its unreachable inside
    T = _relaxed(O.fmm2d, cost, GOAL1)
    assert np.isinf(T[43, 63]) and np.isfinite(T).sum() > 0.8 * H1 * W1
    cells = np.argwhere(np.isfinite(T))
    pick = cells[rng.choice(len(cells), 35, replace=False)]
    starts = [(float(x) + f, float(y) + g) for (y, x), f, g in zip(pick, rng.random(35) * 0.9, rng.random(35) * 0.9)]
    starts = [(min(x, W1 - 1.5), min(y, H1 - 1.5)) for x, y in starts]
    starts += [(gx + 1.0, gy + 0.5),        # inside the stop radius
               (gx + 1.6, gy + 0.0),        # just outside it
               POCKET,                      # NaN fallback
               (float("nan"), 50.0),        # NaN coordinate
               (W1 + 5.0, 20.0),            # outside the raster
               (12.25, H1 + 3.0)]
    return T, np.array(starts, np.float64), np.array(GOAL1, np.float64)


@pytest.fixture(scope="module")
def singles1(ctx, field1):
    """The single-path entry's result for every start of case 1, per tau (computed once, shared)."""
    T, starts, goal = field1
    return {tau: [ctx.path2d(T, s, goal, tau) for s in starts] for tau in (0.5, 1.7)}


@pytest.mark.parametrize("tau", [0.5, 1.7])
def test_one_field_many_starts(ctx, field1, singles1, tau):
    T, starts, goal = field1
    ref = singles1[tau]
    got = ctx.path2d_batch(T, starts, goal, tau)
    _assert_all_same(got, ref, f"tau {tau}")
    from eikonal import _lib as L

    st = [s for _, s in ref]
    assert st[-4] == L.PATH_FALLBACK and st[-3] == st[-2] == st[-1] == L.PATH_ERROR  # the special starts took their exits
    assert len(ref[-6][0]) <= 4 and len(ref[-5][0]) <= 4                              # stop radius: a step or two
    assert max(len(p) for p, _ in ref) > 100 / tau                                   # and long walks cross windows
    for p in range(3):  # to the oracle directly
        o, ost = O.gdm2d(T, starts[p], goal, tau)
        path, s = got[p]
        assert s == ost and path.shape == o.shape and np.abs(path - o).max() <= PATH_ATOL


# ------------------------------------------------------------------ device-entry helpers
def _dev():
    import torch

    return torch, torch.device("cuda", 0)


def _single_dev(c, ptr, dtype, H, W, start, goal, tau, cap, dim=2, Lz=None):
    """eik_path2d_dev / eik_path3d_dev on a device field -> (rows, status)."""
    from eikonal import _lib as L

    torch, dev = _dev()
    out = torch.full((cap, dim), FILL, dtype=torch.float64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    a, b = np.array(start, np.float64), np.array(goal, np.float64)
    if dim == 2:
        c._chk(L.lib().eik_path2d_dev(c._h, ptr, dtype, H, W, a, b, tau, out.data_ptr(), cap, n.data_ptr(),
                                      st.data_ptr(), s))
    else:
        c._chk(L.lib().eik_path3d_dev(c._h, ptr, dtype, H, W, Lz, a, b, tau, out.data_ptr(), cap, n.data_ptr(),
                                      st.data_ptr(), s))
    k = int(n.item())
    return out[:k].cpu().numpy(), int(st.item())


class _Batch2d:
    """One eik_path2d_batch_dev call's device results, issued on torch's current stream (no sync)."""

    def __init__(self, c, ptr, dtype, B, H, W, starts, goals, tau, cap, map_of=None):
        from eikonal import _lib as L

        torch, dev = _dev()
        starts = np.array(starts, np.float64).reshape(-1, 2)  # copies: overwritten below
        P = len(starts)
        goals = np.array(np.broadcast_to(np.asarray(goals, np.float64).reshape(-1, 2), (P, 2)), order="C")
        self.P, self.cap = P, cap
        self.out = torch.full((P, cap, 2), FILL, dtype=torch.float64, device=dev)
        self.n = torch.full((P,), -1, dtype=torch.int64, device=dev)
        self.st = torch.full((P,), -1, dtype=torch.int32, device=dev)
        m = None if map_of is None else np.ascontiguousarray(map_of, np.int32)
        self.rc = L.lib().eik_path2d_batch_dev(c._h, ptr, dtype, B, H, W, P, None if m is None else m.ctypes.data,
                                               starts, goals, tau, self.out.data_ptr(), cap, self.n.data_ptr(),
                                               self.st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        # the entry has read its host arrays: the caller may reuse them at once
        starts.fill(np.nan)
        goals.fill(np.nan)
        if m is not None:
            m.fill(-5)

    def results(self):
        out, n, st = self.out.cpu().numpy(), self.n.cpu().numpy(), self.st.cpu().numpy()
        return [(out[p, : n[p]].copy(), int(st[p])) for p in range(self.P)], out, n


def test_paired_maps_on_device_fp32(ctx):
    from eikonal import _lib as L

    torch, dev = _dev()
    rng = np.random.default_rng(32)
    B, H, W = 6, 96, 112
    costs = rng.uniform(1, 5, (B, H, W)).astype(np.float32)
    costs[rng.random((B, H, W)) < 0.06] = np.inf
    costs[:, 0, :] = costs[:, -1, :] = costs[:, :, 0] = costs[:, :, -1] = np.inf
    goals = np.array([(W - 10 - 3 * b, H - 8 - 2 * b) for b in range(B)], np.int64)
    starts = np.array([(7.4 + b, 9.1 + 2 * b) for b in range(B)], np.float64)
    for b in range(B):
        costs[b, goals[b, 1], goals[b, 0]] = 1.0
        costs[b, int(starts[b, 1]):int(starts[b, 1]) + 2, int(starts[b, 0]):int(starts[b, 0]) + 2] = 1.0
    T = ctx.tmap2d_batch(costs, goals)
    Td = torch.from_numpy(T).to(dev)
    cap, tau = 30004, 0.5
    ptr = lambda b: Td.data_ptr() + 4 * b * H * W
    single = lambda b, s: _single_dev(ctx, ptr(b), L.EIK_F32, H, W, s, goals[b].astype(float), tau, cap)
    # map_of = None with P == B: path p walks map p
    bt = _Batch2d(ctx, Td.data_ptr(), L.EIK_F32, B, H, W, starts, goals.astype(float), tau, cap)
    assert bt.rc == L.EIK_OK
    got, _, _ = bt.results()
    _assert_all_same(got, [single(b, starts[b]) for b in range(B)], "paired")
    assert max(len(p) for p, _ in got) > 100
    # an explicit map_of: map 2 takes three paths, map 4 none
    map_of = [0, 1, 2, 2, 2, 3, 5]
    st2 = np.array([starts[m] + (0.0 if k in (0, 1, 2, 5, 6) else 3.5 * (k - 2)) for k, m in enumerate(map_of)])
    bt = _Batch2d(ctx, Td.data_ptr(), L.EIK_F32, B, H, W, st2, goals[map_of].astype(float), tau, cap, map_of)
    assert bt.rc == L.EIK_OK
    got, _, _ = bt.results()
    _assert_all_same(got, [single(m, st2[k]) for k, m in enumerate(map_of)], "map_of")


def test_more_paths_than_cus(ctx):
    """P = 300 workgroups of a whole CU's LDS each: more than the device's CUs, so the later ones start
    as the earlier ones finish."""
    rng = np.random.default_rng(33)
    N, P = 96, 300
    cost = rng.uniform(1, 4, (N, N))
    cost[rng.random((N, N)) < 0.05] = np.inf
    cost[0, :] = cost[-1, :] = cost[:, 0] = cost[:, -1] = np.inf
    goal = (N // 2, N // 2 + 5)
    cost[goal[1] - 1:goal[1] + 2, goal[0] - 1:goal[0] + 2] = 1.0
    T = _relaxed(O.fmm2d, cost, goal)
    cells = np.argwhere(np.isfinite(T))
    pick = cells[rng.choice(len(cells), P, replace=False)]
    starts = np.minimum(pick[:, ::-1] + rng.random((P, 2)) * 0.9, N - 1.5)
    g = np.array(goal, np.float64)
    got = ctx.path2d_batch(T, starts, g, 0.5)
    _assert_all_same(got, [ctx.path2d(T, s, g, 0.5) for s in starts], "P = 300")


@pytest.mark.parametrize("cap", [2, 3, 50])
def test_caps_and_slab_isolation(ctx, field1, singles1, cap):
    """Regular walks (budget exits at a small cap: PATH_ERROR; walks shorter than it: done): n, status and
    rows as the single call at that cap, and no row at or beyond n_out[p] of any slab is touched.
    Regular: the single entry ends them PATH_DONE at the full cap.  (A NaN fallback pops points it has
    already stored, in the reference and in both entries: rows past its n are not untouched.)"""
    from eikonal import _lib as L

    torch, dev = _dev()
    T, starts, goal = field1
    gx, gy = GOAL1
    regular = [p for p in range(35) if singles1[0.5][p][1] == L.PATH_DONE][:8]
    assert len(regular) == 8
    sel = np.vstack([starts[regular], [(gx + 1.0, gy + 0.5), (gx + 1.6, gy + 0.0), (gx - 2.9, gy + 2.9), (gx + 9.0, gy - 7.5)]])
    Td = torch.from_numpy(np.ascontiguousarray(T)).to(dev)
    bt = _Batch2d(ctx, Td.data_ptr(), L.EIK_F64, 1, H1, W1, sel, goal, 0.5, cap)
    assert bt.rc == L.EIK_OK
    got, out, n = bt.results()
    ref = [_single_dev(ctx, Td.data_ptr(), L.EIK_F64, H1, W1, s, goal, 0.5, cap) for s in sel]
    _assert_all_same(got, ref, f"cap {cap}")
    st = [s for _, s in ref]
    assert L.PATH_ERROR in st and (cap < 50 or L.PATH_DONE in st)
    assert all(0 < k <= cap for k in n)
    for p in range(len(sel)):
        assert np.all(out[p, n[p]:] == FILL), p


def test_two_calls_one_stream_no_sync(ctx, field1, singles1):
    """Back-to-back calls on one stream: the second call's descriptors must not overwrite the first's
    before its kernel has read them."""
    from eikonal import _lib as L

    torch, dev = _dev()
    T, starts, goal = field1
    Td = torch.from_numpy(np.ascontiguousarray(T)).to(dev)
    ia, ib = list(range(0, 12)), list(range(20, 41))
    a = _Batch2d(ctx, Td.data_ptr(), L.EIK_F64, 1, H1, W1, starts[ia], goal, 0.5, 30004)
    b = _Batch2d(ctx, Td.data_ptr(), L.EIK_F64, 1, H1, W1, starts[ib], goal, 0.5, 30004)
    assert a.rc == L.EIK_OK and b.rc == L.EIK_OK
    torch.cuda.synchronize(dev)
    _assert_all_same(a.results()[0], [singles1[0.5][i] for i in ia], "first call")
    _assert_all_same(b.results()[0], [singles1[0.5][i] for i in ib], "second call")


def test_loop_forms_from_the_batch_entry(field1, singles1):
    """EIK_OPT_PATH_LOOP 0 (the reference's statement order) and 4 (lane pairs, the default): equal bits."""
    import eikonal
    from eikonal import _lib as L

    T, starts, goal = field1
    res = {}
    for form in (0, 4):
        c = eikonal.Context(0)
        try:
            c.set_option(L.OPT_PATH_LOOP, form)
            res[form] = {tau: c.path2d_batch(T, starts, goal, tau) for tau in (0.5, 1.7)}
        finally:
            c.close()
    for tau in (0.5, 1.7):
        _assert_all_same(res[0][tau], res[4][tau], f"forms, tau {tau}")
        _assert_all_same(res[4][tau], singles1[tau], f"form 4 vs single, tau {tau}")


# ------------------------------------------------------------------ 3D
def _layered(seed, goal_xy):
    """z-padded 60 x 70 x (3 + 2) volume, 5 % obstacles: window 35 x 35 x 5, integer descent."""
    rng = np.random.default_rng(seed)
    shape = (60, 70, 3)
    c = rng.uniform(1, 3, shape)
    c[rng.random(shape) < 0.05] = np.inf
    inf = np.full(shape[:2] + (1,), np.inf)
    c = np.concatenate([inf, c, inf], axis=2)
    goal = np.array([goal_xy[0], goal_xy[1], 2])
    c[goal[1], goal[0], goal[2]] = 1.0
    T = _relaxed(O.fmm3d, c, goal, None)
    cells = np.argwhere(np.isfinite(T))
    far = cells[np.abs(cells[:, 0] - goal[1]) + np.abs(cells[:, 1] - goal[0]) > 45]
    pick = far[rng.choice(len(far), 8, replace=False)]
    return T, pick[:, [1, 0, 2]].astype(np.float64), goal.astype(np.float64)


def _cube():
    """40 x 44 x 36, obstacle-free: window 19 x 19 x 16, trilinear steps all the way."""
    rng = np.random.default_rng(35)
    c = rng.uniform(1, 3, (40, 44, 36))
    goal = np.array([38, 35, 30])
    T = _relaxed(O.fmm3d, c, goal, None)
    starts = np.array([(3.0, 4.0, 2.0), (5.5, 30.25, 8.0), (20.0, 3.0, 33.5), (3.5, 3.5, 30.0), (36.0, 4.0, 3.0),
                       (10.0, 36.0, 20.0), (40.5, 37.0, 31.0), (25.0, 20.0, 5.5)])
    return T, starts, goal.astype(np.float64)


@pytest.mark.parametrize("kind", ["layered", "cube"])
def test_path3d_batch_one_volume(ctx, kind):
    T, starts, goal = _layered(34, (62, 52)) if kind == "layered" else _cube()
    got = ctx.path3d_batch(T, starts, goal, 0.5)
    ref = [ctx.path3d(T, s, goal, 0.5) for s in starts]
    _assert_all_same(got, ref, kind)
    assert max(len(p) for p, _ in ref) > 40  # longer than a window
    o, ost = O.gdm3d(T, starts[0], goal, 0.5)
    assert got[0][1] == ost and got[0][0].shape == o.shape and np.abs(got[0][0] - o).max() <= PATH_ATOL


def test_path3d_batch_stacked_volumes(ctx):
    vols = [_layered(36, (62, 52)), _layered(37, (8, 50)), _layered(38, (35, 6))]
    T = np.stack([v[0] for v in vols])
    # paired: path b walks volume b to its own goal
    starts = np.array([v[1][0] for v in vols])
    goals = np.array([v[2] for v in vols])
    got = ctx.path3d_batch(T, starts, goals, 0.5)
    _assert_all_same(got, [ctx.path3d(vols[b][0], starts[b], goals[b], 0.5) for b in range(3)], "paired volumes")
    for b in range(3):
        o, ost = O.gdm3d(vols[b][0], starts[b], goals[b], 0.5)
        assert got[b][1] == ost and got[b][0].shape == o.shape and np.abs(got[b][0] - o).max() <= PATH_ATOL
    # and two walks per volume through map_of
    map_of = [0, 0, 1, 1, 2, 2]
    st6 = np.array([vols[m][1][1 + (k & 1)] for k, m in enumerate(map_of)])
    got = ctx.path3d_batch(T, st6, goals[map_of], 0.5, map_of=map_of)
    _assert_all_same(got, [ctx.path3d(vols[m][0], st6[k], goals[m], 0.5) for k, m in enumerate(map_of)], "map_of volumes")


# ------------------------------------------------------------------ end to end
def test_plan2d_batch(ctx):
    from eikonal import _lib as L

    torch, dev = _dev()
    rng = np.random.default_rng(39)
    B, H, W = 4, 130, 150
    costs = rng.uniform(1, 5, (B, H, W)).astype(np.float32)
    costs[rng.random((B, H, W)) < 0.06] = np.inf
    costs[:, 0, :] = costs[:, -1, :] = costs[:, :, 0] = costs[:, :, -1] = np.inf
    goals = np.array([(W - 12, H - 9), (10, H - 14), (W - 20, 11), (W // 2, H // 2)], np.int64)
    starts = np.array([(8.5, 7.25), (W - 9.0, 6.5), (6.0, H - 8.75), (W + 4.0, 12.0)])  # the last: outside its map
    for b in range(B):
        costs[b, goals[b, 1], goals[b, 0]] = 1.0
        if starts[b, 0] < W:
            costs[b, int(starts[b, 1]):int(starts[b, 1]) + 2, int(starts[b, 0]):int(starts[b, 0]) + 2] = 1.0
    T = ctx.tmap2d_batch(costs, goals)
    Td = torch.from_numpy(T).to(dev)
    ref = [_single_dev(ctx, Td.data_ptr() + 4 * b * H * W, L.EIK_F32, H, W, starts[b], goals[b].astype(float), 0.5, 30004)
           for b in range(B)]
    got = ctx.plan2d_batch(costs, goals, starts, 0.5)
    _assert_all_same(got, ref, "plan2d_batch")
    assert got[3][1] == L.PATH_ERROR and len(got[3][0]) == 1  # a start outside its map: that path's error only
    assert max(len(p) for p, _ in got) > 100
    got2, fields = ctx.plan2d_batch(costs, goals, starts, 0.5, want_fields=True)
    _assert_all_same(got2, ref, "plan2d_batch with fields")
    assert fields.dtype == np.float32 and np.array_equal(fields, T)


# ------------------------------------------------------------------ argument errors
def test_argument_errors(ctx, field1):
    from eikonal import _lib as L

    torch, dev = _dev()
    T, starts, goal = field1
    B = 3
    Td = torch.from_numpy(np.ascontiguousarray(np.stack([T] * B))).to(dev)
    lib = L.lib()

    def call(P, cap, map_of, nB=B):
        n_rows = max(P, 1)
        s = np.ascontiguousarray(starts[:n_rows])
        g = np.ascontiguousarray(np.broadcast_to(goal, (n_rows, 2)))
        out = torch.full((n_rows, max(cap, 2), 2), FILL, dtype=torch.float64, device=dev)
        n = torch.full((n_rows,), -1, dtype=torch.int64, device=dev)
        st = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
        m = None if map_of is None else np.ascontiguousarray(map_of, np.int32)
        rc = lib.eik_path2d_batch_dev(ctx._h, Td.data_ptr(), L.EIK_F64, nB, H1, W1, P,
                                      None if m is None else m.ctypes.data, s, g, 0.5, out.data_ptr(), cap,
                                      n.data_ptr(), st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        msg = lib.eik_last_error(ctx._h).decode()
        torch.cuda.synchronize(dev)
        # nothing was launched: the result buffers are as they were
        assert bool((out == FILL).all()) and bool((n == -1).all()) and bool((st == -1).all())
        return rc, msg

    for args in ((3, 100, [0, 1, B]),      # a map_of entry = B
                 (3, 100, [0, -1, 1]),
                 (0, 100, None),           # P = 0
                 (3, 1, [0, 1, 2]),        # cap = 1
                 (2, 100, None)):          # map_of = None with P != B and B > 1
        rc, msg = call(*args)
        assert rc == L.EIK_ERR_ARG and msg, args
    # the host entry and the Python method report the same errors
    with pytest.raises(L.EikError) as e:
        ctx.path2d_batch(np.stack([T] * B), starts[:2], goal)
    assert e.value.code == L.EIK_ERR_ARG and "map_of" in str(e.value)
    with pytest.raises(L.EikError):
        ctx.path2d_batch(T, starts[:2], goal, map_of=[0, 1])
    with pytest.raises(L.EikError):
        ctx.path2d_batch(T, starts[:2], goal, cap=1)
    # B == 1 with map_of = None: every path walks map 0 (no error)
    ok = _Batch2d(ctx, Td.data_ptr(), L.EIK_F64, 1, H1, W1, starts[:2], goal, 0.5, 30004)
    assert ok.rc == L.EIK_OK


# ------------------------------------------------------------------ drop-ins
def _five_starts(T, first, single, seed):
    """`first` plus four more finite cells from which the single-path drop-in returns a path."""
    rng = np.random.default_rng(seed)
    cells = np.argwhere(np.isfinite(T))
    order = rng.permutation(len(cells))
    starts = [np.asarray(first, np.float64)]
    for k in order:
        c = cells[k]
        s = np.array([c[1], c[0]] + list(c[2:]), np.float64)
        try:
            single(s)
        except IndexError:
            continue
        starts.append(s)
        if len(starts) == 5:
            break
    assert len(starts) == 5
    return np.array(starts)


def test_dropin_2d(golden):
    import FastMarching.FastMarching as FM

    d = golden("fmm2d_fields")
    T, goal = d["c3_T"], d["c3_goal"]
    starts = _five_starts(T, d["c3_start"], lambda s: FM.getPathGDM(T, s, goal, 0.5), 40)
    paths = FM.getPathsGDM(T, starts, goal, 0.5)
    ref = [FM.getPathGDM(T, s, goal, 0.5) for s in starts]
    assert isinstance(paths, list) and len(paths) == 5
    for a, b in zip(paths, ref):
        assert a.shape == b.shape and a.shape[1] == 2 and np.array_equal(a, b)
    assert np.abs(paths[0] - d["c3_path"]).max() <= PATH_ATOL
    with pytest.raises(IndexError):
        FM.getPathsGDM(T, np.vstack([starts, [[T.shape[1] + 3.0, 5.0]]]), goal, 0.5)


def test_dropin_3d(golden):
    import FastMarching.FastMarching3D as FM3D

    d = golden("fmm3d")
    T, goal = d["v1_T_early"], d["v1_goal"]
    starts = _five_starts(T, d["v1_start"], lambda s: FM3D.getPathGDM(T, s, goal, 0.5), 41)
    paths = FM3D.getPathsGDM(T, starts, goal, 0.5)
    ref = [FM3D.getPathGDM(T, s, goal, 0.5) for s in starts]
    assert isinstance(paths, list) and len(paths) == 5
    for a, b in zip(paths, ref):
        assert a.shape == b.shape and a.shape[1] == 3 and np.array_equal(a, b)
    with pytest.raises(IndexError):
        FM3D.getPathsGDM(T, np.vstack([starts, [[T.shape[1] + 3.0, 5.0, 1.0]]]), goal, 0.5)
