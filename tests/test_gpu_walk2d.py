"""The default 2D path walker (gdm2d_kernel, csrc/gdm.hip, all five loop forms, fp64 and fp32, single
and grid launch) on the crafted fields of tests/walk2d.py against the oracle: one walk per branch --
the coordinate-to-index rule (walks that leave through each side, the cells (-1, 0), starts no index
type holds), the step's arithmetic and the fast step's domain exits, the NaN fallback with its pops
and the wrapped node read, stop radius and point budget edges, and the window machinery (raster sides
around 64, walks over several windows, reversals, steps longer than a window).
tests/test_walk2d_cases.py checks (no GPU) that each field still takes the branch it is named for.

Per walk: the oracle's status, its row count, its rows within 1e-9 cells (the suite's PATH_ATOL;
non-finite rows equal, NaN matching NaN), and nothing written past the rows the walk ever held (the
output is filled with a sentinel and has guard rows past `cap`; row 0, the start, is written by every
walk; rows that the NaN fallback popped -- up to the oracle's count of the most rows held -- keep
the points they had, as nothing clears them).
fp32: the field is rounded to float32 and the oracle walks that rounded field, so every decision is
the same and the tolerance stays.  A walk with no row left for a point or for `end` is ERROR with
n == cap (walk2d.expected).
"""
import numpy as np
import pytest

import oracle as O
import walk2d as W2

pytestmark = pytest.mark.gpu
PATH_ATOL = 1e-9
FILL = -7.0   # sentinel of unwritten rows (no case's path holds it)
GUARD = 8     # rows past cap, which no walk may touch

_dev_fields = {}


def _dev():
    import torch

    return torch, torch.device("cuda", 0)


def _ctx(form=None):
    import eikonal
    from eikonal import _lib as L

    c = eikonal.Context(0)
    if form is not None:
        c.set_option(L.OPT_PATH_LOOP, form)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


def dev_field(name, f32):
    if (name, f32) not in _dev_fields:
        torch, dev = _dev()
        _dev_fields[(name, f32)] = torch.from_numpy(W2.field(name, f32).copy()).to(dev)
    return _dev_fields[(name, f32)]


def check_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    if fin.any():
        assert np.isfinite(got[fin]).all(), what
        err = np.abs(got[fin] - want[fin]).max()
        assert err <= PATH_ATOL, (what, err)


def held(name, f32, n, cap):
    """The first row a walk that returned n rows cannot have written."""
    return max(n, 1, min(W2.reference(name, f32)[2]["peak_rows"], cap) if n < cap else 0)


def walk_dev(c, Td, f32, shape, start, end, tau, cap):
    """eik_path2d_dev into a sentinel-filled output of cap + GUARD rows -> (all rows, n, status)."""
    from eikonal import _lib as L

    torch, dev = _dev()
    H, W = shape
    out = torch.full((cap + GUARD, 2), FILL, dtype=torch.float64, device=dev)
    n = torch.full((1,), -1, dtype=torch.int64, device=dev)
    st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    c._chk(L.lib().eik_path2d_dev(c._h, Td.data_ptr(), L.EIK_F32 if f32 else L.EIK_F64, H, W,
                                  np.array(start, np.float64), np.array(end, np.float64), tau, out.data_ptr(), cap,
                                  n.data_ptr(), st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out.cpu().numpy(), int(n.item()), int(st.item())


def check_case(c, name, f32, what):
    T, start, end, tau, cap = W2.case(name)
    want, wst = W2.expected(name, f32)
    rows, n, st = walk_dev(c, dev_field(name, f32), f32, T.shape, start, end, tau, cap)
    assert (st, n) == (wst, len(want)), (what, st, n, wst, len(want))
    check_rows(rows[:n], want, what)
    # nothing past the rows returned -- past the most rows the path ever held, where the fallback
    # popped some --, none past cap.  Row 0 always holds the start, as the reference's gamma does
    # before its loop: a walk that pops it (n = 0) leaves it there.
    assert (rows[held(name, f32, n, cap):] == FILL).all(), what
    if n == 0:
        assert np.array_equal(rows[0], start, equal_nan=True), what


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(W2.CASES))
def test_walk(ctx, name, f32):
    """The default loop form."""
    check_case(ctx, name, f32, name)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_walk_form(form):
    """EIK_OPT_PATH_LOOP 0-3 in fp64: every case against the oracle (not against another form)."""
    c = _ctx(form)
    try:
        for name in W2.CASES:
            check_case(c, name, False, (name, form))
    finally:
        c.close()


HOST_CASES = list(W2.FULL_BUDGET) + ["leave_x0", "neg_cell_y", "start_x_pinf", "start_y_two32m", "hop_pops_to_empty",
                                     "wrap_low_x", "odd_zero_norm"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_walk_host_entry(ctx, name):
    """eik_path2d_f64 (Context.path2d): the field uploaded by the call, the full point budget."""
    T, start, end, tau, cap = W2.case(name)
    assert cap == W2.full_cap(tau)  # the budget path2d allocates
    want, wst = W2.expected(name)
    path, st = ctx.path2d(T, start, end, tau)
    assert (st, len(path)) == (wst, len(want))
    check_rows(path, want, name)


# one launch, every kind of exit: (case, status and rows under BATCH_CAP)
BATCH_CAP = 12
BATCH = [("neg_cell_x", 0, 8), ("start_in_radius", 0, 3), ("wrap_low_x_inf", 1, 0), ("wrap_low_y", 1, 1),
         ("constant", 1, 1), ("leave_x0", 2, 10), ("leave_yhi", 2, 7), ("start_x_nan", 2, 1), ("start_y_two32m", 2, 1),
         ("start_y_ninf", 2, 1), ("zero_gradient", 2, 2), ("full_budget", 2, 12), ("cone_tau05", 2, 12),
         ("walk_into_nan", 2, 12), ("crease_unit_steps", 2, 12)]


def test_batch_mixes_exits(ctx):
    """One eik_path2d_batch_dev launch on a stack of 12 x 14 fields with a 12-row budget: walks that end
    DONE, FALLBACK (with no row, and with the one node row), ERROR of four kinds (left through a low
    and a high side, a NaN, an infinite and a 2^32 start, a NaN row) and four that run into the budget
    (one of them on the very point whose gradient is NaN).  Every path equals its single call bit for
    bit and the oracle to 1e-9, each status is its own, and no walk writes into a neighbour's rows."""
    from eikonal import _lib as L

    torch, dev = _dev()
    names = [b[0] for b in BATCH]
    cases = [W2.case(nm) for nm in names]
    assert all(c[0].shape == W2.SHAPE and c[3] == 0.5 for c in cases)
    stack = np.stack([c[0] for c in cases])
    Td = torch.from_numpy(stack).to(dev)
    P, cap = len(cases), BATCH_CAP
    inits = np.ascontiguousarray([c[1] for c in cases])
    ends = np.ascontiguousarray([c[2] for c in cases])
    out = torch.full((P, cap, 2), FILL, dtype=torch.float64, device=dev)
    n = torch.full((P,), -1, dtype=torch.int64, device=dev)
    st = torch.full((P,), -1, dtype=torch.int32, device=dev)
    ctx._chk(L.lib().eik_path2d_batch_dev(ctx._h, Td.data_ptr(), L.EIK_F64, P, *W2.SHAPE, P, None, inits, ends, 0.5,
                                          out.data_ptr(), cap, n.data_ptr(), st.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream))
    out, n, st = out.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()
    for p, (nm, wst, wn) in enumerate(BATCH):
        want, est = W2.expected(nm, cap=cap)
        assert (est, len(want)) == (wst, wn), nm  # the exits this test is about
        assert (int(st[p]), int(n[p])) == (wst, wn), (nm, st[p], n[p])
        check_rows(out[p, : n[p]], want, nm)
        assert (out[p, held(nm, False, int(n[p]), cap):] == FILL).all(), nm  # the rest of its block, up to the neighbour's
        rows, n1, st1 = walk_dev(ctx, Td[p], False, W2.SHAPE, cases[p][1], cases[p][2], 0.5, cap)
        assert (st1, n1) == (int(st[p]), int(n[p])) and np.array_equal(rows[:n1], out[p, :n1], equal_nan=True), nm
    # the host entry returns the same
    got = ctx.path2d_batch(stack, inits, ends, 0.5, cap=cap)
    for p, (path, s) in enumerate(got):
        assert s == int(st[p]) and np.array_equal(path, out[p, : n[p]], equal_nan=True), names[p]


def test_gradient_crafted_field(ctx):
    """computeGradient (gradient2d_kernel) on a 9 x 11 field with +inf cells that takes every branch of
    FastMarching.py:262-294 on both axes (tests/test_walk2d_cases.py checks that it does), 0 / 0 = NaN
    included: the oracle's NaN mask, its values within 1e-15."""
    T = W2.gradient_field()
    gx, gy = ctx.gradient2d(T)
    rx, ry = O.gradient2d(T)
    for g, r in ((gx, rx), (gy, ry)):
        assert np.array_equal(np.isnan(g), np.isnan(r))
        m = ~np.isnan(r)
        assert np.isfinite(r[m]).all() and np.abs(g[m] - r[m]).max() <= 1e-15
