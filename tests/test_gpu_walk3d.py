"""The 3D path walker (gdm3d_kernel, csrc/gdm.hip) on the crafted volumes of tests/walk3d.py against
the oracle: one walk per branch -- back-tracking below the 256-point ring, the integer-descent run
loop with its budget, stop-radius and cap exits, face nodes, normalised steps, walks that leave the
volume, non-finite coordinates, degenerate starts.  tests/test_walk3d_cases.py checks (no GPU) that
each volume still takes the branch it is named for.

Per walk: the oracle's status, its point count, its rows within 1e-9 cells (the suite's PATH_ATOL;
non-finite rows equal, NaN matching NaN), and nothing written past the rows returned (the output is
filled with a sentinel and has guard rows past `cap`; row 0, the start, is written by every walk).
fp32: the field is rounded to float32 and the oracle walks that rounded field, so every decision is
the same and the tolerance stays.  A capped case expects status ERROR, n == cap and the first cap
rows of the oracle's uncapped walk.
"""
import numpy as np
import pytest

import oracle as O
import walk3d as W3

pytestmark = pytest.mark.gpu
PATH_ATOL = 1e-9
FILL = -7.0   # sentinel of unwritten rows (no case's path holds it)
GUARD = 8     # rows past cap, which no walk may touch


@pytest.fixture(scope="module")
def ctx():
    import eikonal

    c = eikonal.Context(0)
    yield c
    c.close()


def _dev():
    import torch

    return torch, torch.device("cuda", 0)


def expected(name, f32):
    """(rows, status) the walker must return for the case."""
    path, st, _ = W3.reference(name, f32)
    cap = W3.case(name)[4]
    if name in W3.CAPPED:
        assert len(path) > cap
        return path[:cap], O.GDM_ERROR
    assert len(path) <= cap
    return path, st


def check_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    if fin.any():
        assert np.isfinite(got[fin]).all(), what
        err = np.abs(got[fin] - want[fin]).max()
        assert err <= PATH_ATOL, (what, err)


def walk_dev(c, Td, f32, shape, start, end, tau, cap):
    """eik_path3d_dev into a sentinel-filled output of cap + GUARD rows -> (all rows, n, status)."""
    from eikonal import _lib as L

    torch, dev = _dev()
    H, W, Lz = shape
    out = torch.full((cap + GUARD, 3), FILL, dtype=torch.float64, device=dev)
    n = torch.full((1,), -1, dtype=torch.int64, device=dev)
    st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    c._chk(L.lib().eik_path3d_dev(c._h, Td.data_ptr(), L.EIK_F32 if f32 else L.EIK_F64, H, W, Lz,
                                  np.array(start, np.float64), np.array(end, np.float64), tau, out.data_ptr(), cap,
                                  n.data_ptr(), st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out.cpu().numpy(), int(n.item()), int(st.item())


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(W3.CASES))
def test_walk(ctx, name, f32):
    torch, dev = _dev()
    T, start, end, tau, cap = W3.case(name)
    want, wst = expected(name, f32)
    Td = torch.from_numpy(W3.field(name, f32).copy()).to(dev)
    rows, n, st = walk_dev(ctx, Td, f32, T.shape, start, end, tau, cap)
    assert (st, n) == (wst, len(want)), (name, st, n, wst, len(want))
    check_rows(rows[:n], want, name)
    # nothing past the rows returned, none past cap.  Row 0 always holds the start, as the reference's
    # gamma does before its loop: a walk that pops it (n = 0) leaves it there.
    assert (rows[max(n, 1):] == FILL).all(), name
    if n == 0:
        assert np.array_equal(rows[0], start)


HOST_CASES = ["run_stretch", "cone_tau17", "low_face", "low_face_wrapped_move", "high_face_error", "leave_low",
              "leave_high", "leave_flat", "leave_two_layers", "one_layer", "nan_start", "inf_cell", "inf_cell_mirror",
              "nan_cells_around", "step_into_wall", "start_is_end", "start_all_inf"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_walk_host_entry(ctx, name):
    """eik_path3d_f64 (Context.path3d): the field uploaded by the call, the full point budget."""
    T, start, end, tau, cap = W3.case(name)
    assert cap == W3.full_cap(tau)  # the budget path3d allocates
    want, wst = expected(name, False)
    path, st = ctx.path3d(T, start, end, tau)
    assert (st, len(path)) == (wst, len(want))
    check_rows(path, want, name)


# one launch, five kinds of exit: (case, how it ends under BATCH_CAP)
BATCH_CAP = 12
BATCH = ["nan_cells_beside", "leave_low", "cone_tau05", "leave_high", "start_node_inf", "start_in_radius",
         "leave_flat"]


def test_batch_mixes_exits(ctx):
    """One path3d batch launch on a stack of 10 x 12 x 9 fields with a 12-row budget: walks that end
    DONE (11 and 3 points), the two that leave through x = 0 and x = W - 1 (ERROR, 4 and 3 points), a
    start with no path (ERROR, n = 0) and two that run into the budget (the cone's 30002-point walk
    and the flat field's 21 points: ERROR, n = cap, the walk's first 12 rows -- trilinear steps never
    pop, so the prefix is well defined).  Every path equals its single call bit for bit and the
    oracle to 1e-9, each status is its own, and no walk writes into a neighbour's rows."""
    from eikonal import _lib as L

    torch, dev = _dev()
    cases = [W3.case(nm) for nm in BATCH]
    assert all(c[0].shape == W3.SHAPE and c[3] == 0.5 for c in cases)
    stack = np.stack([c[0] for c in cases])
    Td = torch.from_numpy(stack).to(dev)
    P, cap = len(cases), BATCH_CAP
    inits = np.ascontiguousarray([c[1] for c in cases])
    ends = np.ascontiguousarray([c[2] for c in cases])
    out = torch.full((P, cap, 3), FILL, dtype=torch.float64, device=dev)
    n = torch.full((P,), -1, dtype=torch.int64, device=dev)
    st = torch.full((P,), -1, dtype=torch.int32, device=dev)
    ctx._chk(L.lib().eik_path3d_batch_dev(ctx._h, Td.data_ptr(), L.EIK_F64, P, *W3.SHAPE, P, None, inits, ends, 0.5,
                                          out.data_ptr(), cap, n.data_ptr(), st.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream))
    out, n, st = out.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()
    want_n, want_st = [], []
    for p, nm in enumerate(BATCH):
        path, ost, _ = W3.reference(nm)
        capped = len(path) > cap
        want = path[:cap] if capped else path
        want_n.append(len(want))
        want_st.append(O.GDM_ERROR if capped else ost)
        assert (int(st[p]), int(n[p])) == (want_st[-1], len(want)), (nm, st[p], n[p])
        check_rows(out[p, : n[p]], want, nm)
        assert (out[p, max(n[p], 1):] == FILL).all(), nm  # the rest of its own block, up to the neighbour's rows
        rows, n1, st1 = walk_dev(ctx, Td[p], False, W3.SHAPE, cases[p][1], cases[p][2], 0.5, cap)
        assert (st1, n1) == (int(st[p]), int(n[p])) and np.array_equal(rows[:n1], out[p, :n1], equal_nan=True), nm
    assert want_n == [11, 4, 12, 3, 0, 3, 12] and want_st == [0, 2, 2, 2, 2, 0, 2]
    # the host entry returns the same
    got = ctx.path3d_batch(stack, inits, ends, 0.5, cap=cap)
    for p, (path, s) in enumerate(got):
        assert s == int(st[p]) and np.array_equal(path, out[p, : n[p]], equal_nan=True), BATCH[p]
