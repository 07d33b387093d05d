"""The constructions of tests/handoff3d.py, checked on the oracle alone (no GPU): every hand-off
volume tests what it names.  The volume's far corners are reachable, and re-closing the named gap
cell (or pinhole column) changes the oracle's field in the tile across the named face -- a case with
one gap and no chain loses its finite mask there entirely, a multi-gap or chain case (where a detour
through another tile exists) changes a value there by more than 1e-6 relative.  So a solver that
loses the named flag cannot produce the expected field by another route."""
import numpy as np
import pytest

import handoff3d as H3
import oracle as O


def solve(cost, goal):
    O.set_strict(False)
    try:
        return O.fmm3d(cost, np.asarray(goal, np.int64), None)
    finally:
        O.set_strict(True)


def check_reclosed(R, Rc, across, entirely):
    """R: the case's field, Rc: the field with the named gap closed, across: index of the tile across
    the named face."""
    a, b = R[across], Rc[across]
    assert np.isfinite(a).any()
    if entirely:
        assert not np.isfinite(b).any()
        return
    fin = np.isfinite(a)
    with np.errstate(invalid="ignore"):
        rel = np.where(np.isfinite(b[fin]), np.abs(b[fin] - a[fin]) / a[fin], np.inf)
    assert rel.max() > 1e-6


# ----------------------------------------------------------------------------- tile geometry
def test_tile_shapes():
    assert [H3.tile_shape3(L) for L in (1, 3, 4, 5, 8, 9, 24)] == [(16, 16, 1), (16, 16, 3), (16, 16, 4), (16, 8, 5),
                                                                  (16, 8, 8), (16, 8, 8), (16, 8, 8)]
    tx, ty, tz = H3.tile_shape3(H3.SHELL_SHAPE[2])
    assert H3.SHELL_SHAPE == (3 * ty, 3 * tx, 3 * tz)
    assert H3.SHELL_LO == (tx, ty, tz) and H3.SHELL_HI == (2 * tx - 1, 2 * ty - 1, 2 * tz - 1)


# ----------------------------------------------------------------- A. the walled-in 16 x 8 x 8 tile
def test_closed_shell_is_sealed():
    R = solve(H3.shell_cost(()), H3.SHELL_GOAL)
    fin = np.isfinite(R)
    assert fin.sum() == 14 * 6 * 6
    (x0, y0, z0), (x1, y1, z1) = H3.SHELL_LO, H3.SHELL_HI
    assert fin[y0 + 1:y1, x0 + 1:x1, z0 + 1:z1].all()


def test_shell_gap_cells():
    assert H3.shell_gap("x-", "centre") == ((16, 12, 12), ())
    assert H3.shell_gap("x-", "corner") == ((16, 8, 8), ((17, 8, 8), (17, 9, 8)))
    assert H3.shell_gap("z+", "edge") == ((31, 12, 15), ((31, 12, 14),))
    for f in H3.FACES:
        a, plus = H3._axis_side(f)
        face = (H3.SHELL_HI if plus else H3.SHELL_LO)[a]
        for pos in ("centre", "edge", "corner"):
            cell, chain = H3.shell_gap(f, pos)
            assert cell[a] == face and all(q[a] != face for q in chain)
            assert len(chain) == {"centre": 0, "edge": 1, "corner": 2}[pos]
            # every opened cell was a shell cell
            closed = H3.shell_cost(())
            assert all(np.isinf(closed[y, x, z]) for x, y, z in (cell,) + chain)


@pytest.mark.parametrize("gaps", H3.SHELL_CASES, ids=H3.shell_id)
def test_shell_case(gaps):
    cost = H3.shell_cost(gaps)
    R = H3.oracle_field(("shell", gaps), cost, H3.SHELL_GOAL)
    assert H3.corners_finite(R)
    assert np.array_equal(np.isfinite(R), np.isfinite(cost))  # everything open is reached
    for face, pos in gaps:
        (x, y, z), chain = H3.shell_gap(face, pos)
        closed = cost.copy()
        closed[y, x, z] = np.inf
        check_reclosed(R, solve(closed, H3.SHELL_GOAL), H3.shell_across(face), entirely=len(gaps) == 1 and not chain)


@pytest.mark.parametrize("shape,side,z", H3.FLAT_CASES, ids=H3.flat_id)
def test_flat_case(shape, side, z):
    goal = H3.flat_goal(shape)
    cost = H3.flat_cost(shape, ((side, z),))
    R = H3.oracle_field(("flat", shape, side, z), cost, goal)
    assert H3.corners_finite(R) and np.array_equal(np.isfinite(R), np.isfinite(cost))
    closed = H3.flat_cost(shape, ())
    Rc = solve(closed, goal)
    tx, ty, tz = H3.tile_shape3(shape[2])
    assert np.isfinite(Rc).sum() == (tx - 2) * (ty - 2) * tz
    check_reclosed(R, Rc, H3.flat_across(shape, side), entirely=True)


# ------------------------------------------------------------------------ B. layered side flags
@pytest.mark.parametrize("f64,nl,gaps", H3.ring_cases(), ids=H3.ring_id)
def test_ring_case(f64, nl, gaps):
    th = H3.layered_rows(f64)
    cost = H3.ring_cost(th, nl, gaps)
    R = H3.oracle_field(("ring", th, nl, gaps, False), cost, H3.ring_goal(th))
    assert H3.corners_finite(R) and np.array_equal(np.isfinite(R), np.isfinite(cost))
    (side, lane, z), = gaps
    r, q = H3.ring_gap(th, side, lane)
    closed = cost.copy()
    closed[r, q, z] = np.inf
    corner = lane in (0, H3.side_lanes(th, side) - 1)
    check_reclosed(R, solve(closed, H3.ring_goal(th)), H3.ring_across(th, side), entirely=not corner)


@pytest.mark.parametrize("f64,nl,gaps", H3.ring_pad_cases(), ids=H3.ring_id)
def test_ring_pad_case(f64, nl, gaps):
    th = H3.layered_rows(f64)
    cost = H3.ring_cost(th, nl, gaps, pad=True)
    assert cost.shape[2] == nl + 2 and np.isinf(cost[:, :, 0]).all() and np.isinf(cost[:, :, -1]).all()
    goal = H3.ring_goal(th, 1)
    R = H3.oracle_field(("ring", th, nl, gaps, True), cost, goal)
    assert np.isfinite(R[np.ix_((0, -1), (0, -1), (1, nl))]).all()
    (side, lane, z), = gaps
    r, q = H3.ring_gap(th, side, lane)
    closed = cost.copy()
    closed[r, q, z + 1] = np.inf
    check_reclosed(R, solve(closed, goal), H3.ring_across(th, side), entirely=True)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_four_gap_case(f64):
    th = H3.layered_rows(f64)
    nl, gaps = H3.four_gaps(f64)
    assert len({z for _, _, z in gaps}) == min(nl, 4)
    cost = H3.ring_cost(th, nl, gaps)
    R = H3.oracle_field(("ring", th, nl, gaps, False), cost, H3.ring_goal(th))
    assert H3.corners_finite(R)
    for side, lane, z in gaps:
        r, q = H3.ring_gap(th, side, lane)
        closed = cost.copy()
        closed[r, q, z] = np.inf
        check_reclosed(R, solve(closed, H3.ring_goal(th)), H3.ring_across(th, side), entirely=False)


# --------------------------------------------------------------------- the goal's own hand-off
def lone_cases():
    out = [(H3.LONE3_SHAPE, H3.lone3_goal(f), f) for f in H3.FACES]
    for th in (H3.L32_ROWS, H3.L64_ROWS):
        out += [(H3.lone2_shape(th, nl), H3.lone2_goal(th, s), H3.LONE_SIDES[s]) for nl in (1, 3) for s in "NSWE"]
    return out


@pytest.mark.parametrize("shape,goal,face", lone_cases(), ids=H3.flat_id)
def test_lone_exit_case(shape, goal, face):
    """Everything is reached through the one open neighbour, which lies in another tile than the goal;
    with it closed nothing but the goal is."""
    cost = H3.lone_exit_cost(shape, goal, face)
    R = H3.oracle_field(("lone", shape, goal, face), cost, goal)
    assert H3.corners_finite(R) and np.array_equal(np.isfinite(R), np.isfinite(cost))
    x, y, z = H3.lone_exit_cell(goal, face)
    tx, ty, tz = H3.tile_shape3(shape[2]) if shape == H3.LONE3_SHAPE else (H3.LCOLS, shape[0] // 2, shape[2])
    assert (x // tx, y // ty, z // tz) != (goal[0] // tx, goal[1] // ty, goal[2] // tz)
    closed = cost.copy()
    closed[y, x, z] = np.inf
    assert np.isfinite(solve(closed, goal)).sum() == 1


# ------------------------------------------------------------------------------ C. z pinholes
@pytest.mark.parametrize("f64,nl,name,shape,pin", H3.PIN_CASES,
                         ids=[f"{'f64' if c[0] else 'f32'}-nl{c[1]}-{c[2]}" for c in H3.PIN_CASES])
def test_pinhole_case(f64, nl, name, shape, pin):
    assert 0 <= pin[0] < shape[1] and 0 <= pin[1] < shape[0]
    cost = H3.pinhole_cost(shape, pin)
    R = H3.oracle_field(("pin", shape, pin), cost, H3.PIN_GOAL)
    assert H3.corners_finite(R) and np.array_equal(np.isfinite(R), np.isfinite(cost))
    closed = cost.copy()
    closed[pin[1], pin[0], 1:nl - 1] = np.inf
    check_reclosed(R, solve(closed, H3.PIN_GOAL), (slice(None), slice(None), nl - 1), entirely=True)


def test_pinhole_rows_named():
    """The fp64 last-row cases are rows 39 and 79 of a 120-row volume, the cut cases lie in the cut
    last tile row / column of a (2 TH + 1) x 129 volume."""
    for th in (H3.L32_ROWS, H3.L64_ROWS):
        cases = {n: (hw, pin) for n, hw, pin in H3.pinhole_cases(th)}
        assert cases["lastrow1"] == ((3 * th, 128), (30, th - 1)) and cases["lastrow2"][1][1] == 2 * th - 1
        assert cases["lane0row0"][1] == (64, th)
        for n in ("cut_corner", "cut_row", "cut_col"):
            hw, (px, py) = cases[n]
            assert hw == (2 * th + 1, 129) and (px == 128 or py == 2 * th)
    assert [p[1] for n, _, p in H3.pinhole_cases(40) if n.startswith("lastrow")] == [39, 79]
