"""The constructions of tests/walk2d.py, checked on the oracle alone (no GPU): every crafted walk still
takes the branch it is named for.  The oracle's event counts (orc_gdm2d_events) say which branches a
walk took; the table below pins them with the status and the row count, and the tests after it state,
per group, the condition that makes a case what it is -- so a later edit of a builder cannot silently
turn a case into a plain walk.  The window cases, which the oracle knows nothing of, are pinned by
the geometry of the oracle's path: the 64-column and 64-row lines it crosses and its reversals.

Conditioning: the GPU walker squares with exact products where the reference's scalar `x**2` goes
through libm pow.  Every case is walked both ways, on the float64 field and on the field rounded to
float32; the two walks must agree in status and length and to 1e-11 in every row, 100 times under
the 1e-9 the GPU tests allow, so that a GPU mismatch is the kernel's and not the case's."""
import numpy as np
import pytest

import oracle as O
import walk2d as W2

DONE, FALLBACK, ERROR = O.GDM_DONE, O.GDM_FALLBACK, O.GDM_ERROR
COND_ATOL = 1e-11

# name: (status, rows, (steps, |g| < 0.01 steps, a == 0 only, b == 0 only, both 0, points with a coordinate in
# (-1, 0), pops on +inf nodes, pops within 1 of the node, wrapped node reads, exit kind, most rows held,
# steps outside the fast step's domain)) of the walk with the reference's own budget, on the float64 field
EXPECT = {
    "leave_x0": (2, 10, (9, 0, 0, 0, 0, 2, 0, 0, 0, 6, 10, 0)),
    "leave_y0": (2, 10, (9, 0, 0, 0, 0, 2, 0, 0, 0, 6, 10, 0)),
    "leave_xhi": (2, 7, (6, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 0)),
    "leave_yhi": (2, 7, (6, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 0)),
    "neg_cell_x": (0, 8, (6, 0, 0, 0, 0, 1, 0, 0, 0, 0, 8, 0)),
    "neg_cell_y": (0, 8, (6, 0, 0, 0, 0, 1, 0, 0, 0, 0, 8, 0)),
    "start_x_nan": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 0)),
    "start_x_pinf": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 0)),
    "start_x_ninf": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 0)),
    "start_x_m1": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_x_m1eps": (2, 2, (1, 0, 0, 0, 0, 1, 0, 0, 0, 6, 2, 0)),
    "start_x_two31": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_x_two32m": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_x_two32p": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_y_nan": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 0)),
    "start_y_pinf": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 0)),
    "start_y_ninf": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 0)),
    "start_y_m1": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_y_m1eps": (2, 2, (1, 0, 0, 0, 0, 1, 0, 0, 0, 6, 2, 0)),
    "start_y_two31": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_y_two32m": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_y_two32p": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_last_col": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_below_last_col": (0, 9, (7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 0)),
    "start_last_row": (2, 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, 0)),
    "start_below_last_row": (0, 9, (7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 0)),
    "cone_tau05": (0, 14, (12, 0, 0, 0, 0, 0, 0, 0, 0, 0, 14, 0)),
    "cone_tau17": (0, 6, (4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 0)),
    "crease_unit_steps": (0, 17, (15, 15, 0, 7, 0, 0, 0, 0, 0, 0, 17, 0)),
    "start_on_node": (0, 10, (8, 0, 0, 4, 4, 0, 0, 0, 0, 0, 10, 0)),
    "start_on_line_a0": (0, 10, (8, 0, 8, 0, 0, 0, 0, 0, 0, 0, 10, 0)),
    "start_on_line_b0": (0, 10, (8, 0, 0, 8, 0, 0, 0, 0, 0, 0, 10, 0)),
    "zero_gradient": (2, 2, (1, 1, 0, 0, 0, 0, 0, 0, 0, 5, 2, 1)),
    "tiny_tau_capped": (0, 4802, (4800, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4802, 0)),
    "odd_tiny_component": (2, 4, (3, 0, 0, 0, 0, 2, 0, 0, 0, 6, 4, 3)),
    "odd_tiny_norm": (0, 9, (7, 7, 3, 0, 0, 0, 0, 0, 0, 0, 9, 7)),
    "odd_zero_norm": (2, 2, (1, 1, 0, 0, 0, 0, 0, 0, 0, 5, 2, 1)),
    "odd_inf_gradient": (2, 2, (1, 0, 0, 0, 1, 0, 0, 0, 0, 5, 2, 1)),
    "inf_gradient_off_node": (1, 1, (0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 1, 0)),
    "constant": (1, 1, (0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 1, 0)),
    "hop_pops_to_empty": (1, 0, (3, 0, 0, 4, 0, 0, 4, 0, 0, 3, 4, 0)),
    "hop_pops_to_node": (1, 1, (3, 0, 0, 4, 0, 0, 3, 1, 0, 2, 4, 0)),
    "walk_into_nan": (1, 10, (11, 0, 0, 0, 0, 0, 0, 3, 0, 2, 12, 0)),
    "wrap_low_x": (1, 1, (0, 0, 0, 0, 0, 1, 0, 1, 1, 2, 1, 0)),
    "wrap_low_y": (1, 1, (0, 0, 0, 0, 0, 1, 0, 1, 1, 2, 1, 0)),
    "wrap_low_x_inf": (1, 0, (0, 0, 0, 0, 0, 1, 1, 0, 1, 3, 1, 0)),
    "wrap_low_y_inf": (1, 0, (0, 0, 0, 0, 0, 1, 1, 0, 1, 3, 1, 0)),
    "fallback_at_cap": (1, 10, (11, 0, 0, 0, 0, 0, 0, 3, 0, 2, 12, 0)),
    "fallback_below_cap": (1, 10, (11, 0, 0, 0, 0, 0, 0, 3, 0, 2, 12, 0)),
    "start_in_radius": (0, 3, (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0)),
    "start_outside_radius": (0, 4, (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0)),
    "long_cap2": (0, 30002, (30000, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30002, 0)),
    "long_cap3": (0, 30002, (30000, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30002, 0)),
    "long_cap50": (0, 30002, (30000, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30002, 0)),
    "end_fits": (0, 16, (14, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0)),
    "end_does_not_fit": (0, 16, (14, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0)),
    "full_budget": (0, 30002, (30000, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30002, 0)),
    "full_budget_fits": (0, 30002, (30000, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30002, 0)),
    "full_budget_one_short": (0, 30002, (30000, 0, 0, 0, 0, 0, 0, 0, 0, 1, 30002, 0)),
    "side_x3": (0, 17, (15, 0, 0, 0, 0, 0, 0, 0, 0, 0, 17, 0)),
    "side_x63": (0, 122, (120, 0, 0, 0, 0, 0, 0, 0, 0, 0, 122, 0)),
    "side_x64": (0, 124, (122, 0, 0, 0, 0, 0, 0, 0, 0, 0, 124, 0)),
    "side_x65": (0, 126, (124, 0, 0, 0, 0, 0, 0, 0, 0, 0, 126, 0)),
    "side_x66": (0, 128, (126, 0, 0, 0, 0, 0, 0, 0, 0, 0, 128, 0)),
    "side_x80": (0, 155, (153, 0, 0, 0, 0, 0, 0, 0, 0, 0, 155, 0)),
    "side_y3": (0, 21, (19, 0, 0, 0, 0, 0, 0, 0, 0, 0, 21, 0)),
    "side_y63": (0, 122, (120, 0, 0, 0, 0, 0, 0, 0, 0, 0, 122, 0)),
    "side_y64": (0, 124, (122, 0, 0, 0, 0, 0, 0, 0, 0, 0, 124, 0)),
    "side_y65": (0, 126, (124, 0, 0, 0, 0, 0, 0, 0, 0, 0, 126, 0)),
    "side_y66": (0, 128, (126, 0, 0, 0, 0, 0, 0, 0, 0, 0, 128, 0)),
    "side_y80": (0, 156, (154, 0, 0, 0, 0, 0, 0, 0, 0, 0, 156, 0)),
    "windows_x": (0, 454, (452, 0, 0, 0, 0, 0, 0, 0, 0, 0, 454, 0)),
    "windows_y": (0, 454, (452, 0, 0, 0, 0, 0, 0, 0, 0, 0, 454, 0)),
    "windows_diag": (0, 417, (415, 0, 0, 0, 0, 0, 0, 0, 0, 0, 417, 0)),
    "serpentine_tau05": (0, 1492, (1490, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1492, 0)),
    "serpentine_tau17": (0, 446, (444, 0, 0, 0, 0, 0, 0, 0, 0, 0, 446, 0)),
    "tau70": (0, 216, (214, 0, 0, 0, 0, 0, 0, 0, 0, 1, 216, 0)),
}
# the cases whose float32 field walks differently: 2^-950, 2^-410 and 2^-600 round to 0 in float32, so
# the gradients these cases are built on are exact zeros there (no float32 field holds a normalised
# gradient component below 2^-900: the ratio of two float32 differences is 0 or above 2^-277)
EXPECT_F32 = {
    "odd_tiny_component": (2, 4, (3, 0, 0, 0, 0, 2, 0, 0, 0, 6, 4, 0)),
    "odd_tiny_norm": (2, 2, (1, 1, 0, 0, 0, 0, 0, 0, 0, 5, 2, 1)),
    "odd_inf_gradient": (1, 1, (0, 0, 0, 0, 1, 0, 0, 1, 0, 2, 1, 0)),
}


def ref(name, f32=False):
    return W2.reference(name, f32)


def test_every_case_is_pinned():
    assert set(EXPECT) == set(W2.CASES) and set(EXPECT_F32) <= set(EXPECT)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(W2.CASES))
def test_case_events(name, f32):
    path, st, ev = ref(name, f32)
    want = EXPECT_F32[name] if f32 and name in EXPECT_F32 else EXPECT[name]
    assert (st, len(path), tuple(ev.values())) == want


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(W2.CASES))
def test_case_is_well_conditioned(name, f32):
    """libm pow against exact products: same status, same length, rows within 1e-11."""
    path, st, _ = ref(name, f32)
    exact, est, _ = W2.walk(name, f32, exact=True)
    assert (est, len(exact)) == (st, len(path))
    fin = np.isfinite(path)
    assert np.array_equal(path[~fin], exact[~fin], equal_nan=True)
    if fin.any():
        assert np.abs(path[fin] - exact[fin]).max() <= COND_ATOL


def test_fields_are_small():
    for name in W2.CASES:
        H, W = W2.case(name)[0].shape
        assert 3 <= min(H, W) and max(H, W) <= 230 and H * W <= 150 * 230, name


# ------------------------------------------------------------------------------ conversions
@pytest.mark.parametrize("name,axis,low", [("leave_x0", 0, True), ("leave_y0", 1, True), ("leave_xhi", 0, False),
                                           ("leave_yhi", 1, False)])
def test_leaving_walks(name, axis, low):
    path, st, ev = ref(name)
    T = W2.case(name)[0]
    last = T.shape[1 - axis] - 1
    assert st == ERROR and ev["exit"] == O.EXIT_INDEX and np.isfinite(path).all()
    c = path[:, axis]
    if low:  # passes (-1, 0) -- walked through with a negative fraction -- and raises at the first p <= -1
        assert c[-1] <= -1 and (c[:-1] > -1).all() and ((c > -1) & (c < 0)).sum() == 2 == ev["negative_cell_points"]
    else:
        assert c[-1] >= last and (c[:-1] < last).all()


def test_leave_x0_is_the_walk_that_crashed_the_unchecked_cast():
    """12 x 14, T = x, start (3.2, 5.5), tau = 0.5: the cast of -1.3 to uint32 gave 2^32 - 1, i + 1
    wrapped to 0 and the gradient was read 32 GB past the field."""
    T, start, end, tau, _ = W2.case("leave_x0")
    assert T.shape == (12, 14) and np.array_equal(T, np.tile(np.arange(14.0), (12, 1)))
    assert start.tolist() == [3.2, 5.5] and end.tolist() == [12.0, 10.0] and tau == 0.5
    path = ref("leave_x0")[0]
    assert np.allclose(path[-3:, 0], [-0.3, -0.8, -1.3], atol=1e-12)


@pytest.mark.parametrize("name,axis", [("neg_cell_x", 0), ("neg_cell_y", 1)])
def test_negative_cell_is_walked_through(name, axis):
    path, st, ev = ref(name)
    assert st == DONE and ev["exit"] == O.EXIT_STOP and ev["negative_cell_points"] == 1
    assert np.allclose(path[-3:-1, axis], [-0.3, -0.8], atol=1e-12)  # -0.8 is within 1.5 of the end


@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_bad_starts(axis):
    a = "xy"[axis]
    for k in ("nan", "pinf", "ninf"):  # computeGradient's int(point), outside the try
        path, st, ev = ref(f"start_{a}_{k}")
        assert st == ERROR and ev["exit"] == O.EXIT_NONFINITE and len(path) == 1 and not np.isfinite(path[0, axis])
    for k in ("m1", "two31", "two32m", "two32p"):  # IndexError; 2^32 + 5.5 is not wrapped to cell 5
        path, st, ev = ref(f"start_{a}_{k}")
        assert st == ERROR and ev["exit"] == O.EXIT_INDEX and len(path) == 1
        assert path[0, axis] == W2.BAD_STARTS[k]
    path, st, ev = ref(f"start_{a}_m1eps")  # cell 0, fraction -1 + 2^-52: one step, then p <= -1
    assert st == ERROR and len(path) == 2 and ev["negative_cell_points"] == 1 and path[0, axis] > -1 >= path[1, axis]


def test_last_cell_starts():
    for name, axis in (("start_last_col", 0), ("start_last_row", 1)):
        path, st, ev = ref(name)
        last = W2.SHAPE[1 - axis] - 1
        assert st == ERROR and ev["exit"] == O.EXIT_INDEX and len(path) == 1 and path[0, axis] == last
        path, st, ev = ref(name.replace("start_", "start_below_"))
        assert st == DONE and last - 1 < path[0, axis] < last


# -------------------------------------------------------------------------- step arithmetic
def test_cones():
    for name in ("cone_tau05", "cone_tau17"):
        path, st, ev = ref(name)
        tau = W2.case(name)[3]
        assert st == DONE and ev["exit"] == O.EXIT_STOP and ev["unit_steps"] == 0
        assert np.allclose(np.linalg.norm(np.diff(path[:-1], axis=0), axis=1), tau, atol=1e-2)
    assert np.abs(np.diff(ref("cone_tau17")[0][:-1], axis=0)).max() > 1.0  # more than one cell per step


def test_crease_takes_unit_steps():
    path, st, ev = ref("crease_unit_steps")
    assert st == DONE and ev["unit_steps"] == ev["steps"] == 15
    assert (path[:, 0] == 6.5).all() and np.allclose(np.diff(path[:-1, 1]), -0.5, atol=1e-12)


def test_zero_fractions():
    assert ref("start_on_node")[2]["ab_zero"] == 4 and ref("start_on_node")[2]["b_zero"] == 4
    ev = ref("start_on_line_a0")[2]
    assert ev["a_zero"] == ev["steps"] == 8 and ev["b_zero"] == ev["ab_zero"] == 0
    ev = ref("start_on_line_b0")[2]
    assert ev["b_zero"] == ev["steps"] == 8 and ev["a_zero"] == ev["ab_zero"] == 0


def test_zero_gradient_divides_by_zero():
    path, st, ev = ref("zero_gradient")
    assert st == ERROR and ev["exit"] == O.EXIT_NONFINITE and len(path) == 2 and np.isnan(path[1]).all()


def test_fast_step_domain_exits():
    """gdm_walk.hpp walk_odd: a nonzero component below 2^-900, |g|^2 below 2^-767 (nonzero, and
    underflowed to 0), |g|^2 = +inf -- each on every step of its walk."""
    path, st, ev = ref("odd_tiny_component")
    assert ev["odd_steps"] == ev["steps"] == 3 and st == ERROR and np.isfinite(path).all()
    path, st, ev = ref("odd_tiny_norm")
    assert ev["odd_steps"] == ev["steps"] == ev["unit_steps"] == 7 and st == DONE
    assert (path[:-1, 1] == 0.5).all() and np.allclose(np.diff(path[:-1, 0]), -0.5)
    path, st, ev = ref("odd_zero_norm")  # 2^-941 / sqrt(0) and 0 / sqrt(0): a step to (-inf, NaN), a row that stays
    assert ev["odd_steps"] == 1 and st == ERROR and path[1, 0] == -np.inf and np.isnan(path[1, 1])
    path, st, ev = ref("odd_inf_gradient")  # inf / inf
    assert ev["odd_steps"] == 1 and ev["ab_zero"] == 1 and st == ERROR and np.isnan(path[1]).all()
    path, st, ev = ref("inf_gradient_off_node")  # inf - inf in the interpolation: the NaN fallback
    assert st == FALLBACK and path.tolist() == [[5.0, 5.0]]


def test_tiny_tau_runs_into_its_cap():
    path, st, ev = ref("tiny_tau_capped")
    cap = W2.case("tiny_tau_capped")[4]
    rows, est = W2.expected("tiny_tau_capped")
    assert st == DONE and len(path) > cap and est == ERROR and np.array_equal(rows, path[:cap])


# ----------------------------------------------------------------------------- NaN fallback
def test_fallbacks():
    path, st, ev = ref("constant")
    assert st == FALLBACK and path.tolist() == [[4.0, 5.0]] and ev["near_pops"] == 1
    path, st, ev = ref("hop_pops_to_empty")
    assert st == FALLBACK and len(path) == 0 and ev["inf_pops"] == 4 == ev["peak_rows"] and ev["exit"] == O.EXIT_FB_EMPTY
    path, st, ev = ref("hop_pops_to_node")
    assert st == FALLBACK and path.tolist() == [[11.0, 5.0]] and (ev["inf_pops"], ev["near_pops"]) == (3, 1)
    path, st, ev = ref("walk_into_nan")
    assert st == FALLBACK and ev["near_pops"] == 3 and ev["peak_rows"] == 12 and len(path) == 10
    assert path[-1].tolist() == [4.0, 6.0] or path[-1].tolist() == [4.0, 5.0]


@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_wrapped_node_read(axis):
    a = "xy"[axis]
    path, st, ev = ref(f"wrap_low_{a}")
    assert st == FALLBACK and ev["wrapped_reads"] == 1 and len(path) == 1 and path[0, axis] == -1.0
    path, st, ev = ref(f"wrap_low_{a}_inf")  # the wrapped node is +inf: the start is popped
    assert st == FALLBACK and ev["wrapped_reads"] == 1 and ev["inf_pops"] == 1 and len(path) == 0


def test_fallback_at_the_cap_is_a_budget_exit():
    """The walk's NaN gradient is at its 12th point.  With 13 rows the fallback is reached; with 12
    the budget runs out first (no step is taken from a point that fills the last row), so a fallback
    with n == cap cannot happen: ERROR with the 12 points."""
    path, st, ev = ref("fallback_at_cap")
    assert st == FALLBACK and ev["steps"] == 11
    rows, est = W2.expected("fallback_at_cap")
    assert est == ERROR and len(rows) == 12 == W2.case("fallback_at_cap")[4] and np.array_equal(rows[:9], path[:9])
    rows, est = W2.expected("fallback_below_cap")
    assert est == FALLBACK and np.array_equal(rows, path)


# --------------------------------------------------------------------------- stop and budget
def test_stop_radius_starts():
    path, st, _ = ref("start_in_radius")
    assert st == DONE and len(path) == 3 and np.linalg.norm(path[0] - path[-1]) < 1.5
    path, st, _ = ref("start_outside_radius")
    assert st == DONE and len(path) == 4 and np.linalg.norm(path[0] - path[-1]) >= 1.5


def test_budgets():
    full = ref("full_budget")[0]
    assert len(full) == 30002 and ref("full_budget")[2]["exit"] == O.EXIT_BUDGET
    assert np.linalg.norm(full[-2] - full[-1]) >= 1.5
    for c in W2.LONG_CAPS:
        rows, st = W2.expected(f"long_cap{c}")
        assert st == ERROR and np.array_equal(rows, full[:c])
    rows, st = W2.expected("full_budget")
    assert st == DONE and len(rows) == 30002
    rows, st = W2.expected("full_budget_fits")
    assert st == DONE and len(rows) == 30002 == W2.case("full_budget_fits")[4]
    rows, st = W2.expected("full_budget_one_short")  # every step taken, no row left for `end`
    assert st == ERROR and np.array_equal(rows, full[:30001])


def test_end_row_edge():
    """The stop radius is reached by the step that writes row 14: with 16 rows `end` fits, with 15 it
    does not and the walk is out of budget (ERROR, n = cap), as any walk with no row left for `end`."""
    path, st, ev = ref("end_fits")
    assert st == DONE and len(path) == 16 and ev["exit"] == O.EXIT_STOP
    rows, est = W2.expected("end_fits")
    assert est == DONE and np.array_equal(rows, path)
    rows, est = W2.expected("end_does_not_fit")
    assert est == ERROR and np.array_equal(rows, path[:15])


# ------------------------------------------------------------------------ window machinery
def lines_crossed(c):
    """The multiples of 64 between consecutive cells of the coordinate sequence c, in walk order."""
    cells = np.floor(c).astype(int) // 64
    return int((np.diff(cells) != 0).sum())


@pytest.mark.parametrize("s", W2.SIDES)
def test_sides(s):
    """Raster sides around the 64-node window: xmax / ymax (gdm_walk.hpp Walk2Win) = 0, 0, 0, 1, 2, 16."""
    assert max(s - 64, 0) == {3: 0, 63: 0, 64: 0, 65: 1, 66: 2, 80: 16}[s]
    for name, axis in ((f"side_x{s}", 0), (f"side_y{s}", 1)):
        path, st, _ = ref(name)
        T = W2.case(name)[0]
        assert T.shape[1 - axis] == s and st == DONE
        c = path[:-1, axis]
        assert c[0] == s - 1.5 and c.min() < 2.7  # from the last cell of the axis to the first ones


def test_straight_walks_cross_three_windows():
    for name, axes in (("windows_x", (0,)), ("windows_y", (1,)), ("windows_diag", (0, 1))):
        path, st, _ = ref(name)
        assert st == DONE
        for axis in axes:
            assert lines_crossed(path[:-1, axis]) >= 2 and np.ptp(path[:-1, axis]) > 128


@pytest.mark.parametrize("name", ["serpentine_tau05", "serpentine_tau17"])
def test_serpentine_reverses(name):
    """Four runs over more than 128 columns, alternating in direction: a window prefetched ahead of the
    walk is abandoned at every turn."""
    path, st, _ = ref(name)
    assert st == DONE and W2.case(name)[0].shape == W2.SERP_SHAPE
    x = path[:-1, 0]
    assert x.min() < 30 and x.max() > 200
    far = np.where(x > 192, 1, np.where(x < 64, -1, 0))  # past the last / before the first 64-column line
    far = far[far != 0]
    turns = int((np.diff(far) != 0).sum())
    assert turns >= 4 and lines_crossed(x) >= 12 and lines_crossed(path[:-1, 1]) >= 2


def test_tau70_leaves_both_windows_every_step():
    path, st, ev = ref("tau70")
    assert st == DONE and ev["exit"] == O.EXIT_BUDGET and ev["steps"] == 214
    assert np.allclose(np.abs(np.diff(path[:-1, 0])), 70.0, atol=1e-9)  # a window is 64 nodes wide


# ------------------------------------------------------------------------ computeGradient
def test_gradient_field_takes_every_branch():
    T = W2.gradient_field()
    br = W2.gradient_branches(T)
    assert T.shape == (9, 11)
    for ax in (0, 1):
        assert set(np.unique(br[ax])) == {0, 1, 2, 3, 4, 5}
    gx, gy = O.gradient2d(T)
    assert (br[0, 4, 4], br[1, 4, 4]) == (2, 2) and np.isnan(gx[4, 4]) and np.isnan(gy[4, 4])  # 0 / 0
    assert br[1, 7, 8] == 2 and gx[7, 8] == 0 and abs(gy[7, 8]) == 1  # only x gives 0
    assert br[0, 2, 9] == 2 and gy[2, 9] == 0 and abs(gx[2, 9]) == 1  # only y
    assert np.isfinite(gx).sum() > 60  # most of the field is ordinary


# --------------------------------------------------------------- the oracle's conversions
def test_oracle_walk_is_total():
    """The walks that killed the process (exit 139) or went unreported before orc_gdm2d was made total."""
    T = W2.ramp_x()
    for start in ((3.2, 5.5), (4294967295.5, 5.5), (5.5, 4294967295.5), (-1e300, 5.5), (1e300, 5.5)):
        path, st = O.gdm2d(T, start, (12.0, 10.0), 0.5)
        assert st == ERROR
    for start in ((np.inf, 5.5), (5.5, np.inf), (-np.inf, 5.5)):  # was FALLBACK with one row
        path, st = O.gdm2d(T, start, (12.0, 10.0), 0.5)
        assert st == ERROR and len(path) == 1
