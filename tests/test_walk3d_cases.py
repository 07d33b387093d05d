"""The constructions of tests/walk3d.py, checked on the oracle alone (no GPU): every crafted walk
still takes the branch it is named for.  The oracle's event counts (orc_gdm3d_events) say which
branches a walk took; the table below pins them with the status and the point count, and the tests
after it state, per group, the condition that makes the case what it is -- so a later edit of a
builder cannot silently turn a case into a plain walk.  The counts are the same on the field rounded
to float32 (the GPU tests' fp32 runs), which the table test checks as well."""
import numpy as np
import pytest

import oracle as O
import walk3d as W3

DONE, ERROR = O.GDM_DONE, O.GDM_ERROR

# name: (status, points, (NaN-branch entries, deepest back-track, isinf-loop pops, wrapped neighbour
# reads, normalised steps, steps)) -- the capped cases: of the walk with the full budget
EXPECT = {
    "backtrack_int_start": (0, 8007, (5, 617, 0, 0, 0, 9150)),
    "backtrack_frac_start": (0, 7517, (5, 617, 0, 0, 0, 8660)),
    "backtrack_tau003": (0, 4896, (5, 402, 0, 0, 0, 5639)),
    "backtrack_tau0031": (0, 4739, (5, 389, 0, 0, 0, 5458)),
    "run_budget_tau1": (0, 15002, (15000, 1, 0, 0, 0, 15000)),
    "run_budget_tau2": (0, 7502, (7500, 1, 0, 0, 0, 7500)),
    "run_stretch": (0, 401, (399, 1, 0, 0, 0, 399)),
    "run_full_tau05": (0, 15930, (15928, 1, 0, 0, 0, 15928)),
    "run_cap2": (0, 401, (399, 1, 0, 0, 0, 399)),
    "run_cap3": (0, 401, (399, 1, 0, 0, 0, 399)),
    "run_cap50": (0, 401, (399, 1, 0, 0, 0, 399)),
    "run_cap257": (0, 401, (399, 1, 0, 0, 0, 399)),
    "run_cap258": (0, 401, (399, 1, 0, 0, 0, 399)),
    "run_cap400": (0, 401, (399, 1, 0, 0, 0, 399)),
    "cone_tau05": (0, 30002, (0, 0, 0, 0, 3527, 30000)),
    "cone_tau17": (0, 8826, (0, 0, 0, 0, 1103, 8824)),
    "constant": (2, 2, (0, 0, 0, 0, 1, 1)),
    "low_face": (0, 8, (6, 1, 0, 6, 0, 6)),
    "low_face_z": (0, 8, (6, 1, 0, 6, 0, 6)),
    "low_face_wrapped_move": (2, 2, (1, 1, 0, 1, 0, 1)),
    "high_face_error": (2, 1, (1, 1, 0, 0, 0, 0)),
    "high_face_done": (0, 10, (6, 1, 0, 0, 0, 8)),
    "leave_low": (2, 4, (0, 0, 0, 0, 0, 3)),
    "leave_high": (2, 3, (0, 0, 0, 0, 0, 2)),
    "leave_flat": (2, 21, (0, 0, 0, 0, 20, 20)),
    "leave_two_layers": (2, 4, (0, 0, 0, 0, 0, 3)),
    "one_layer": (2, 1, (0, 0, 0, 0, 0, 0)),
    "nan_start": (2, 1, (1, 0, 0, 0, 0, 0)),
    "nan_start_all": (2, 1, (1, 0, 0, 0, 0, 0)),
    "inf_cell": (2, 14, (1, 0, 0, 0, 0, 13)),
    "inf_cell_mirror": (2, 15, (1, 0, 0, 0, 0, 14)),
    "nan_cells_beside": (0, 11, (4, 3, 0, 0, 0, 11)),
    "nan_cells_around": (2, 20, (7, 6, 0, 0, 0, 24)),
    "nan_cells_node": (2, 2, (1, 1, 0, 0, 0, 1)),
    "step_into_wall": (2, 13, (11, 2, 1, 6, 0, 13)),
    "start_in_radius": (0, 3, (0, 0, 0, 0, 0, 1)),
    "start_is_end": (0, 3, (0, 0, 0, 0, 0, 1)),
    "start_out_of_range": (2, 1, (0, 0, 0, 0, 0, 0)),
    "start_all_inf": (2, 0, (1, 1, 1, 0, 0, 0)),
    "start_node_inf": (2, 0, (1, 1, 1, 0, 0, 0)),
}


def ref(name, f32=False):
    path, st, ev = W3.reference(name, f32)
    return path, st, ev


def test_every_case_is_pinned():
    assert set(EXPECT) == set(W3.CASES)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(W3.CASES))
def test_case_events(name, f32):
    path, st, ev = ref(name, f32)
    assert (st, len(path), tuple(ev.values())) == EXPECT[name]


def exact_unit_moves(tau):
    """gdm.hip int_moves: the descent's step tau * (1 / tau) is exactly one cell."""
    return tau * (1.0 / tau) == 1.0


# ---------------------------------------------------------------- back-track below the ring
@pytest.mark.parametrize("name", ["backtrack_int_start", "backtrack_frac_start", "backtrack_tau003",
                                  "backtrack_tau0031"])
def test_backtrack_is_deeper_than_the_ring(name):
    path, st, ev = ref(name)
    assert st == DONE and ev["deepest_backtrack"] > W3.RING
    assert len(path) > 2 * W3.RING and len(path) < W3.case(name)[4]  # ends on the stop radius, not the cap
    assert np.linalg.norm(path[-2] - path[-1]) < 1.5


def test_backtrack_tau0031_moves_are_not_integers():
    """tau * (1 / tau) is exactly 1 at tau = 1/512 and at 0.003, not at 0.0031: after a descent move that
    walk is off the nodes and the kernel's run loop is never entered."""
    assert exact_unit_moves(1 / 512) and exact_unit_moves(0.003) and not exact_unit_moves(0.0031)


# ---------------------------------------------------------------- integer-descent run loop
def test_corridor_lengths():
    assert len(W3.corridor_cells(180)) == 15930 and len(W3.corridor_cells(130)) == 8255
    for side in (130, 180):
        T, cells = W3.corridor_field(side)
        c = np.array(cells)
        assert np.abs(np.diff(c, axis=0)).sum(1).tolist() == [1] * (len(cells) - 1)  # 6-connected chain
        assert c.min() >= 1 and c.max() <= side - 2  # interior nodes: the run loop's range
        assert np.isfinite(T).sum() == len(cells) and np.isinf(T[:, :, [0, 1, 3, 4]]).all()


@pytest.mark.parametrize("name,tau", [("run_budget_tau1", 1.0), ("run_budget_tau2", 2.0)])
def test_run_ends_on_the_step_budget(name, tau):
    """More corridor cells than steps: DONE by the budget, n = steps + 2, one integer move per step."""
    path, st, ev = ref(name)
    steps = int(round(15000 / tau))
    assert exact_unit_moves(tau)
    assert st == DONE and len(path) == steps + 2 and ev["steps"] == ev["nan_entries"] == steps
    assert np.linalg.norm(path[-2] - path[-1]) >= 1.5  # not the stop radius
    assert np.array_equal(path[:-1], np.rint(path[:-1]))
    assert np.abs(np.diff(path[:-1], axis=0)).sum(1).tolist() == [1.0] * steps


@pytest.mark.parametrize("name,moves", [("run_stretch", 399), ("run_full_tau05", 15928)])
def test_run_ends_on_the_stop_radius(name, moves):
    path, st, ev = ref(name)
    tau = W3.case(name)[3]
    assert exact_unit_moves(tau) and moves < int(round(15000 / tau))
    assert st == DONE and ev["steps"] == moves and len(path) == moves + 2
    assert np.linalg.norm(path[-2] - path[-1]) < 1.5


@pytest.mark.parametrize("name", W3.CAPPED)
def test_capped_stretch_has_a_prefix(name):
    """The integer walk puts every node back into its own slot, so the first cap rows of the walk
    with the full budget are what a walk with that cap holds when it runs out."""
    path, st, ev = ref(name)
    cap = W3.case(name)[4]
    assert 2 <= cap < len(path) and ev["deepest_backtrack"] == 1
    assert np.array_equal(path, W3.reference("run_stretch")[0])


# ------------------------------------------------------------- trilinear steps on the cone
@pytest.mark.parametrize("name", ["cone_tau05", "cone_tau17"])
def test_cone_runs_out_of_steps_with_normalised_steps(name):
    path, st, ev = ref(name)
    tau = W3.case(name)[3]
    steps = int(round(15000 / tau))
    assert st == DONE and ev["nan_entries"] == 0 and ev["normalised_steps"] > 0
    assert ev["steps"] == steps and len(path) == steps + 2
    if tau > 1:
        assert np.abs(np.diff(path[:-1], axis=0)).max() > 1.0  # steps over more than one cell


def test_constant_field_divides_by_zero():
    path, st, ev = ref("constant")
    assert st == ERROR and len(path) == 2 and np.isnan(path[1]).all() and ev["normalised_steps"] == 1


# ------------------------------------------------------------------------------------ faces
@pytest.mark.parametrize("name,axis", [("low_face", 0), ("low_face_z", 2)])
def test_low_face_reads_wrap(name, axis):
    path, st, ev = ref(name)
    assert st == DONE and len(path) == 8 and ev["wrapped_reads"] == 6
    assert (path[:, axis] == 0).all()


def test_low_face_wrapped_move_is_taken():
    path, st, ev = ref("low_face_wrapped_move")
    assert st == ERROR and ev["wrapped_reads"] == 1
    assert path.tolist() == [[0.0, 8.0, 4.0], [-1.0, 8.0, 4.0]]


def test_high_face():
    path, st, ev = ref("high_face_error")
    assert st == ERROR and path.tolist() == [[W3.SHAPE[1] - 1.0, 6.0, 4.0]] and ev["nan_entries"] == 1
    path, st, ev = ref("high_face_done")
    assert st == DONE and path[0].tolist() == [W3.SHAPE[1] - 2.0, 6.0, 4.0]


# ----------------------------------------------------------------------- leaving the volume
def test_leaving_walks():
    path, st, _ = ref("leave_low")
    assert st == ERROR and np.allclose(path[:, 0], [2.2, 0.7, -0.8, -2.3], atol=1e-12)
    assert -1 < path[2, 0] < 0  # a point in (-1, 0) is walked through, with a negative fraction
    path, st, _ = ref("leave_high")
    assert st == ERROR and len(path) == 3 and path[-1, 0] > W3.SHAPE[1] - 1
    path, st, ev = ref("leave_flat")
    assert st == ERROR and ev["normalised_steps"] == 20 and path[-1, 1] <= -1 and (path[:-1, :] > -1).all()
    path, st, _ = ref("leave_two_layers")
    assert st == ERROR and len(path) == 4 and path[-1, 2] <= -1 and -1 < path[-2, 2] < 0
    path, st, _ = ref("one_layer")
    assert st == ERROR and len(path) == 1


# ------------------------------------------------------------------------------- non-finite
def test_non_finite_coordinates():
    for name in ("nan_start", "nan_start_all"):
        path, st, ev = ref(name)
        assert st == ERROR and len(path) == 1 and np.isnan(path[0, 0]) and ev["nan_entries"] == 1
    path, st, ev = ref("inf_cell")
    assert st == ERROR and path[-1, 0] == np.inf and np.isfinite(path[:-1]).all() and ev["nan_entries"] == 1
    path, st, ev = ref("inf_cell_mirror")
    assert st == ERROR and path[-1, 0] == -np.inf and np.isfinite(path[:-1]).all() and ev["nan_entries"] == 1


def test_nan_cells():
    path, st, ev = ref("nan_cells_beside")
    assert st == DONE and ev["nan_entries"] > 0 and np.isfinite(path).all()
    path, st, ev = ref("nan_cells_around")
    assert st == ERROR and ev["nan_entries"] == 7 and np.isfinite(path).all() and path[-1, 0] <= -1
    path, st, ev = ref("nan_cells_node")
    assert st == ERROR and len(path) == 2 and np.isnan(path[-1]).all()
    T = W3.case("nan_cells_node")[0]
    x, y, z = (int(v) for v in path[0])
    assert np.isnan(T[y, x, z])


def test_step_into_wall_pops_in_the_isinf_loop():
    path, st, ev = ref("step_into_wall")
    assert ev["inf_pops"] == 1 and ev["wrapped_reads"] > 0
    assert st == ERROR and path[-2].tolist() == [6.0, 0.0, 0.0] and np.isnan(path[-1, 0])


# ----------------------------------------------------------------------------------- starts
def test_starts():
    for name in ("start_in_radius", "start_is_end"):
        path, st, _ = ref(name)
        assert st == DONE and len(path) == 3
    assert np.array_equal(ref("start_is_end")[0][0], ref("start_is_end")[0][2])
    path, st, _ = ref("start_out_of_range")
    assert st == ERROR and len(path) == 1
    for name in ("start_all_inf", "start_node_inf"):
        path, st, ev = ref(name)
        assert st == ERROR and len(path) == 0 and ev["inf_pops"] == 1
    T, start = W3.case("start_node_inf")[:2]
    assert np.isfinite(T).any() and np.isinf(T[tuple(int(round(v)) for v in start[[1, 0, 2]])])


# --------------------------------------------------------------- the oracle's conversions
def test_interp3_conversions_are_total():
    """np.uint32(np.fix(p)) as numpy on x86-64 has it: non-finite -> index 0 with the fraction
    computed from it (a NaN or infinite value, no error); p <= -1 -> IndexError."""
    M = W3.slope_field()
    for p in ((-1.0, 5.0, 4.0), (3.0, -1.3, 4.0), (3.0, 5.0, -1e300), (3.0, 5.0, 1e300), (2.0 ** 31, 5.0, 4.0)):
        with pytest.raises(O.RefError) as e:
            O.interp3(p, M)
        assert e.value.name == "IndexError"
    assert O.interp3((-0.5, 5.0, 4.0), M) == pytest.approx(-0.5 + 0.25 + 0.12)
    for p in ((np.nan, 5.0, 4.0), (np.inf, 5.0, 4.0), (3.0, -np.inf, 4.0)):
        assert not np.isfinite(O.interp3(p, M))
