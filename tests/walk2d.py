"""Crafted fields for the default 2D path walker (gdm2d_kernel in csrc/gdm.hip, all five loop forms),
one per branch of FastMarching.getPathGDM (:164-236), of interpolatePoint's coordinate-to-index
conversion (:306-307, the 2D table of DESIGN 3.4b) and of the kernel's own machinery: the LDS windows and
their prefetch, the fast step's walk_odd exits, the point budget.  tests/test_walk2d_cases.py checks
on the oracle alone (through its event counts) that every case takes the branch it is named for and
is well conditioned; tests/test_gpu_walk2d.py runs them on the GPU.

A case is (T, start, end, tau, cap): T[y][x] float64, start / end (x, y), cap the point budget of the
output.  CASES maps a name to its builder; case(name) builds it once and shares it read-only;
reference(name, f32) is the oracle's walk on T (or on T rounded to float32) with the reference's own
budget, computed once; expected(name, f32) is what a walker with the case's cap must return.
"""
import numpy as np

import oracle as O

NAN, INF = float("nan"), float("inf")
SHAPE = (12, 14)   # the small field most cases use (H, W)
ROOM = 1 << 15     # rows the oracle gets at most (a walk that needs more is an error of the case)
TWO31, TWO32 = 2.0 ** 31, 2.0 ** 32


def full_cap(tau):
    return int(round(15000 / tau)) + 4


def _grid(shape=SHAPE):
    y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return x, y


def _mk(field, start, end, tau=0.5, cap=None):
    return lambda: (field() if callable(field) else field, start, end, tau, cap or full_cap(tau))


# ---------------------------------------------------------------------------------- fields
def ramp_x(shape=SHAPE, sign=1.0):
    return sign * _grid(shape)[0]


def ramp_y(shape=SHAPE, sign=1.0):
    return sign * _grid(shape)[1]


def cone(shape=SHAPE, sink=(8.3, 4.6)):
    x, y = _grid(shape)
    return np.sqrt((x - sink[0]) ** 2 + (y - sink[1]) ** 2)


def crease():
    """3 |x - 6.5| + y / 100: on the line x = 6.5 the interpolated gradient is (0, 0.0067): |g| < 0.01."""
    x, y = _grid()
    return 3.0 * np.abs(x - 6.5) + 0.01 * y


def bounce(shape=SHAPE, mid=6.5):
    """|x - mid|: the walk jumps across the crease and back, tau per step, for the whole budget."""
    return np.abs(_grid(shape)[0] - mid)


def diamond():
    x, y = _grid()
    return np.abs(x - 6.5) + np.abs(y - 5.5)


def tiny_row(exp):
    """Row 0 holds 2^exp x, row 1 the constant c = 2^-10, row 2 -c, then falling: the normalised
    gradient is (2^(exp + 10), 1) on row 0 and (0, -1) on row 1, so in the cells of row 0 the
    interpolated dx is 2^(exp + 10) (1 - b) and dy = 1 - 2 b."""
    x, y = _grid()
    c = 2.0 ** -10
    T = -c * (y - 1.0)
    T[1] = c
    T[0] = 2.0 ** exp * x[0]
    return T


def underflow():
    """2^-600 (x + y): every node's |grad|^2 underflows to 0, its normalised gradient is (inf, inf)."""
    x, y = _grid()
    return 2.0 ** -600 * (x + y)


def hop_field(last_inf):
    """T = x with isolated +inf nodes (11, 5), (8, 5), (5, 5) -- a node whose four neighbours are
    finite has a finite gradient, and so have its neighbours -- and the pair (1, 5), (2, 5): walked
    along y = 5 with tau = 3 from x = 11.2, every point's rint node is +inf and the first NaN gradient
    comes at x = 2.2.  last_inf False: (11, 5) is finite, the pops end on it."""
    T = ramp_x().copy()
    for i in (1, 2, 5, 8) + ((11,) if last_inf else ()):
        T[5, i] = INF
    return T


def low_edge_field(axis, wrapped_inf):
    """T = x (axis 0) or y (axis 1) with the node (0, 5) / (5, 0) +inf: a point in the first cell has a
    NaN gradient; with a coordinate in (-1, -0.5) its rint node is -1, which Python wraps to the last
    column / row (made +inf with wrapped_inf)."""
    T = (ramp_x() if axis == 0 else ramp_y()).copy()
    if axis == 0:
        T[5, 0] = INF
        if wrapped_inf:
            T[5, -1] = INF
    else:
        T[0, 5] = INF
        if wrapped_inf:
            T[-1, 5] = INF
    return T


def nan_at(x0):
    """T = x with the node (x0, 5) +inf and its left neighbour too: the gradient at (x0, 5) is NaN."""
    T = ramp_x().copy()
    T[5, x0 - 1:x0 + 1] = INF
    return T


def gradient_field():
    """9 x 11 for computeGradient (:262-294): a smooth field with +inf cells placed so that, on each
    axis, every branch is taken -- first and last node, both neighbours +inf (-> 0), only the next one,
    only the previous one, neither -- and at (4, 4) both axes give 0, so the normalised gradient is
    0 / 0 = NaN; at (8, 7) only x gives 0, at (9, 2) only y."""
    x, y = _grid((9, 11))
    T = 1.3 * x + 0.7 * y + 0.1 * x * y
    for i, j in ((3, 4), (5, 4), (4, 3), (4, 5), (7, 7), (9, 7), (9, 1), (9, 3)):
        T[j, i] = INF
    return T


def gradient_branches(T):
    """Per node and axis (0: y, 1: x) the branch of :262-294 it takes: 0 first node, 1 last node, 2 both
    neighbours +inf, 3 only the next one, 4 only the previous one, 5 neither."""
    out = np.empty((2,) + T.shape, int)
    for ax in (0, 1):
        n = T.shape[ax]
        idx = np.arange(n).reshape((-1, 1) if ax == 0 else (1, -1)) + np.zeros(T.shape, int)
        nxt = np.isinf(np.take(T, np.minimum(np.arange(n) + 1, n - 1), axis=ax))
        prv = np.isinf(np.take(T, np.maximum(np.arange(n) - 1, 0), axis=ax))
        out[ax] = np.where(idx == 0, 0, np.where(idx == n - 1, 1, np.where(nxt & prv, 2, np.where(nxt, 3, np.where(prv, 4, 5)))))
    return out


SERP_SHAPE = (150, 230)


def serpentine():
    """150 x 230, unit cost, four 4-row walls of cost 1e4 with 26-column gaps at alternating ends, an
    +inf border, goal below the last wall: the path runs the width of the raster four times."""
    H, W = SERP_SHAPE
    cost = np.ones(SERP_SHAPE)
    for w, y0 in enumerate((28, 58, 88, 118)):
        cost[y0:y0 + 4, :] = 1e4
        if w % 2 == 0:
            cost[y0:y0 + 4, W - 28:W - 2] = 1.0
        else:
            cost[y0:y0 + 4, 2:28] = 1.0
    cost[0, :] = cost[-1, :] = cost[:, 0] = cost[:, -1] = INF
    O.set_strict(False)
    try:
        return O.fmm2d(cost, (30, 140))
    finally:
        O.set_strict(True)


SERP_START, SERP_END = (30.4, 10.3), (30.0, 140.0)

# ----------------------------------------------------------------------------------- cases
BAD_STARTS = {"nan": NAN, "pinf": INF, "ninf": -INF, "m1": -1.0, "m1eps": -1.0 + 2.0 ** -52, "two31": TWO31,
              "two32m": 4294967295.5, "two32p": TWO32 + 5.5}
SIDES = (3, 63, 64, 65, 66, 80)
LONG_CAPS = (2, 3, 50)

CASES = {
    # conversions: leaving the raster, the cells (-1, 0), starts the index type cannot hold
    "leave_x0": _mk(ramp_x, (3.2, 5.5), (12.0, 10.0)),
    "leave_y0": _mk(ramp_y, (5.5, 3.2), (12.0, 10.0)),
    "leave_xhi": _mk(lambda: ramp_x(sign=-1.0), (10.2, 5.5), (2.0, 2.0)),
    "leave_yhi": _mk(lambda: ramp_y(sign=-1.0), (5.5, 8.2), (2.0, 2.0)),
    "neg_cell_x": _mk(ramp_x, (2.2, 5.5), (-2.2, 5.5)),
    "neg_cell_y": _mk(ramp_y, (5.5, 2.2), (5.5, -2.2)),
    **{f"start_x_{k}": _mk(ramp_x, (v, 5.5), (1.0, 5.5)) for k, v in BAD_STARTS.items()},
    **{f"start_y_{k}": _mk(ramp_y, (5.5, v), (5.5, 1.0)) for k, v in BAD_STARTS.items()},
    "start_last_col": _mk(ramp_x, (13.0, 5.5), (8.0, 5.5)),
    "start_below_last_col": _mk(ramp_x, (float(np.nextafter(13.0, 0.0)), 5.5), (8.0, 5.5)),
    "start_last_row": _mk(ramp_y, (5.5, 11.0), (5.5, 6.0)),
    "start_below_last_row": _mk(ramp_y, (5.5, float(np.nextafter(11.0, 0.0))), (5.5, 6.0)),
    # step arithmetic
    "cone_tau05": _mk(cone, (2.4, 9.7), (8.0, 5.0)),
    "cone_tau17": _mk(cone, (2.4, 9.7), (8.0, 5.0), 1.7),
    "crease_unit_steps": _mk(crease, (6.5, 10.5), (6.5, 2.0)),
    "start_on_node": _mk(ramp_x, (7.0, 5.0), (2.0, 5.0)),
    "start_on_line_a0": _mk(ramp_y, (3.0, 7.25), (3.0, 2.0)),
    "start_on_line_b0": _mk(ramp_x, (7.25, 5.0), (2.0, 5.0)),
    "zero_gradient": _mk(diamond, (6.5, 5.5), (1.0, 1.0)),
    "tiny_tau_capped": _mk(ramp_x, (7.3, 5.5), (1.0, 5.5), 1e-3, 3000),
    "odd_tiny_component": _mk(lambda: tiny_row(-950), (5.5, 0.1), (5.5, -3.0)),
    "odd_tiny_norm": _mk(lambda: tiny_row(-410), (5.5, 0.5), (1.0, 0.5)),
    "odd_zero_norm": _mk(lambda: tiny_row(-950), (5.5, 0.5), (1.0, 0.5)),
    "odd_inf_gradient": _mk(underflow, (5.0, 5.0), (1.0, 1.0)),
    "inf_gradient_off_node": _mk(underflow, (5.3, 5.4), (1.0, 1.0)),
    # NaN fallback
    "constant": _mk(lambda: np.full(SHAPE, 3.0), (4.4, 5.3), (1.0, 1.0)),
    "hop_pops_to_empty": _mk(lambda: hop_field(True), (11.2, 5.0), (-8.0, 5.0), 3.0),
    "hop_pops_to_node": _mk(lambda: hop_field(False), (11.2, 5.0), (-8.0, 5.0), 3.0),
    "walk_into_nan": _mk(lambda: nan_at(3), (9.3, 5.5), (0.0, 5.5)),
    "wrap_low_x": _mk(lambda: low_edge_field(0, False), (-0.7, 5.3), (5.0, 5.0)),
    "wrap_low_y": _mk(lambda: low_edge_field(1, False), (5.3, -0.7), (5.0, 5.0)),
    "wrap_low_x_inf": _mk(lambda: low_edge_field(0, True), (-0.7, 5.3), (5.0, 5.0)),
    "wrap_low_y_inf": _mk(lambda: low_edge_field(1, True), (5.3, -0.7), (5.0, 5.0)),
    "fallback_at_cap": _mk(lambda: nan_at(3), (9.3, 5.5), (0.0, 5.5), 0.5, 12),
    "fallback_below_cap": _mk(lambda: nan_at(3), (9.3, 5.5), (0.0, 5.5), 0.5, 13),
    # stop radius and budgets
    "start_in_radius": _mk(ramp_x, (2.0, 5.5), (1.0, 5.5)),
    "start_outside_radius": _mk(ramp_x, (3.1, 5.5), (1.0, 5.5)),
    **{f"long_cap{c}": _mk(bounce, (6.3, 5.5), (1.0, 1.0), 0.5, c) for c in LONG_CAPS},
    "end_fits": _mk(ramp_x, (9.3, 5.5), (1.0, 5.5), 0.5, 16),
    "end_does_not_fit": _mk(ramp_x, (9.3, 5.5), (1.0, 5.5), 0.5, 15),
    "full_budget": _mk(bounce, (6.3, 5.5), (1.0, 1.0)),
    "full_budget_fits": _mk(bounce, (6.3, 5.5), (1.0, 1.0), 0.5, 30002),
    "full_budget_one_short": _mk(bounce, (6.3, 5.5), (1.0, 1.0), 0.5, 30001),
    # window machinery
    **{f"side_x{s}": _mk(lambda s=s: cone((12, s), (1.2, 1.3)), (s - 1.5, 9.5), (1.0, 1.0)) for s in SIDES},
    **{f"side_y{s}": _mk(lambda s=s: cone((s, 14), (1.2, 1.3)), (11.5, s - 1.5), (1.0, 1.0)) for s in SIDES},
    "windows_x": _mk(lambda: ramp_x((12, 230)), (228.3, 5.5), (1.0, 5.5)),
    "windows_y": _mk(lambda: ramp_y((230, 14)), (5.5, 228.3), (5.5, 1.0)),
    "windows_diag": _mk(lambda: ramp_x((150, 150)) + ramp_y((150, 150)), (148.3, 148.6), (1.0, 1.0)),
    "serpentine_tau05": _mk(serpentine, SERP_START, SERP_END),
    "serpentine_tau17": _mk(serpentine, SERP_START, SERP_END, 1.7),
    "tau70": _mk(lambda: bounce((12, 230), 115.5), (100.3, 5.5), (1.0, 1.0), 70.0),
}
FULL_BUDGET = ("full_budget", "tau70")  # run out of steps with the full point budget: the host entry's cases

_cases, _refs, _limited = {}, {}, {}


def case(name):
    if name not in _cases:
        build = CASES[name]
        T, start, end, tau, cap = build()
        T = np.ascontiguousarray(T, np.float64)
        T.setflags(write=False)
        _cases[name] = (T, np.array(start, np.float64), np.array(end, np.float64), float(tau), int(cap))
    return _cases[name]


def field(name, f32):
    """The case's field as the walker gets it: float64, or rounded to float32."""
    T = case(name)[0]
    with np.errstate(over="ignore", under="ignore"):
        return T.astype(np.float32) if f32 else T


def walk(name, f32=False, exact=False, max_steps=0):
    """The oracle's walk of the case (events included), uncached."""
    _, start, end, tau, _ = case(name)
    room = min(full_cap(tau), ROOM)
    return O.gdm2d(field(name, f32).astype(np.float64), start, end, tau, max_out=room, events=True, exact=exact,
                   max_steps=max_steps)


def reference(name, f32=False):
    """(path, status, events) of the oracle on the case's field with the reference's own budget."""
    if (name, f32) not in _refs:
        path, st, ev = walk(name, f32)
        path.setflags(write=False)
        _refs[(name, f32)] = (path, st, ev)
    return _refs[(name, f32)]


def expected(name, f32=False, cap=None):
    """(rows, status) a walker with the case's point budget (or `cap`) must return.  The budget is the
    project's own (the reference's gamma grows without bound): a walk takes a step only while a row
    is left for its point, so with s the steps of the unbounded walk, every exit of it that comes
    with s + 1 < cap rows is reached as it is; one that raises with exactly cap rows too; any other
    walk holds, when the budget runs out, the cap rows of the walk cut to cap - 1 steps -- status
    ERROR, n = cap, also when only `end` did not fit."""
    path, st, ev = reference(name, f32)
    cap = case(name)[4] if cap is None else cap
    s = ev["steps"]
    if s + 1 < cap or (s + 1 == cap and st == O.GDM_ERROR):
        assert ev["peak_rows"] <= cap and len(path) <= cap
        return path, st
    if (name, f32, cap) not in _limited:
        cut, cst, cev = walk(name, f32, max_steps=cap - 1)
        assert cst == O.GDM_DONE and cev["exit"] in (O.EXIT_BUDGET, O.EXIT_STOP) and len(cut) == cap + 1
        cut = cut[:cap]
        cut.setflags(write=False)
        _limited[(name, f32, cap)] = cut
    return _limited[(name, f32, cap)], O.GDM_ERROR
