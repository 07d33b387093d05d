"""Crafted volumes for the 3D path walker (gdm3d_kernel in csrc/gdm.hip), one per branch of
FastMarching3D.getPathGDM (:198-271) and of the kernel's own machinery: the 256-point ring, the
integer-descent run loop and its exits, face nodes (Python's negative-index wrap at low faces,
IndexError at high faces), the normalised step, walks that leave the volume and non-finite
coordinates.  tests/test_walk3d_cases.py checks on the oracle alone (through its event counts) that
every case takes the branch it is named for; tests/test_gpu_walk3d.py runs them on the GPU.

A case is (T, start, end, tau, cap): T[y][x][z] float64, start / end (x, y, z), cap the point budget
of the output.  CASES maps a name to its builder; case(name) builds it once and shares it read-only;
reference(name, f32) is the oracle's walk on T (or on T rounded to float32), computed once.
"""
import numpy as np

import oracle as O

NAN, INF = float("nan"), float("inf")
RING = 256          # gdm.hip kRing
SHAPE = (10, 12, 9)  # the small volume most cases use (H, W, L)


def full_cap(tau):
    return int(round(15000 / tau)) + 4


def _solve(cost, goal):
    O.set_strict(False)
    try:
        return O.fmm3d(np.asarray(cost, np.float64), np.asarray(goal, np.int64), None)
    finally:
        O.set_strict(True)


def _grid(shape=SHAPE):
    y, x, z = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return x, y, z


# ---------------------------------------------------------------- back-track below the ring
def wall_field():
    """14 x 30 x 10, unit cost, a wall at x = 12 with a 2 x 2 gap (y 10-11, z 4-5), goal (4, 7, 5)."""
    cost = np.ones((14, 30, 10))
    cost[:, 12, :] = INF
    cost[10:12, 12, 4:6] = 1.0
    return _solve(cost, (4, 7, 5))


def _backtrack(start, tau):
    return lambda: (wall_field(), start, (4.0, 7.0, 5.0), tau, 1 << 17)


# ---------------------------------------------------------------- integer-descent run loop
def corridor_cells(side):
    """The serpentine of layer 2: rows 1, 3, ... of x = 1 .. side - 2, joined at alternating ends."""
    cells = []
    rows = list(range(1, side - 1, 2))
    for r, y in enumerate(rows):
        xs = range(1, side - 1) if r % 2 == 0 else range(side - 2, 0, -1)
        cells += [(x, y) for x in xs]
        if y != rows[-1]:
            cells.append((cells[-1][0], y + 1))
    return cells


def corridor_field(side):
    """side x side x 5: T = index along the corridor in layer 2, +inf elsewhere."""
    T = np.full((side, side, 5), INF)
    cells = corridor_cells(side)
    xs, ys = np.array(cells).T
    T[ys, xs, 2] = np.arange(len(cells), dtype=np.float64)
    return T, cells


def _corridor(side, tau, first, last=0, cap=None):
    """Walk from corridor cell `first` (negative: from the far end) down to cell `last`."""
    def build():
        T, cells = corridor_field(side)
        (sx, sy), (ex, ey) = cells[first], cells[last]
        return T, (float(sx), float(sy), 2.0), (float(ex), float(ey), 2.0), tau, cap or full_cap(tau)
    return build


STRETCH_CAPS = (2, 3, 50, 257, 258, 400)  # 400: the 401-row walk less its `end` row

# ---------------------------------------------------------------- trilinear steps on a cone
SINK = (8.3, 4.6, 4.2)


def cone_field():
    x, y, z = _grid()
    return np.sqrt((x - SINK[0]) ** 2 + (y - SINK[1]) ** 2 + (z - SINK[2]) ** 2)


def _cone(tau):
    return lambda: (cone_field(), (2.4, 7.7, 6.3), (0.0, 8.0, 7.0), tau, full_cap(tau))


def _constant():
    return np.full(SHAPE, 3.0), (4.5, 5.5, 4.5), (0.0, 8.0, 7.0), 0.5, full_cap(0.5)


# ------------------------------------------------------------------------------------ faces
def low_face_field():
    """10 x 12 x 9, a wall at x = 2 opened at y = 8, goal (0, 1, 4) on the x = 0 face: in the strip
    x = 0, 1 every gradient sample next to the wall is non-finite, so the walk is the integer
    descent along the face and reads the neighbour x - 1 = -1, which wraps to x = W - 1."""
    cost = np.ones(SHAPE)
    cost[:, 2, :] = INF
    cost[8, 2, :] = 1.0
    return _solve(cost, (0, 1, 4))


def _low_face():
    return low_face_field(), (0.3, 7.6, 4.2), (0.0, 1.0, 4.0), 0.5, full_cap(0.5)


def _low_face_z():
    """The same volume with x and z exchanged: the face is z = 0."""
    T = np.ascontiguousarray(low_face_field().transpose(0, 2, 1))
    return T, (4.2, 7.6, 0.3), (4.0, 1.0, 0.0), 0.5, full_cap(0.5)


def _low_face_wrapped_move():
    """The wrapped plane x = W - 1 below everything: the move to x = -1 is taken."""
    T = low_face_field().copy()
    T[:, -1, :] = -1.0
    return T, (0.3, 7.6, 4.2), (0.0, 1.0, 4.0), 0.5, full_cap(0.5)


def high_face_field():
    """A wall at x = W - 3 opened at y = 8, goal (4, 8, 4): the strip x = W - 2, W - 1 behind it."""
    cost = np.ones(SHAPE)
    cost[:, SHAPE[1] - 3, :] = INF
    cost[8, SHAPE[1] - 3, :] = 1.0
    return _solve(cost, (4, 8, 4))


def _high_face(dx):
    W = SHAPE[1]
    return lambda: (high_face_field(), (W - dx, 6.0, 4.0), (4.0, 8.0, 4.0), 0.5, full_cap(0.5))


# ----------------------------------------------------------------------- leaving the volume
def _ramp(sign, start):
    def build():
        x, _, _ = _grid()
        return sign * 3.0 * x, start, (6.0, 2.0, 4.0), 0.5, full_cap(0.5)
    return build


def _flat():
    x, y, _ = _grid()
    return 1e-3 * x + 2e-3 * y, (9.5, 7.5, 4.5), (2.0, 2.0, 4.0), 0.5, full_cap(0.5)


def _thin(L):
    def build():
        x, y, z = _grid((4, 4, L))
        return x + y + z, (2.5, 2.5, 0.5 if L > 1 else 0.0), (0.0, 0.0, 0.0), 0.5, full_cap(0.5)
    return build


# ------------------------------------------------------------------------------- non-finite
def slope_field():
    x, y, z = _grid()
    return x + 0.05 * y + 0.03 * z


def _nan_start(start):
    return lambda: (slope_field(), start, (1.0, 5.0, 4.0), 0.5, full_cap(0.5))


def _inf_cell(mirror):
    """One +inf cell among the gradient's samples beside a smooth slope: a gradient of +-inf, not
    NaN, so the walk steps to x = +inf (the mirrored volume: -inf) and raises at the next point."""
    def build():
        T = slope_field().copy()
        T[5, 4, 5] = INF
        if not mirror:
            return T, (9.0, 5.0, 5.0), (1.0, 5.0, 5.0), 0.5, full_cap(0.5)
        W = SHAPE[1]
        return np.ascontiguousarray(T[:, ::-1, :]), (W - 1 - 9.0, 5.0, 5.0), (W - 1 - 1.0, 5.0, 5.0), 0.5, full_cap(0.5)
    return build


def _nan_cells(start):
    """NaN cells inside T: passed beside them the walk takes the NaN branch and goes on (a walk heading
    for them is turned aside by the descent, misses the stop radius and leaves through x = 0); a
    walk whose rint node is one of them has no lower neighbour (no comparison with NaN holds), keeps
    its NaN gradient and ends on a NaN point."""
    def build():
        T = slope_field().copy()
        T[4:6, 4, 4:6] = NAN
        return T, start, (1.0, 5.0, 4.0), 0.5, full_cap(0.5)
    return build


def _step_into_wall():
    """A step of 1.7 cells lands in a +inf wall (x = 5): the isinf loop (:217-222) pops it, the walk
    descends along the wall to the corner (6, 0, 0), where no neighbour is lower: a NaN point."""
    T = slope_field().copy()
    T[:, 5, :] = INF
    return T, (8.8, 5.3, 4.2), (1.0, 5.0, 4.0), 1.7, full_cap(1.7)


# ----------------------------------------------------------------------------------- starts
def _start(start, end=(1.0, 5.0, 4.0)):
    return lambda: (slope_field(), start, end, 0.5, full_cap(0.5))


def _start_in_inf(behind):
    """Start in a +inf region: all of it (nothing finite to fall back on), or a start whose rint node
    is +inf with no earlier point behind it."""
    def build():
        T = slope_field().copy()
        if behind:
            T[:] = INF
        else:
            T[4:8, 4:8, 3:7] = INF
        return T, (5.6, 5.4, 4.5), (1.0, 5.0, 4.0), 0.5, full_cap(0.5)
    return build


CASES = {
    "backtrack_int_start": _backtrack((22.0, 3.0, 5.0), 1 / 512),
    "backtrack_frac_start": _backtrack((22.3, 3.6, 5.2), 1 / 512),
    "backtrack_tau003": _backtrack((22.3, 3.6, 5.2), 0.003),
    "backtrack_tau0031": _backtrack((22.3, 3.6, 5.2), 0.0031),
    "run_budget_tau1": _corridor(180, 1.0, -1),
    "run_budget_tau2": _corridor(130, 2.0, -1),
    "run_stretch": _corridor(180, 1.0, 400),
    "run_full_tau05": _corridor(180, 0.5, -1),
    **{f"run_cap{c}": _corridor(180, 1.0, 400, cap=c) for c in STRETCH_CAPS},
    "cone_tau05": _cone(0.5),
    "cone_tau17": _cone(1.7),
    "constant": _constant,
    "low_face": _low_face,
    "low_face_z": _low_face_z,
    "low_face_wrapped_move": _low_face_wrapped_move,
    "high_face_error": _high_face(1.4),
    "high_face_done": _high_face(1.6),
    "leave_low": _ramp(1.0, (2.2, 5.0, 4.0)),
    "leave_high": _ramp(-1.0, (8.2, 5.0, 4.0)),
    "leave_flat": _flat,
    "leave_two_layers": _thin(2),
    "one_layer": _thin(1),
    "nan_start": _nan_start((NAN, 5.0, 4.0)),
    "nan_start_all": _nan_start((NAN, NAN, NAN)),
    "inf_cell": _inf_cell(False),
    "inf_cell_mirror": _inf_cell(True),
    "nan_cells_beside": _nan_cells((9.0, 5.2, 3.4)),
    "nan_cells_around": _nan_cells((9.0, 5.0, 5.0)),
    "nan_cells_node": _nan_cells((4.2, 4.4, 4.3)),
    "step_into_wall": _step_into_wall,
    "start_in_radius": _start((2.0, 5.5, 4.5)),
    "start_is_end": _start((1.0, 5.0, 4.0)),
    "start_out_of_range": _start((11.5, 5.0, 4.0)),
    "start_all_inf": _start_in_inf(True),
    "start_node_inf": _start_in_inf(False),
}
CAPPED = tuple(f"run_cap{c}" for c in STRETCH_CAPS)

_cases, _refs = {}, {}


def case(name):
    if name not in _cases:
        T, start, end, tau, cap = CASES[name]()
        T = np.ascontiguousarray(T, np.float64)
        T.setflags(write=False)
        _cases[name] = (T, np.array(start, np.float64), np.array(end, np.float64), float(tau), int(cap))
    return _cases[name]


def field(name, f32):
    """The case's field as the walker gets it: float64, or rounded to float32."""
    T = case(name)[0]
    with np.errstate(over="ignore"):
        return T.astype(np.float32) if f32 else T


def reference(name, f32=False):
    """(path, status, events) of the oracle on the case's field (the float32 field widened again), with
    the full budget: a capped case's expected rows are the first `cap` rows of it."""
    if (name, f32) not in _refs:
        _, start, end, tau, cap = case(name)
        room = max(cap, full_cap(tau)) if name in CAPPED else cap
        path, st, ev = O.gdm3d(field(name, f32).astype(np.float64), start, end, tau, max_out=room, events=True)
        path.setflags(write=False)
        _refs[(name, f32)] = (path, st, ev)
    return _refs[(name, f32)]
