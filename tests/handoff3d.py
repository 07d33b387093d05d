"""Volume builders of the 3D hand-off tests (tests/test_gpu_writeback3d.py on the GPU,
tests/test_handoff3d_cases.py on the oracle alone) and their cached oracle call.

Every hand-off volume is built so that ONE activation flag of one tile visit carries the field into
the rest of the volume: a tile walled in by +inf cells with a single open gap (fim3d.hip's six face
flags, fim2dl.hip's per-layer side flags), or two open layers joined by a single z column
(fim2dl.hip's layer groups, which see each other's values only through LDS).  A lost flag, a wrong
neighbour or a layer group that misses its z neighbour then shows in the finite mask instead of
hiding behind an alternative route of nearly the same length.

Layout as everywhere: cost[y][x][z], nodes and goals (x, y, z).
"""
import numpy as np

import oracle as O

RTOL32 = 2e-5  # tests/test_gpu_fim3d.py check, tests/test_gpu_writeback.py check_field
ATOL64 = 1e-9

# ------------------------------------------------------------------------------ tile geometry
L32_ROWS = 64   # fim2dl.hip EIK_L32_ROWS: rows of the layered solver's fp32 tile
L64_ROWS = 40   # fim2dl.hip EIK_L64_ROWS: rows of its fp64 tile
LCOLS = 64      # fim2dl.hip / fim_engine.hpp kTile: its columns, both dtypes
L32_MAX_LAYERS = 4  # eikonal_api.cpp layered_plan kmax: layers the layered solver takes in fp32
L64_MAX_LAYERS = 3  # ... and in fp64


def layered_rows(f64):
    return L64_ROWS if f64 else L32_ROWS


def tile_shape3(L):
    """(TX, TY, TZ) of the general solver for a volume of L layers: fim3d.hip fim3d_tile_shape."""
    if L <= 4:
        return 16, 16, L
    if L <= 8:
        return 16, 8, L
    return 16, 8, 8


# ------------------------------------------------------------------------------------ oracle
_oracle_cache = {}


def oracle_field(key, cost, goal):
    """O.fmm3d(cost, goal, None), non-strict, computed once per key and shared read-only."""
    if key not in _oracle_cache:
        O.set_strict(False)
        try:
            R = O.fmm3d(np.asarray(cost, np.float64), np.asarray(goal, np.int64), None)
        finally:
            O.set_strict(True)
        R.setflags(write=False)
        _oracle_cache[key] = R
    return _oracle_cache[key]


def check_field(T, R, goal, f64):
    """Masks identical, T[goal] == 0, fp64 <= 1e-9 absolute, fp32 <= 2e-5 relative."""
    assert T.shape == R.shape
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    assert T[goal[1], goal[0], goal[2]] == 0
    err = np.abs(T[fin].astype(np.float64) - R[fin])
    if f64:
        assert err.max() <= ATOL64, err.max()
    else:
        rel = err / np.maximum(np.abs(R[fin]), 1e-30)
        rel[R[fin] == 0] = err[R[fin] == 0]
        assert rel.max() <= RTOL32, rel.max()


def corners_finite(R):
    return bool(np.all(np.isfinite(R[np.ix_((0, -1), (0, -1), (0, -1))])))


def cut_cost3(shape, goal, salt=0):
    """tests/test_gpu_writeback.py cut_cost in 3D: uniform(1, 10) through float32, 5 % +inf, goal cell 1."""
    H, W, L = shape
    rng = np.random.default_rng((H * 1000 + W) * 1000 + L + 1000003 * salt)
    c = rng.uniform(1, 10, shape)
    c[rng.random(shape) < 0.05] = np.inf
    c = c.astype(np.float32).astype(np.float64)
    c[goal[1], goal[0], goal[2]] = 1.0
    return c


# ------------------------------------------------------- A. general solver: the walled-in tile
# 3 x 3 x 3 tiles of 16 x 8 x 8 (L > 8): H = 24, W = 48, L = 24.  The centre tile's one-cell shell
# is +inf, its 14 x 6 x 6 interior and everything outside it cost 1, the goal is at its centre.
SHELL_SHAPE = (24, 48, 24)
SHELL_LO = (16, 8, 8)    # the centre tile's first cell (x, y, z)
SHELL_HI = (31, 15, 15)  # ... and its last
SHELL_GOAL = (24, 12, 12)
SHELL_TILE = (1, 1, 1)   # its tile coordinates (bx, by, bz)
FACES = ("x-", "x+", "y-", "y+", "z-", "z+")  # fim3d.hip process_tile3 flag bits 0..5


def _axis_side(face):
    return "xyz".index(face[0]), face[1] == "+"


def shell_gap(face, pos):
    """(gap cell, chain) of `face`, pos in centre / edge / corner; cells are (x, y, z).

    An edge or corner cell of the shell has no interior neighbour: the chain is the shortest run of
    further shell cells linking it to the interior, stepping first one cell inwards along the face's
    own axis, so that no chain cell lies on the named face (x- corner (16, 8, 8): (17, 8, 8),
    (17, 9, 8)).  "-" faces use the low ends of the other two axes, "+" faces the high ends.
    """
    a, plus = _axis_side(face)
    b, c = [k for k in range(3) if k != a]
    p = list(SHELL_GOAL)
    p[a] = SHELL_HI[a] if plus else SHELL_LO[a]
    end = SHELL_HI if plus else SHELL_LO
    inward = -1 if plus else 1
    chain = []
    if pos in ("edge", "corner"):
        p[b] = end[b]
        if pos == "corner":
            p[c] = end[c]
        q = list(p)
        q[a] += inward
        chain.append(tuple(q))
        if pos == "corner":
            q = list(q)
            q[b] += inward
            chain.append(tuple(q))
    elif pos != "centre":
        raise ValueError(pos)
    return tuple(p), tuple(chain)


def shell_cost(gaps, fill=None):
    """The walled-in centre tile with the gaps ((face, pos), ...) opened; fill: the open cells' costs
    (default 1 everywhere)."""
    H, W, L = SHELL_SHAPE
    c = np.ones(SHELL_SHAPE) if fill is None else np.array(fill, np.float64)
    (x0, y0, z0), (x1, y1, z1) = SHELL_LO, SHELL_HI
    inner = c[y0 + 1:y1, x0 + 1:x1, z0 + 1:z1].copy()
    c[y0:y1 + 1, x0:x1 + 1, z0:z1 + 1] = np.inf
    c[y0 + 1:y1, x0 + 1:x1, z0 + 1:z1] = inner
    for face, pos in gaps:
        cell, chain = shell_gap(face, pos)
        for x, y, z in (cell,) + chain:
            c[y, x, z] = 1.0 if fill is None else fill[y, x, z]
    return c


def shell_across(face):
    """Index (slices y, x, z) of the tile across `face` of the centre tile."""
    a, plus = _axis_side(face)
    t = list(SHELL_TILE)
    t[a] += 1 if plus else -1
    tx, ty, tz = tile_shape3(SHELL_SHAPE[2])
    return (slice(t[1] * ty, (t[1] + 1) * ty), slice(t[0] * tx, (t[0] + 1) * tx), slice(t[2] * tz, (t[2] + 1) * tz))


SIX_GAPS = tuple((f, "centre") for f in FACES)
SHELL_CASES = [((f, p),) for f in FACES for p in ("centre", "edge", "corner")] + [SIX_GAPS]


def shell_id(gaps):
    return "+".join(f"{f}{p}" for f, p in gaps)


# ---- few-layer tile shapes: one tile layer (ntz = 1), so x and y faces only.  The centre tile's
# border ring is +inf in EVERY layer, the gap is one ring cell of ONE layer at the side's middle lane.
FLAT_SHAPES = ((48, 48, 3), (48, 48, 4), (24, 48, 6))  # tiles 16 x 16 x 3, 16 x 16 x 4, 16 x 8 x 6
FLAT_SIDES = ("x-", "x+", "y-", "y+")


def flat_box(shape):
    """((x0, y0), (x1, y1)) of the centre tile of a 3 x 3 x 1-tile volume."""
    tx, ty, tz = tile_shape3(shape[2])
    assert shape == (3 * ty, 3 * tx, tz)
    return (tx, ty), (2 * tx - 1, 2 * ty - 1)


def flat_goal(shape):
    (x0, y0), (x1, y1) = flat_box(shape)
    return ((x0 + x1 + 1) // 2, (y0 + y1 + 1) // 2, 0)


def flat_gap(shape, side, z):
    (x0, y0), (x1, y1) = flat_box(shape)
    xm, ym = (x0 + x1) // 2, (y0 + y1) // 2
    return {"x-": (x0, ym, z), "x+": (x1, ym, z), "y-": (xm, y0, z), "y+": (xm, y1, z)}[side]


def flat_cost(shape, gaps):
    """gaps: ((side, z), ...)"""
    c = np.ones(shape)
    (x0, y0), (x1, y1) = flat_box(shape)
    c[y0, x0:x1 + 1, :] = c[y1, x0:x1 + 1, :] = c[y0:y1 + 1, x0, :] = c[y0:y1 + 1, x1, :] = np.inf
    for side, z in gaps:
        x, y, _ = flat_gap(shape, side, z)
        c[y, x, z] = 1.0
    return c


def flat_across(shape, side):
    tx, ty, _ = tile_shape3(shape[2])
    bx, by = {"x-": (0, 1), "x+": (2, 1), "y-": (1, 0), "y+": (1, 2)}[side]
    return (slice(by * ty, (by + 1) * ty), slice(bx * tx, (bx + 1) * tx), slice(None))


FLAT_CASES = [(s, side, z) for s in FLAT_SHAPES for side in FLAT_SIDES for z in range(s[2])]


def flat_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# --------------------------------------------- B. layered solver: one cell of one layer of one side
# 3 x 3 tiles of TH x 64, NL layers: H = 3 TH, W = 192.  The centre tile's border ring (rows TH and
# 2 TH - 1, columns 64 and 127) is +inf in every layer, the goal at its centre in layer 0, the gap one
# ring cell of one layer.  Sides as fim2dl.hip's flag bits: N (1, row 0), S (2, row TH - 1), W (4,
# lane 0), E (8, lane 63); a lane runs along the side (column offset on N / S, row offset on W / E).
def ring_shape(th, nl):
    return (3 * th, 3 * LCOLS, nl)


def ring_goal(th, z0=0):
    return (LCOLS + LCOLS // 2, th + th // 2, z0)


def side_lanes(th, side):
    return LCOLS if side in "NS" else th


def mid_lane(th, side):
    return 31 if side in "NS" else th // 2


def ring_gap(th, side, lane):
    """(row, col) of lane `lane` of the centre tile's side."""
    r0, r1, q0, q1 = th, 2 * th - 1, LCOLS, 2 * LCOLS - 1
    return {"N": (r0, q0 + lane), "S": (r1, q0 + lane), "W": (r0 + lane, q0), "E": (r0 + lane, q1)}[side]


def ring_cost(th, nl, gaps, pad=False):
    """gaps: ((side, lane, z), ...), z among the nl solved layers; pad: an all-+inf layer before and
    after them (the reference's z padding: the solver then takes layers 1 .. nl of nl + 2)."""
    c = np.ones(ring_shape(th, nl))
    r0, r1, q0, q1 = th, 2 * th - 1, LCOLS, 2 * LCOLS - 1
    c[r0, q0:q1 + 1, :] = c[r1, q0:q1 + 1, :] = c[r0:r1 + 1, q0, :] = c[r0:r1 + 1, q1, :] = np.inf
    for side, lane, z in gaps:
        r, q = ring_gap(th, side, lane)
        c[r, q, z] = 1.0
        if lane in (0, side_lanes(th, side) - 1):
            # a corner of the ring: its two neighbours inside the tile are ring cells, so the one on
            # the adjoining side is opened in the same layer (tests/test_gpu_writeback.py ring_cost)
            if side in "NS":
                c[r + (1 if side == "N" else -1), q, z] = 1.0
            else:
                c[r, q + (1 if side == "W" else -1), z] = 1.0
    if pad:
        inf = np.full(c.shape[:2] + (1,), np.inf)
        c = np.concatenate([inf, c, inf], axis=2)
    return c


def ring_across(th, side):
    """Index (rows, columns) of the tile across `side`."""
    by, bx = {"N": (0, 1), "S": (2, 1), "W": (1, 0), "E": (1, 2)}[side]
    return (slice(by * th, (by + 1) * th), slice(bx * LCOLS, (bx + 1) * LCOLS))


# (f64, NL): fp64 NL = 3 has one layer per wave group, fp32 groups {0, 1} and {2[, 3]}; NL = 1 is the
# one-group kernel
RING_LAYERS = ((False, 1), (False, 2), (False, 3), (False, 4), (True, 1), (True, 3))


def ring_cases():
    """(f64, nl, gaps): every side x layer at the middle lane; the two corner lanes of every side in
    the last layer (fp64 NL = 3 side S, the partial row group of the 40-row tile, among them)."""
    out = []
    for f64, nl in RING_LAYERS:
        th = layered_rows(f64)
        for side in "NSWE":
            out += [(f64, nl, ((side, mid_lane(th, side), z),)) for z in range(nl)]
            out += [(f64, nl, ((side, lane, nl - 1),)) for lane in (0, side_lanes(th, side) - 1)]
    return out


def ring_pad_cases():
    """One side per layer with the two pad layers added."""
    out = []
    for f64, nl in ((False, 3), (False, 4), (True, 3)):
        th = layered_rows(f64)
        out += [(f64, nl, (("NSWE"[z % 4], mid_lane(th, "NSWE"[z % 4]), z),)) for z in range(nl)]
    return out


def four_gaps(f64):
    """(nl, gaps): one gap per side, each in another layer where the layer count allows."""
    th = layered_rows(f64)
    nl = L64_MAX_LAYERS if f64 else L32_MAX_LAYERS
    return nl, tuple((s, mid_lane(th, s), k % nl) for k, s in enumerate("NSWE"))


def ring_id(v):
    if isinstance(v, tuple):
        return "+".join(f"{s}{lane}z{z}" for s, lane, z in v)
    if isinstance(v, bool):
        return "f64" if v else "f32"
    return f"nl{v}"


# ---------------------------------------------------- the goal's own hand-off (every solver)
# The goal is never lowered, so no write-back flags a side for it: T = 0 normally crosses a tile side
# through an in-tile neighbour of the goal.  Here the goal sits on a tile side / face and every
# neighbour of it is +inf but the one across that side: only the seeding can hand the goal over.
STEPS = {"x-": (-1, 0, 0), "x+": (1, 0, 0), "y-": (0, -1, 0), "y+": (0, 1, 0), "z-": (0, 0, -1), "z+": (0, 0, 1)}


def lone_exit_cost(shape, goal, face):
    """Unit cost; the goal's neighbours are +inf except the one across `face`."""
    H, W, L = shape
    c = np.ones(shape)
    for f, (dx, dy, dz) in STEPS.items():
        x, y, z = goal[0] + dx, goal[1] + dy, goal[2] + dz
        if f != face and 0 <= x < W and 0 <= y < H and 0 <= z < L:
            c[y, x, z] = np.inf
    return c


def lone_exit_cell(goal, face):
    return tuple(g + d for g, d in zip(goal, STEPS[face]))


LONE3_SHAPE = (16, 32, 16)  # 2 x 2 x 2 tiles of 16 x 8 x 8


def lone3_goal(face):
    """The first cell of the last tile for a "-" face, the last cell of the first tile for a "+" face."""
    tx, ty, tz = tile_shape3(LONE3_SHAPE[2])
    return (tx - 1, ty - 1, tz - 1) if face[1] == "+" else (tx, ty, tz)


LONE_SIDES = {"N": "y-", "S": "y+", "W": "x-", "E": "x+"}  # a layered / 2D tile's sides as faces


def lone2_shape(th, nl):
    return (2 * th, 2 * LCOLS, nl)  # 2 x 2 tiles of th rows


def lone2_goal(th, side):
    return (LCOLS - 1, th - 1, 0) if side in "SE" else (LCOLS, th, 0)


# ------------------------------------------------ C. z pinholes: two open layers, one z column
PIN_GOAL = (3, 2, 0)


def pinhole_cost(shape, pin):
    """Layers 0 and NL - 1 open (uniform(1, 4) through float32), the layers between +inf except the
    column pin = (px, py) at cost 1."""
    H, W, nl = shape
    assert nl >= 3
    rng = np.random.default_rng(H * 1000 + W + 7 * nl)
    c = rng.uniform(1, 4, shape).astype(np.float32).astype(np.float64)
    c[:, :, 1:nl - 1] = np.inf
    c[pin[1], pin[0], :] = 1.0
    c[PIN_GOAL[1], PIN_GOAL[0], PIN_GOAL[2]] = 1.0
    return c


def pinhole_cases(th):
    """(name, (H, W), (px, py)) for tiles of th rows."""
    return [
        ("interior", (2 * th, 128), (64 + 37, th + 17)),
        ("lane0row0", (2 * th, 128), (64, th)),
        ("lastrow1", (3 * th, 128), (30, th - 1)),
        ("lastrow2", (3 * th, 128), (64 + 30, 2 * th - 1)),
        ("cut_corner", (2 * th + 1, 129), (128, 2 * th)),
        ("cut_row", (2 * th + 1, 129), (70, 2 * th)),
        ("cut_col", (2 * th + 1, 129), (128, th + 5)),
    ]


# (f64, NL): NL = 4 in fp64 is past the layered solver's 3 layers and goes to fim3d.hip
PIN_LAYERS = ((False, 3), (True, 3), (False, 4), (True, 4))
PIN_CASES = [(f64, nl, name, hw + (nl,), pin) for f64, nl in PIN_LAYERS for name, hw, pin in pinhole_cases(layered_rows(f64))]
