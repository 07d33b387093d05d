"""The cost diff's rule on the CPU: tests/cost_diff_np.py's restatement on seeded pairs
of rasters -- every changed cell is covered, no LOWERED rectangle holds a raised cell, the count stays
within the cap, blocks are powers of two and come out in (block row, block column) order -- and, with
tests/test_replan_rule.py's closure and the oracle, the rectangles and kinds it emits are enough for the
incremental re-solve: the cone of the ANY rectangles set to +inf relaxes to the oracle's field of the new
cost (masks equal, values within 1e-9: that file's bound and method).
"""
import numpy as np
import pytest

import cost_diff_np as D
from test_replan_rule import closure, jacobi, oracle_field, rect_mask

SHAPES = [(190, 170), (1, 200), (64, 64), (65, 129)]
SHAPES += [tuple(int(v) for v in np.random.default_rng(s).integers(60, 201, 2)) for s in (21, 22)]
CHANGES = ["raise_inf", "halve", "mixed_tile", "corner", "inf_to_finite", "signed_zero", "equal"]
CAPS = [1, 2, 5, 1024]


def block(shape, rng, lo=3, hi=40):
    H, W = shape
    h, w = min(H, int(rng.integers(lo, hi))), min(W, int(rng.integers(lo, hi)))
    y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    return slice(y0, y0 + h), slice(x0, x0 + w)


def make_pair(shape, change, seed):
    """(old, new, goal): U(1, 10) costs, the goal's own cost equal in both"""
    rng = np.random.default_rng(seed)
    H, W = shape
    old = rng.uniform(1, 10, shape)
    goal = (W // 3, H // 2)
    b = block(shape, rng)
    if change == "inf_to_finite":
        old[b] = np.inf
    if change == "signed_zero":
        old[b] = 0.0
    new = old.copy()
    if change == "raise_inf":
        new[b] = np.inf
        new[block(shape, rng)] = np.inf
    elif change == "halve":
        new[b] *= 0.5
    elif change == "mixed_tile":  # one raised and one lowered cell in the first tile
        new[0, 0] = old[0, 0] + 1.0
        new[min(H - 1, 40), min(W - 1, 50)] *= 0.5
    elif change == "corner":  # both sides of the tile corner (64, 64), or of the edge the shape has
        new[60:68, 60:68] = np.inf
        new[max(0, min(H, 64) - 2):min(H, 66), 70:75] *= 0.5
    elif change == "inf_to_finite":
        new[b] = 2.0
    elif change == "signed_zero":
        new[b] = -0.0
    new[goal[1], goal[0]] = old[goal[1], goal[0]]
    return old, new, goal


CASES = [(s, c) for s in SHAPES for c in CHANGES]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape,change", CASES)
def test_rectangles_cover_the_change(shape, change, cap):
    old, new, goal = make_pair(shape, change, 100 * SHAPES.index(shape) + CHANGES.index(change))
    changed, raised, invalid = D.cell_masks(old, new)
    rects, kinds, info = D.cost_diff(old, new, cap)
    assert not invalid.any() and info["cells_invalid"] == 0
    assert info["cells_changed"] == int(changed.sum()) and info["cells_raised"] == int(raised.sum())
    if change in ("signed_zero", "equal"):
        assert not changed.any() and rects == [] and kinds == [] and info["block_side"] == 0 and info["tiles_changed"] == 0
        return
    assert changed.any()
    assert 0 < len(rects) <= cap and len(kinds) == len(rects)
    side = info["block_side"]
    assert side >= 1 and side & (side - 1) == 0
    assert not (changed & ~rect_mask(shape, rects)).any(), "a changed cell is not covered"
    lowered = [r for r, k in zip(rects, kinds) if k == D.LOWERED]
    assert not (raised & rect_mask(shape, lowered)).any(), "a LOWERED rectangle holds a raised cell"
    assert set(kinds) <= {D.ANY, D.LOWERED}
    # every rectangle lies in one block of side x side tiles; the blocks ascend by (row, column)
    span = side * D.TILE
    keys = []
    for x0, y0, x1, y1 in rects:
        assert 0 <= x0 < x1 <= shape[1] and 0 <= y0 < y1 <= shape[0]
        assert x0 // span == (x1 - 1) // span and y0 // span == (y1 - 1) // span
        keys.append((y0 // span, x0 // span))
    assert keys == sorted(set(keys))
    if side > 1:  # coarsened only because the finer blocks were too many
        assert len(D.rects_from_records(D.tile_records(old, new), (shape[1] + 63) // 64, 1 << 30)[0]) > cap
    if change == "halve":
        assert all(k == D.LOWERED for k in kinds)
    if change == "mixed_tile":
        assert kinds[0] == D.ANY  # the first tile holds both


def test_kinds_of_special_values():
    old = np.array([[1.0, np.inf, 0.0, 2.0, np.inf, 3.0, 5.0]])
    new = np.array([[np.inf, 1.0, -0.0, np.nan, np.inf, -1.0, 5.0]])
    changed, raised, invalid = D.cell_masks(old, new)
    assert changed.tolist() == [[True, True, False, True, False, True, False]]
    assert raised.tolist() == [[True, False, False, False, False, False, False]]  # finite -> inf raised, inf -> finite lowered
    assert invalid.tolist() == [[False, False, False, True, False, True, False]]
    assert D.cell_masks(np.array([[np.nan]]), np.array([[np.nan]]))[0].all()  # an invalid cell is changed


def test_coarsening_unites_blocks_aligned_to_the_origin():
    old = np.ones((200, 300))
    new = old.copy()
    new[10, 10] = 2.0     # tile (0, 0) raised
    new[70, 70] = 0.5     # tile (1, 1) lowered: same 2 x 2 block
    new[130, 250] = 0.5   # tile (2, 3) lowered: block (1, 1) of 2 x 2
    r1, k1, i1 = D.cost_diff(old, new, 1024)
    assert r1 == [(10, 10, 11, 11), (70, 70, 71, 71), (250, 130, 251, 131)] and k1 == [0, 1, 1] and i1["block_side"] == 1
    r2, k2, i2 = D.cost_diff(old, new, 2)
    assert r2 == [(10, 10, 71, 71), (250, 130, 251, 131)] and k2 == [0, 1] and i2["block_side"] == 2
    r3, k3, i3 = D.cost_diff(old, new, 1)
    assert r3 == [(10, 10, 251, 131)] and k3 == [0] and i3["block_side"] == 4
    assert i1["tiles_changed"] == i3["tiles_changed"] == 3 and i3["cells_changed"] == 3 and i3["cells_raised"] == 1


ORACLE_CHANGES = ["raise_inf", "halve", "mixed_tile", "corner", "inf_to_finite"]


@pytest.mark.parametrize("cap", [2, 1024])
@pytest.mark.parametrize("shape", SHAPES[:4])
@pytest.mark.parametrize("change", ORACLE_CHANGES)
def test_cone_of_the_emitted_rectangles_relaxes_to_the_new_field(change, shape, cap):
    old, new, goal = make_pair(shape, change, 100 * SHAPES.index(shape) + CHANGES.index(change))
    rects, kinds, _ = D.cost_diff(old, new, cap)
    T_old = oracle_field(old, goal)
    R = oracle_field(new, goal)
    any_rects = [r for r, k in zip(rects, kinds) if k == D.ANY]
    cone = closure(T_old, rect_mask(shape, any_rects), goal)
    T = jacobi(np.where(cone, np.inf, T_old), new)
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(T), fin), "reachability mask differs"
    assert T[goal[1], goal[0]] == 0
    if fin.any():
        assert np.abs(T[fin] - R[fin]).max() <= 1e-9
