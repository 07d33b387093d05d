"""The cases of tests/seeds_layered_cases.py on the numpy specification alone (no GPU): each volume has the
property its GPU test relies on -- which seeds are dominated, where the tiles' sides lie, which layers are
padding, which solver the routing rule must pick."""
import numpy as np
import pytest

import handoff3d as HO
import seeds_layered_cases as SC
from seeds3d_np import undominated3

F64 = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])


def exact32(t0):
    return all(float(np.float32(v)) == v for v in t0)


@F64
def test_corners(f64):
    cost, seeds, t0, R = SC.case("corners", f64)
    th = HO.layered_rows(f64)
    H, W, L = cost.shape
    assert (H, W, L) == (131, 133, 3) and th == (40 if f64 else 64)
    # 3 x 3 tiles in fp32 and 4 x 3 in fp64, the last row and column of tiles cut
    assert (-(-H // th), -(-W // HO.LCOLS)) == ((4, 3) if f64 else (3, 3)) and H % th and W % HO.LCOLS
    (x0, y0, _), (x1, y1, _) = seeds[0], seeds[1]
    assert (x0 % 64, y0 % th) == (63, th - 1) and (x1 % 64, y1 % th) == (0, 0)  # last cell / first cell ...
    assert (x1 // 64, y1 // th) == (x0 // 64 + 1, y0 // th + 1)                 # ... of the diagonal neighbour
    assert seeds[4] == (W - 1, H - 1, 2) and {z for _, _, z in seeds} == {0, 1, 2}
    assert all(cost[y, x, z] == 1.0 for x, y, z in seeds)
    assert exact32(t0)
    assert undominated3(R, seeds, t0) == SC.CORNERS_UNDOMINATED == [True, True, True, False, True]
    share = np.isfinite(R).mean()
    print(f"finite share {share:.3f}")
    assert 0.94 < share < 0.96
    assert np.array_equal(np.isfinite(R), np.isfinite(cost))  # 5 % walls cut nothing off in three layers
    assert SC.expect_layered("corners", f64) == (1, 0, 3)


@F64
def test_padded(f64):
    cost, seeds, t0, R = SC.case("padded", f64)
    assert cost.shape == (131, 133, 5)
    assert np.isinf(cost[:, :, 0]).all() and np.isinf(cost[:, :, 4]).all()
    assert np.isinf(R[:, :, 0]).all() and np.isinf(R[:, :, 4]).all()
    assert any(undominated3(R, seeds, t0)) and exact32(t0)
    # the padding changes nothing between its layers
    assert np.array_equal(R[:, :, 1:4], SC.case("corners", f64)[3])
    assert SC.expect_layered("padded", f64) == (1, 1, 3)


@F64
def test_pad_seed(f64):
    cost, seeds, t0, R = SC.case("pad_seed", f64)
    x, y, z = SC.PAD_SEED
    assert seeds[-1] == SC.PAD_SEED and z == 0 and np.isinf(cost[:, :, 0]).all() and cost[y, x, 1] == 1.0
    und = undominated3(R, seeds, t0)
    assert und[-1] and R[y, x, 0] == SC.PAD_SEED_T0 and exact32(t0)
    # the padding seed feeds its z neighbour, which the waves of the seeds in the solved layers reach far later
    assert R[y, x, 1] == SC.PAD_SEED_T0 + 1.0 < SC.case("padded", f64)[3][y, x, 1]
    assert np.isinf(np.delete(R[:, :, 0].ravel(), y * cost.shape[1] + x)).all()
    assert SC.expect_layered("pad_seed", f64) == (0, 0, 0)


@F64
def test_inf_seed(f64):
    cost, seeds, t0, R = SC.case("inf_seed", f64)
    (x, y, z), (nx, ny, nz) = SC.INF_SEED, SC.INF_NEXT
    assert seeds[1] == SC.INF_SEED and np.isinf(cost[y, x, z]) and cost[ny, nx, nz] == 1.0
    assert R[y, x, z] == 2.0 and R[ny, nx, nz] == 3.0  # it keeps its t0 and feeds the open neighbour
    assert undominated3(R, seeds, t0) == [True, True] and exact32(t0)
    assert SC.expect_layered("inf_seed", f64) == (1, 0, 3)


@F64
def test_column(f64):
    cost, seeds, t0, R = SC.case("column", f64)
    x, y = SC.COLUMN
    assert seeds == [(x, y, 0), (x, y, 2)] and np.isinf(cost[y, x, 1]) and np.isinf(R[y, x, 1])
    assert undominated3(R, seeds, t0) == [True, True] and t0[0] != t0[1] and exact32(t0)
    # both seeds matter: each owns cells the other's wave alone would reach later
    from seeds3d_np import seeded_reference3
    only0 = seeded_reference3(cost, seeds[:1], t0[:1])
    only1 = seeded_reference3(cost, seeds[1:], t0[1:])
    fin = np.isfinite(R)
    assert (R[fin] < only0[fin]).any() and (R[fin] < only1[fin]).any()
    assert SC.expect_layered("column", f64) == (1, 0, 3)


@F64
def test_pair(f64):
    cost, seeds, t0, R = SC.case("pair", f64)
    x, y, z = seeds[0]
    assert seeds[0] == seeds[1] and R[y, x, z] == 3.0 and undominated3(R, seeds, t0) == [False, True] and exact32(t0)


@F64
@pytest.mark.parametrize("name", list(SC.TINY))
def test_tiny(name, f64):
    cost, seeds, t0, R = SC.case(name, f64)
    H, W, L = cost.shape
    assert any(undominated3(R, seeds, t0)) and exact32(t0) and np.isfinite(R).any()
    if name == "tiny20x30x3":
        assert H <= HO.L64_ROWS and W <= HO.LCOLS  # one tile in either dtype
        assert SC.expect_layered(name, f64) == (1, 0, 3)
    if name == "tiny20x65x3":
        assert W == HO.LCOLS + 1 and seeds[0][0] == HO.LCOLS  # the cut tile is one cell wide and holds a seed
        assert SC.expect_layered(name, f64) == (1, 0, 3)
    if name == "open4":
        assert L == 4 and np.isfinite(cost[:, :, 0]).any() and np.isfinite(cost[:, :, 3]).any()
        # four open layers: fp32 takes them, fp64 (three at most, no padding to drop) falls back
        assert SC.expect_layered(name, f64) == ((0, 0, 0) if f64 else (1, 0, 4))
