"""Goal sets on the layered 3D solver (EIK_OPT_SEEDS_LAYERED): the volumes and seed lists
of tests/test_gpu_seeds_layered.py (GPU) and tests/test_seeds_layered_cases.py (their properties on the
numpy specification alone), and the cached reference of each.

The layered solver's tiles are 64 columns of th rows, th = 64 in fp32 and 40 in fp64 (handoff3d.layered_rows),
so a case that places seeds against tile sides is built per dtype: every builder takes f64.  The expected
field is tests/seeds3d_np.seeded_reference3 -- the same specification as for the general solver: which
solver runs must not show in the field.

Layout as everywhere: cost[y][x][z], nodes and seeds (x, y, z).
"""
import functools

import numpy as np

import handoff3d as HO
from seeds3d_np import seeded_reference3

# ------------------------------------------------------------------------------------ corners
# 131 x 133 x 3: 3 x 3 fp32 tiles and 4 x 3 fp64 tiles, cut tiles on both far sides (131 = 2 x 64 + 3 =
# 3 x 40 + 11, 133 = 2 x 64 + 5).
CORNERS_SHAPE = (131, 133, 3)
CORNERS_T0 = [3.0, 0.0, 12.5, 1e4, 40.0]
CORNERS_UNDOMINATED = [True, True, True, False, True]


def corners_seeds(f64):
    """the last cell of a tile in layer 0; the first cell of its diagonal neighbour in layer 2; an interior
    cell; a cell whose 1e4 another wave undercuts; the volume's last cell, in a tile cut on both sides"""
    th = HO.layered_rows(f64)
    H, W, _ = CORNERS_SHAPE
    return [(HO.LCOLS - 1, th - 1, 0), (HO.LCOLS, th, 2), (5, 5, 1), (70, th + 3, 1), (W - 1, H - 1, 2)]


def _open(cost, seeds):
    for x, y, z in seeds:
        cost[y, x, z] = 1.0
    return cost


def corners(f64):
    seeds = corners_seeds(f64)
    return _open(HO.cut_cost3(CORNERS_SHAPE, seeds[0], salt=3), seeds), seeds, list(CORNERS_T0)


def _pad(cost):
    """an all-+inf layer before and after (the reference's z padding: the layered solver then takes the
    layers between)"""
    inf = np.full(cost.shape[:2] + (1,), np.inf)
    return np.concatenate([inf, cost, inf], axis=2)


def padded(f64):
    """corners between two all-+inf layers, every seed one layer up: layers 1 .. 3 of 5 are solved"""
    cost, seeds, t0 = corners(f64)
    return _pad(cost), [(x, y, z + 1) for x, y, z in seeds], t0


# a seed IN the padding: cell (100, 20, 0), above the open cell (100, 20, 1) of cost 1.  The padding cell's
# cost is +inf, so nothing lowers its 0.5, and the specification hands 0.5 + 1 down to layer 1 -- far below
# what the other seeds' waves bring there.  The layered solver never reads layer 0: this list must fall back.
PAD_SEED, PAD_SEED_T0 = (100, 20, 0), 0.5


def pad_seed(f64):
    cost, seeds, t0 = padded(f64)
    x, y, z = PAD_SEED
    cost[y, x, z + 1] = 1.0
    return cost, seeds + [PAD_SEED], t0 + [PAD_SEED_T0]


# ------------------------------------------------------------------------------ the small cases
def small_shape(f64):
    """2 x 2 tiles, the far ones cut"""
    return (HO.layered_rows(f64) + 9, HO.LCOLS + 6, 3)


# a seed on a +inf cell of a SOLVED layer, its x+1 neighbour open at cost 1: the seed keeps its 2 and the
# neighbour holds 3 (the first seed's wave is tens of cells of cost >= 1 away)
INF_SEED, INF_NEXT = (40, 30, 1), (41, 30, 1)


def inf_seed(f64):
    shape = small_shape(f64)
    seeds = [(3, 3, 0), INF_SEED]
    cost = _open(HO.cut_cost3(shape, seeds[0], salt=5), seeds[:1])
    cost[INF_SEED[1], INF_SEED[0], INF_SEED[2]] = np.inf
    cost[INF_NEXT[1], INF_NEXT[0], INF_NEXT[2]] = 1.0
    return cost, seeds, [0.0, 2.0]


# seeds in layers 0 and 2 of one column whose layer-1 cell is +inf: two layer groups of the kernel, each with
# a seed of its own, that see each other only through LDS.  0 and 0.75: no tie anywhere between the waves.
COLUMN = (20, 17)


def column(f64):
    shape = small_shape(f64)
    x, y = COLUMN
    seeds = [(x, y, 0), (x, y, 2)]
    cost = _open(HO.cut_cost3(shape, seeds[0], salt=6), seeds)
    cost[y, x, 1] = np.inf
    return cost, seeds, [0.0, 0.75]


def pair(f64):
    """two seeds on one cell at 7 and 3: the lower holds"""
    shape = small_shape(f64)
    seeds = [(20, 9, 1), (20, 9, 1)]
    return _open(HO.cut_cost3(shape, seeds[0], salt=7), seeds), seeds, [7.0, 3.0]


def _tiny(shape, seeds, t0, salt):
    return lambda f64: (_open(HO.cut_cost3(shape, seeds[0], salt=salt), seeds), list(seeds), list(t0))


# one tile; a cut tile ONE cell wide with a seed in it (x = 64: the seeding alone activates that tile's
# west neighbour); four open layers: fp32 the layered solver's (nl = 4), fp64 past its three -- the general solver
TINY = {
    "tiny20x30x3": _tiny((20, 30, 3), [(4, 4, 0), (25, 15, 2)], [0.0, 1.5], 8),
    "tiny20x65x3": _tiny((20, 65, 3), [(64, 10, 1), (3, 3, 2)], [0.0, 2.5], 9),
    "open4": _tiny((20, 30, 4), [(4, 4, 0), (25, 15, 3)], [0.0, 1.5], 10),
}

CASES = dict(corners=corners, padded=padded, pad_seed=pad_seed, inf_seed=inf_seed, column=column, pair=pair, **TINY)


def expect_layered(name, f64):
    """(layered, z0, nl) that eik_fim3d_last_solver must report for the case with the option on: the rule of
    eikonal_api.cpp's layered_plan (fp32 <= 4 layers, fp64 <= 3, or two more when the outer two are all
    +inf) and every seed's z among the solved layers"""
    cost, seeds, _ = CASES[name](f64)
    L = cost.shape[2]
    kmax = HO.L64_MAX_LAYERS if f64 else HO.L32_MAX_LAYERS
    if L <= kmax:
        z0, nl = 0, L
    elif L <= kmax + 2 and np.isinf(cost[:, :, 0]).all() and np.isinf(cost[:, :, -1]).all():
        z0, nl = 1, L - 2
    else:
        return 0, 0, 0
    if not all(z0 <= z < z0 + nl for _, _, z in seeds):
        return 0, 0, 0
    return 1, z0, nl


@functools.lru_cache(maxsize=None)
def case(name, f64):
    """(cost, seeds, t0, R): built and solved on the specification once, shared read-only"""
    cost, seeds, t0 = CASES[name](bool(f64))
    R = seeded_reference3(cost, seeds, t0)
    cost.setflags(write=False)
    R.setflags(write=False)
    return cost, seeds, t0, R
