"""The cost-raster builder (csrc/costmap.hip) where tests/test_gpu_costmap.py does not reach: the
dispatch branches for rows wider than 8192, radii above 250 and single-row rasters, the cost tail
(:1180-1216) through its own entry at ragged, non-square and tiny shapes, other constants than the
reference's defaults, DEMs with negative heights (the rover path's heights too: they alone see min(Z)
itself), and hole filling below one 32 x 32 tile and across its border on thin rasters.
References: oracle/costmap_oracle.py, and tests/morph_stamp.py at radius 251 (pinned to the oracle
in tests/test_costmap_oracle.py).  Rules as in test_gpu_costmap.py: masks bit-exact, costs the same
finite set and <= 1e-12 relative (the blur's summation order), normals <= 1e-12 absolute.  Every
test first asserts, on the CPU, the property of its input that makes it select what it is for."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import costmap_oracle as CO
import morph_stamp
import terrain_np

pytestmark = pytest.mark.gpu

ROW_MAX = 8192  # kEdtRowMax = kBndRowMax (csrc/costmap.hip): wider rows leave the LDS row kernels
R_BOUNDED = 250  # cm_morph: larger radii take the full EDT instead of the uint8 bounded transform


@pytest.fixture(scope="module")
def ctx():
    import eikonal

    c = eikonal.Context(0)
    yield c
    c.close()


def check_cost(cost, obst, cref, oref):
    """cost [y][x], obst uint8 from the GPU against the oracle's (cMap [x, y], obstMap float64)."""
    R = cref.T
    assert not np.isnan(R).any()
    assert np.array_equal(obst.astype(np.float64), oref)
    fin = np.isfinite(R)
    assert np.array_equal(np.isfinite(cost), fin)
    assert np.array_equal(cost[~fin], R[~fin])  # +inf where the reference has it
    if fin.any():
        assert (np.abs(cost[fin] - R[fin]) / R[fin]).max() <= 1e-12


# ---- a. disk morphology: the branches cm_morph selects by width, radius and height -------------
def sparse_mask(shape, r):
    """Seeded single pixels (dilation's input; erosion gets 1 - a): 5 or 6 at radius 251.  Narrow
    rasters keep them in the left 45 % of the columns so that the disks cannot cover the image; wide
    ones get one more whose disk ends beyond column 8192, and at small radii the two corners."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W + r)
    k = {3: 1200, 20: 50}.get(r, 5)
    xmax = W if W > ROW_MAX else int(0.45 * W)
    a = np.zeros(shape, np.uint8)
    a[rng.integers(0, H, k), rng.integers(0, xmax, k)] = 1
    if W > ROW_MAX:
        if r <= R_BOUNDED:
            a[H // 2, ROW_MAX + 58] = a[0, 0] = a[H - 1, W - 1] = 1
        else:
            a[H // 2, ROW_MAX - 200] = 1
    return a


MORPH_EDGE_CASES = [((40, 8300), 3), ((24, 8300), 20), ((300, 560), 251), ((40, 8300), 251), ((1, 8300), 251),
                    ((1, 700), 251), ((2, 700), 251)]


@functools.lru_cache(maxsize=None)
def morph_reference(shape, r):
    """(a, dilate(a), erode(1 - a)) once per case, for both erode values."""
    a = sparse_mask(shape, r)
    if r > R_BOUNDED:
        dil, ero = morph_stamp.dilate(a, r), morph_stamp.erode(1 - a, r)
    else:
        se = CO.structural_disk(r)
        dil, ero = CO.dilate(a, se), CO.erode(1 - a, se)
    for m in (a, dil, ero):
        m.setflags(write=False)
    return a, dil, ero


@pytest.mark.parametrize("shape,r", MORPH_EDGE_CASES, ids=[f"{s[0]}x{s[1]}-r{r}" for s, r in MORPH_EDGE_CASES])
@pytest.mark.parametrize("erode", [False, True])
def test_disk_morphology_branches(ctx, shape, r, erode):
    """cm_morph's untested dispatch: W > 8192 with r <= 250 -> cm_bnd_rows_wide_kernel; r > 250 -> the
    full cm_edt (val = 1 dilating, val = 0 eroding) and cm_morph_kernel, with segmented columns (H >= 2)
    or cm_edt_cols_kernel (H = 1), LDS rows (W <= 8192) or the envelope cm_edt_rows_kernel (W > 8192)."""
    a, dil, ero = morph_reference(shape, r)
    share = dil.mean()
    print(f"dilated share {share:.4f}, set pixels {int(a.sum())}")
    assert 0.05 < share < 0.98  # neither an all-zero nor an all-one output passes
    assert np.array_equal(ero, 1 - dil)  # the two references agree (symmetric disk)
    if shape[1] > ROW_MAX:
        assert dil[:, ROW_MAX:].any() and not dil[:, ROW_MAX:].all()  # both values beyond column 8192
    got = ctx.disk_morph(1 - a if erode else a, r, erode)
    ref = ero if erode else dil
    assert np.array_equal(got, ref), (shape, r, erode, int((got != ref).sum()))


@pytest.mark.parametrize("shape", [(70, 130), (2, 8300), (1, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("r", [10, 251])
@pytest.mark.parametrize("erode", [False, True])
def test_disk_morphology_featureless(ctx, shape, r, erode):
    """No feature anywhere (the transforms' "none" values: r + 1 bounded, INT32_MAX in both row passes
    of the full EDT): dilating the empty mask and eroding the full one return the input."""
    im = np.full(shape, 1 if erode else 0, np.uint8)
    assert not (im != im[0, 0]).any()
    assert np.array_equal(ctx.disk_morph(im, r, erode), im)


# ---- b. the cost tail (:1180-1216) through eik_cost_tail_u8 -------------------------------------
def params(**kw):
    from eikonal import _lib as L

    d = dict(slope_max=0.20, diagonal=0.9, expansion=1.0, gradient=10.0, high=300.0)
    d.update(kw)
    return L.CostmapParams(d["slope_max"], d["diagonal"], d["expansion"], d["gradient"], d["high"])


def blocks_mask(shape, blocks):
    m = np.zeros(shape, np.uint8)
    for y0, y1, x0, x1 in blocks:
        m[y0:y1, x0:x1] = 1
    return m


def rocks_mask(H, W):
    """25 rocks of 5 x 5 in the left third: the far right is farther from any obstacle than every
    sample of the ramp's 16-pixel grid, and most pixels are provably below the sample maximum."""
    rng = np.random.default_rng(3)
    m = np.zeros((H, W), np.uint8)
    for cy, cx in zip(rng.integers(5, H - 5, 25), rng.integers(5, W // 3, 25)):
        m[cy - 2:cy + 3, cx - 2:cx + 3] = 1
    return m


def ramp_scan_stats(m):
    """What cm_edt_sample_kernel / cm_edt_rows_ramp_kernel decide on the mask m (border set as :1180-1183),
    restated from scipy's transform: (share of pixels whose scan is capped at r, max D, sample max)."""
    b = np.array(m, dtype=np.uint8)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = 1
    D = np.rint(ndimage.distance_transform_edt(b == 0) ** 2).astype(np.int64)
    H, W = D.shape
    ds = D[::16, ::16]
    ny, nx = ds.shape
    assert (ny, nx) == ((H + 15) // 16, (W + 15) // 16)
    lb = int(ds.max())
    sy = np.minimum((np.arange(H) + 8) // 16, ny - 1)
    sx = np.minimum((np.arange(W) + 8) // 16, nx - 1)
    ub = np.sqrt(ds[np.ix_(sy, sx)].astype(np.float64)) + 21.22
    full = ub * ub > float(lb)
    return 1.0 - full.mean(), int(D.max()), lb


def capped_leftover_above_max(m, r):
    """Number of capped pixels whose scan over |k| <= r ends on a value above max D (only the clamp to
    the sample maximum keeps those out of the maximum): min_k k^2 + g(x + k)^2 with g the distance to
    the nearest obstacle in the column, as cm_edt_rows_ramp_kernel computes it."""
    b = np.array(m, dtype=np.uint8)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = 1
    H, W = b.shape
    D = np.rint(ndimage.distance_transform_edt(b == 0) ** 2).astype(np.int64)
    g = np.stack([ndimage.distance_transform_edt(b[:, x] == 0) for x in range(W)], axis=1).astype(np.int64)
    ds = D[::16, ::16]
    sy = np.minimum((np.arange(H) + 8) // 16, ds.shape[0] - 1)
    sx = np.minimum((np.arange(W) + 8) // 16, ds.shape[1] - 1)
    ub = np.sqrt(ds[np.ix_(sy, sx)].astype(np.float64)) + 21.22
    capped = ub * ub <= float(ds.max())
    best = np.full((H, W), np.iinfo(np.int64).max)
    for k in range(-r, r + 1):
        x0, x1 = max(0, -k), min(W, W - k)
        best[:, x0:x1] = np.minimum(best[:, x0:x1], k * k + g[:, x0 + k:x1 + k] ** 2)
    return int((capped & (best > D.max())).sum())


@pytest.mark.parametrize("shape,res,off_grid", [((200, 300), 1 / 20, True), ((160, 420), 1 / 10, False),
                                                ((168, 420), 1 / 10, True)],
                         ids=["200x300-r20", "160x420-r10", "168x420-r10"])
def test_cost_tail_capped_ramp_scan(ctx, shape, res, off_grid):
    """cm_edt_ramp's capped scans: the stored D of a capped pixel outside the dilation is a stand-in, and
    the maximum of D (which normalises the ramp, :1196) must come out exact.  With the right two thirds
    free that maximum lies on the ridge midway between the top and bottom border, (H / 2 - 1)^2: off the
    16-pixel sample grid at H = 200 (rows 99, 100; 9801 against the samples' 9216) and H = 168 (rows 83,
    84), where only the full scans of the uncapped pixels find it; at H = 160 row 80 is a sample row, so
    there the maximum is a sample (6241) and every pixel below it is capped."""
    m = rocks_mask(*shape)
    capped, dmax, smax = ramp_scan_stats(m)
    print(f"capped share {capped:.4f}, max D {dmax}, sample max {smax}")
    assert capped >= 0.5 and dmax == (shape[0] // 2 - 1) ** 2
    assert dmax > smax if off_grid else dmax == smax
    cref, oref = CO.cost_tail(m, res)
    cost, obst = ctx.cost_tail(m, res)
    check_cost(cost, obst, cref, oref)


@pytest.mark.parametrize("shape,blocks", [((300, 120), ()), ((120, 300), ((40, 80, 140, 160),))],
                         ids=["300x120", "120x300"])
def test_cost_tail_capped_scan_clamp(ctx, shape, blocks):
    """A corridor taller than wide: near its side walls the scans are capped, and over +-r columns they
    see only the long free columns (distance^2 far above max D, which the walls bound).  Those leftovers
    must not reach the maximum of :1196.  The wide raster is the counterpart where none is left over."""
    res, r3 = 0.05, 20
    m = blocks_mask(shape, blocks)
    capped, dmax, smax = ramp_scan_stats(m)
    left = capped_leftover_above_max(m, r3)
    print(f"capped share {capped:.4f}, max D {dmax}, sample max {smax}, leftovers above max D {left}")
    assert capped >= 0.25
    assert left > 1000 if shape[0] > shape[1] else left == 0
    cref, oref = CO.cost_tail(m, res)
    cost, obst = ctx.cost_tail(m, res)
    check_cost(cost, obst, cref, oref)


def test_cost_tail_envelope_rows(ctx):
    """Rows wider than 8192: cm_edt_ramp falls back to the full cm_edt with the envelope row pass, the
    dilation of :1192 to cm_bnd_rows_wide_kernel."""
    shape, res = (60, 8200), 0.1
    m = blocks_mask(shape, [(20, 30, 100, 110), (5, 8, 8000, 8010)])
    assert shape[1] > ROW_MAX and m[1:-1, 1:-1].any() and not m[1:-1, 1:-1].all()
    cref, oref = CO.cost_tail(m, res)
    cost, obst = ctx.cost_tail(m, res)
    check_cost(cost, obst, cref, oref)


TAIL_SHAPES = [((3, 3), ()), ((3, 70), ((1, 2, 30, 33),)), ((30, 45), ()), ((30, 45), ((10, 14, 20, 25),)),
               ((49, 50), ((5, 9, 5, 9), (30, 36, 35, 40))), ((65, 129), ((60, 64, 100, 110), (10, 20, 10, 12))),
               ((131, 66), ((64, 70, 30, 40),))]


@pytest.mark.parametrize("shape,blocks", TAIL_SHAPES, ids=[f"{s[0]}x{s[1]}-{len(b)}blocks" for s, b in TAIL_SHAPES])
def test_cost_tail_shapes(ctx, shape, blocks):
    """Rasters smaller than the 50-tap blur window and the 64 x 64 blur tile, just past one tile, ragged
    and non-square: the blur's fill value on every side, the tile kernels' bounds, the sample grid."""
    m = blocks_mask(shape, blocks)
    inner = m[1:-1, 1:-1]
    assert inner.size > 0 and (inner == 0).any() and inner.sum() == sum((b[1] - b[0]) * (b[3] - b[2]) for b in blocks)
    cref, oref = CO.cost_tail(m, 0.05)
    cost, obst = ctx.cost_tail(m, 0.05)
    check_cost(cost, obst, cref, oref)


@pytest.mark.parametrize("kw", [{}, {"gradient": 25.0}, {"expansion": 0.5}, {"expansion": 2.0}, {"high": 150.0}],
                         ids=["defaults", "gradient25", "expansion0.5", "expansion2", "high150"])
def test_cost_tail_constants(ctx, kw):
    """eik_costmap_params through the tail: the ramp radius r3 = 20 / 10 / 40, its scale, the obstacle
    cost (the blur's fill stays 300)."""
    res = 0.05
    m = blocks_mask((97, 131), [(20, 28, 30, 36), (60, 63, 90, 110), (75, 90, 15, 20)])
    r3 = int(round(kw.get("expansion", 1.0) / res))
    assert r3 == {0.5: 10, 1.0: 20, 2.0: 40}[kw.get("expansion", 1.0)]
    assert m[1:-1, 1:-1].any() and not m[1:-1, 1:-1].all()
    cref, oref = CO.cost_tail(m, res, **kw)
    if kw:  # the constant takes part in the result
        assert not np.array_equal(cref, CO.cost_tail(m, res)[0])
    cost, obst = ctx.cost_tail(m, res, params(**kw))
    check_cost(cost, obst, cref, oref)


# ---- c. the full chain with other constants and DEMs below zero ---------------------------------
CHAIN_CASES = {  # n, res, constants, rms_slope, seed, shift ("low": - 1000; "mixed": min at - ptp / 2), (r2, r3)
    "n160-r3-5": (160, 0.1, dict(slope_max=0.15, diagonal=0.6, expansion=0.5, gradient=4.0), 0.14, 31, "low", (3, 5)),
    "n200-r26-80": (200, 0.025, dict(slope_max=0.3, diagonal=1.3, expansion=2.0), 0.30, 32, "low", (26, 80)),
    "n130-gradient25-a": (130, 0.05, dict(gradient=25.0), 0.25, 31, "low", (9, 20)),
    "n130-gradient25-b": (130, 0.05, dict(gradient=25.0), 0.30, 33, "low", (9, 20)),
    "n96-defaults": (96, 0.05, {}, 0.20, 32, "low", (9, 20)),
    "n60-defaults": (60, 0.05, {}, 0.25, 31, "low", (9, 20)),
    "n96-mixed-sign": (96, 0.05, {}, 0.20, 32, "mixed", (9, 20)),
}


@functools.lru_cache(maxsize=None)
def chain_reference(name):
    n, res, kw, rms, seed, shift, _ = CHAIN_CASES[name]
    Z = terrain_np.dem(n, n, seed, rms_slope=rms, res=res)
    Z = Z - 1000.0 if shift == "low" else Z - Z.min() - 0.5 * np.ptp(Z)
    cref, oref = CO.cost_map(Z, res, n * res, **kw)
    for a in (Z, cref, oref):
        a.setflags(write=False)
    return Z, cref, oref


def chain_preconditions(name):
    n, res, kw, _, _, shift, radii = CHAIN_CASES[name]
    Z, cref, oref = chain_reference(name)
    p = dict(diagonal=0.9, expansion=1.0)
    p.update(kw)
    assert (int(round((p["diagonal"] / 2) / res)), int(round(p["expansion"] / res))) == radii
    if shift == "low":
        assert Z.max() < 0  # dkey's negative branch for every element
    else:
        assert Z.min() < 0 < Z.max() and (Z < 0).mean() > 0.1 and (Z > 0).mean() > 0.1
    share = oref[1:-1, 1:-1].mean()
    print(f"interior obstacle share {share:.4f}")
    assert 0.05 <= share <= 0.6
    return Z, cref, oref


@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_costmap_constants_negative_dem(ctx, name):
    """eik_costmap_f64 with constants other than the defaults (r2 = 3 / 26, r3 = 5 / 80, slope, gradient)
    on DEMs whose minimum is negative: min(Z) through the order-preserving key's negative branch."""
    n, res, kw = CHAIN_CASES[name][:3]
    Z, cref, oref = chain_preconditions(name)
    cost, obst = ctx.costmap(Z, res, n * res, params(**kw))
    check_cost(cost, obst, cref, oref)


def test_costmap_dropin_constants(ctx):
    """costmap.cost_map's keywords reach the builder (the drop-in holds cMap [x, y], obstMap float64)."""
    import costmap

    name = "n160-r3-5"
    n, res, kw = CHAIN_CASES[name][:3]
    Z, cref, oref = chain_preconditions(name)
    assert set(kw) == {"slope_max", "diagonal", "expansion", "gradient"}
    cmap, obst = costmap.cost_map(Z, res, n * res, **kw)
    assert obst.dtype == np.float64
    check_cost(cmap.T, obst, cref, oref)


def test_surface_normal_negative_dem(ctx):
    """The normals entry shifts by min(Z) itself: a DEM near -1000 against the oracle on Z - min(Z) (the
    same subtraction on the same doubles)."""
    n, res = CHAIN_CASES["n96-defaults"][:2]
    Z = chain_reference("n96-defaults")[0]
    assert -1001 < Z.min() < -999 and Z.max() < 0
    ref = CO.surface_normal(res, n * res, Z - Z.min())
    got = ctx.surface_normal(Z, n * res)
    for g, r in zip(got, ref):
        assert np.abs(g - r).max() <= 1e-12


@pytest.mark.parametrize("name", ["n160-r3-5", "n96-mixed-sign"])
def test_rover_path_z_negative_dem(ctx, name):
    """min(Z) itself, not only differences of Z - min(Z) (which the normals see): the rover path's
    heights are zp + (Z - min Z) at its waypoints (:1101, :1246), with min Z decoded from the builder's
    key on the host.  A wrong minimum of a negative DEM shifts every height."""
    import planner

    n, res, kw = CHAIN_CASES[name][:3]
    Z, cref, _ = chain_preconditions(name)
    assert Z.min() < 0
    ys, xs = np.nonzero(np.isfinite(cref.T) & (cref.T < 5))
    far = np.argmax((xs - xs[0]) ** 2 + (ys - ys[0]) ** 2)  # two free cells far apart
    assert (xs[far] - xs[0]) ** 2 + (ys[far] - ys[0]) ** 2 > (n // 4) ** 2
    q = planner.query(res * (xs[0] + 1), res * (ys[0] + 1), res * (xs[far] + 1), res * (ys[far] + 1), 0.4, res, n * res)
    path, _, _ = ctx.rover_path(Z, q, params(**kw))
    assert len(path) > 10
    Zs = Z - Z.min()
    iy = np.round(path[:, 1] / res).astype(np.int64)
    ix = np.round(path[:, 0] / res).astype(np.int64)
    assert np.array_equal(path[:, 2], planner.ZP + Zs[iy, ix])


# ---- d. hole filling below and around one 32 x 32 union-find tile -------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (40, 1), (2, 33), (31, 31), (32, 33), (33, 64)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_filling_small(ctx, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    im = (rng.random(shape) < 0.5).astype(np.uint8)
    assert im.shape == shape and (im.size == 1 or 0 < im.sum() < im.size)
    for s in (0, 1):  # seed pixel free / obstacle (the reference fills everything then)
        im[0, 0] = s
        ref = CO.image_filling(im)
        assert s == 0 or ref.all()
        assert np.array_equal(ctx.image_fill(im), ref)


def _line_masks():
    line = np.array([0] * 36 + [1] + [0] * 3, np.uint8)  # free run across pixel 31 | 32, a wall, a hole
    two = np.zeros((2, 33), np.uint8)
    two[0, 20:] = 1  # the seed's set crosses column 31 | 32 in row 1 only
    two[0, 32] = 0  # reached from below
    tall = np.zeros((33, 2), np.uint8)
    tall[20:, 0] = 1
    tall[32, 0] = 0
    return {"1x40": line[None, :], "40x1": line[:, None], "2x33": two, "33x2": tall}


@pytest.mark.parametrize("name", list(_line_masks()))
def test_image_filling_across_tile_border(ctx, name):
    """Rasters one or two pixels thin whose seed component crosses the 32-pixel tile border of the
    union-find (a random thin mask almost never does: it needs 33 equal pixels in a row): the single
    border pair, with no neighbouring pair, joins the two tiles."""
    im = _line_masks()[name]
    ref = CO.image_filling(im)
    long_axis = int(np.argmax(im.shape))
    beyond = np.take(ref == 0, range(32, im.shape[long_axis]), axis=long_axis)
    assert beyond.any()  # pixels past the tile border stay free, i.e. were reached through it
    if min(im.shape) == 1:
        assert (ref != im).sum() == 3  # the hole behind the wall is filled
    assert np.array_equal(ctx.image_fill(im), ref)
    assert np.array_equal(ctx.image_fill(1 - im), CO.image_filling(1 - im))  # seed value 1
