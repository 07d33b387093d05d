"""The cost diff's rule (include/eikonal.h) restated in numpy: what the device
kernels and the host's coarsening are compared with, cell for cell and count for count.

Per cell: changed when old != new as values (+0 == -0, +inf == +inf) or the new value is invalid;
raised when new > old; invalid when new is NaN or < 0.  Per 64 x 64 tile: the bounding box of the changed
cells.  A changed tile's rectangle is its box, ANY (0) with a raised cell, else LOWERED (1); more than
`cap` of them are united per block of 2 x 2 tiles aligned to the grid's origin, then 4 x 4, ... and
emitted in ascending (block row, block column).
"""
import numpy as np

TILE = 64
ANY, LOWERED = 0, 1


def cell_masks(old, new):
    """(changed, raised, invalid) boolean masks"""
    old, new = np.asarray(old), np.asarray(new)
    with np.errstate(invalid="ignore"):
        invalid = np.isnan(new) | (new < 0)
        changed = (old != new) | invalid
        raised = new > old
    return changed, raised, invalid


def tile_records(old, new):
    """One record per changed tile, in ascending tile index: dicts with tile, the box x0, y0, x1, y1 (half-open,
    raster coordinates) and the counts changed, raised, invalid"""
    changed, raised, invalid = cell_masks(old, new)
    H, W = changed.shape
    ntx = (W + TILE - 1) // TILE
    recs = []
    for ty in range((H + TILE - 1) // TILE):
        for tx in range(ntx):
            sl = (slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE))
            ys, xs = np.nonzero(changed[sl])
            if len(ys):
                recs.append(dict(tile=ty * ntx + tx, x0=tx * TILE + int(xs.min()), y0=ty * TILE + int(ys.min()),
                                 x1=tx * TILE + int(xs.max()) + 1, y1=ty * TILE + int(ys.max()) + 1,
                                 changed=len(ys), raised=int(raised[sl].sum()), invalid=int(invalid[sl].sum())))
    return recs


def rects_from_records(recs, ntx, cap):
    """(rects [(x0, y0, x1, y1)], kinds, block side in tiles; 0 when nothing changed)"""
    if not recs:
        return [], [], 0
    side = 1
    while True:
        blocks = {}
        for r in recs:
            key = (r["tile"] // ntx // side, r["tile"] % ntx // side)
            kind = ANY if r["raised"] else LOWERED
            if key in blocks:
                b = blocks[key]
                blocks[key] = (min(b[0], r["x0"]), min(b[1], r["y0"]), max(b[2], r["x1"]), max(b[3], r["y1"]), min(b[4], kind))
            else:
                blocks[key] = (r["x0"], r["y0"], r["x1"], r["y1"], kind)
        if len(blocks) <= cap:
            keys = sorted(blocks)
            return [blocks[k][:4] for k in keys], [blocks[k][4] for k in keys], side
        side *= 2


def cost_diff(old, new, cap=1024):
    """(rects, kinds, info) as eikonal.Context.cost_diff returns them (info without the device time)"""
    changed, raised, invalid = cell_masks(old, new)
    recs = tile_records(old, new)
    ntx = (changed.shape[1] + TILE - 1) // TILE
    rects, kinds, side = rects_from_records(recs, ntx, cap)
    info = dict(cells_changed=int(changed.sum()), cells_raised=int(raised.sum()), cells_invalid=int(invalid.sum()),
                tiles_changed=len(recs), block_side=side)
    return rects, kinds, info
