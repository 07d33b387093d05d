"""Disk morphology of sparse 0/1 masks by stamping (numpy; a reference for radii where the
oracle's O(r^2 H W) shifts are unusable).  Dilation with structural_disk(r) is the OR of the disk
stamped, clipped to the image, at every set pixel; the disk is symmetric and pixels outside the
image take no part (cv2's border rule), so erosion is 1 - dilate(1 - im).  Pinned bit-exact to
costmap_oracle.dilate / erode in tests/test_costmap_oracle.py."""
import functools

import numpy as np

import costmap_oracle as CO


@functools.lru_cache(maxsize=None)
def _disk(r):
    return CO.structural_disk(r).astype(bool)


def dilate(im, r):
    im = np.asarray(im)
    H, W = im.shape
    se = _disk(r)
    out = np.zeros((H, W), bool)
    for y, x in np.argwhere(im != 0):
        y0, y1 = max(0, y - r), min(H, y + r + 1)
        x0, x1 = max(0, x - r), min(W, x + r + 1)
        out[y0:y1, x0:x1] |= se[y0 - y + r:y1 - y + r, x0 - x + r:x1 - x + r]
    return out.astype(np.uint8)


def erode(im, r):
    return (1 - dilate(1 - np.asarray(im, dtype=np.uint8), r)).astype(np.uint8)
