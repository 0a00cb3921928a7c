"""float64 numpy reference of sampling a dense image at sub-pixel points, with the semantics of
``F.grid_sample(image[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)`` for UN-NORMALISED sample
coordinates (ix = continuous column index, iy = continuous row index): what ``gs.alpha_blending_points`` computes without the
dense image.  Shared by test_track_query_cpu.py and the GPU tests of the operator and of the tracker."""
import numpy as np


def corners(points, W, H):
    """(cx, cy, weight, inside) of the four bilinear corners nw, ne, sw, se of every point: [Q, 4] each.  The in / out test is made
    on the floating-point corner coordinates; a non-finite point has no corner inside."""
    p = np.asarray(points, np.float64)
    ix, iy = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        x0, y0 = np.floor(ix), np.floor(iy)
        k = np.arange(4)
        cx, cy = x0[:, None] + (k & 1), y0[:, None] + (k >> 1)
        wx = np.stack([x0 + 1 - ix, ix - x0], 1)
        wy = np.stack([y0 + 1 - iy, iy - y0], 1)
        w = wx[:, k & 1] * wy[:, k >> 1]
        inside = np.isfinite(cx) & np.isfinite(cy) & (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
    return cx, cy, w, inside


def sample_points(image, points):
    """image [C, H, W], points [Q, 2] = (ix, iy) -> [Q, C] float64: sum over the corners inside the image of weight * pixel
    (nw, ne, sw, se); a corner outside contributes nothing, so a point fully outside (1e9, NaN, inf) gives a row of zeros"""
    img = np.asarray(image, np.float64)
    C, H, W = img.shape
    cx, cy, w, inside = corners(points, W, H)
    out = np.zeros((cx.shape[0], C), np.float64)
    for k in range(4):
        m = inside[:, k]
        xi, yi = cx[m, k].astype(np.int64), cy[m, k].astype(np.int64)
        out[m] += w[m, k, None] * img[:, yi, xi].T
    return out


def corner_pixels(points, W, H):
    """integer (x, y) of the four corners and the inside mask: [Q, 4] each (x = y = 0 where outside)"""
    cx, cy, _, inside = corners(points, W, H)
    xi = np.where(inside, cx, 0).astype(np.int64)
    yi = np.where(inside, cy, 0).astype(np.int64)
    return xi, yi, inside
