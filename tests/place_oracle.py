"""NumPy restatement of map placement (include/rbpf_hip.h, rbpf_place_map): the resampling rule in float64
with every operation rounded on its own, in the order the header writes it, and the three merge modes.  NumPy's elementwise
float64 arithmetic rounds each operation once and fuses nothing, so `warp` is bit for bit what kernels_place.hip computes.

`resample` is the same max-of-samples rule with a destination frame of its own (any cell size, origin and yaw); the tests
use it to write a room as another mapping tool would have."""
import math

import numpy as np

REPLACE, KNOWN, ADD = 0, 1, 2


def _gather(src, u, w, best, cov):
    """Folds the samples at source coordinates (u, w) into the running maximum and the covered mask."""
    nsx, nsy = src.shape
    fu, fw = np.floor(u), np.floor(w)
    inside = (fu >= 0) & (fu < nsx) & (fw >= 0) & (fw < nsy)              # NaN and infinities fail every comparison
    iu = np.where(inside, fu, 0).astype(np.int64)
    iw = np.where(inside, fw, 0).astype(np.int64)
    val = src[iu, iw].astype(np.int16)
    np.maximum(best, np.where(inside, val, -128), out=best)
    cov |= inside


def warp(src, src_cell, src_pose, box, cs, S):
    """(warped int8, covered uint8) [x1-x0][y1-y0] of the mosaic cells `box` = (x0, x1, y0, y1) of size `cs` = tile_len / dim,
    for the source `src` [nsx][nsy] int8 with cells of `src_cell` metres and the corner of cell (0, 0) at `src_pose` =
    (ox, oy, yaw); S samples per axis."""
    src = np.asarray(src)
    ox, oy, yaw = (float(v) for v in src_pose)
    c, s = math.cos(yaw), math.sin(yaw)
    src_cell, cs = float(src_cell), float(cs)
    X = np.arange(box[0], box[1], dtype=np.float64)
    Y = np.arange(box[2], box[3], dtype=np.float64)
    best = np.full((len(X), len(Y)), -128, dtype=np.int16)
    cov = np.zeros((len(X), len(Y)), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(S):
            fa = (a + 0.5) / S
            dx = (X + fa) * cs - ox
            cdx, sdx = c * dx, s * dx
            for b in range(S):
                fb = (b + 0.5) / S
                dy = (Y + fb) * cs - oy
                u = (cdx[:, None] + (s * dy)[None, :]) / src_cell
                w = ((c * dy)[None, :] - sdx[:, None]) / src_cell
                _gather(src, u, w, best, cov)
    return np.where(cov, best, 0).astype(np.int8), cov.astype(np.uint8)


def merge(old, warped, covered, mode, vmin, vmax):
    """The cells of the box after a placement: `old` int8 with the covered cells replaced (REPLACE), replaced where the warped
    value is not 0 (KNOWN), or set to clamp(old + warped, vmin, vmax) (ADD); vmin, vmax in units of quantum."""
    old, warped, cov = np.asarray(old), np.asarray(warped), np.asarray(covered).astype(bool)
    if mode == REPLACE:
        return np.where(cov, warped, old).astype(np.int8)
    if mode == KNOWN:
        return np.where(cov & (warped != 0), warped, old).astype(np.int8)
    if mode == ADD:
        return np.where(cov, np.clip(old.astype(np.int16) + warped.astype(np.int16), vmin, vmax), old).astype(np.int8)
    raise ValueError(f"unknown mode {mode!r}")


def resample(src, src_cell, src_pose, shape, dst_cell, dst_pose, S):
    """The same rule into a raster with a frame of its own: destination cell (i, j) of `shape` has cells of `dst_cell` metres
    and the corner of cell (0, 0) at `dst_pose` = (x, y, yaw).  Returns (cells int8, covered uint8).  Not bit-pinned: the
    tests only use it to make inputs."""
    src = np.asarray(src)
    ox, oy, yaw = (float(v) for v in src_pose)
    c, s = math.cos(yaw), math.sin(yaw)
    qx, qy, qyaw = (float(v) for v in dst_pose)
    dc, ds = math.cos(qyaw), math.sin(qyaw)
    I = np.arange(shape[0], dtype=np.float64)
    J = np.arange(shape[1], dtype=np.float64)
    best = np.full(shape, -128, dtype=np.int16)
    cov = np.zeros(shape, dtype=bool)
    for a in range(S):
        p = ((I + (a + 0.5) / S) * dst_cell)[:, None]
        for b in range(S):
            q = ((J + (b + 0.5) / S) * dst_cell)[None, :]
            dx = qx + dc * p - ds * q - ox
            dy = qy + ds * p + dc * q - oy
            _gather(src, (c * dx + s * dy) / src_cell, (c * dy - s * dx) / src_cell, best, cov)
    return np.where(cov, best, 0).astype(np.int8), cov.astype(np.uint8)
