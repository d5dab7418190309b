"""NumPy restatement of the local-map specification (include/rbpf_hip.h: rbpf_local_map), written from the
specification and not from the kernels.  Plain Python floats and np.float64 arrays are IEEE float64, every NumPy operation
rounds on its own (no fused multiply-add between two ufunc calls), and math.cos / math.sin are the libm the library's host code
calls, so the GPU tests compare by equality.  crop_scalar is the cell-by-cell form, crop the same operations on arrays."""
import math

import numpy as np


def tables(n, S, cell_out, offset=(0.0, 0.0)):
    """(gx, gy) [n S] float64: ((q / S) + ((q % S) + 0.5) / S - 0.5 n) * cell_out + f, in that order."""
    q = np.arange(n * S)
    u = (((q // S).astype(np.float64) + ((q % S).astype(np.float64) + 0.5) / np.float64(S)) - 0.5 * np.float64(n)) * np.float64(cell_out)
    return u + np.float64(offset[0]), u + np.float64(offset[1])


def reach(n, cell_out, offset, inv):
    h = 0.5 * n * cell_out
    return math.ceil(math.hypot(abs(offset[0]) + h, abs(offset[1]) + h) * inv) + 2


def value(cells, x0, y0, X, Y):
    """v(X, Y) of a rendered map cells[X - x0][Y - y0]: 0 outside the raster (no tile, outside a written box, off the lattice)."""
    i, j = X - x0, Y - y0
    return int(cells[i][j]) if 0 <= i < cells.shape[0] and 0 <= j < cells.shape[1] else 0


def crop_scalar(cells, x0, y0, pose, n, S, cell_out, offset, inv):
    """[n][n] int8, one cell and one sample at a time."""
    gx, gy = tables(n, S, cell_out, offset)
    x, y, th = (float(v) for v in pose)
    c, s = math.cos(th), math.sin(th)
    out = np.zeros((n, n), np.int8)
    for i in range(n):
        for j in range(n):
            m = -128
            for qa in range(i * S, i * S + S):
                for qb in range(j * S, j * S + S):
                    lx, ly = float(gx[qa]), float(gy[qb])
                    cx, sy, sx, cy = c * lx, s * ly, s * lx, c * ly
                    rx, ry = cx - sy, sx + cy
                    wx, wy = x + rx, y + ry
                    m = max(m, value(cells, x0, y0, math.floor(wx * inv), math.floor(wy * inv)))
            out[i, j] = m
    return out


def crop(cells, x0, y0, pose, n, S, cell_out, offset, inv):
    """[n][n] int8: the operations of crop_scalar on arrays."""
    gx, gy = tables(n, S, cell_out, offset)
    x, y, th = (np.float64(v) for v in pose)
    c, s = np.float64(math.cos(float(th))), np.float64(math.sin(float(th)))
    cx, sx, sy, cy = c * gx, s * gx, s * gy, c * gy
    rx, ry = cx[:, None] - sy[None, :], sx[:, None] + cy[None, :]
    wx, wy = x + rx, y + ry
    X = np.floor(wx * np.float64(inv)).astype(np.int64) - x0
    Y = np.floor(wy * np.float64(inv)).astype(np.int64) - y0
    inside = (X >= 0) & (X < cells.shape[0]) & (Y >= 0) & (Y < cells.shape[1])
    v = np.where(inside, cells[np.clip(X, 0, cells.shape[0] - 1), np.clip(Y, 0, cells.shape[1] - 1)], 0).astype(np.int8)
    return v.reshape(n, S, n, S).max(axis=(1, 3))


def fuse(crops, wq, thr):
    """[n][n][4] int64 {occ_w, free_w, unknown_w, sum_wv} of crops [N][n][n] with integer weights wq [N] (None: all 1);
    thr = occupied_threshold / quantum, strict."""
    crops = np.asarray(crops).astype(np.int64)
    w = (np.ones(crops.shape[0], np.int64) if wq is None else np.asarray(wq).astype(np.int64))[:, None, None]
    return np.stack([((crops > thr) * w).sum(0), ((crops < 0) * w).sum(0), ((crops == 0) * w).sum(0), (crops * w).sum(0)], axis=-1)
