"""NumPy restatement of the global-localization specification (include/rbpf_hip.h: rbpf_locate_scan), written
from the specification and not from the kernels.  Scores are integers, so the GPU tests compare bit for bit.  Every cosine and
sine comes from math.cos / math.sin, the libm the library's host code calls; the products and sums are single IEEE float64
operations in NumPy as in plain Python."""
import math

import numpy as np

TWO_PI = 6.283185307179586


def used_beams(ranges, angles, min_range, max_range):
    """(bx [n_used], by [n_used]): sensor-frame end points of the beams with min_range < range < max_range, in beam order."""
    bx, by = [], []
    for r, a in zip(ranges, angles):
        r, a = float(r), float(a)
        if min_range < r < max_range:
            bx.append(r * math.cos(a))
            by.append(r * math.sin(a))
    return np.array(bx, dtype=np.float64), np.array(by, dtype=np.float64)


def offsets(bx, by, n_rot, inv):
    """(u, w) int64 [n_rot][n_used]: the cell offset of every beam's end point from the candidate cell."""
    u = np.empty((n_rot, len(bx)), dtype=np.int64)
    w = np.empty((n_rot, len(bx)), dtype=np.int64)
    for r in range(n_rot):
        th = (r * TWO_PI) / n_rot
        c, s = math.cos(th), math.sin(th)
        u[r] = np.floor(0.5 + (c * bx - s * by) * inv)
        w[r] = np.floor(0.5 + (s * bx + c * by) * inv)
    return u, w


def window(cells, x0, y0, wx0, wx1, wy0, wy1):
    """cells (origin x0, y0; 0 outside) cut or zero-padded to the box [wx0, wx1) x [wy0, wy1)."""
    out = np.zeros((wx1 - wx0, wy1 - wy0), dtype=cells.dtype)
    a0, a1 = max(wx0, x0), min(wx1, x0 + cells.shape[0])
    b0, b1 = max(wy0, y0), min(wy1, y0 + cells.shape[1])
    if a0 < a1 and b0 < b1:
        out[a0 - wx0:a1 - wx0, b0 - wy0:b1 - wy0] = cells[a0 - x0:a1 - x0, b0 - y0:b1 - y0]
    return out


def field(v, quantum, occupied_threshold):
    """F = occ + dil of a raster whose surroundings are 0 (the outermost ring of the result is not to be used)."""
    occ = (v.astype(np.float64) * quantum > occupied_threshold)
    p = np.pad(occ, 1)
    dil = np.zeros_like(occ)
    for di in range(3):
        for dj in range(3):
            dil |= p[di:di + occ.shape[0], dj:dj + occ.shape[1]]
    return occ.astype(np.uint8) + dil.astype(np.uint8)


def locate(cells, x0, y0, box, ranges, angles, n_rot, inv, quantum, occupied_threshold, min_range, max_range):
    """cells[X - x0][Y - y0]: int8 lattice values of a rendered map, 0 outside the raster.  Returns (best, rot, n_used):
    int32 [x1-x0][y1-y0] rasters over `box`, -1 where the cell is no candidate; one shifted-slice add per (rotation, beam)."""
    bx0, bx1, by0, by1 = (int(q) for q in box)
    nx, ny = bx1 - bx0, by1 - by0
    bx, by = used_beams(ranges, angles, min_range, max_range)
    u, w = offsets(bx, by, n_rot, inv)
    m = int(max(np.abs(u).max(), np.abs(w).max())) if len(bx) else 0
    g = m + 1                                            # one ring more: the dilation of the outermost cells read
    F = field(window(cells, x0, y0, bx0 - g, bx1 + g, by0 - g, by1 + g), quantum, occupied_threshold)
    cand = window(cells, x0, y0, bx0, bx1, by0, by1) < 0
    best = np.full((nx, ny), -1, dtype=np.int32)
    rot = np.full((nx, ny), -1, dtype=np.int32)
    for r in range(n_rot):
        s = np.zeros((nx, ny), dtype=np.int32)
        for k in range(len(bx)):
            i, j = g + int(u[r, k]), g + int(w[r, k])
            s += F[i:i + nx, j:j + ny]
        better = s > best                                # strictly: the smallest r that attains the maximum is kept
        best[better] = s[better]
        rot[better] = r
    best[~cand] = -1
    rot[~cand] = -1
    return best, rot, len(bx)


def locate_scalar(cells, x0, y0, X, Y, ranges, angles, n_rot, inv, quantum, occupied_threshold, min_range, max_range):
    """(best, rot) of the one cell (X, Y), by loops over rotations and beams in plain Python."""
    rows = cells.tolist()

    def v(a, b):
        i, j = a - x0, b - y0
        return rows[i][j] if 0 <= i < len(rows) and 0 <= j < len(rows[0]) else 0

    def occ(a, b):
        return 1 if v(a, b) * quantum > occupied_threshold else 0

    def F(a, b):
        return occ(a, b) + max(occ(a + da, b + db) for da in (-1, 0, 1) for db in (-1, 0, 1))

    if not v(X, Y) < 0:
        return -1, -1
    pts = [(float(r) * math.cos(float(a)), float(r) * math.sin(float(a))) for r, a in zip(ranges, angles)
           if min_range < float(r) < max_range]
    best, rot = -1, -1
    for r in range(n_rot):
        th = (r * TWO_PI) / n_rot
        c, s = math.cos(th), math.sin(th)
        score = 0
        for px, py in pts:
            score += F(X + math.floor(0.5 + (c * px - s * py) * inv), Y + math.floor(0.5 + (s * px + c * py) * inv))
        if score > best:
            best, rot = score, r
    return best, rot


# ---- the asymmetric test room ---------------------------------------------------------------------------------------------------
ROOM_HALF = 8.0
PILLARS = [(4.0, 4.0), (-4.0, 4.0), (-4.0, -4.0), (4.0, -4.0)]
PILLAR_HALF = 0.5
BLOCKS = [(1.0, 2.5, 5.0, 6.0), (-6.5, -5.5, -3.0, -0.5)]       # x_lo, x_hi, y_lo, y_hi in metres: off axis, unlike the pillars


def asym_room(cell):
    """room16's outline (synthetic.py: the 16 m square, four 1 m pillars) plus two off-axis blocks, as a map a SLAM run would
    leave: the floor observed free (-30), every surface one occupied cell thick (+30), everything behind it unknown (0).
    Returns (cells [n][n] int8, x0, y0); faces lie on cell boundaries for cell = 0.1, 0.05 and 0.025 m."""
    n = int(round(20.0 / cell))
    x0 = -(n // 2)
    c = (np.arange(x0, x0 + n) + 0.5) * cell
    inside = np.abs(c) < ROOM_HALF
    floor = np.outer(inside, inside)
    solid = np.zeros((n, n), dtype=bool)
    for px, py in PILLARS:
        solid |= np.outer(np.abs(c - px) < PILLAR_HALF, np.abs(c - py) < PILLAR_HALF)
    for xl, xh, yl, yh in BLOCKS:
        solid |= np.outer((c > xl) & (c < xh), (c > yl) & (c < yh))
    free = floor & ~solid
    p = np.pad(free, 1)
    near = np.zeros_like(free)
    for di in range(3):
        for dj in range(3):
            near |= p[di:di + n, dj:dj + n]
    cells = np.zeros((n, n), dtype=np.int8)
    cells[free] = -30
    cells[near & ~free] = 30                             # the cells that touch the floor: walls and shells of pillars and blocks
    return cells, x0, x0
