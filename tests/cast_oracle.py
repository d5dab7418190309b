"""Scalar restatement of the scan-casting specification (include/rbpf_hip.h: rbpf_cast_scans), written from
the specification and not from the kernel.  Plain Python floats are IEEE float64 and math.cos / math.sin are the libm the
library's host code calls, so the GPU tests compare bit for bit."""
import math

import numpy as np


def lattice_bounds(dim, R):
    """[lo, hi): the mosaic cells of the tile lattice -R .. R (include/rbpf_hip.h, "Rasters are indexed in mosaic cells")."""
    return -R * dim - dim // 2, (R + 1) * dim - dim // 2


def cast(cells, x0, y0, lo, hi, inv, quantum, occupied_threshold, pose, angles, max_range):
    """cells[X - x0][Y - y0]: int8 lattice values of a rendered map, 0 outside the raster; inv = dim / tile_len (cells per
    metre).  Returns (ranges [B] float64, status [B] uint8, steps taken)."""
    x, y, th = (float(q) for q in pose)
    c, s = math.cos(th), math.sin(th)
    ox, oy = x * inv, y * inv
    tlim = max_range * inv
    nxc, nyc = cells.shape
    rows = cells.tolist()
    out, st, steps = np.full(len(angles), float(max_range)), np.zeros(len(angles), np.uint8), 0
    for b, a in enumerate(angles):
        ca, sa = math.cos(a), math.sin(a)
        dx, dy = c * ca - s * sa, s * ca + c * sa
        fX, fY = math.floor(ox), math.floor(oy)
        if not (lo <= fX < hi and lo <= fY < hi):
            st[b] = 2
            continue
        X, Y = int(fX), int(fY)
        sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
        tdx = 1.0 / abs(dx) if dx != 0 else math.inf
        tdy = 1.0 / abs(dy) if dy != 0 else math.inf
        fx = (X + 1) - ox if dx > 0 else ox - X
        fy = (Y + 1) - oy if dy > 0 else oy - Y
        nx = ny = 0
        t = 0.0
        while True:
            if not (lo <= X < hi and lo <= Y < hi):
                st[b] = 2
                break
            i, j = X - x0, Y - y0
            if 0 <= i < nxc and 0 <= j < nyc and rows[i][j] * quantum > occupied_threshold:
                st[b], out[b] = 1, t / inv
                break
            tmx = (nx + fx) * tdx if dx != 0 else math.inf
            tmy = (ny + fy) * tdy if dy != 0 else math.inf
            if tmx < tmy:
                t, nx, X = tmx, nx + 1, X + sx
            else:
                t, ny, Y = tmy, ny + 1, Y + sy
            steps += 1
            if t > tlim:
                break
    return out, st, steps


def room16_cells(value=30):
    """synthetic.py's room at 0.05 m, exactly: every wall and pillar face lies on a cell boundary (8.0 m = cell 160, the
    pillars 3.5 .. 4.5 m = cells 70 .. 89), so the raster IS the room.  Returns (cells [400][400], x0, y0): walls 40
    cells thick around the free square, the four pillars inside."""
    from thesis_amd.datasets import synthetic
    n, x0 = 400, -200
    centre = (np.arange(x0, x0 + n) + 0.5) * 0.05
    wall = np.abs(centre) > synthetic.ROOM_HALF
    cells = np.zeros((n, n), np.int8)
    cells[wall, :] = value
    cells[:, wall] = value
    for px, py in synthetic.PILLARS:
        cells[np.ix_(np.abs(centre - px) < synthetic.PILLAR_HALF, np.abs(centre - py) < synthetic.PILLAR_HALF)] = value
    return cells, x0, x0
