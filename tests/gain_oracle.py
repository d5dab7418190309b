"""Scalar restatement of the view-gain specification (include/rbpf_hip.h: rbpf_view_gain), written from the
specification and not from the kernel: the loop of cast_oracle.cast, collecting the cells it tests into a Python set, then
the set classified on a rendered raster.  All outputs are integers, so the GPU tests compare for equality."""
import math

import numpy as np

from tests.cast_oracle import lattice_bounds, room16_cells  # noqa: F401  (re-exported for the tests)


def visited(cells, x0, y0, lo, hi, inv, quantum, occupied_threshold, pose, angles, max_range):
    """The set of mosaic cells (X, Y) the beams of `pose` test (cells[X - x0][Y - y0]: int8 lattice values, 0 outside the
    raster; [lo, hi) the lattice), and the number of walk steps.  Asserts the window bound on every cell collected."""
    x, y, th = (float(q) for q in pose)
    c, s = math.cos(th), math.sin(th)
    ox, oy = x * inv, y * inv
    tlim = max_range * inv
    M = math.ceil(tlim) + 2
    nxc, nyc = cells.shape
    rows = cells.tolist()
    V, steps = set(), 0
    fX, fY = math.floor(ox), math.floor(oy)
    if not (lo <= fX < hi and lo <= fY < hi):
        return V, steps
    X0, Y0 = int(fX), int(fY)
    for a in angles:
        ca, sa = math.cos(a), math.sin(a)
        dx, dy = c * ca - s * sa, s * ca + c * sa
        X, Y = X0, Y0
        sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
        tdx = 1.0 / abs(dx) if dx != 0 else math.inf
        tdy = 1.0 / abs(dy) if dy != 0 else math.inf
        fx = (X + 1) - ox if dx > 0 else ox - X
        fy = (Y + 1) - oy if dy > 0 else oy - Y
        nx = ny = 0
        while True:
            if not (lo <= X < hi and lo <= Y < hi):
                break
            assert abs(X - X0) <= M and abs(Y - Y0) <= M, ("window bound", X - X0, Y - Y0, M)
            V.add((X, Y))
            i, j = X - x0, Y - y0
            if 0 <= i < nxc and 0 <= j < nyc and rows[i][j] * quantum > occupied_threshold:
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
    return V, steps


def classify(V, cells, x0, y0, vmin, table):
    """(gain, seen, unknown) of a visited set on the raster: v(c) = 0 outside it."""
    nxc, nyc = cells.shape
    tab = [int(q) for q in table]
    g = u = 0
    for X, Y in V:
        i, j = X - x0, Y - y0
        v = int(cells[i, j]) if 0 <= i < nxc and 0 <= j < nyc else 0
        g += tab[v - vmin]
        u += v == 0
    return g, len(V), u


def view_gain(cells, x0, y0, lo, hi, inv, quantum, occupied_threshold, vmin, table, poses, angles, max_range):
    """(gain [N] int64, seen [N] int32, unknown [N] int32, steps): the visited set of every pose classified on the raster."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    gain, seen, unknown = np.zeros(len(poses), np.int64), np.zeros(len(poses), np.int32), np.zeros(len(poses), np.int32)
    steps = 0
    for n, pose in enumerate(poses):
        V, st = visited(cells, x0, y0, lo, hi, inv, quantum, occupied_threshold, pose, angles, max_range)
        steps += st
        gain[n], seen[n], unknown[n] = classify(V, cells, x0, y0, vmin, table)
    return gain, seen, unknown, steps
