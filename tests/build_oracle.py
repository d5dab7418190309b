"""Scalar restatement of the map-building specification (include/rbpf_hip.h: rbpf_build_map), written from the
specification and not from the kernel: one beam at a time, the walk of cast_oracle.cast with no map to test, the cells of a scan
collected in two Python sets, the sets added into two integer rasters.  The GPU tests compare both rasters for equality."""
import math

import numpy as np


def walk(pose, angle, inv, tend):
    """The cells C0 .. Ck of one beam, in order: Ck is the last one entered at a parameter <= tend."""
    x, y, th = (float(q) for q in pose)
    c, s = math.cos(th), math.sin(th)
    ca, sa = math.cos(float(angle)), math.sin(float(angle))
    return walk_dir(x * inv, y * inv, c * ca - s * sa, s * ca + c * sa, tend)


def walk_dir(ox, oy, dx, dy, tend):
    """The same from the origin (ox, oy) in cells along (dx, dy)."""
    X, Y = math.floor(ox), math.floor(oy)
    sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    tdx = 1.0 / abs(dx) if dx != 0 else math.inf
    tdy = 1.0 / abs(dy) if dy != 0 else math.inf
    fx = (X + 1) - ox if dx > 0 else ox - X
    fy = (Y + 1) - oy if dy > 0 else oy - Y
    nx = ny = 0
    cells = [(X, Y)]
    while True:
        tmx = (nx + fx) * tdx if dx != 0 else math.inf
        tmy = (ny + fy) * tdy if dy != 0 else math.inf
        if tmx < tmy:                                    # a tie steps in y
            t, nx, X = tmx, nx + 1, X + sx
        else:
            t, ny, Y = tmy, ny + 1, Y + sy
        if t > tend:
            return cells
        cells.append((X, Y))


def scan_sets(pose, ranges, angles, inv, min_range, max_range):
    """(H, V, steps) of one scan: the cells hit by its return beams, the cells passed or ended in by its beams that are not
    skipped, and the number of cells walked.  Asserts the window bound on every cell."""
    M = math.ceil(max_range * inv) + 2
    X0, Y0 = math.floor(float(pose[0]) * inv), math.floor(float(pose[1]) * inv)
    H, V, steps = set(), set(), 0
    for r, a in zip(ranges, angles):
        r = float(r)
        if math.isnan(r) or r < min_range:
            continue
        free = r > max_range
        cells = walk(pose, a, inv, max_range * inv if free else r * inv)
        steps += len(cells)
        for X, Y in cells:
            assert abs(X - X0) <= M and abs(Y - Y0) <= M, ("window bound", X - X0, Y - Y0, M)
        V.update(cells)
        if not free:
            H.add(cells[-1])
    return H, V, steps


def build_map(poses, ranges, angles, inv, box, min_range, max_range):
    """(hits, seen, steps): int32 [x1-x0][y1-y0] over box = (x0, x1, y0, y1), half-open, in cells of size 1 / inv."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(len(poses), -1)
    x0, x1, y0, y1 = (int(q) for q in box)
    hits, seen = np.zeros((x1 - x0, y1 - y0), np.int32), np.zeros((x1 - x0, y1 - y0), np.int32)
    steps = 0
    for pose, rg in zip(poses, ranges):
        H, V, st = scan_sets(pose, rg, angles, inv, min_range, max_range)
        steps += st
        for S, out in ((H, hits), (V, seen)):
            for X, Y in S:
                if x0 <= X < x1 and y0 <= Y < y1:
                    out[X - x0, Y - y0] += 1
    return hits, seen, steps
