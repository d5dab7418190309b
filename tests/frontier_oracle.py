"""Scalar oracle of rbpf_frontier_regions (include/rbpf_hip.h) on a rendered raster: the mask cell by cell, the
components by a queue flood fill in row-major seed order (so a region's label is its seed's L), table, rep and ordering as the
specification words them.  It shares nothing with the kernels' method (bit planes, minimum propagation in blocks, atomics).

The raster is the box grown by margin(clear) = max(clear, 1) cells on every side (ParticleEngine.render_map of the grown box: 0
outside the tiles and outside the lattice), so that the real map decides at the box edge as the specification demands."""
from collections import deque

import numpy as np

FIELDS = ("label", "size", "sum_dx", "sum_dy", "x_min", "x_max", "y_min", "y_max", "rep_X", "rep_Y")
NEIGHBOURS8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def margin(clear):
    return max(int(clear), 1)


def grown_box(box, clear):
    m = margin(clear)
    return (box[0] - m, box[1] + m, box[2] - m, box[3] + m)


def mask(grown, clear, quantum, occupied_threshold):
    """bool [nx, ny]: front(c) for the cells of the box inside `grown`."""
    m, k = margin(clear), int(clear)
    g = np.asarray(grown).astype(np.int64).tolist()
    nx, ny = len(g) - 2 * m, len(g[0]) - 2 * m
    occ = [[v * float(quantum) > float(occupied_threshold) for v in row] for row in g]
    out = np.zeros((nx, ny), bool)
    for i in range(nx):
        for j in range(ny):
            a, b = i + m, j + m
            if not g[a][b] < 0:
                continue
            if not (g[a - 1][b] == 0 or g[a + 1][b] == 0 or g[a][b - 1] == 0 or g[a][b + 1] == 0):
                continue
            if any(occ[a + di][b + dj] for di in range(-k, k + 1) for dj in range(-k, k + 1)):
                continue
            out[i, j] = True
    return out


def components(F):
    """(label int32 [nx, ny], members): label = L of the region's first cell in row-major order, -1 outside F; members = the
    cells (i, j) of every region, regions in seed order."""
    nx, ny = F.shape
    f = F.tolist()
    label = [[-1] * ny for _ in range(nx)]
    members = []
    for i in range(nx):
        for j in range(ny):
            if not f[i][j] or label[i][j] >= 0:
                continue
            seed = i * ny + j
            label[i][j] = seed
            cells, queue = [], deque([(i, j)])
            while queue:
                a, b = queue.popleft()
                cells.append((a, b))
                for da, db in NEIGHBOURS8:
                    p, q = a + da, b + db
                    if 0 <= p < nx and 0 <= q < ny and f[p][q] and label[p][q] < 0:
                        label[p][q] = seed
                        queue.append((p, q))
            members.append(cells)
    return np.array(label, dtype=np.int32).reshape(nx, ny), members


def region_row(cells, box):
    """The ten table entries of one region from its member cells (box-relative)."""
    ny = box[3] - box[2]
    size = len(cells)
    sum_dx, sum_dy = sum(c[0] for c in cells), sum(c[1] for c in cells)
    cx, cy = (2 * sum_dx + size) // (2 * size), (2 * sum_dy + size) // (2 * size)
    rep = min(cells, key=lambda c: ((c[0] - cx) ** 2 + (c[1] - cy) ** 2, c[0] * ny + c[1]))
    return [min(c[0] * ny + c[1] for c in cells), size, sum_dx, sum_dy,
            box[0] + min(c[0] for c in cells), box[0] + max(c[0] for c in cells),
            box[2] + min(c[1] for c in cells), box[2] + max(c[1] for c in cells), box[0] + rep[0], box[2] + rep[1]]


def regions(grown, box, clear, min_size, max_regions, quantum, occupied_threshold):
    """(label int32 [nx, ny], regions int64 [max_regions, 10], counts int32 [3]) of rbpf_frontier_regions for one map.
    `grown` is the raster of grown_box(box, clear)."""
    assert 0 <= clear <= 16 and min_size >= 1 and 1 <= max_regions <= 1024
    nx, ny = box[1] - box[0], box[3] - box[2]
    m = margin(clear)
    assert np.asarray(grown).shape == (nx + 2 * m, ny + 2 * m)
    F = mask(grown, clear, quantum, occupied_threshold)
    label, members = components(F)
    rows = [region_row(cells, box) for cells in members]
    kept = sorted((r for r in rows if r[1] >= min_size), key=lambda r: (-r[1], r[0]))[:max_regions]
    table = np.full((max_regions, 10), -1, np.int64)
    if kept:
        table[:len(kept)] = np.array(kept, dtype=np.int64)
    return label, table, np.array([int(F.sum()), len(rows), len(kept)], dtype=np.int32)
