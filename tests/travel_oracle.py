"""Scalar oracle of rbpf_travel_cost (include/rbpf_hip.h) on a rendered raster: the clearance by its closed
form over every offset, the cost by Dijkstra with heapq, the same start, goal and traversable-set rules.  It shares nothing with
the kernels' method (nearest occupied cell per row, block relaxation).

The raster is the box grown by m = margin(clear_max) cells on every side (ParticleEngine.render_map of the grown box: 0 outside
the tiles and outside the lattice), so that occupied cells outside the box count as the specification demands."""
import heapq

import numpy as np

AXIAL, DIAGONAL = 5, 7
NEIGHBOURS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]


def margin(clear_max):
    return (int(clear_max) + 4) // 5


def grown_box(box, clear_max):
    m = margin(clear_max)
    return (box[0] - m, box[1] + m, box[2] - m, box[3] + m)


def cells_of(xy, inv):
    """[n, 2] int64 mosaic cells of points in metres: floor(x * inv) in float64."""
    return np.floor(np.asarray(xy, dtype=np.float64).reshape(-1, 2) * np.float64(inv)).astype(np.int64)


def clearance(grown, clear_max, quantum, occupied_threshold):
    """uint16 [nx, ny] of the box inside `grown`: min(d, clear_max), d = min over occupied cells of 5 max + 2 min."""
    m = margin(clear_max)
    g = np.asarray(grown)
    occ = g.astype(np.float64) * float(quantum) > float(occupied_threshold)
    nx, ny = g.shape[0] - 2 * m, g.shape[1] - 2 * m
    out = np.full((nx, ny), int(clear_max), np.int64)
    for dx in range(-m, m + 1):
        for dy in range(-m, m + 1):
            w = AXIAL * max(abs(dx), abs(dy)) + (DIAGONAL - AXIAL) * min(abs(dx), abs(dy))
            if w >= clear_max:
                continue
            o = occ[m + dx:m + dx + nx, m + dy:m + dy + ny]
            out[o] = np.minimum(out[o], w)
    return out.astype(np.uint16)


def traversable(grown, clear, inflate, clear_max, quantum, occupied_threshold, start_cells, through_unknown=False):
    """bool [nx, ny]: T of the specification; start_cells are box-relative (i, j), those outside the box are ignored."""
    m = margin(clear_max)
    nx, ny = clear.shape
    v = np.asarray(grown)[m:m + nx, m:m + ny].astype(np.int64)
    blocked = (v.astype(np.float64) * float(quantum) > float(occupied_threshold)) if through_unknown else v >= 0
    T = ~blocked & (clear.astype(np.int64) > int(inflate))
    for i, j in start_cells:
        if 0 <= i < nx and 0 <= j < ny:
            T[i, j] = True
    return T


def dijkstra(T, start_cells):
    """int32 [nx, ny]: shortest 5 / 7 path cost over T from any start cell, corners not cut, -1 where there is none."""
    nx, ny = T.shape
    INF = 1 << 60
    dist = [[INF] * ny for _ in range(nx)]
    t = T.tolist()
    heap = []
    for i, j in start_cells:
        if 0 <= i < nx and 0 <= j < ny and dist[i][j] != 0:
            dist[i][j] = 0
            heap.append((0, int(i), int(j)))
    heapq.heapify(heap)
    while heap:
        d, i, j = heapq.heappop(heap)
        if d != dist[i][j]:
            continue
        for di, dj in NEIGHBOURS:
            a, b = i + di, j + dj
            if not (0 <= a < nx and 0 <= b < ny) or not t[a][b]:
                continue
            if di and dj and not (t[a][j] and t[i][b]):
                continue
            nd = d + (DIAGONAL if di and dj else AXIAL)
            if nd < dist[a][b]:
                dist[a][b] = nd
                heapq.heappush(heap, (nd, a, b))
    out = np.array(dist, dtype=np.int64)
    out[out >= INF] = -1
    return out.astype(np.int32)


def travel(grown, box, inv, quantum, occupied_threshold, starts_xy, goals_xy, inflate, clear_max, through_unknown=False):
    """(cost int32 [nx, ny], clearance uint16 [nx, ny], goal_cost int32 [n_goals]) of rbpf_travel_cost for one map.
    `grown` is the raster of grown_box(box, clear_max); starts_xy / goals_xy are in metres."""
    assert 0 <= inflate < clear_max <= 320
    nx, ny = box[1] - box[0], box[3] - box[2]
    m = margin(clear_max)
    assert np.asarray(grown).shape == (nx + 2 * m, ny + 2 * m)
    origin = np.array([box[0], box[2]])
    s = [tuple(int(q) for q in c) for c in cells_of(starts_xy, inv) - origin]
    clear = clearance(grown, clear_max, quantum, occupied_threshold)
    T = traversable(grown, clear, inflate, clear_max, quantum, occupied_threshold, s, through_unknown)
    cost = dijkstra(T, s)
    goal = np.full(0 if goals_xy is None else len(np.asarray(goals_xy).reshape(-1, 2)), -1, np.int32)
    if goals_xy is not None:
        for k, (i, j) in enumerate(cells_of(goals_xy, inv) - origin):
            if 0 <= i < nx and 0 <= j < ny:
                goal[k] = cost[i, j]
    return cost, clear, goal
