"""Paths from a travel-cost field (ParticleEngine.travel_cost; include/rbpf_hip.h, rbpf_travel_cost).  Host side,
NumPy only: the field is the work of the GPU, a path is a walk down it."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

AXIAL, DIAGONAL = 5, 7
# the order in which path_to tries the neighbours of a cell
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


class Travel(NamedTuple):
    cost: Optional[np.ndarray]       # int32 [x1-x0, y1-y0] chamfer units (5 per axial step), -1 unreachable; None with particle=None
    clearance: Optional[np.ndarray]  # uint16 [x1-x0, y1-y0] min(chamfer distance to the nearest occupied cell, clear_max); None likewise
    goal_cost: Optional[np.ndarray]  # int32 [n_goals], or [P, n_goals] with particle=None; None without goals
    rounds: int                      # relaxation rounds launched (a diagnostic)
    box: tuple                       # (x0, x1, y0, y1) in mosaic cells
    cell: float                      # metres per cell (tile_len / dim)
    inv: float                       # cells per metre as the engine forms it (dim / tile_len): a point lies in cell floor(x * inv)
    inflate: int                     # cells of T have clearance > inflate
    clear_max: int


def cost_metres(cost, cell: float):
    """Chamfer units -> metres (float64), NaN where the cost is -1."""
    c = np.asarray(cost)
    return np.where(c >= 0, c.astype(np.float64) * (float(cell) / AXIAL), np.nan)


def path_to(travel: Travel, goal_xy):
    """[k, 2] cell centres in metres from a start cell to the cell of `goal_xy` (metres), or None where its cost is -1 or it lies
    outside the box.  Walks down the field: from c to the first neighbour n, in the order of NEIGHBOURS, with cost[n] >= 0 and
    cost[n] + w == cost[c] (w = 5 axial, 7 diagonal; for a diagonal both side cells must have cost >= 0).  Such a
    neighbour exists wherever cost > 0: a traversable cell next to a reached one is reached, so cost >= 0 stands for "in T"."""
    cost = np.asarray(travel.cost)
    x0, _, y0, _ = travel.box
    g = np.floor(np.asarray(goal_xy, dtype=np.float64)[:2] * np.float64(travel.inv))
    i, j = int(g[0]) - x0, int(g[1]) - y0
    nx, ny = cost.shape
    if not (0 <= i < nx and 0 <= j < ny) or cost[i, j] < 0:
        return None
    cells = [(i, j)]
    while cost[i, j] > 0:
        for di, dj in NEIGHBOURS:
            a, b = i + di, j + dj
            if not (0 <= a < nx and 0 <= b < ny) or cost[a, b] < 0:
                continue
            if di and dj and (cost[a, j] < 0 or cost[i, b] < 0):
                continue
            if int(cost[a, b]) + (DIAGONAL if di and dj else AXIAL) == int(cost[i, j]):
                i, j = a, b
                break
        else:
            raise ValueError(f"cost field is no fixed point at cell {(i + x0, j + y0)}")
        cells.append((i, j))
    out = np.array(cells[::-1], dtype=np.float64) + np.array([x0 + 0.5, y0 + 0.5])
    return out * float(travel.cell)
