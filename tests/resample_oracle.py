"""NumPy model of what a resample MOVES (main.py:68-79 with Robot.copy, robot.py:141-149; kernels_resample.hip): given the state
before, the ancestors and whether the trigger fired, the state after - poses, covariances, weights and each particle's whole
tile set - and the two counters that follow from it.  It knows nothing of slots, jobs, boxes or the pool: a new particle simply
has what its ancestor had.  tests/test_resample_oracle.py ties it to oracle.rbpf_oracle.resample on deep copies of OracleRobot.

Beside the model: the geometry a test needs to look at a map through the engine's public calls - the written box of a tile,
a particle's extent and its mosaic raster (the coordinates of rbpf_map_extent / rbpf_render_map) - and the bytes one copy job
moves, from the written boxes alone (include/rbpf_hip.h: bytes_copied)."""
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

Centre = Tuple[float, float]
Tiles = Dict[Centre, np.ndarray]                         # tile centre (metres) -> int8 cells [dim, dim] indexed [x][y]
Box = Optional[Tuple[int, int, int, int]]                # tile-local written box (x0, x1, y0, y1), inclusive; None: nothing written


class Moved(NamedTuple):
    poses: np.ndarray          # [P, 3]
    covs: np.ndarray           # [P, 3, 3]
    weights: np.ndarray        # [P]
    maps: List[Tiles]          # new particle j holds the tiles of idx[j] (the same objects: treat them as read-only)
    tiles_in_use: int          # sum over the new particles of their tile counts
    copies: int                # increment of resample_copies: the tiles of every j whose ancestor is that of j - 1


def move(poses, covs, weights, maps: Sequence[Tiles], idx, did: bool) -> Moved:
    poses, covs, weights = np.asarray(poses, np.float64), np.asarray(covs, np.float64), np.asarray(weights, np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    P = len(idx)
    assert poses.shape == (P, 3) and covs.shape == (P, 3, 3) and weights.shape == (P,) and len(maps) == P
    assert idx.min() >= 0 and idx.max() < P and np.all(np.diff(idx) >= 0)
    new_maps = [maps[i] for i in idx]
    copies = sum(len(maps[idx[j]]) for j in copy_destinations(idx))
    return Moved(poses[idx].copy(), covs[idx].copy(), np.ones(P) if did else weights.copy(), new_maps,
                 sum(len(m) for m in new_maps), copies)


def copy_destinations(idx) -> List[int]:
    """The new particles that are copies (main.py:70-74): those whose ancestor is also the ancestor of the one before."""
    idx = np.asarray(idx)
    return [int(j) for j in np.nonzero(idx[1:] == idx[:-1])[0] + 1]


# ---- looking at a map -----------------------------------------------------------------------------------------------------------
def written_box(cells) -> Box:
    """The box of the non-zero cells of a tile."""
    rows, cols = np.nonzero(np.any(cells, axis=1))[0], np.nonzero(np.any(cells, axis=0))[0]
    return None if len(rows) == 0 else (int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1]))


def tile_origin(centre: Centre, dim: int, tile_len: float) -> Tuple[int, int]:
    """Mosaic cell of the tile's cell (0, 0): the tile centred (0, 0) covers the mosaic cells -dim/2 .. dim/2 - 1."""
    a, b = round(centre[0] / tile_len), round(centre[1] / tile_len)
    return a * dim - dim // 2, b * dim - dim // 2


def extent(tiles: Tiles, dim: int, tile_len: float, boxes: Optional[Dict[Centre, Box]] = None):
    """(x0, x1, y0, y1), half-open, mosaic cells: the smallest box holding the written boxes of all tiles, None without any.
    `boxes` gives the written boxes where they are known to be larger than the non-zero cells (a loaded raster's zeros)."""
    lo, hi = [None, None], [None, None]
    for c, cells in tiles.items():
        b = boxes[c] if boxes is not None else written_box(cells)
        if b is None:
            continue
        o = tile_origin(c, dim, tile_len)
        for k in range(2):
            p, q = o[k] + b[2 * k], o[k] + b[2 * k + 1] + 1
            lo[k] = p if lo[k] is None else min(lo[k], p)
            hi[k] = q if hi[k] is None else max(hi[k], q)
    return None if lo[0] is None else (lo[0], hi[0], lo[1], hi[1])


def mosaic(tiles: Tiles, box, dim: int, tile_len: float) -> np.ndarray:
    """int8 [x1-x0, y1-y0]: the cells of `box` (mosaic cells, half-open), 0 where the particle has no tile."""
    out = np.zeros((box[1] - box[0], box[3] - box[2]), dtype=np.int8)
    for c, cells in tiles.items():
        ox, oy = tile_origin(c, dim, tile_len)
        x0, x1, y0, y1 = max(box[0], ox), min(box[1], ox + dim), max(box[2], oy), min(box[3], oy + dim)
        if x0 < x1 and y0 < y1:
            out[x0 - box[0]:x1 - box[0], y0 - box[2]:y1 - box[2]] = cells[x0 - ox:x1 - ox, y0 - oy:y1 - oy]
    return out


# ---- the bytes a copy job moves ------------------------------------------------------------------------------------------------
def union(s: Box, d: Box) -> Box:
    if s is None or d is None:
        return s if d is None else d
    return (min(s[0], d[0]), max(s[1], d[1]), min(s[2], d[2]), max(s[3], d[3]))


def copy_bytes(src_boxes: Dict[Centre, Box], dst_boxes: Dict[Centre, Box], dim: int) -> int:
    """Read + written bytes of the copy of one particle's tiles over another's: per tile of the source the union of both
    written boxes (the destination's is empty where it has no tile), its columns rounded out to groups of 16, capped at dim."""
    total = 0
    for c, s in src_boxes.items():
        u = union(s, dst_boxes.get(c))
        if u is not None:
            ya, yb = u[2] // 16 * 16, min((u[3] // 16 + 1) * 16, dim)
            total += 2 * (u[1] - u[0] + 1) * (yb - ya)
    return total
