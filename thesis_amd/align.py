"""Alignment of a map of unknown pose on the host: a SourceMap turned into the point set ``ParticleEngine.align_points``
scores, its rasters turned into poses for ``SourceMap.moved``, and the coarse-to-fine search of
``ParticleEngine.align_map``.  NumPy only; the search itself is a callable, so the same code drives the GPU and an oracle."""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple

import numpy as np

from . import locate
from .locate import Hypotheses, TWO_PI
from .mapio import SourceMap, inverse_pose

MAX_POINTS = 32767                                       # n_occ + n_free of one rbpf_align_points call


def _thin(idx: np.ndarray, cap: int) -> np.ndarray:
    """`idx` whole if it fits `cap`, else every ceil(n / cap)-th entry from the first; nothing when cap <= 0."""
    n = len(idx)
    if cap <= 0:
        return idx[:0]
    if n <= cap:
        return idx
    return idx[::-(-n // cap)]


def points_from_source(src: SourceMap, occupied_threshold: float, max_points: int = MAX_POINTS):
    """(occ_xy [n_occ, 2], free_xy [n_free, 2], anchor): the centres ((i + 0.5) cell, (j + 0.5) cell) of the source cells with
    v * quantum > occupied_threshold, and of those with v < 0, relative to the anchor a = the centre of the source raster
    (nsx cell / 2, nsy cell / 2), both in row-major order, float64 metres in the raster's own frame.  Thinning: the
    occupied cells are kept whole if they fit `max_points`, else every ceil(n / max_points)-th of them is taken, from the
    first; the free cells get the remaining budget by the same rule."""
    if not 1 <= int(max_points) <= MAX_POINTS:
        raise ValueError(f"max_points must lie in 1 .. {MAX_POINTS}")
    cells = np.asarray(src.cells.cpu() if hasattr(src.cells, "cpu") else src.cells)
    if cells.ndim != 2:
        raise ValueError("source cells must be 2-D [nsx][nsy]")
    cs = float(src.cell_size)
    anchor = (cells.shape[0] * cs / 2.0, cells.shape[1] * cs / 2.0)
    occ = np.flatnonzero((cells.astype(np.float64) * float(src.quantum) > float(occupied_threshold)).ravel())
    occ = _thin(occ, int(max_points))
    free = _thin(np.flatnonzero((cells < 0).ravel()), int(max_points) - len(occ))

    def centres(idx):
        i, j = np.divmod(idx, cells.shape[1])
        return np.stack([(i + 0.5) * cs - anchor[0], (j + 0.5) * cs - anchor[1]], axis=1).astype(np.float64).reshape(-1, 2)
    return centres(occ), centres(free), anchor


def compose(a, b) -> Tuple[float, float, float]:
    """The rigid transform "b, then a": q -> a(b(q))."""
    ax, ay, ath = (float(v) for v in a)
    bx, by, bth = (float(v) for v in b)
    c, s = math.cos(ath), math.sin(ath)
    return (ax + (c * bx - s * by), ay + (s * bx + c * by), ath + bth)


def pose_of(cell, rot: int, n_rot: int, cell_size: float, anchor, origin=(0.0, 0.0, 0.0)) -> Tuple[float, float, float]:
    """The rigid transform `pose` for SourceMap.moved that an alignment result stands for.  With theta = rot 2 pi / n_rot and
    C = ((X + 0.5) cell_size, (Y + 0.5) cell_size) the centre of `cell` = (X, Y), a point q of the raster's frame (corner of
    cell (0, 0) at 0) goes to R(theta)(q - anchor) + C, i.e. the raster's corner gets the pose T = (C - R(theta) anchor,
    theta).  The source places that corner at `origin`, so pose = T o inverse_pose(origin), and src.moved(pose).origin is
    T."""
    th = (int(rot) * TWO_PI) / int(n_rot)
    c, s = math.cos(th), math.sin(th)
    cx, cy = (int(cell[0]) + 0.5) * float(cell_size), (int(cell[1]) + 0.5) * float(cell_size)
    ax, ay = float(anchor[0]), float(anchor[1])
    return compose((cx - (c * ax - s * ay), cy - (s * ax + c * ay), th), inverse_pose(origin))


def hypotheses(best, rot, box, n_rot: int, cell_size: float, n_occ: int, n_free: int, k: int = 4,
               nms_cells: int = 10) -> Hypotheses:
    """locate.hypotheses of an align_points result: every cell is a candidate, so the scores are shifted by the bias
    2 n_free (score + 2 n_free >= 0) on the way in and back on the way out.  `poses` are cell centres and theta_rot (the pose
    of the point set's frame origin); n_used is n_occ (a score is at most 2 n_occ)."""
    bias = 2 * int(n_free)
    h = locate.hypotheses(np.asarray(best).astype(np.int64) + bias, rot, box, n_rot, cell_size, k=k, nms_cells=nms_cells,
                          n_used=int(n_occ))
    return h._replace(scores=h.scores - bias)


Search = Callable[..., Tuple[np.ndarray, np.ndarray]]    # (occ_xy, free_xy, box, n_rot, r_begin, r_count) -> (best, rot)


def refine_hypothesis(search: Search, occ_xy, free_xy, cell, n_rot: int, refine: int, limits) -> Tuple[int, int, int, int]:
    """The fine pass round one coarse hypothesis `cell` = (X, Y, r): n_rot * refine rotations, the window of the 2 refine + 1
    fine rotations within one coarse step of r (cut in two where it wraps past 0), the box of 5 x 5 cells round (X, Y)
    clipped to `limits` = (lo, hi) of the tile lattice.  Returns (X, Y, fine rotation, score) of the best fine pose: the
    largest score; on a tie the piece of smaller rotation indices, then the first cell in row-major order (with the smallest
    rotation that attains it there)."""
    X, Y, r = (int(v) for v in cell)
    nf = int(n_rot) * int(refine)
    lo, hi = int(limits[0]), int(limits[1])
    box = (max(X - 2, lo), min(X + 3, hi), max(Y - 2, lo), min(Y + 3, hi))
    first, count = r * refine - refine, min(2 * refine + 1, nf)
    pieces = [(first, count)] if first >= 0 and first + count <= nf else None
    if pieces is None:
        first %= nf
        head = nf - first
        pieces = [(0, count - head), (first, head)] if count > head else [(first, count)]
    found = None
    for r_begin, r_count in sorted(pieces):              # ascending rotation index: on a tie the earlier piece stays
        best, rot = search(occ_xy, free_xy, box, nf, r_begin, r_count)
        best, rot = np.asarray(best), np.asarray(rot)
        n = int(np.argmax(best))
        i, j = divmod(n, best.shape[1])
        cand = (box[0] + i, box[2] + j, int(rot[i, j]), int(best[i, j]))
        if found is None or cand[3] > found[3]:
            found = cand
    return found


def align_map(search: Search, src: SourceMap, occupied_threshold: float, cell_size: float, box, limits, k: int = 4,
              n_rot: int = 360, refine: int = 8, nms_cells: int = 10, max_points: int = MAX_POINTS) -> Hypotheses:
    """Coarse-to-fine alignment of `src` with the scorer `search`: a coarse pass over `box` at `n_rot` rotations, the `k`
    best hypotheses (hypotheses above), a fine pass round each (refine_hypothesis), and the result ordered by fine score
    (descending, coarse order on ties).  poses[n] is the transform for src.moved (pose_of); cells[n] = (X, Y, fine rotation
    of n_rot * refine); n_used = n_occ."""
    if int(refine) < 1 or int(n_rot) * int(refine) > 4096:
        raise ValueError("refine >= 1 and n_rot * refine <= 4096 are required")
    occ_xy, free_xy, anchor = points_from_source(src, occupied_threshold, max_points)
    if len(occ_xy) == 0:
        raise ValueError("the source holds no occupied cell: nothing to align")
    best, rot = search(occ_xy, free_xy, tuple(int(b) for b in box), int(n_rot), 0, int(n_rot))
    coarse = hypotheses(best, rot, box, n_rot, cell_size, len(occ_xy), len(free_xy), k=k, nms_cells=nms_cells)
    fine = [refine_hypothesis(search, occ_xy, free_xy, c, n_rot, refine, limits) for c in coarse.cells]
    order = sorted(range(len(fine)), key=lambda n: -fine[n][3])
    nf = int(n_rot) * int(refine)
    poses = np.array([pose_of(fine[n][:2], fine[n][2], nf, cell_size, anchor, src.origin) for n in order]).reshape(-1, 3)
    cells = np.array([fine[n][:3] for n in order], dtype=np.int64).reshape(-1, 3)
    scores = np.array([fine[n][3] for n in order], dtype=np.int64)
    return Hypotheses(poses, scores, cells, len(occ_xy))
