"""Where should the robot look next?  Candidate view poses on the frontier of a map, ranked by the map cells a scan taken
there would observe (ParticleEngine.view_gain; include/rbpf_hip.h, rbpf_view_gain), from single frontier cells
or from the frontier regions the GPU labels in every particle's map (ParticleEngine.frontier_regions).  Host side, NumPy only:
the GPU call is the work, this module turns a map into candidates and the gains into a ranking."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from .engine import particle_index


def entropy_table(cfg) -> np.ndarray:
    """int32 table over the lattice values vmin .. vmax (61 with the default constants): round(65536 H2(sigma(|v| quantum))),
    H2 the binary entropy in bits, sigma(o) = e^o / (1 + e^o) as in rbpf_render_map.  H2(sigma(o)) is even in o, so the table
    is formed from |v| and is symmetric to the last bit; v = 0 gives 65536, so view_gain's gain / 65536 reads as bits."""
    q = float(cfg.quantum)
    vmin, vmax = int(round(float(cfg.min_odds_emp) / q)), int(round(float(cfg.max_odds_occ) / q))
    out = np.empty(vmax - vmin + 1, np.int32)
    for v in range(vmin, vmax + 1):
        e = math.exp(abs(v) * q)
        p, r = e / (1.0 + e), 1.0 / (1.0 + e)
        out[v - vmin] = int(round(65536.0 * -(p * math.log2(p) + r * math.log2(r))))
    return out


def frontier_cells(raster) -> np.ndarray:
    """[n, 2] mosaic cells (X, Y), in row-major order, of the observed-free cells (v < 0) of a particle's raster
    (ParticleEngine.render_map) that have a 4-neighbour with v == 0.  Cells outside the raster are 0, as in the map."""
    c = np.pad(np.asarray(raster.cells), 1)
    unknown = c == 0
    near = unknown[:-2, 1:-1] | unknown[2:, 1:-1] | unknown[1:-1, :-2] | unknown[1:-1, 2:]
    ij = np.argwhere((c[1:-1, 1:-1] < 0) & near)
    return ij + np.array([int(raster.x0), int(raster.y0)])


def candidate_poses(raster, spacing_m: float = 1.0, n_headings: int = 8, clearance_cells: int = 4,
                    occupied_threshold: float = 1.0) -> np.ndarray:
    """[n, 3] view poses (x, y, theta) from a particle's raster: the frontier cells with no occupied cell
    (v quantum > occupied_threshold) within `clearance_cells` on either axis, thinned to the first one (row-major) of every
    `spacing_m` square, each at its cell centre and once per heading 2 pi k / n_headings."""
    cells = np.asarray(raster.cells)
    cell = float(raster.tile_len) / int(raster.dim)
    f = frontier_cells(raster)
    k = int(clearance_cells)
    occ = np.pad(cells * float(raster.quantum) > occupied_threshold, k)
    blocked = np.zeros(cells.shape, bool)
    for di in range(2 * k + 1):
        for dj in range(2 * k + 1):
            blocked |= occ[di:di + cells.shape[0], dj:dj + cells.shape[1]]
    f = f[~blocked[f[:, 0] - int(raster.x0), f[:, 1] - int(raster.y0)]]
    square = np.floor((f + 0.5) * cell / float(spacing_m)).astype(np.int64)
    _, first = np.unique(square, axis=0, return_index=True)
    xy = (f[np.sort(first)] + 0.5) * cell
    th = 2.0 * np.pi * np.arange(int(n_headings)) / int(n_headings)
    return np.concatenate([np.repeat(xy, len(th), axis=0), np.tile(th, len(xy))[:, None]], axis=1).reshape(-1, 3)


class NextViews(NamedTuple):
    poses: np.ndarray       # [k, 3] the best view poses, best first
    scores: np.ndarray      # [k] float64: expected gain in table units / 65536 (bits with the entropy table)
    order: np.ndarray       # [k] their indices among the candidates
    candidates: np.ndarray  # [n, 3] every candidate scored
    gain: np.ndarray        # view_gain's gain for them: [n], or [P, n] with particle=None


def rank(gain, weights=None, k: int = 8):
    """(order [k], scores [n]): scores = gain / 65536, for a [P, n] gain its weighted mean over the particles (uniform by
    default); order = the k best candidates, ties to the lower index."""
    g = np.asarray(gain, dtype=np.float64)
    if g.ndim == 2:
        w = np.ones(g.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
        g = (w[:, None] * g).sum(axis=0) / w.sum()
    scores = g / 65536.0
    return np.argsort(-scores, kind="stable")[:int(k)], scores


def next_view(engine, angles, particle="best", weights=None, k: int = 8, spacing_m: float = 1.0, n_headings: int = 8,
              clearance_cells: int = 4, max_range: Optional[float] = None, table=None) -> NextViews:
    """The k candidate poses whose scan would observe the most: candidates from the map of `particle` (an index or "best";
    with None the best particle's map), scored by view_gain in that map, or with particle=None in every particle's map and
    averaged with `weights` (uniform by default)."""
    src = particle_index(engine, "best" if particle is None else particle)
    cand = candidate_poses(engine.render_map(src), spacing_m, n_headings, clearance_cells, float(engine.cfg.occupied_threshold))
    if len(cand) == 0:
        raise ValueError("the map has no frontier cell with that clearance: nowhere to look")
    res = engine.view_gain(cand, angles, particle=None if particle is None else src, max_range=max_range, table=table)
    order, scores = rank(res.gain, weights, k)
    return NextViews(cand[order], scores[order], order, cand, res.gain)


class ReachableViews(NamedTuple):
    poses: np.ndarray       # [k', 3] the best reachable view poses, best first (k' <= k)
    scores: np.ndarray      # [k'] float64: expected gain in bits minus travel_weight times the expected way there in metres
    order: np.ndarray       # [k'] their indices among the candidates
    candidates: np.ndarray  # [n, 3] every candidate scored
    gain: np.ndarray        # view_gain's gain for them: [n], or [P, n] with particle=None
    goal_cost: np.ndarray   # travel_cost's goal_cost for them, same shape: chamfer units, -1 unreachable
    reach: np.ndarray       # [n] weighted share of the particles in whose map the candidate can be reached


def next_reachable_view(engine, angles, start, particle="best", weights=None, k: int = 8, radius_m: float = 0.2,
                        travel_weight: float = 0.0, min_reach: float = 0.5, spacing_m: float = 1.0, n_headings: int = 8,
                        clearance_cells: int = 4, max_range: Optional[float] = None, table=None,
                        through_unknown: bool = False) -> ReachableViews:
    """next_view with the way there: candidates as in next_view, scored by view_gain as there, and travel_cost from `start`
    ((x, y, ...) in metres; with particle=None also [P, 2+], start n in particle n's map) to each of them with walls inflated by
    `radius_m`.  reach = the weighted share of particles in whose map the candidate has a cost >= 0; candidates with
    reach < min_reach are dropped; score = gain in bits - travel_weight * (weighted mean of the cost in metres over the
    particles that reach it).  The k best are returned, ties to the lower index; none if no candidate can be reached."""
    from .plan import cost_metres
    src = particle_index(engine, "best" if particle is None else particle)
    cand = candidate_poses(engine.render_map(src), spacing_m, n_headings, clearance_cells, float(engine.cfg.occupied_threshold))
    if len(cand) == 0:
        raise ValueError("the map has no frontier cell with that clearance: nowhere to look")
    which = None if particle is None else src
    gain = np.asarray(engine.view_gain(cand, angles, particle=which, max_range=max_range, table=table).gain)
    tr = engine.travel_cost(start, goals=cand[:, :2], particle=which, radius_m=radius_m, through_unknown=through_unknown)
    goal_cost = np.asarray(tr.goal_cost)
    g2, c2 = np.atleast_2d(gain).astype(np.float64), np.atleast_2d(goal_cost)
    w = np.ones(g2.shape[0]) if weights is None or g2.shape[0] == 1 else np.asarray(weights, dtype=np.float64)
    ok = c2 >= 0
    wsum = (w[:, None] * ok).sum(axis=0)
    reach = wsum / w.sum()
    metres = (w[:, None] * np.where(ok, np.nan_to_num(cost_metres(c2, tr.cell)), 0.0)).sum(axis=0) / np.where(wsum > 0, wsum, 1.0)
    scores = (w[:, None] * g2).sum(axis=0) / w.sum() / 65536.0 - float(travel_weight) * metres
    keep = (reach >= float(min_reach)) & (wsum > 0)
    order = np.argsort(np.where(keep, -scores, np.inf), kind="stable")[:int(k)]
    order = order[keep[order]]
    return ReachableViews(cand[order], scores[order], order, cand, gain, goal_cost, reach)


# ---- frontier regions (ParticleEngine.frontier_regions; include/rbpf_hip.h, rbpf_frontier_regions) -----------------
REGION_FIELDS = ("label", "size", "sum_dx", "sum_dy", "x_min", "x_max", "y_min", "y_max", "rep_X", "rep_Y")
REGION_DTYPE = np.dtype([(name, np.int64) for name in REGION_FIELDS])


class Frontiers(NamedTuple):
    label: Optional[np.ndarray]  # int32 [x1-x0, y1-y0]: the smallest dx * ny + dy of the cell's region, -1 off the frontier; or None
    regions: np.ndarray     # REGION_DTYPE [max_regions], or [P, max_regions] with particle=None: largest first, -1 past the last
    counts: np.ndarray      # int32 [3] or [P, 3]: frontier cells, regions, regions in the table
    box: tuple              # (x0, x1, y0, y1) in mosaic cells
    cell: float             # metres per cell


def region_poses(fr: Frontiers, n_headings: int = 8) -> np.ndarray:
    """[n_kept * n_headings, 3] view poses (x, y, theta) of one particle's Frontiers: the centre of every kept region's rep
    cell, once per heading 2 pi k / n_headings, regions in the table's order."""
    if np.ndim(fr.counts) != 1:
        raise ValueError("region_poses takes the Frontiers of one particle")
    r = fr.regions[:int(fr.counts[2])]
    xy = (np.stack([r["rep_X"], r["rep_Y"]], axis=1) + 0.5) * float(fr.cell)
    th = 2.0 * np.pi * np.arange(int(n_headings)) / int(n_headings)
    return np.concatenate([np.repeat(xy, len(th), axis=0), np.tile(th, len(xy))[:, None]], axis=1).reshape(-1, 3)


class PosteriorRegions(NamedTuple):
    cells: np.ndarray       # [n, 2] int64 mosaic cells (X, Y): one per square
    support: np.ndarray     # [n] float64: weighted share of the particles with a rep cell in the square
    size: np.ndarray        # [n] int64: the largest region any particle proposed there


def posterior_regions(fr_all: Frontiers, weights=None, spacing_m: float = 1.0, min_support: float = 0.0,
                      max_candidates: int = 256) -> PosteriorRegions:
    """Pools the rep cells of every particle's kept regions (Frontiers of particle=None) into squares of `spacing_m`, the
    squares of candidate_poses.  The support of a square is the weighted share (`weights`, uniform by default) of the particles
    with at least one rep in it; its cell is the rep proposed with the largest weight sum, ties to the smaller (X, Y).  Squares
    with support >= min_support come back by support descending, ties row-major, at most `max_candidates` of them."""
    counts = np.asarray(fr_all.counts)
    if counts.ndim != 2:
        raise ValueError("posterior_regions takes the Frontiers of particle=None")
    P, K = fr_all.regions.shape
    w = np.ones(P) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (P,):
        raise ValueError(f"weights must have shape ({P},)")
    pidx, kidx = np.nonzero(np.arange(K)[None, :] < counts[:, 2:3])
    r = fr_all.regions[pidx, kidx]
    XY = np.stack([r["rep_X"], r["rep_Y"]], axis=1).astype(np.int64).reshape(-1, 2)
    if len(XY) == 0:
        return PosteriorRegions(np.zeros((0, 2), np.int64), np.zeros(0), np.zeros(0, np.int64))
    square = np.floor((XY + 0.5) * float(fr_all.cell) / float(spacing_m)).astype(np.int64)
    _, s = np.unique(square, axis=0, return_inverse=True)                  # squares in row-major order
    s = s.reshape(-1)
    n = int(s.max()) + 1
    support = np.zeros(n)
    sp = np.unique(np.stack([s, pidx], axis=1), axis=0)                    # a particle counts once per square
    np.add.at(support, sp[:, 0], w[sp[:, 1]])
    support /= w.sum()
    size = np.zeros(n, np.int64)
    np.maximum.at(size, s, r["size"].astype(np.int64))
    cp = np.unique(np.concatenate([s[:, None], XY, pidx[:, None]], axis=1), axis=0)   # and once per cell
    cells, c = np.unique(cp[:, :3], axis=0, return_inverse=True)           # (square, X, Y), sorted
    wsum = np.zeros(len(cells))
    np.add.at(wsum, c.reshape(-1), w[cp[:, 3]])
    best = np.lexsort((cells[:, 2], cells[:, 1], -wsum, cells[:, 0]))      # per square: weight descending, then (X, Y)
    first = best[np.unique(cells[best, 0], return_index=True)[1]]
    keep = np.nonzero(support >= float(min_support))[0]
    order = keep[np.argsort(-support[keep], kind="stable")][:int(max_candidates)]
    return PosteriorRegions(cells[first][order, 1:], support[order], size[order])


class FrontierViews(NamedTuple):
    poses: np.ndarray       # [k, 3] the best view poses, best first
    scores: np.ndarray      # [k] float64: expected gain in table units / 65536 (bits with the entropy table)
    order: np.ndarray       # [k] their indices among the candidates
    candidates: np.ndarray  # [n, 3] every candidate scored
    gain: np.ndarray        # view_gain's gain for them: [n], or [P, n] with particle=None
    size: np.ndarray        # [k] cells of the frontier region a pose stands for (with particle=None the largest proposed there)
    support: np.ndarray     # [k] weighted share of the particles that propose it (1 with one particle)


def next_frontier_view(engine, angles, particle="best", weights=None, k: int = 8, min_size: int = 4, max_regions: int = 64,
                       n_headings: int = 8, clearance_cells: int = 4, spacing_m: float = 1.0, min_support: float = 0.0,
                       max_range: Optional[float] = None, table=None) -> FrontierViews:
    """next_view with regions for candidates: the rep cells of the frontier regions of at least `min_size` cells
    (ParticleEngine.frontier_regions) of `particle` (an index or "best"), scored by view_gain in that map.  particle=None: the
    regions of EVERY particle's map, pooled by posterior_regions with `weights` (uniform by default), so that a frontier the best
    map lacks is proposed too, scored in every map and averaged."""
    which = particle_index(engine, particle)
    th = 2.0 * np.pi * np.arange(int(n_headings)) / int(n_headings)
    if particle is None:
        fr = engine.frontier_regions(None, clearance_cells=clearance_cells, min_size=min_size, max_regions=max_regions, labels=False)
        pr = posterior_regions(fr, weights, spacing_m, min_support)
        xy = (pr.cells + 0.5) * float(fr.cell)
        cand = np.concatenate([np.repeat(xy, len(th), axis=0), np.tile(th, len(xy))[:, None]], axis=1).reshape(-1, 3)
        size, support, which = pr.size, pr.support, None
    else:
        fr = engine.frontier_regions(which, clearance_cells=clearance_cells, min_size=min_size, max_regions=max_regions, labels=False)
        cand = region_poses(fr, n_headings)
        size = np.asarray(fr.regions["size"][:int(fr.counts[2])], dtype=np.int64)
        support = np.ones(len(size))
    if len(cand) == 0:
        raise ValueError("the map has no frontier region of that size and clearance: nowhere to look")
    res = engine.view_gain(cand, angles, particle=which, max_range=max_range, table=table)
    order, scores = rank(res.gain, weights, k)
    return FrontierViews(cand[order], scores[order], order, cand, res.gain, size[order // len(th)], support[order // len(th)])
