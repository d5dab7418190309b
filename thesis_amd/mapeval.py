"""How good is a map?  Particles' maps scored against a reference map (ParticleEngine.score_maps; include/rbpf_hip.h,
rbpf_score_maps): against a known truth, against another particle's map, against the filter's consensus.

The counting runs on the GPU and gives exact integers; everything here is host float64 arithmetic on those few integers per
particle, and says so where it rounds (consensus).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Tuple

import numpy as np

from .mapio import MapRaster, SourceMap, cells_from_probability, placed_box

F, U, O = 0, 1, 2                     # the classes of a lattice value: free (v < 0), unknown (neither), occupied (past the threshold)
LOWER_IS_BETTER = ("mean_abs_logodds", "entropy_bits")


def _ratio(num, den) -> np.ndarray:
    """num / den in float64, NaN where den == 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


@dataclass
class MapScores:
    """The integers of rbpf_score_maps for one particle (scalars, n [3, 3]) or for every particle (leading axis P): n[a, b]
    counts the cells of `box` with the map in class a and the reference in class b (F, U, O = 0, 1, 2); hit_m / hit_r the
    occupied cells of the map / of the reference with an occupied cell of the other within `tol` cells; l1 the sum of |v - r|
    in units of `quantum`; tab the table sum (with explore.entropy_table: 65536 x bits).  Every method returns float64, NaN
    where its denominator is 0."""
    n: np.ndarray
    hit_m: np.ndarray
    hit_r: np.ndarray
    l1: np.ndarray
    tab: np.ndarray
    box: Tuple[int, int, int, int]
    tol: int
    quantum: float

    @classmethod
    def from_fields(cls, fields, box, tol: int, quantum: float) -> "MapScores":
        """From the [..., 13] int64 rows of rbpf_score_maps (numpy, or a torch tensor)."""
        f = np.asarray(fields.cpu() if hasattr(fields, "cpu") else fields, dtype=np.int64)
        if f.shape[-1] != 13:
            raise ValueError("score rows have 13 fields")
        return cls(n=f[..., :9].reshape(f.shape[:-1] + (3, 3)).copy(), hit_m=f[..., 9].copy(), hit_r=f[..., 10].copy(),
                   l1=f[..., 11].copy(), tab=f[..., 12].copy(), box=tuple(int(x) for x in box), tol=int(tol), quantum=float(quantum))

    def cells(self) -> int:
        return (self.box[1] - self.box[0]) * (self.box[3] - self.box[2])

    def precision(self) -> np.ndarray:
        """The share of the map's occupied cells that the reference confirms within tol."""
        return _ratio(self.hit_m, self.n[..., O, :].sum(-1))

    def recall(self) -> np.ndarray:
        """The share of the reference's occupied cells that the map has found within tol."""
        return _ratio(self.hit_r, self.n[..., :, O].sum(-1))

    def f1(self) -> np.ndarray:
        p, r = self.precision(), self.recall()
        return _ratio(2.0 * p * r, p + r)              # NaN stays NaN; p + r == 0 is NaN

    def _known(self) -> np.ndarray:
        return self.n[..., F, F] + self.n[..., F, O] + self.n[..., O, F] + self.n[..., O, O]

    def accuracy(self) -> np.ndarray:
        """Of the cells known (free or occupied) on both sides, the share on which they agree."""
        return _ratio(self.n[..., F, F] + self.n[..., O, O], self._known())

    def coverage(self) -> np.ndarray:
        """Of the cells the reference knows, the share the map knows too."""
        return _ratio(self._known(), self.n[..., :, F].sum(-1) + self.n[..., :, O].sum(-1))

    def entropy_bits(self) -> np.ndarray:
        return np.asarray(self.tab, dtype=np.float64) / 65536.0

    def mean_abs_logodds(self) -> np.ndarray:
        return _ratio(np.asarray(self.l1, dtype=np.float64) * self.quantum, self.cells())


def _lattice_bounds(cfg) -> Tuple[float, float, float]:
    return float(cfg.quantum), float(cfg.min_odds_emp), float(cfg.max_odds_occ)


def consensus_from_probability(raster: MapRaster, cfg) -> MapRaster:
    """A whole-filter raster's `prob` turned back into lattice values: clip(rint(logit(prob) / quantum), vmin, vmax), exactly 0
    where prob == 0.5.  Host float64 math on float32 probabilities: the result is a rounding, not a count - but a probability
    that is sigma(v quantum) of one lattice value v, rounded to float32, gives that v back (the step between neighbouring
    values is 10^4 times the error of the round trip)."""
    if raster.prob is None:
        raise ValueError("the raster has no prob")
    q, lo, hi = _lattice_bounds(cfg)
    return MapRaster(x0=raster.x0, y0=raster.y0, cell_size=raster.cell_size, quantum=raster.quantum, dim=raster.dim,
                     tile_len=raster.tile_len, cells=cells_from_probability(raster.prob, q, lo, hi))


def consensus(engine, weights=None, box=None) -> MapRaster:
    """The filter's weighted mean map (render_map(None, weights=...)) as a MapRaster of lattice values over `box` (default
    map_extent(None)): see consensus_from_probability.  A filter whose particles all hold one map gets that map back exactly."""
    return consensus_from_probability(engine.render_map(None, box=box, weights=weights, fields=("prob",)), engine.cfg)


def against_consensus(engine, weights=None, tol_cells: int = 1) -> MapScores:
    """Every particle's map against the consensus of all of them: which particle agrees most with the rest."""
    return engine.score_maps(consensus(engine, weights), tol_cells=tol_cells)


def against_particle(engine, ref_particle="best", tol_cells: int = 1) -> MapScores:
    """Every particle's map against the map of `ref_particle` (an index or "best") over map_extent(None).  The reference is
    rendered to device memory and read there: no raster crosses to the host."""
    box = engine.map_extent(None)
    if box is None:
        raise ValueError("no particle has a map")
    ref = engine.render_map(ref_particle, box=box, device=True)
    return engine.score_maps(ref.cells, box=box, tol_cells=tol_cells)


def against_truth(engine, src: SourceMap, tol_cells: int = 1, samples: int = 4, particle=None) -> MapScores:
    """The maps of `particle` (None: every particle) against the known map `src`, resampled onto the engine's cells with
    warp_map over the union of its cover and the filter's extent; cells `src` does not cover are unknown in the reference.
    With align_map's pose through SourceMap.moved, a map of unknown pose can be scored too."""
    cell = float(engine.cfg.tile_len_m) / engine.dim
    box = placed_box(src, cell, engine.dim, int(engine.cfg.lattice_radius))
    ext = engine.map_extent(None)
    if ext is not None:
        box = ext if box[0] == box[1] or box[2] == box[3] else (min(box[0], ext[0]), max(box[1], ext[1]), min(box[2], ext[2]), max(box[3], ext[3]))
    warped, _, box = engine.warp_map(src, box=box, samples=samples)
    return engine.score_maps(warped, particle=particle, box=box, tol_cells=tol_cells)


def rank(scores: MapScores, key: str = "f1") -> np.ndarray:
    """Particle indices, best first, by the method of MapScores named `key`: larger is better, except for LOWER_IS_BETTER.
    Ties go to the lower index, NaN comes last."""
    val = np.atleast_1d(np.asarray(getattr(scores, key)(), dtype=np.float64))
    if key in LOWER_IS_BETTER:
        val = -val
    nan = np.isnan(val)
    return np.lexsort((np.arange(val.size), -np.where(nan, 0.0, val), nan)).astype(np.int64)


class Spread(NamedTuple):
    disagreement: float               # weighted mean of 1 - accuracy
    mean_abs_logodds: float           # weighted mean of mean_abs_logodds


def spread(scores: MapScores, weights=None) -> Spread:
    """How far the particles' maps stand from the reference they were scored against (against_consensus, against_particle):
    the weighted means of 1 - accuracy and of mean_abs_logodds over the particles (`weights`: None for uniform, else one
    non-negative value per particle; particles whose value is NaN are left out of that mean).  Both are 0 exactly when every
    map equals the reference: after a resample that left one map, the gauge of particle depletion."""
    vals = [np.atleast_1d(1.0 - scores.accuracy()), np.atleast_1d(scores.mean_abs_logodds())]
    w = np.ones(vals[0].shape) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != vals[0].shape or (w < 0).any():
        raise ValueError("weights must be one non-negative value per particle")
    out = []
    for v in vals:
        ok = ~np.isnan(v)
        s = w[ok].sum()
        out.append(float((w[ok] * v[ok]).sum() / s) if s > 0 else float("nan"))
    return Spread(*out)
