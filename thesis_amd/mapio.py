"""Rendered occupancy maps (ParticleEngine.render_map) and their export to the common 2-D occupancy-map format: an 8-bit
binary PGM image and a YAML file with its resolution, origin and thresholds, as standard map tools read them.

Rasters are indexed in mosaic cells (include/rbpf_hip.h, rbpf_render_map): element [X - x0][Y - y0] is the cell whose
world square is [X cs, (X+1) cs) x [Y cs, (Y+1) cs) when dim cs equals the tile length.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np


@dataclass
class MapRaster:
    """A dense map of the cells [x0, x0 + nx) x [y0, y0 + ny).  One particle's map has `cells` (int8, units of `quantum`);
    the whole filter's has `prob` (weighted mean occupancy probability) and / or `occ_frac` (weight share that calls the
    cell occupied), float32.  Fields not asked for are None.  Arrays are numpy, or torch tensors on the GPU."""
    x0: int
    y0: int
    cell_size: float
    quantum: float
    dim: int                          # cells per tile edge
    tile_len: float                   # tile edge in metres
    cells: Optional[Any] = None
    prob: Optional[Any] = None
    occ_frac: Optional[Any] = None


def resample_weights(weights) -> np.ndarray:
    """The distribution the reference resamples from (main.py:52-56): -inf -> 0, then, if the smallest weight is
    negative, its magnitude is added to every non-zero weight."""
    w = np.array(weights, dtype=np.float64)
    w[w == -np.inf] = 0.0
    if len(w) and w.min() < 0:
        w[w != 0] += abs(w.min())
    return w


def _host(a) -> np.ndarray:
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def occupancy_probability(raster: MapRaster) -> np.ndarray:
    """[nx][ny] float64 probability that a cell is occupied: `prob`, or sigma(v quantum) of a single particle's cells
    (get_pr_at, hybridmap.py:74-83)."""
    if raster.prob is not None:
        return _host(raster.prob).astype(np.float64)
    if raster.cells is not None:
        e = np.exp(_host(raster.cells).astype(np.float64) * raster.quantum)
        return e / (1.0 + e)
    raise ValueError("the raster has neither prob nor cells")


def write_occupancy_map(stem: str, raster: MapRaster, occupied_thresh: float = 0.65, free_thresh: float = 0.196):
    """Writes `stem`.pgm (binary P5, 8 bit, pixel = round(255 (1 - p)), row 0 = largest Y) and `stem`.yaml.
    Returns the two paths."""
    if abs(raster.dim * raster.cell_size - raster.tile_len) > 1e-9 * raster.tile_len:
        raise ValueError(f"dim * cell_size = {raster.dim * raster.cell_size!r} differs from the tile length "
                         f"{raster.tile_len!r}: the mosaic of such tiles is not a world grid")
    p = occupancy_probability(raster)
    if p.ndim != 2:
        raise ValueError("raster arrays must be 2-D [nx][ny]")
    pix = np.clip(np.rint(255.0 * (1.0 - p)), 0, 255).astype(np.uint8)
    img = np.ascontiguousarray(pix.T[::-1, :])          # rows: Y from y0 + ny - 1 down to y0; columns: X from x0
    pgm, yml = stem + ".pgm", stem + ".yaml"
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())
    cs = float(raster.cell_size)
    with open(yml, "w") as f:
        f.write(f"image: {os.path.basename(pgm)}\n")
        f.write(f"resolution: {cs!r}\n")
        f.write(f"origin: [{float(raster.x0 * cs)!r}, {float(raster.y0 * cs)!r}, 0.0]\n")
        f.write("negate: 0\n")
        f.write(f"occupied_thresh: {float(occupied_thresh)!r}\n")
        f.write(f"free_thresh: {float(free_thresh)!r}\n")
    return pgm, yml
