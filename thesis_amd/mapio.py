"""Rendered occupancy maps (ParticleEngine.render_map) and their export to the common 2-D occupancy-map format: an 8-bit
binary PGM image and a YAML file with its resolution, origin and thresholds, as standard map tools read them.

Rasters are indexed in mosaic cells (include/rbpf_hip.h, rbpf_render_map): element [X - x0][Y - y0] is the cell whose
world square is [X cs, (X+1) cs) x [Y cs, (Y+1) cs) when dim cs equals the tile length.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, replace
from typing import Any, Optional, Tuple

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


@dataclass
class SourceMap:
    """A map in a frame of its own, as ParticleEngine.place_map / warp_map resample it (include/rbpf_hip.h, rbpf_place_map):
    `cells` [nsx][nsy] int8 in units of `quantum` (numpy, or a torch tensor on the GPU), `cell_size` metres per cell, and
    `origin` = (x, y, yaw), the world pose of the corner of cell (0, 0) - the origin of the PGM + YAML map format.  Cell
    (i, j) covers [i, i+1) x [j, j+1) times cell_size in the frame at (x, y) rotated by yaw."""
    cells: Any
    cell_size: float
    origin: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    quantum: float = 0.1

    def moved(self, pose) -> "SourceMap":
        """The same map after the rigid transform `pose` = (x, y, theta) of the world: a point q goes to R(theta) q + (x, y),
        so the origin (ox, oy, yaw) becomes (x + cos(theta) ox - sin(theta) oy, y + sin(theta) ox + cos(theta) oy,
        yaw + theta).  With the pose relocalize found for yesterday's map frame, this puts that map into today's frame;
        inverse_pose(pose) undoes it."""
        x, y, th = (float(v) for v in pose)
        ox, oy, yaw = (float(v) for v in self.origin)
        c, s = math.cos(th), math.sin(th)
        return replace(self, origin=(x + (c * ox - s * oy), y + (s * ox + c * oy), yaw + th))


def inverse_pose(pose) -> Tuple[float, float, float]:
    """The rigid transform that undoes `pose` = (x, y, theta): (-(cos(theta) x + sin(theta) y), sin(theta) x - cos(theta) y,
    -theta)."""
    x, y, th = (float(v) for v in pose)
    c, s = math.cos(th), math.sin(th)
    return (-(c * x + s * y), s * x - c * y, -th)


def source_from_raster(raster: MapRaster) -> SourceMap:
    """A single particle's raster (MapRaster with int8 `cells`) as a SourceMap at origin (x0 cs, y0 cs, 0): what moves a map
    into an engine of another cell size, or - after moved() - into another frame."""
    if raster.cells is None:
        raise ValueError("the raster has no int8 cells (a whole-filter render has prob / occ_frac): convert them with "
                         "cells_from_probability first")
    cs = float(raster.cell_size)
    return SourceMap(cells=raster.cells, cell_size=cs, origin=(raster.x0 * cs, raster.y0 * cs, 0.0), quantum=float(raster.quantum))


def placed_box(src: SourceMap, cell_size: float, dim: int, lattice_radius: int) -> Tuple[int, int, int, int]:
    """(x0, x1, y0, y1), half-open, in mosaic cells of `cell_size`: the smallest box holding the four corners of the source,
    clipped to the tile lattice.  Corner (p, q) in {0, nsx} x {0, nsy} lies at
    (ox + cell (cos(yaw) p - sin(yaw) q), oy + cell (sin(yaw) p + cos(yaw) q)); x0 = floor(min x / cell_size),
    x1 = floor(max x / cell_size) + 1, the same in y; the lattice holds the mosaic cells [-R dim - dim // 2,
    (R + 1) dim - dim // 2) on both axes.  A source wholly outside the lattice gives an empty box."""
    nsx, nsy = (int(n) for n in src.cells.shape)
    ox, oy, yaw = (float(v) for v in src.origin)
    c, s, sc = math.cos(yaw), math.sin(yaw), float(src.cell_size)
    xs = [ox + sc * (c * p - s * q) for p in (0, nsx) for q in (0, nsy)]
    ys = [oy + sc * (s * p + c * q) for p in (0, nsx) for q in (0, nsy)]
    lo = -int(lattice_radius) * int(dim) - int(dim) // 2
    hi = lo + (2 * int(lattice_radius) + 1) * int(dim)
    out = []
    for v in (xs, ys):
        a = min(max(math.floor(min(v) / cell_size), lo), hi)
        b = min(max(math.floor(max(v) / cell_size) + 1, lo), hi)
        out += [a, max(a, b)]
    return tuple(out)


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


def cells_from_probability(p, quantum: float, vmin: float, vmax: float) -> np.ndarray:
    """int8 lattice values of occupancy probabilities: clip(rint(logit(p) / quantum)) to [vmin, vmax] / quantum (log-odds
    bounds, e.g. min_odds_emp and max_odds_occ).  The way to load a whole-filter `prob` raster into particles."""
    p = np.asarray(_host(p), dtype=np.float64)
    lo, hi = int(np.rint(vmin / quantum)), int(np.rint(vmax / quantum))
    if not (-128 <= lo <= 0 <= hi <= 127):
        raise ValueError(f"[vmin, vmax] / quantum = [{lo}, {hi}] must hold 0 and fit int8")
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.log(p) - np.log1p(-p)                     # +-inf at p = 1 / 0: clipped below
    if np.isnan(o).any():
        raise ValueError("probabilities must lie in [0, 1]")
    return np.clip(np.rint(o / quantum), lo, hi).astype(np.int8)


def _read_pgm(path: str) -> np.ndarray:
    """An 8-bit binary (P5) PGM image as uint8 [rows][columns]; `#` comments in the header are skipped."""
    with open(path, "rb") as f:
        data = f.read()
    fields, pos = [], 0
    while len(fields) < 4:
        while pos < len(data) and (data[pos:pos + 1].isspace() or data[pos:pos + 1] == b"#"):
            if data[pos:pos + 1] == b"#":                # a comment runs to the end of its line
                while pos < len(data) and data[pos:pos + 1] not in (b"\n", b"\r"):
                    pos += 1
            pos += 1
        end = pos
        while end < len(data) and not data[end:end + 1].isspace() and data[end:end + 1] != b"#":
            end += 1
        if end == pos:
            raise ValueError(f"{path}: truncated PGM header")
        fields.append(data[pos:end])
        pos = end
        if len(fields) == 1 and fields[0] != b"P5":
            raise ValueError(f"{path}: not a binary PGM (P5) image (magic {fields[0][:8]!r})")
    pos += 1                                             # the single whitespace byte after maxval
    try:
        w, h, maxval = int(fields[1]), int(fields[2]), int(fields[3])
    except ValueError:
        raise ValueError(f"{path}: malformed PGM header") from None
    if maxval != 255:
        raise ValueError(f"{path}: maxval {maxval}, only 8-bit images (255) are read")
    img = np.frombuffer(data, dtype=np.uint8, count=w * h, offset=pos) if len(data) - pos >= w * h else None
    if img is None:
        raise ValueError(f"{path}: {w} x {h} pixels announced, {len(data) - pos} bytes present")
    return img.reshape(h, w)


def _read_yaml(path: str) -> dict:
    """The flat `key: value` YAML of an occupancy map (numbers, strings, one-line [lists]); `#` starts a comment."""
    out = {}
    for line in open(path):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if ":" not in line:
            raise ValueError(f"{path}: cannot read line {line!r}")
        k, v = (x.strip() for x in line.split(":", 1))
        if v.startswith("[") and v.endswith("]"):
            out[k] = [float(x) for x in v[1:-1].split(",") if x.strip()]
        else:
            v = v.strip("\"'")
            try:
                out[k] = float(v)
            except ValueError:
                out[k] = v
    return out


def _read_map_meta(yaml_path: str):
    """The YAML of a map, its resolution and its origin [x, y, yaw]."""
    meta = _read_yaml(yaml_path)
    for k in ("image", "resolution", "origin"):
        if k not in meta:
            raise ValueError(f"{yaml_path}: no {k!r}")
    origin = list(meta["origin"])
    return meta, float(meta["resolution"]), origin


def _read_map_cells(meta: dict, yaml_path: str, quantum: float, vmin: float, vmax: float, mode: str) -> np.ndarray:
    """int8 cells [column][rows - 1 - row] of the map's image (image row 0 is the largest y of the map's frame)."""
    img_path = str(meta["image"])
    if not os.path.isabs(img_path):
        img_path = os.path.join(os.path.dirname(os.path.abspath(yaml_path)), img_path)
    pix = _read_pgm(img_path).astype(np.float64)
    p = pix / 255.0 if int(meta.get("negate", 0)) else (255.0 - pix) / 255.0
    p = np.ascontiguousarray(p[::-1, :].T)               # [X - x0][Y - y0]
    if mode == "scale":
        return cells_from_probability(p, quantum, vmin, vmax)
    occ_t, free_t = float(meta.get("occupied_thresh", 0.65)), float(meta.get("free_thresh", 0.196))
    cells = np.zeros(p.shape, dtype=np.int8)
    cells[p > occ_t] = int(np.rint(vmax / quantum))
    cells[p < free_t] = int(np.rint(vmin / quantum))
    return cells


def read_map_image(yaml_path: str, quantum: float, vmin: float, vmax: float, mode: str = "trinary") -> SourceMap:
    """Reads a map in the common PGM + YAML format, whatever its resolution (> 0), origin and yaw, into a SourceMap for
    ParticleEngine.place_map: cells[i][j] is the pixel of image column i and row (rows - 1 - j), cell_size the YAML's
    resolution, origin its [x, y, yaw].  `mode` as read_occupancy_map: "trinary" (the default: maps of other tools) or
    "scale"."""
    if mode not in ("scale", "trinary"):
        raise ValueError(f"unknown mode {mode!r}")
    meta, res, origin = _read_map_meta(yaml_path)
    if not (math.isfinite(res) and res > 0.0):
        raise ValueError(f"{yaml_path}: resolution {res!r} must be positive")
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"{yaml_path}: origin must be [x, y, yaw], finite")
    cells = _read_map_cells(meta, yaml_path, quantum, vmin, vmax, mode)
    return SourceMap(cells=cells, cell_size=res, origin=(float(origin[0]), float(origin[1]), float(origin[2])), quantum=float(quantum))


def read_occupancy_map(yaml_path: str, quantum: float, vmin: float, vmax: float, mode: str = "scale", *,
                       cell_size: float = 0.05, tile_len: float = 40.0) -> MapRaster:
    """Reads a map in the common PGM + YAML format into a MapRaster with int8 `cells` (units of `quantum`), ready for
    ParticleEngine.load_map.  x0 = origin x / resolution, y0 = origin y / resolution; image row 0 is the largest Y.
    mode "scale": the pixel's probability through cells_from_probability (write_occupancy_map's output round-trips
    exactly); "trinary": above occupied_thresh -> vmax, below free_thresh -> vmin, else 0 (for maps of other tools).
    Refused: a resolution other than `cell_size`, an origin off the cell grid, a non-zero yaw (read_map_image reads such
    maps, for ParticleEngine.place_map)."""
    if mode not in ("scale", "trinary"):
        raise ValueError(f"unknown mode {mode!r}")
    meta, res, origin = _read_map_meta(yaml_path)
    if abs(res - cell_size) > 1e-9 * cell_size:
        raise ValueError(f"{yaml_path}: resolution {res!r} differs from the cell size {cell_size!r} (maps are not resampled)")
    if len(origin) != 3:
        raise ValueError(f"{yaml_path}: origin must be [x, y, yaw]")
    if origin[2] != 0.0:
        raise ValueError(f"{yaml_path}: origin yaw {origin[2]!r}: only unrotated maps are read")
    x0f, y0f = origin[0] / res, origin[1] / res
    x0, y0 = int(round(x0f)), int(round(y0f))
    if abs(x0f - x0) > 1e-6 or abs(y0f - y0) > 1e-6:
        raise ValueError(f"{yaml_path}: origin ({origin[0]!r}, {origin[1]!r}) is not a whole number of cells")
    cells = _read_map_cells(meta, yaml_path, quantum, vmin, vmax, mode)
    dim = int(round(tile_len / cell_size))
    return MapRaster(x0=x0, y0=y0, cell_size=float(cell_size), quantum=float(quantum), dim=dim, tile_len=float(tile_len),
                     cells=cells)
