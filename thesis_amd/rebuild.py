"""The final map of a run, drawn again from a chosen trajectory and the logged scans (ParticleEngine.build_map;
include/rbpf_hip.h, rbpf_build_map).

The maps the particles carry were drawn one scan at a time at the pose each particle then believed, at the engine's cell size,
as clamped log-odds.  build_map returns, for any cell size, how often each cell was hit and how often it was seen; this module
keeps the scans (ScanLog), picks the poses (rebuild) and turns the counts into the rasters the rest of the package reads
(to_cells, as_raster, as_source, hit_ratio).  Everything here is host NumPy; the counting runs on the GPU.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .engine import BuiltMap
from .mapio import MapRaster, SourceMap

CHUNK = 4096           # scans per build_map call of rebuild()


def _host(a) -> np.ndarray:
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def sensor_model(engine=None, occ: Optional[int] = None, emp: Optional[int] = None, vmin: Optional[int] = None,
                 vmax: Optional[int] = None, quantum: Optional[float] = None) -> Tuple[int, int, int, int, Optional[float]]:
    """(occ, emp, vmin, vmax, quantum): what a hit and a miss add to a cell and the clamps, integers in units of `quantum`.
    Whatever is None comes from `engine`'s configuration: log_odds_occ, log_odds_emp, min_odds_emp, max_odds_occ, quantum."""
    if engine is None and None in (occ, emp, vmin, vmax):
        raise ValueError("give occ, emp, vmin and vmax, or an engine to take them from")
    if quantum is None:
        quantum = float(engine.cfg.quantum) if engine is not None else None   # to_cells needs none; as_raster / as_source do
    pick = lambda v, name: int(v) if v is not None else int(round(float(getattr(engine.cfg, name)) / quantum))
    occ, emp = pick(occ, "log_odds_occ"), pick(emp, "log_odds_emp")
    vmin, vmax = pick(vmin, "min_odds_emp"), pick(vmax, "max_odds_occ")
    if not (-128 <= vmin <= 0 <= vmax <= 127):
        raise ValueError(f"[vmin, vmax] = [{vmin}, {vmax}] must hold 0 and fit int8")
    return occ, emp, vmin, vmax, quantum if quantum is None else float(quantum)


def _quantum(engine, model) -> float:
    q = sensor_model(engine, **model)[4]
    if q is None:
        raise ValueError("give quantum, or an engine to take it from")
    return q


def to_cells(built: BuiltMap, occ: Optional[int] = None, emp: Optional[int] = None, vmin: Optional[int] = None,
             vmax: Optional[int] = None, quantum: Optional[float] = None, engine=None) -> np.ndarray:
    """The int8 log-odds raster of the counts: clip(hits * occ + (seen - hits) * emp, vmin, vmax), and 0 where seen == 0.  A
    scan that hit a cell adds occ, a scan that only saw it adds emp (sensor_model has the units and the defaults)."""
    occ, emp, vmin, vmax, _ = sensor_model(engine, occ, emp, vmin, vmax, quantum)
    hits, seen = _host(built.hits).astype(np.int64), _host(built.seen).astype(np.int64)
    v = np.clip(hits * occ + (seen - hits) * emp, vmin, vmax)
    v[seen == 0] = 0
    return v.astype(np.int8)


def hit_ratio(built: BuiltMap) -> np.ndarray:
    """hits / seen as float32, NaN where the cell was never seen: the count-map reading of the same data."""
    hits, seen = _host(built.hits), _host(built.seen)
    out = np.full(hits.shape, np.nan, dtype=np.float32)
    m = seen > 0
    out[m] = hits[m] / seen[m]
    return out


def as_raster(built: BuiltMap, tile_len: Optional[float] = None, engine=None, **model) -> MapRaster:
    """to_cells(built, **model) as a MapRaster on the world grid of the built cell size: tiles of `tile_len` metres (default the
    engine's) must hold a whole number of cells.  At the engine's own cell size it loads with load_map; at any admitted size it
    goes to mapio.write_occupancy_map and mapeval.against_truth."""
    if tile_len is None:
        if engine is None:
            raise ValueError("give tile_len, or an engine to take it from")
        tile_len = float(engine.cfg.tile_len_m)
    quantum = _quantum(engine, model)
    dim = int(round(tile_len * built.cells_per_m))
    if dim < 1 or abs(dim - tile_len * built.cells_per_m) > 1e-9 * dim:
        raise ValueError(f"a tile of {tile_len!r} m does not hold a whole number of {built.cell_size!r} m cells: use as_source")
    return MapRaster(x0=int(built.x0), y0=int(built.y0), cell_size=float(built.cell_size), quantum=quantum, dim=dim,
                     tile_len=float(tile_len), cells=to_cells(built, engine=engine, **model))


def as_source(built: BuiltMap, engine=None, **model) -> SourceMap:
    """to_cells(built, **model) as a SourceMap of any cell size, origin (x0 cs, y0 cs, 0): what place_map resamples into an
    engine and align_map matches."""
    quantum = _quantum(engine, model)
    cs = float(built.cell_size)
    return SourceMap(cells=to_cells(built, engine=engine, **model), cell_size=cs, origin=(built.x0 * cs, built.y0 * cs, 0.0), quantum=quantum)


class ScanLog:
    """The scans of a run on the host, each under the trajectory record (ParticleEngine.track) written for it.  Scans arrive
    from the host anyway; nothing about them needs the device until a rebuild.  Records must arrive in increasing order."""

    def __init__(self):
        self.records: List[int] = []
        self._ranges: List[np.ndarray] = []

    def __len__(self):
        return len(self.records)

    def append(self, record: int, ranges):
        r = np.array(ranges, dtype=np.float64).reshape(-1)
        if self._ranges and r.shape != self._ranges[0].shape:
            raise ValueError(f"a scan of {r.size} beams in a log of scans of {self._ranges[0].size}")
        if self.records and int(record) <= self.records[-1]:
            raise ValueError(f"record {int(record)} does not follow record {self.records[-1]}")
        self.records.append(int(record))
        self._ranges.append(r)

    def ranges_for(self, t0: int = 0, t1: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(records [n] int64, ranges [n, B]) of the scans whose record lies in [t0, t1) (t1 None: to the end)."""
        rec = np.asarray(self.records, dtype=np.int64)
        keep = (rec >= int(t0)) if t1 is None else (rec >= int(t0)) & (rec < int(t1))
        B = self._ranges[0].size if self._ranges else 0
        picked = [r for r, k in zip(self._ranges, keep) if k]
        return rec[keep], (np.stack(picked) if picked else np.empty((0, B)))


def rebuild(engine, log: ScanLog, angles, particle="best", cell_size: Optional[float] = None, **build_args) -> BuiltMap:
    """The counts of every logged scan at the pose the chosen trajectory has at the scan's record.  `particle`: an index or
    "best" (estimate().best): the recorded poses of that particle's ancestors (lineage); "mean": the smoothed trajectory
    (trajectory_summary().pose).  Records without a scan (imu steps, record 0) are left out.  `build_args` go to
    ParticleEngine.build_map (box, min_range, max_range, device); the scans go in chunks of at most CHUNK, added into one
    BuiltMap."""
    n = engine.track_info()["n_records"]
    if isinstance(particle, str) and particle == "mean":
        traj = engine.trajectory_summary().pose
    elif isinstance(particle, str):
        traj = engine.trajectory(particle)               # "best", or a ValueError
    else:
        traj = engine.lineage([int(particle)])[1][:, 0, :]
    records, ranges = log.ranges_for(0, n)
    if len(records) == 0:
        raise ValueError("the scan log holds no scan of a record of this engine's trajectory log")
    poses = np.ascontiguousarray(traj[records])
    if build_args.get("box") is None:                    # one box for every chunk
        inv = engine.dim / float(engine.cfg.tile_len_m) if cell_size is None else 1.0 / float(cell_size)
        mr = build_args.get("max_range")
        build_args["box"] = engine.build_box(poses, inv, float(engine.cfg.max_ray_m if mr is None else mr))
    built = None
    for k in range(0, len(records), CHUNK):
        built = engine.build_map(poses[k:k + CHUNK], ranges[k:k + CHUNK], angles, cell_size=cell_size, into=built, **build_args)
    return built


def rebuild_at(engine, poses, ranges, angles, cell_size: Optional[float] = None, **build_args) -> BuiltMap:
    """The counts of the scans `ranges` [n, B] at the explicit poses `poses` [n, 3]: rebuild()'s loop without a trajectory log
    (thesis_amd/refine.py draws the map again from refined poses with it).  One box for every chunk, chunks of at most CHUNK."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.ascontiguousarray(ranges, dtype=np.float64).reshape(len(poses), -1)
    if len(poses) == 0:
        raise ValueError("no scan to build a map from")
    if build_args.get("box") is None:
        inv = engine.dim / float(engine.cfg.tile_len_m) if cell_size is None else 1.0 / float(cell_size)
        mr = build_args.get("max_range")
        build_args["box"] = engine.build_box(poses, inv, float(engine.cfg.max_ray_m if mr is None else mr))
    built = None
    for k in range(0, len(poses), CHUNK):
        built = engine.build_map(poses[k:k + CHUNK], ranges[k:k + CHUNK], angles, cell_size=cell_size, into=built, **build_args)
    return built
