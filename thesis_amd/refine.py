"""Poses corrected against the map their scans drew (ParticleEngine.refine_poses; include/rbpf_hip.h, rbpf_refine_poses;
DESIGN.md 3.17).

A filter's smoothed trajectory is a chain of sampled poses, and rebuild() draws their noise into the walls.  refine_trajectory
matches every logged scan against the map of all scans, moves the poses and draws the map again; follow tracks a sensor through
a known map without a filter.  Everything here is host NumPy; the search runs on the GPU.  Each scan is matched against a map
that holds the scan itself (no leave-one-out): a pose is pulled towards where it already drew its scan, which slows the
correction down and does not bias it.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import rebuild as _rebuild
from .engine import BuiltMap, RefineResult

CHUNK = 1024           # scans per refine_poses call of refine_trajectory()


def _host(a) -> np.ndarray:
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def _ratio(score, n_used) -> np.ndarray:
    s, n = _host(score).astype(np.float64), _host(n_used).astype(np.float64)
    out = np.zeros(s.shape, dtype=np.float64)
    m = n > 0
    out[m] = s[m] / (2.0 * n[m])
    return out


def fraction(res: RefineResult) -> np.ndarray:
    """score / (2 n_used) per scan, float64 in [0, 1]: 1 where every used beam ends in an occupied cell; 0 where no beam was
    used."""
    return _ratio(res.score, res.n_used)


def moved(res: RefineResult) -> np.ndarray:
    """The indices of the scans whose best candidate is not the guess: index != (0, 0, 0)."""
    return np.flatnonzero(np.any(_host(res.index) != 0, axis=1))


def follow(engine, scans, angles, start_pose, particle="best", **search) -> Tuple[np.ndarray, np.ndarray]:
    """Tracking in a map without a filter: scan t of `scans` [T, B] is refined from the result of scan t - 1, scan 0 from
    `start_pose`.  Returns (path [T, 3], fraction [T]).  `search` goes to ParticleEngine.refine_poses (substeps, window,
    rotations, rot_step, min_range, max_range): the window has to cover the motion between two scans."""
    scans = np.ascontiguousarray(scans, dtype=np.float64)
    if scans.ndim != 2:
        raise ValueError("scans must be [T, B]")
    for bad in ("return_scores", "device"):
        if bad in search:
            raise ValueError(f"follow() reads every result on the host: {bad} is not for it")
    if isinstance(particle, str) and particle == "best":
        particle = int(np.argmax(engine.weights()))      # once: the map does not change
    pose = np.array(start_pose, dtype=np.float64).reshape(3)
    path, frac = np.empty((len(scans), 3)), np.empty(len(scans))
    for t, r in enumerate(scans):
        res = engine.refine_poses(pose, r, angles, particle=particle, **search)
        pose = np.array(res.poses[0], dtype=np.float64)
        path[t], frac[t] = pose, fraction(res)[0]
    return path, frac


class RefineRound(NamedTuple):
    before: float        # mean over the scans of score_guess / (2 n_used): how well the poses fitted the map they drew
    after: float         # mean fraction() of the refined poses in the same map
    moved: int           # scans whose pose changed


class RefinedTrajectory(NamedTuple):
    poses: np.ndarray    # [n, 3] the refined poses of the scans
    records: np.ndarray  # [n] int64: the trajectory record of each
    built: BuiltMap      # the map the refined poses draw
    rounds: List[RefineRound]


def scan_poses(engine, log, particle="best") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(records [n], poses [n, 3], ranges [n, B]): the logged scans and the pose the chosen trajectory has at each, chosen
    exactly as rebuild.rebuild chooses them ("best", an index, or "mean")."""
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
    return records, np.ascontiguousarray(traj[records], dtype=np.float64), ranges


def _map_engine(engine, box, cell_size: float, n_beams: int):
    from .engine import ParticleEngine
    dim = int(round(float(engine.cfg.tile_len_m) / cell_size))
    tiles = ((box[1] - box[0]) // dim + 2) * ((box[3] - box[2]) // dim + 2)
    return ParticleEngine(1, cell_size=cell_size, tile_len_m=int(engine.cfg.tile_len_m), lattice_radius=int(engine.cfg.lattice_radius),
                          max_beams=int(n_beams), pool_tiles=int(tiles), device=int(engine.cfg.device))


def refine_trajectory(engine, log, angles, particle="best", rounds: int = 2, cell_size: Optional[float] = None, map_engine=None,
                      build_args: Optional[dict] = None, poses=None, **search) -> RefinedTrajectory:
    """Refines the poses of every logged scan against the map of all scans, `rounds` times: build_map at the poses, the map
    (rebuild.as_source) placed into particle 0 of a one-particle engine of `cell_size` (default the engine's own; `map_engine`
    supplies that engine, otherwise one is created and closed), refine_poses on all scans in chunks of CHUNK, build_map again
    at the new poses.  `particle` picks the starting trajectory as rebuild.rebuild does.  `search` goes to refine_poses,
    `build_args` (min_range, max_range, device) to build_map: at 0.025 m its window admits a max_range of 12.7 m, less than
    the default cfg.max_ray_m.  One box serves every round: the first poses' box grown by what `rounds` windows can move a pose.
    `poses` [n, 3] replaces the chosen trajectory's poses of the logged scans (loops.close_loops hands its result on this way)."""
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    records, chosen, ranges = scan_poses(engine, log, particle)
    poses = chosen if poses is None else np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    if len(poses) != len(records):
        raise ValueError(f"{len(poses)} poses for {len(records)} logged scans")
    cs = float(engine.cfg.cell_size if cell_size is None else cell_size)
    inv = engine.dim / float(engine.cfg.tile_len_m) if cell_size is None else 1.0 / cs
    build_args = dict(build_args or {})
    if "box" in build_args:
        raise ValueError("refine_trajectory() chooses the box itself")
    mr = build_args.get("max_range")
    reach = float(engine.cfg.max_ray_m if mr is None else mr) + rounds * (int(search.get("window", 12)) / int(search.get("substeps", 4)) + 1) * cs
    box = engine.build_box(poses, inv, reach)
    own = map_engine is None
    me = _map_engine(engine, box, cs, ranges.shape[1]) if own else map_engine
    try:
        built = _rebuild.rebuild_at(engine, poses, ranges, angles, cell_size=cell_size, box=box, **build_args)
        out: List[RefineRound] = []
        for _ in range(rounds):
            me.place_map(_rebuild.as_source(built, engine=engine), particle=0)
            before, after, n_moved, new = [], [], 0, []
            for k in range(0, len(poses), CHUNK):
                res = me.refine_poses(poses[k:k + CHUNK], ranges[k:k + CHUNK], angles, particle=0, **search)
                before.append(_ratio(res.score_guess, res.n_used))
                after.append(fraction(res))
                n_moved += len(moved(res))
                new.append(_host(res.poses))
            poses = np.ascontiguousarray(np.concatenate(new), dtype=np.float64)
            built = _rebuild.rebuild_at(engine, poses, ranges, angles, cell_size=cell_size, box=box, **build_args)
            out.append(RefineRound(float(np.mean(np.concatenate(before))), float(np.mean(np.concatenate(after))), int(n_moved)))
    finally:
        if own:
            me.close()
    return RefinedTrajectory(poses, records, built, out)
