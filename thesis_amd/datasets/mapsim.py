"""Lidar/odometry logs simulated in an occupancy map held by a ParticleEngine.

Where ``synthetic`` casts its scans in an analytic room, ``make_log`` casts them in a particle's map - one loaded from a
PGM + YAML file (``mapio.read_occupancy_map`` -> ``engine.load_map``) or built by a SLAM run - with one
``engine.cast_scans`` call on the GPU.  The tuple and the noise conventions are ``synthetic.make_log``'s.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np


def make_log(engine, particle, poses, angles, period: float = 0.1, seed: int = 1234, odo_seed: int = 1235,
             noise_sigma: float = 0.01, max_range: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(angles[B], ranges[N, B], odo[N-1, 3] = (vx, vy, omega), true_poses[N, 3]) for the N poses `poses`.

    ``ranges[k]`` is the scan `particle`'s map shows from ``poses[k]`` (``engine.cast_scans``; beams that meet nothing
    read max_range), plus N(0, noise_sigma^2) noise from PCG64(seed), clipped at 0.  ``odo[k]`` moves k -> k+1 over
    `period` seconds: the global-frame velocities between the poses with 1 % multiplicative noise from PCG64(odo_seed).
    With ``synthetic.circle_trajectory(n)`` as `poses` it is a drop-in for ``synthetic.make_log(n)``."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(engine.cast_scans(poses, angles, particle=particle, max_range=max_range), dtype=np.float64)
    if noise_sigma > 0:
        rng = np.random.Generator(np.random.PCG64(seed))
        ranges = ranges + rng.normal(0.0, noise_sigma, size=ranges.shape)
    ranges = np.maximum(ranges, 0.0)
    vel = np.diff(poses, axis=0) / period
    orng = np.random.Generator(np.random.PCG64(odo_seed))
    vel = vel * (1.0 + 0.01 * orng.standard_normal(vel.shape))
    return angles, ranges, vel, poses
