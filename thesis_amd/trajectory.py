"""What to make of trajectories read from the engine's log (ParticleEngine.trajectory, trajectory_summary):
host NumPy on small arrays, no GPU work."""
from __future__ import annotations

import numpy as np


def coalescence(summary) -> int:
    """The last record at which all current particles share one ancestor (n_alive == 1), or -1 if there is none: everything up
    to it is settled, no resample can change it any more.  `summary`: a TrajectorySummary, or its n_alive array."""
    alive = np.asarray(getattr(summary, "n_alive", summary)).reshape(-1)
    one = np.nonzero(alive == 1)[0]
    return int(one[-1]) if len(one) else -1


def path_length(traj) -> float:
    """Metres travelled along a trajectory [T, >= 2] (x, y in the first two columns)."""
    xy = np.asarray(traj, dtype=np.float64)[:, :2]
    return float(np.sqrt((np.diff(xy, axis=0) ** 2).sum(axis=1)).sum()) if len(xy) > 1 else 0.0


def rigid_fit(src, dst):
    """The rotation R [2, 2] and translation t [2] that minimise sum |R src_k + t - dst_k|^2 (closed form in 2-D)."""
    a, b = np.asarray(src, dtype=np.float64)[:, :2], np.asarray(dst, dtype=np.float64)[:, :2]
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    p, q = a - ca, b - cb
    th = np.arctan2((p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]).sum(), (p * q).sum())
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return R, cb - R @ ca


def ate(traj, truth, align: bool = True) -> float:
    """Absolute trajectory error: the RMS distance between the positions of `traj` and `truth` ([T, >= 2] each, same T),
    with align=True after the rigid fit of `traj` onto `truth`."""
    a, b = np.asarray(traj, dtype=np.float64)[:, :2], np.asarray(truth, dtype=np.float64)[:, :2]
    if a.shape != b.shape:
        raise ValueError("traj and truth must have the same number of poses")
    if align:
        R, t = rigid_fit(a, b)
        a = a @ R.T + t
    return float(np.sqrt(((a - b) ** 2).sum(axis=1).mean()))
