"""Global localization on the host: the rasters of ``ParticleEngine.locate_scan`` turned into pose
hypotheses, and the particles shared among them (``ParticleEngine.relocalize``).  NumPy only."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

TWO_PI = 6.283185307179586


class Hypotheses(NamedTuple):
    poses: np.ndarray      # [n, 3] (x, y, theta): cell centres in metres, theta_rot in [0, 2 pi)
    scores: np.ndarray     # [n] int64, descending
    cells: np.ndarray      # [n, 3] int64 (X, Y, rot): the mosaic cell and rotation index of each pose
    n_used: Optional[int]  # beams the scores are sums over (a score is at most 2 * n_used); None if the caller did not say


def hypotheses(best, rot, box, n_rot: int, cell_size: float, k: int = 8, nms_cells: int = 10,
               n_used: Optional[int] = None) -> Hypotheses:
    """The up to `k` best poses of a locate_scan result, no two within `nms_cells` cells of each other.

    The candidates (best >= 0) are ordered by (best descending, X ascending, Y ascending) and accepted greedily: one whose
    Chebyshev distance to an accepted candidate is <= nms_cells is skipped; the search stops at `k`.  A pose is the centre of
    its cell, ((X + 0.5) cell_size, (Y + 0.5) cell_size), with theta = rot * 2 pi / n_rot."""
    best, rot = np.asarray(best), np.asarray(rot)
    x0, y0 = int(box[0]), int(box[2])
    ii, jj = np.nonzero(best >= 0)                       # row-major: X ascending, then Y ascending
    order = np.argsort(-best[ii, jj].astype(np.int64), kind="stable")
    taken = []
    for n in order:
        if len(taken) >= k:
            break
        i, j = int(ii[n]), int(jj[n])
        if all(max(abs(i - a), abs(j - b)) > nms_cells for a, b in taken):
            taken.append((i, j))
    cells = np.array([(x0 + i, y0 + j, int(rot[i, j])) for i, j in taken], dtype=np.int64).reshape(-1, 3)
    scores = np.array([int(best[i, j]) for i, j in taken], dtype=np.int64)
    poses = np.empty((len(taken), 3))
    poses[:, 0] = (cells[:, 0] + 0.5) * cell_size
    poses[:, 1] = (cells[:, 1] + 0.5) * cell_size
    poses[:, 2] = (cells[:, 2] * TWO_PI) / n_rot
    return Hypotheses(poses, scores, cells, n_used)


def allot(scores, n_particles: int) -> np.ndarray:
    """`n_particles` shared among the hypotheses in proportion to `scores` by largest remainder, every hypothesis getting at
    least one (ties of remainders go to the earlier hypothesis; all scores 0 means equal shares).  With more hypotheses
    than particles the first n_particles get one each."""
    s = np.asarray(scores, dtype=np.float64)
    h = len(s)
    if h == 0:
        return np.zeros(0, dtype=np.int64)
    if n_particles <= h:
        return (np.arange(h) < n_particles).astype(np.int64)
    if not s.sum() > 0:
        s = np.ones(h)
    spare = n_particles - h                              # one each first, the rest in proportion
    quota = spare * s / s.sum()
    n = np.floor(quota).astype(np.int64)
    left = spare - int(n.sum())
    n[np.argsort(-(quota - n), kind="stable")[:left]] += 1
    return n + 1


def seed_particles(hyp: Hypotheses, n_particles: int, cell_size: float, n_rot: int, seed: int = 0) -> np.ndarray:
    """[n_particles, 3] start poses: allot(hyp.scores) particles per hypothesis, in hypothesis order, each jittered uniformly
    inside its cell and inside +- half a rotation step (PCG64(seed))."""
    n = allot(hyp.scores, n_particles)
    poses = np.repeat(hyp.poses, n, axis=0)
    rng = np.random.Generator(np.random.PCG64(seed))
    j = rng.uniform(-0.5, 0.5, size=poses.shape)
    return poses + j * np.array([cell_size, cell_size, TWO_PI / n_rot])


def converged(modes, share: float = 0.95) -> bool:
    """True iff the cloud has a mode and the heaviest one (ParticleEngine.pose_modes orders them) holds at least `share` of
    the weight."""
    return int(modes.count) > 0 and float(modes.share[0]) >= share


def kld_size(n_bins: int, epsilon: float = 0.05, z: float = 2.326) -> int:
    """Fox's KLD-sampling bound: the particles that keep the KL divergence of the sampled from the true posterior below `epsilon`
    with the confidence of the upper normal quantile `z` (2.326: 99 %), when the posterior occupies `n_bins` bins (Modes.bins):
    ceil((k - 1) / (2 epsilon) * (1 - 2 / (9 (k - 1)) + sqrt(2 / (9 (k - 1))) z)^3), and 1 for n_bins <= 1.  It only reports:
    the engine's particle count is fixed."""
    k = int(n_bins)
    if k <= 1:
        return 1
    a = 2.0 / (9.0 * (k - 1))
    return int(np.ceil((k - 1) / (2.0 * epsilon) * (1.0 - a + np.sqrt(a) * z) ** 3))
