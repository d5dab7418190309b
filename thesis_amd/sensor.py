"""How well the scan the robot took agrees with the particles' maps: the ray-cast beam model (hit, short, max, random) as
integer tables for ParticleEngine.check_scans (include/rbpf_hip.h, rbpf_check_scans), and what a localiser
does with its answer - posterior weights, the beams a moving object returned, and whether the filter is lost.

    chk = engine.check_scans(engine.poses(), ranges, angles, return_votes=True)     # the scan at every particle's own pose
    moving = sensor.dynamic_beams(chk)
    engine.set_scan(*sensor.keep(ranges, angles, moving))

Nothing here writes to the engine."""
from __future__ import annotations

import math
from typing import Any, NamedTuple, Optional

import numpy as np

# the beam classes of rbpf_check_scans
SKIP, MATCH, LONG, SHORT, NEW, OFF, MISSING, CLEAR = range(8)
CLASS_NAMES = ("SKIP", "MATCH", "LONG", "SHORT", "NEW", "OFF", "MISSING", "CLEAR")
COST_MAX = 1 << 20


class BeamModel(NamedTuple):
    """The integer tables of rbpf_check_scans: a MATCH or LONG beam whose hit lies d cells behind its measured end costs
    class_cost[class] + hit_tab[q + half_bins], q = clamp(floor(d * bins_per_cell + 0.5), -half_bins, half_bins); every other
    beam class_cost[class].  cost / scale reads as bits."""
    hit_tab: np.ndarray      # int32 [2 half_bins + 1]
    class_cost: np.ndarray   # int32 [8]
    half_bins: int
    bins_per_cell: int
    scale: int


def _cost(p: float, scale: int) -> int:
    return COST_MAX if not p > 0.0 else int(min(COST_MAX, max(0, round(-scale * math.log2(min(p, 1.0))))))


def beam_model(cfg, sigma_hit: Optional[float] = None, z_hit: float = 0.85, z_short: float = 0.05, z_max: float = 0.05,
               z_rand: float = 0.05, bins_per_cell: int = 4, scale: int = 65536) -> BeamModel:
    """The beam model of a range finder as costs round(-scale * log2 p), capped at 2^20 (the convention of
    explore.entropy_table).  A range is read to one bin of w = cell_size / bins_per_cell metres; r = cfg.weight_max_range.
      MATCH, LONG   z_hit * G(q) + z_rand * w / r, G(q) the mass of a normal distribution of `sigma_hit` metres (default: one
                    cell) in bin q: the hit table, half_bins = ceil(4 sigma_hit / w) bins to either side; beyond them the
                    clamped bin leaves little more than the random part.  Their class costs are 0.
      SHORT         (z_short + z_rand) * w / r: something the map does not hold, anywhere along the ray
      NEW, OFF      w / r: the map says nothing about the beam's end, any range is as likely as any other
      MISSING       z_max: the sensor gave no return although the map holds a wall in range
      CLEAR         z_max + z_hit: no return, and the map expects none
      SKIP          0: the beam is not used"""
    cell = float(cfg.cell_size)
    r = float(cfg.weight_max_range)
    bpc = int(bins_per_cell)
    sigma = cell if sigma_hit is None else float(sigma_hit)
    if not (sigma > 0.0 and cell > 0.0 and r > 0.0 and 1 <= bpc <= 64 and scale >= 1):
        raise ValueError("sigma_hit, cell_size and weight_max_range must be > 0, 1 <= bins_per_cell <= 64 and scale >= 1")
    if min(z_hit, z_short, z_max, z_rand) < 0.0:
        raise ValueError("the mixture weights must be >= 0")
    w = cell / bpc
    half = int(math.ceil(4.0 * sigma / w))
    if not 1 <= half <= 4096:
        raise ValueError("sigma_hit needs 1 .. 4096 bins to either side: change sigma_hit or bins_per_cell")
    cdf = lambda x: 0.5 * (1.0 + math.erf(x / (sigma * math.sqrt(2.0))))
    one_side = [_cost(z_hit * (cdf((q + 0.5) * w) - cdf((q - 0.5) * w)) + z_rand * w / r, scale) for q in range(half + 1)]
    for q in range(1, half + 1):                             # rounding must not undo the order
        one_side[q] = max(one_side[q], one_side[q - 1])
    hit_tab = np.array(one_side[:0:-1] + one_side, dtype=np.int32)
    cc = np.zeros(8, dtype=np.int32)
    cc[SHORT] = _cost((z_short + z_rand) * w / r, scale)
    cc[NEW] = cc[OFF] = _cost(w / r, scale)
    cc[MISSING] = _cost(z_max, scale)
    cc[CLEAR] = _cost(z_max + z_hit, scale)
    return BeamModel(hit_tab, cc, half, bpc, int(scale))


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


class ScanCheck(NamedTuple):
    """ParticleEngine.check_scans: per pose [N] (numpy arrays, or torch tensors on the GPU; the methods work on the host and
    bring tensors there first)."""
    cost: Any                # int64 [N]: the sum of the beams' costs; cost / scale reads as bits
    counts: Any              # int32 [N, 8]: beams per class
    classes: Any = None      # uint8 [N, B], or None
    votes: Any = None        # int32 [B, 8]: in how many of the N poses the beam fell into each class, or None
    scale: int = 65536       # of the model the costs were taken with

    SKIP, MATCH, LONG, SHORT, NEW, OFF, MISSING, CLEAR = range(8)

    def share(self, cls: int) -> np.ndarray:
        """float64 [N]: the share of the pose's beams that are not SKIP which fell into class `cls`; 0 where every beam is SKIP."""
        c = _host(self.counts).astype(np.float64)
        used = c.sum(axis=1) - c[:, SKIP]
        return np.where(used > 0, c[:, int(cls)] / np.maximum(used, 1.0), 0.0)

    def matched(self) -> np.ndarray:
        """share(MATCH): how much of the scan the map explains from this pose."""
        return self.share(MATCH)

    def log_likelihood(self) -> np.ndarray:
        """float64 [N]: the beam model's log likelihood of the scan at each pose, in nats."""
        return -_host(self.cost).astype(np.float64) / float(self.scale) * math.log(2.0)


def posterior_weights(chk: ScanCheck, prior=None, temperature: float = 1.0) -> np.ndarray:
    """float64 [N], summing to 1: prior * 2^(-cost / (scale * temperature)), the least cost subtracted first.  The form
    estimate(weights=), pose_modes(weights=) and render_map(weights=) accept.  temperature > 1 flattens the weights: the
    beams of a scan are not independent, and the product of their likelihoods is too sure of itself."""
    if not temperature > 0.0:
        raise ValueError("temperature must be > 0")
    c = _host(chk.cost).astype(np.float64)
    w = np.exp2(-(c - c.min()) / (float(chk.scale) * float(temperature)))
    if prior is not None:
        w = w * np.asarray(prior, dtype=np.float64)
    s = w.sum()
    if not (s > 0.0 and np.isfinite(s)):
        raise ValueError("the prior leaves no weight")
    return w / s


def _pose_weights(chk: ScanCheck, weights) -> np.ndarray:
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (_host(chk.cost).shape[0],) or not (w.sum() > 0.0):
        raise ValueError("weights must be [N] with a positive sum")
    return w / w.sum()


def dynamic_beams(chk: ScanCheck, weights=None, min_share: float = 0.5) -> np.ndarray:
    """bool [B]: the beams that are SHORT - ended in observed-free space, on something the map does not hold - in at least
    `min_share` of the poses: of their number with weights=None (from `votes`), else of their weight (from `classes`)."""
    if weights is None:
        if chk.votes is None:
            raise ValueError("dynamic_beams without weights needs votes: check_scans(..., return_votes=True)")
        v = _host(chk.votes).astype(np.float64)
        return v[:, SHORT] >= float(min_share) * v.sum(axis=1)
    if chk.classes is None:
        raise ValueError("dynamic_beams with weights needs classes: check_scans(..., return_classes=True)")
    return _pose_weights(chk, weights) @ (_host(chk.classes) == SHORT).astype(np.float64) >= float(min_share)


def keep(ranges, angles, mask):
    """(ranges[~mask], angles[~mask]): the scan without the masked beams, for set_scan."""
    m = np.asarray(mask, dtype=bool)
    return np.asarray(ranges)[~m], np.asarray(angles)[~m]


def lost(chk: ScanCheck, weights=None, min_matched: float = 0.5) -> bool:
    """True when the weighted mean of matched() over the poses is below `min_matched`: the hypotheses that carry the
    weight do not explain the sensor.  weights=None: the plain mean."""
    m = chk.matched()
    mean = float(m.mean()) if weights is None else float(_pose_weights(chk, weights) @ m)
    return mean < float(min_matched)
