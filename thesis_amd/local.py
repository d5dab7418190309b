"""The local map (ParticleEngine.local_map; include/rbpf_hip.h, rbpf_local_map): what the posterior believes
about the cells round the robot, in the robot's frame.  Every particle's map is cut out at that particle's own pose, so walls the
particles hold at different world positions fall onto the same cells, and the cuts are fused with integer weights:

    lm = e.local_map(size_m=6.4, samples=2)          # [128, 128] at 0.05 m, the robot in the middle, x forward
    stop = lm.blocked(max_p_occ=0.05)[70:90, 54:74].any()

Element [i, j] lies (i + 0.5 - n / 2) cell + offset[0] ahead of the robot and (j + 0.5 - n / 2) cell + offset[1] to its left.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np


def quantise_weights(w, bits: int = 30) -> np.ndarray:
    """floor(w / w.sum() * 2^bits) as uint32: the integer weights rbpf_local_map takes.  The only place where floating-point
    weights become integers; the sum of the result is at most 2^bits.  Raises on a negative or non-finite weight and on a
    sum of 0."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if not 1 <= int(bits) <= 30:
        raise ValueError("1 <= bits <= 30 is required")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weights must be finite and >= 0")
    s = w.sum()
    if not (s > 0 and np.isfinite(s)):
        raise ValueError("the weights sum to 0")
    return np.floor(w / s * float(1 << int(bits))).astype(np.uint32)


def _share(a, total: int):
    """a / total in float64, for a numpy array or a torch tensor of integers."""
    return (a.double() if hasattr(a, "double") else np.asarray(a, dtype=np.float64)) / float(total)


@dataclass
class LocalMap:
    """The fused window: occ_w, free_w, unknown_w (the integer weight of the poses whose cut calls the cell occupied, free,
    unknown) and sum_wv (the weighted sum of the cuts' values, units of quantum), each [n, n] int64, numpy or torch tensors
    on the GPU; `total` the sum of the integer weights; `cell` metres per cell; `offset` the window's centre in the robot's
    frame; `crops` [N, n, n] int8, every pose's own cut, where asked for."""
    occ_w: Any
    free_w: Any
    unknown_w: Any
    sum_wv: Any
    total: int
    cell: float
    offset: Tuple[float, float] = (0.0, 0.0)
    crops: Optional[Any] = None

    def p_occ(self):
        """The weight share that calls a cell occupied."""
        return _share(self.occ_w, self.total)

    def p_free(self):
        return _share(self.free_w, self.total)

    def p_unknown(self):
        return _share(self.unknown_w, self.total)

    def mean_value(self):
        """The weighted mean lattice value, in units of quantum."""
        return _share(self.sum_wv, self.total)

    def blocked(self, max_p_occ: float = 0.05, min_p_free: float = 0.0):
        """A bool mask for a controller: more than max_p_occ of the weight sees a wall there, or less than min_p_free of it
        knows the cell free (min_p_free = 0: unknown cells do not block)."""
        return (self.p_occ() > float(max_p_occ)) | (self.p_free() < float(min_p_free))

    def as_source(self, pose, quantum: float, vmin: float = -128.0, vmax: float = 127.0):
        """The fused window as a mapio.SourceMap standing at the world pose `pose` = (x, y, theta) of the robot: cells =
        rint(mean_value()) clipped to [vmin, vmax], its origin the window's corner (offset - n cell / 2 on both axes of the
        robot's frame) placed at the pose.  mapio.write_occupancy_map(stem, ...) of a raster, or ParticleEngine.place_map,
        takes it from there."""
        from .mapio import SourceMap, _host
        x, y, th = (float(v) for v in pose)
        mv = np.asarray(_host(self.mean_value()), dtype=np.float64)
        cells = np.clip(np.rint(mv), max(float(vmin), -128.0), min(float(vmax), 127.0)).astype(np.int8)
        h = 0.5 * cells.shape[0] * float(self.cell)
        cx, cy = float(self.offset[0]) - h, float(self.offset[1]) - h
        c, s = math.cos(th), math.sin(th)
        return SourceMap(cells=cells, cell_size=float(self.cell), origin=(x + (c * cx - s * cy), y + (s * cx + c * cy), th),
                         quantum=float(quantum))
