"""ParticleEngine -- the batched structure-of-arrays engine behind Robot / HybridMap / resample.

One ParticleEngine owns P particles on one MI355X: poses, covariances, weights and one tiled
int8 occupancy map per particle, all resident in HBM.  Every method is one call into
librbpf_hip.so (include/rbpf_hip.h); numpy arrays cross the boundary as plain pointers.
"""
from __future__ import annotations

import atexit
import ctypes as C
import sys
import weakref
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import RbpfConfig, RbpfCounters, IMU_UNICYCLE, IMU_ABSOLUTE, IMU_VELOCITY

IMU_MODEL_IDS = {"unicycle": IMU_UNICYCLE, "absolute": IMU_ABSOLUTE, "velocity": IMU_VELOCITY}


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _torch_device(cfg):
    """(torch, the engine's device as torch names it).  Called only where a tensor is involved: nothing else imports torch."""
    import torch
    return torch, torch.device("cuda", int(cfg.device))


def particle_index(engine, particle, allow_none: bool = True) -> int:
    """A `particle` argument as the int the library takes: an index, "best" (the first argmax of engine.weights(), read only
    then: it is a device read that also launches a held-back map update) or, where the caller admits it, None (-1: every
    particle).  `engine` needs weights() alone."""
    if isinstance(particle, str):
        if particle != "best":
            raise ValueError(f"unknown particle {particle!r}")
        return int(np.argmax(engine.weights()))
    return -1 if particle is None and allow_none else int(particle)


def _box4(box, default):
    """A `box` argument, or default() for None, as the int32 [4] the library takes, and the shape (nx, ny) of a raster over
    it, clamped at 0: a box with x1 < x0 or y1 < y0 is the library's to refuse."""
    b = np.array([int(x) for x in (default() if box is None else box)], dtype=np.int32)
    if b.shape != (4,):
        raise ValueError("box must be (x0, x1, y0, y1)")
    return b, (max(int(b[1]) - int(b[0]), 0), max(int(b[3]) - int(b[2]), 0))


def _poses_angles(poses, angles):
    """(poses [N, 3], angles [B]) as contiguous float64; a [3] pose is N = 1."""
    ps, a = _f64(poses), _f64(angles)
    if ps.ndim == 1:
        ps = ps.reshape(1, -1)
    if ps.ndim != 2 or ps.shape[1] != 3 or a.ndim != 1:
        raise ValueError("poses must be [N, 3] (or [3]) and angles 1-D")
    return ps, a


def _scan_batch(poses, ranges, angles):
    """(poses [N, 3], ranges [N, B], angles [B]) as contiguous float64; a [3] pose with a [B] scan is N = 1."""
    ps, rg, a = _f64(poses), _f64(ranges), _f64(angles)
    if ps.ndim == 1:
        ps = ps.reshape(1, -1)
    if rg.ndim == 1:
        rg = rg.reshape(1, -1)
    if ps.ndim != 2 or ps.shape[1] != 3 or a.ndim != 1 or rg.shape != (ps.shape[0], a.shape[0]):
        raise ValueError("poses must be [N, 3], angles [B] and ranges [N, B]")
    return ps, rg, a


class _Outputs:
    """The outputs of one library call and its order against torch: the one place that decides whether a call returns numpy
    arrays or tensors on the engine's device, and when a tensor handed to or taken from torch is ready.

        out = self._outputs(device)
        a = out.empty(shape, "int32")            # numpy, or torch on the engine's device with device=True
        t = out.adopt(tensor)                    # an input (or an `into`) that torch's side wrote; held until the call is over
        with out:
            self._check(self._lib.rbpf_...(..., out.ptr(t), out.ptr(a)))

    The rule: torch allocates and writes in the order of its current stream, the library works on the engine's.  Where the
    engine has borrowed that very stream (set_stream) nothing waits.  Else torch's stream is synchronised before the call
    whenever a tensor is involved, and the engine after it whenever the outputs are on the device, so that they are ready
    for work on torch's current stream.  After an exception nothing more is waited for.  Of the engine it reads cfg.device,
    _borrowed_stream and _stream_ptr and calls synchronize(), nothing else."""

    def __init__(self, engine, device: bool):
        self._engine, self.device = engine, bool(device)
        self.torch = self.dev = self._cur = None             # set once a tensor is involved
        self._same_stream, self._held = False, []
        if self.device:
            self._use_torch()

    def _use_torch(self):
        if self.torch is None:
            e = self._engine
            self.torch, self.dev = _torch_device(e.cfg)
            self._cur = self.torch.cuda.current_stream(self.dev)
            self._same_stream = e._borrowed_stream and e._stream_ptr == self._cur.cuda_stream

    def empty(self, shape, dtype, device_dtype=None):
        """An uninitialised output of numpy's `dtype`; on the device of `device_dtype` where torch lacks the other."""
        if not self.device:
            return np.empty(shape, dtype=dtype)
        return self.torch.empty(shape, dtype=getattr(self.torch, np.dtype(device_dtype or dtype).name), device=self.dev)

    def adopt(self, x):
        """Takes an input, or an output that exists already; a tensor puts the call behind torch's stream."""
        if hasattr(x, "data_ptr"):
            self._use_torch()
        self._held.append(x)
        return x

    @staticmethod
    def ptr(x):
        """The address of an array or tensor for the library, None for an absent one; 1 where a zero-size one has none."""
        if x is None:
            return None
        return C.c_void_p((x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data) or 1)

    def __enter__(self):
        if self._cur is not None and not self._same_stream:
            self._cur.synchronize()                          # the tensors were written or allocated in torch's stream order
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None and self.device and not self._same_stream:
            self._engine.synchronize()
        self._held.clear()                                   # kept alive until the call was over
        return False


class ViewGain(NamedTuple):
    """ParticleEngine.view_gain: per pose [N], or per particle and pose [P, N] (numpy arrays, or torch tensors on the GPU)."""
    gain: Any        # int64: sum of table[v - vmin] over the distinct cells a scan there would observe
    seen: Any        # int32: how many cells that is
    unknown: Any     # int32: how many of them have the lattice value 0


class BuiltMap(NamedTuple):
    """ParticleEngine.build_map: hit and visit counts over the cells [x0, x0 + nx) x [y0, y0 + ny) of size `cell_size`
    (numpy arrays, or torch tensors on the GPU); thesis_amd/rebuild.py turns them into maps."""
    hits: Any            # int32 [nx, ny]: scans with a beam that returned from the cell
    seen: Any            # int32 [nx, ny]: scans with a beam that passed or ended in the cell; hits <= seen
    x0: int
    y0: int
    cell_size: float     # metres; the engine's own when build_map was given none
    cells_per_m: float   # what the walk multiplied by: 1 / cell_size, or the engine's dim / tile_len


class RefineResult(NamedTuple):
    """ParticleEngine.refine_poses: per scan [N] (numpy arrays, or torch tensors on the GPU); thesis_amd/refine.py reads them."""
    poses: Any           # float64 [N, 3]: the best candidate's pose, the guess itself (bit for bit) where index is (0, 0, 0)
    index: Any           # int32 [N, 3]: (i, j, k) of the best candidate, in steps of cell_size / substeps and of rot_step
    score: Any           # int32 [N]: its score, the sum of F = occ + dil over the used beams
    score_guess: Any     # int32 [N]: the guess's own score
    n_used: Any          # int32 [N]: beams with min_range < range < max_range; score <= 2 n_used
    scores: Any          # int32 [N, 2 rotations + 1, 2 window + 1, 2 window + 1] indexed [n, k, i, j], or None
    substeps: int
    rot_step: float
    cell_size: float     # metres: a translation step is cell_size / substeps


class PairResult(NamedTuple):
    """ParticleEngine.match_pairs: per pair [M] (numpy arrays, or torch tensors on the GPU); thesis_amd/loops.py reads them."""
    poses: Any           # float64 [M, 3]: the best candidate's pose of the query, the guess itself (bit for bit) where index is (0, 0, 0)
    index: Any           # int32 [M, 3]: (i, j, k) of the best candidate, in steps of cell_size / substeps and of rot_step
    score: Any           # int32 [M]: its score, the sum of F = occ + dil of the run's field over the query's used beams
    score_guess: Any     # int32 [M]: the guess's own score
    n_used: Any          # int32 [M]: the query's beams with min_range < range < max_range; score <= 2 n_used
    n_ref: Any           # int32 [M]: the used beams of the run's scans (beams, not cells)
    scores: Any          # int32 [M, 2 rotations + 1, 2 window + 1, 2 window + 1] indexed [m, k, i, j], or None
    substeps: int
    rot_step: float
    cell_size: float     # metres: a translation step is cell_size / substeps


class ScoreSurface(NamedTuple):
    """ParticleEngine.score_surface: the K best separated peaks of each of N score volumes and the moments of their plateaus
    (include/rbpf_hip.h, rbpf_score_surface).  numpy arrays, or torch tensors on the GPU; the methods work on
    the host and bring tensors there first.  thesis_amd/loops.py reads them."""
    index: Any           # int64 [N, K, 3]: (i, j, k) of peak p, in steps of cell_size / substeps and of rot_step; 0 behind count
    score: Any           # int64 [N, K]: its score
    count: Any           # int32 [N]: peaks found, 1 .. K
    size: Any            # int64 [N, K]: |T|, the cells of the plateau
    moments: Any         # int64 [N, K, 10]: sum w, sum w d (di, dj, dk), sum w d d^T (ii, ij, ik, jj, jk, kk) over the plateau
    drop: Any            # int32 [N]: the plateau reaches this far below its peak
    substeps: Optional[int] = None       # the three below come with a RefineResult or a PairResult, else None
    rot_step: Optional[float] = None
    cell_size: Optional[float] = None

    @classmethod
    def from_records(cls, records, count, drop, substeps=None, rot_step=None, cell_size=None):
        """From the library's records [N, K, 16] (include/rbpf_hip.h)."""
        return cls(records[..., 0:3], records[..., 3], count, records[..., 4], records[..., 5:15], drop, substeps, rot_step, cell_size)

    @staticmethod
    def _host(a):
        return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)

    def ambiguity(self) -> np.ndarray:
        """float64 [N]: score of the second peak / score of the best where there is a second peak and the best score is
        positive, else 0.  Near 1: another place in the window fits almost as well."""
        sc, cnt = self._host(self.score).astype(np.float64), self._host(self.count)
        out = np.zeros(len(cnt))
        if sc.shape[1] >= 2:
            ok = (cnt >= 2) & (sc[:, 0] > 0)
            out[ok] = sc[ok, 1] / sc[ok, 0]
        return out

    def offset(self, peak: int = 0) -> np.ndarray:
        """float64 [N, 3]: the weighted mean offset (di, dj, dk) of the plateau from its peak, in steps; 0 behind count."""
        m = self._host(self.moments)[:, peak].astype(np.float64)
        return m[:, 1:4] / np.maximum(m[:, 0:1], 1.0)

    def second_moment(self, peak: int = 0) -> np.ndarray:
        """float64 [N, 3, 3]: the plateau's second moment about the peak, diag(u) (sum w d d^T / sum w) diag(u) with u =
        (cell_size / substeps, cell_size / substeps, rot_step): metres and radians along the search axes (world x, world y,
        heading).  Needs the steps, so a surface of a RefineResult or a PairResult; 0 behind count."""
        if self.cell_size is None or self.substeps is None or self.rot_step is None:
            raise ValueError("a surface of a bare volume has no step sizes: pass the RefineResult or PairResult")
        m = self._host(self.moments)[:, peak].astype(np.float64)
        ii, ij, ik, jj, jk, kk = (m[:, q] for q in range(4, 10))
        c = np.stack([np.stack([ii, ij, ik], axis=1), np.stack([ij, jj, jk], axis=1), np.stack([ik, jk, kk], axis=1)], axis=1)
        c /= np.maximum(m[:, 0], 1.0)[:, None, None]
        u = np.array([self.cell_size / self.substeps, self.cell_size / self.substeps, self.rot_step])
        return c * u[:, None] * u[None, :]

    def poses(self, guesses) -> np.ndarray:
        """float64 [N, K, 3]: the peaks as poses round `guesses` [N, 3]: (gx + i step, gy + j step, gtheta + k rot_step)."""
        if self.cell_size is None or self.substeps is None or self.rot_step is None:
            raise ValueError("a surface of a bare volume has no step sizes: pass the RefineResult or PairResult")
        g = _f64(guesses).reshape(-1, 1, 3)
        idx = self._host(self.index).astype(np.float64)
        u = np.array([self.cell_size / self.substeps, self.cell_size / self.substeps, self.rot_step])
        return g + idx * u


class ScanDescriptors(NamedTuple):
    """ParticleEngine.describe_scans: per scan [N] (numpy arrays, or torch tensors on the GPU)."""
    desc: Any            # [N, R]: ring g of scan n, bit j = sector j.  numpy uint64; on the GPU int64 with the same bits
    n_used: Any          # int32 [N]: beams with min_range < range < max_range
    n_bits: Any          # int32 [N]: the popcount over the R words


class PlaceMatches(NamedTuple):
    """ParticleEngine.match_places: per query [Q], its k best references best first (numpy arrays, or torch tensors on the GPU);
    thesis_amd/loops.py reads them."""
    ref: Any             # int32 [Q, k]: the reference, -1 in an unused slot
    shift: Any           # int32 [Q, k]: its best turn s in 0 .. 63: the query's heading is the reference's minus s sectors
    score: Any           # int32 [Q, k]: v, the score at that turn
    weight: Any          # int32 [Q, k]: w = popcount(D) + popcount(D') of the reference
    n_bits: Any          # int32 [Q]: the popcount of the query
    count: Any           # int32 [Q]: slots filled

    def similarity(self):
        """score / sqrt(2 n_bits weight) in [0, 1] (score <= min(2 n_bits, weight)), 0 in an unused slot; float64 [Q, k]."""
        if hasattr(self.score, "data_ptr"):
            import torch
            den = torch.sqrt(2.0 * self.n_bits.double()[:, None] * self.weight.double())
            return torch.where(den > 0, self.score.double() / den.clamp(min=1.0), torch.zeros_like(den))
        den = np.sqrt(2.0 * np.asarray(self.n_bits, dtype=np.float64)[:, None] * np.asarray(self.weight, dtype=np.float64))
        return np.where(den > 0, np.asarray(self.score, dtype=np.float64) / np.maximum(den, 1.0), 0.0)


class Proposal(NamedTuple):
    """ParticleEngine.proposal: one particle's proposal frame and its K samples."""
    U: np.ndarray          # [3, 3] pseudo-inverse square root of the matcher covariance: maha = |(g - mean) U|^2
    A: np.ndarray          # [3, 3] sampling matrix: g = mean + A z
    mean: np.ndarray       # [3] the matcher's pose
    log_c: float           # log of the normalisation: pdf = exp(log_c - maha / 2)
    bad: bool              # NaN or indefinite covariance: nothing was proposed, the fields below are stale
    g: np.ndarray          # [K, 3] sample poses
    cos: np.ndarray        # [K]
    sin: np.ndarray        # [K]
    motion_pr: np.ndarray  # [K] pdf * 10 (robot.py:87)
    frame_f32: np.ndarray  # [K, 4] float32 look-up frame: cos / cell, sin / cell, x / cell + off_x, y / cell + off_y
    raw_w: Any             # [K] raw sample weights (robot.py:138), or None without capture


class Estimate(NamedTuple):
    """ParticleEngine.estimate: the filter's weighted pose estimate (include/rbpf_hip.h: the estimate row)."""
    pose: np.ndarray       # [3] weighted mean x, y and circular mean heading
    cov: np.ndarray        # [3, 3] weighted covariance, the heading difference wrapped into (-pi, pi]
    resultant: float       # mean resultant length of the headings, 1 = all equal
    n_eff: float           # effective sample size W^2 / sum w^2
    best: int              # the first argmax of the raw weights
    n_used: int            # particles that contributed (weight > 0, finite pose and weight)
    weight_sum: float      # W


class TrajectorySummary(NamedTuple):
    """ParticleEngine.trajectory_summary / filtered_trajectory: one estimate row per record, leading axis T."""
    pose: np.ndarray       # [T, 3]
    cov: np.ndarray        # [T, 3, 3]
    resultant: np.ndarray  # [T]
    n_eff: np.ndarray      # [T]
    best: np.ndarray       # [T] int32
    n_used: np.ndarray     # [T] int32
    n_alive: np.ndarray    # [T] int32 distinct ancestors of the current particles at the record; -1 in filtered_trajectory
    weight_sum: np.ndarray  # [T]


class Modes(NamedTuple):
    """ParticleEngine.pose_modes: the modes of the particle cloud (include/rbpf_hip.h, rbpf_pose_modes), heaviest
    first, k = min(count, max_modes) of them.  numpy arrays; with device=True torch tensors on the GPU, count / bins / used
    0-d tensors, and all max_modes rows (NaN / -1 / 0 behind `count`): slicing to k would need a host read."""
    count: Any             # modes in the cloud, also those beyond max_modes
    bins: Any              # occupied bins
    used: Any              # contributing particles
    poses: Any             # [k, 3] weighted mean x, y and circular mean heading of each mode
    covs: Any              # [k, 3, 3]
    share: Any             # [k] the mode's share of the weight, Q_c / Q_total
    size: Any              # [k] int32 members
    mode_bins: Any         # [k] int32 bins
    root: Any              # [k] int32 the smallest member index: the mode's label
    best: Any              # [k] int32 the first argmax of the raw weights among the members
    resultant: Any         # [k]
    n_eff: Any             # [k]
    weight_sum: Any        # [k]
    labels: Any = None     # int32 [P]: the root of each particle's mode, -1 for a particle that contributes nothing; None unless asked

    def estimate(self, i: int) -> "Estimate":
        """Mode i as an Estimate: what estimate() returns over the mode's members alone."""
        h = (lambda x: x.cpu().numpy()) if hasattr(self.poses, "cpu") else np.asarray
        return Estimate(pose=h(self.poses[i]).copy(), cov=h(self.covs[i]).copy(), resultant=float(self.resultant[i]), n_eff=float(self.n_eff[i]),
                        best=int(self.best[i]), n_used=int(self.size[i]), weight_sum=float(self.weight_sum[i]))


class TrajectoryModes(NamedTuple):
    """ParticleEngine.trajectory_modes: the modes of the current particles' ancestors at every record, K = max_modes columns
    (NaN / 0 behind `count`)."""
    count: np.ndarray      # [T] int64
    share: np.ndarray      # [T, K]
    poses: np.ndarray      # [T, K, 3]
    size: np.ndarray       # [T, K] int32


def _cov_from_rows(f: np.ndarray) -> np.ndarray:
    """[..., 16] estimate rows -> [..., 3, 3] symmetric covariances."""
    return f[..., [3, 4, 5, 4, 6, 7, 5, 7, 8]].reshape(f.shape[:-1] + (3, 3))


def _summary_from_rows(f: np.ndarray, i: np.ndarray) -> TrajectorySummary:
    return TrajectorySummary(pose=f[:, 0:3].copy(), cov=_cov_from_rows(f), resultant=f[:, 9].copy(), n_eff=f[:, 11].copy(),
                             best=i[:, 0].copy(), n_used=i[:, 1].copy(), n_alive=i[:, 2].copy(), weight_sum=f[:, 10].copy())


class RbpfError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"librbpf_hip error {code}: {msg}")
        self.code = code


# Engines still open when the interpreter exits are closed from an atexit hook, i.e. while the HIP runtime (and torch,
# whose stream an engine may have borrowed) is still alive; __del__ never touches the GPU during interpreter shutdown.
_LIVE = weakref.WeakSet()


def _close_all_engines():
    for e in list(_LIVE):
        try:
            e.close()
        except Exception:                                    # noqa: BLE001 - nothing useful can be done at exit
            pass


atexit.register(_close_all_engines)


class ParticleEngine:
    """P particles, their maps and the per-scan update on one GPU."""

    def __init__(self, n_particles: int, *, n_samples: int = 30, max_beams: int = 1081,
                 cell_size: float = 0.05, tile_len_m: int = 40, lattice_radius: int = 3,
                 pool_tiles: int = 0, device: int = 0, seed: int = 42, **overrides):
        self._lib = _lib.load()
        cfg = RbpfConfig()
        self._check(self._lib.rbpf_default_config(C.byref(cfg)), None)
        cfg.n_particles, cfg.n_samples, cfg.max_beams = n_particles, n_samples, max_beams
        cfg.cell_size, cfg.tile_len_m, cfg.lattice_radius = cell_size, tile_len_m, lattice_radius
        cfg.pool_tiles, cfg.device, cfg.seed = pool_tiles, device, seed
        for k, v in overrides.items():
            if k == "vel_noise":
                for i in range(4):
                    cfg.vel_noise[i] = v[i]
            else:
                if not hasattr(cfg, k):
                    raise TypeError(f"unknown engine option {k!r}")
                setattr(cfg, k, v)
        self.cfg = cfg
        self._h = C.c_void_p()
        rc = self._lib.rbpf_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise RbpfError(rc, (self._lib.rbpf_last_error(None) or b"").decode())
        self.P, self.K = n_particles, n_samples
        d = C.c_int32()
        self._check(self._lib.rbpf_get_dim(self._h, C.byref(d)))
        self.dim = d.value
        self.n_beams = 0
        self._borrowed_stream = False
        self._stream_ptr = None
        self._capture = False
        _LIVE.add(self)

    # -- plumbing ------------------------------------------------------------------------------------
    def _check(self, rc: int, h="self"):
        if rc != 0:
            hh = self._h if h == "self" else None
            raise RbpfError(rc, (self._lib.rbpf_last_error(hh) or b"").decode())

    def close(self):
        """Releases a borrowed stream first (waits for what the engine queued on it), then destroys the handle."""
        if getattr(self, "_h", None) and self._h.value:
            if self._borrowed_stream:
                self._lib.rbpf_release_stream(self._h)
                self._borrowed_stream = False
                self._stream_ptr = None
            self._lib.rbpf_destroy(self._h)
            self._h = C.c_void_p()
        _LIVE.discard(self)

    def __del__(self):
        if sys is None or sys.is_finalizing():               # interpreter shutdown: the atexit hook has run already
            return
        try:
            self.close()
        except Exception:                                    # noqa: BLE001
            pass

    def set_stream(self, stream_ptr: int):
        """Work on the caller's stream from now on (borrowed: never destroyed by the engine)."""
        self._check(self._lib.rbpf_set_stream(self._h, C.c_void_p(stream_ptr)))
        self._borrowed_stream = True
        self._stream_ptr = stream_ptr

    def release_stream(self):
        """Give a borrowed stream back; the engine works on a stream of its own again."""
        self._check(self._lib.rbpf_release_stream(self._h))
        self._borrowed_stream = False
        self._stream_ptr = None

    def synchronize(self):
        self._check(self._lib.rbpf_synchronize(self._h))

    def _outputs(self, device: bool) -> _Outputs:
        return _Outputs(self, device)

    def _particle(self, particle, allow_none: bool = True) -> int:
        return particle_index(self, particle, allow_none)

    def _int8_cells(self, cells, what: str, axes: str):
        """A raster argument as (contiguous 2-D int8 numpy array, or int8 tensor on the engine's device; its shape); `what`
        and `axes` word the caller's errors."""
        if hasattr(cells, "data_ptr"):                   # a torch tensor
            torch, dev = _torch_device(self.cfg)
            if cells.dtype != torch.int8 or cells.device != dev or cells.dim() != 2:
                raise ValueError(f"a tensor {what} must be 2-D int8 on {dev}")
            cells = cells.contiguous()
            return cells, tuple(cells.shape)
        a = np.asarray(cells)
        if a.ndim != 2:
            raise ValueError(f"{what} cells must be 2-D {axes}")
        if a.dtype != np.int8:
            if a.dtype.kind not in "iu" or (a.size and (a.min() < -128 or a.max() > 127)):
                raise ValueError(f"{what} cells must be int8 lattice values")
        a = np.ascontiguousarray(a, dtype=np.int8)
        return a, a.shape

    def _value_table(self, table) -> np.ndarray:
        """A `table` argument as int32, one entry per lattice value; None is explore.entropy_table(cfg)."""
        if table is None:
            from .explore import entropy_table
            table = entropy_table(self.cfg)
        tab = np.ascontiguousarray(table, dtype=np.int32)
        nv = int(round((float(self.cfg.max_odds_occ) - float(self.cfg.min_odds_emp)) / float(self.cfg.quantum))) + 1
        if tab.shape != (nv,):
            raise ValueError(f"table must have {nv} entries, one per lattice value")
        return tab

    def set_profiling(self, on):
        """True / False: timing events around every kernel family / none; a list of family names (KERNELS): only those
        (each record costs a few microseconds of stream time).  Restarts the counters."""
        if isinstance(on, (list, tuple, set)):
            mask = 0
            for k in on:
                mask |= 1 << self.KERNELS[k]
            self._check(self._lib.rbpf_set_profiling_families(self._h, mask))
        else:
            self._check(self._lib.rbpf_set_profiling(self._h, int(bool(on))))

    KERNELS = {"raycast": 0, "weight": 1, "resample": 2, "match": 3, "ndt": 4}

    def kernel_ms(self, which) -> np.ndarray:
        """Per-launch durations (ms, HIP events on the engine's stream) since set_profiling(True)."""
        k = self.KERNELS[which] if isinstance(which, str) else int(which)
        out = np.empty(512)
        n = C.c_int32()
        self._check(self._lib.rbpf_get_kernel_ms(self._h, k, _dp(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def counters(self) -> Dict[str, float]:
        c = RbpfCounters()
        self._check(self._lib.rbpf_get_counters(self._h, C.byref(c)))
        out = {k: getattr(c, k) for k, _ in RbpfCounters._fields_ if k not in ("reserved", "stamp7")}
        out["stamps"] = list(c.reserved) + [c.stamp7]        # eight phase stamps of a -DRBPF_STAMPS build, else zeros
        return out

    # -- a1 ------------------------------------------------------------------------------------------
    def set_scan(self, ranges, angles):
        r, a = _f64(ranges), _f64(angles)
        if r.shape != a.shape or r.ndim != 1:
            raise ValueError("ranges and angles must be 1-D arrays of equal length")
        self._check(self._lib.rbpf_set_scan(self._h, _dp(r), _dp(a), len(r)))
        self.n_beams = len(r)

    def set_scan_xy(self, x, y):
        """The scan from its sensor-frame end points (what a reference Scan object holds, lidar.py:76-87)."""
        x, y = _f64(x), _f64(y)
        if x.shape != y.shape or x.ndim != 1:
            raise ValueError("x and y must be 1-D arrays of equal length")
        self._check(self._lib.rbpf_set_scan_xy(self._h, _dp(x), _dp(y), len(x)))
        self.n_beams = len(x)

    # -- a2 ------------------------------------------------------------------------------------------
    def imu_update(self, model, data, dt_ticks: float):
        mid = IMU_MODEL_IDS[model] if isinstance(model, str) else int(model)
        d = np.zeros(3)
        d[:len(data)] = np.asarray(data, dtype=np.float64)[:3]
        self._check(self._lib.rbpf_imu_update(self._h, mid, _dp(d), float(dt_ticks)))

    # -- a4 ------------------------------------------------------------------------------------------
    def weight_samples(self, guesses, motion_prs) -> np.ndarray:
        g = _f64(guesses)
        K = g.shape[-2]
        g = g.reshape(self.P, K, 3)
        m = _f64(motion_prs).reshape(self.P, K)
        out = np.empty((self.P, K), dtype=np.float64)
        self._check(self._lib.rbpf_weight_samples(self._h, _dp(g), _dp(m), K, _dp(out)))
        return out

    # -- a5 ------------------------------------------------------------------------------------------
    def map_update(self, poses=None):
        if poses is None:
            self._check(self._lib.rbpf_map_update(self._h, None))
        else:
            p = _f64(poses).reshape(self.P, 3)
            self._check(self._lib.rbpf_map_update(self._h, _dp(p)))

    # -- full step -----------------------------------------------------------------------------------
    def scan_update(self, adj: bool = False, last_scan_xy=None, match_override=None, guesses=None):
        """Robot.map_update for every particle (rbpf_scan_update).  In filters of more than four particles per CU of the device
        the library holds the map update back until the next call:
        resample() / resample_async() right behind it launch it without the particles they discard (counters()
        ["map_updates_skipped"]); any other call launches it whole first, so every result is what it would be without."""
        ls = None if last_scan_xy is None else _f64(last_scan_xy).reshape(-1, 2)
        mo = None if match_override is None else _f64(match_override).reshape(self.P, 13)
        gs = None if guesses is None else _f64(guesses).reshape(self.P, self.K, 3)
        self._check(self._lib.rbpf_scan_update(
            self._h, int(adj), None if ls is None else _dp(ls), 0 if ls is None else len(ls),
            None if mo is None else _dp(mo), None if gs is None else _dp(gs)))

    def refresh_last_scan(self, particle: int = 0):
        """main.py:167-168 on the device: the current scan at `particle`'s pose becomes the previous scan that
        scan_update(adj=True, last_scan_xy=None) matches against."""
        self._check(self._lib.rbpf_refresh_last_scan(self._h, int(particle)))

    def scan_update_begin(self, adj: bool = False, last_scan_xy=None, match_override=None, guesses=None):
        """First half of scan_update: matcher, proposal, weighting (robot.py:62-114); follow with scan_update_end()."""
        ls = None if last_scan_xy is None else _f64(last_scan_xy).reshape(-1, 2)
        mo = None if match_override is None else _f64(match_override).reshape(self.P, 13)
        gs = None if guesses is None else _f64(guesses).reshape(self.P, self.K, 3)
        self._check(self._lib.rbpf_scan_update_begin(
            self._h, int(adj), None if ls is None else _dp(ls), 0 if ls is None else len(ls),
            None if mo is None else _dp(mo), None if gs is None else _dp(gs)))

    def scan_update_end(self):
        """Second half: the map update at the new mean pose and the NaN branch (robot.py:115, 73-78)."""
        self._check(self._lib.rbpf_scan_update_end(self._h))

    def set_proposal_capture(self, on: bool):
        """True: the following scan updates keep every sample's raw weight for proposal().  Off by default; changes no result."""
        self._check(self._lib.rbpf_set_proposal_capture(self._h, int(bool(on))))
        self._capture = bool(on)

    def proposal(self, particle: int) -> "Proposal":
        """The proposal of the last scan_update / scan_update_begin for one particle, as the kernels left it.
        Test/inspection entry; raw_w is None with capture off (turned on only after that update: an RbpfError)."""
        frame, samp = np.empty(24), np.empty((self.K, 6))
        f32 = np.empty((self.K, 4), dtype=np.float32)
        w = np.empty(self.K) if self._capture else None
        self._check(self._lib.rbpf_get_proposal(self._h, int(particle), _dp(frame), _dp(samp), f32.ctypes.data_as(C.POINTER(C.c_float)),
                                                None if w is None else _dp(w)))
        return Proposal(U=frame[0:9].reshape(3, 3).copy(), A=frame[9:18].reshape(3, 3).copy(), mean=frame[18:21].copy(),
                        log_c=float(frame[21]), bad=bool(frame[22] != 0.0), g=samp[:, 0:3].copy(), cos=samp[:, 3].copy(),
                        sin=samp[:, 4].copy(), motion_pr=samp[:, 5].copy(), frame_f32=f32, raw_w=w)

    def match_inputs(self, particle: int, guess, cap_ref: int = 1 << 16):
        """The (curr, ref) point lists HybridMap.get_scan_match would hand to the matcher (hybridmap.py:210-242)."""
        g = _f64(guess).reshape(3)
        curr = np.empty((max(self.n_beams, 1), 2)); ref = np.empty((cap_ref, 2))
        nc, nr = C.c_int32(), C.c_int32()
        self._check(self._lib.rbpf_match_inputs(self._h, particle, _dp(g), _dp(curr), C.byref(nc), _dp(ref), C.byref(nr), cap_ref))
        return curr[:nc.value].copy(), ref[:min(nr.value, cap_ref)].copy()

    def match_results(self) -> np.ndarray:
        """[P, 13] pose, covariance (row-major 3x3) and score of every particle as the last built-in matcher wrote them
        (a duplicate particle gets its representative's row).  Test/inspection entry."""
        out = np.empty((self.P, 13))
        self._check(self._lib.rbpf_match_results(self._h, _dp(out)))
        return out

    def native_sincosf(self, x) -> Tuple[np.ndarray, np.ndarray]:
        """The device's __sincosf of float32 angles, as the matcher's grid stage evaluates it.  Test/inspection entry."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        s, c = np.empty_like(x), np.empty_like(x)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.rbpf_native_sincosf(self._h, x.ctypes.data_as(fp), len(x), s.ctypes.data_as(fp), c.ctypes.data_as(fp)))
        return s, c

    def resample(self, u: float = float("nan"), indices: bool = True) -> Tuple[bool, Optional[np.ndarray]]:
        """(did it resample, ancestor index of every new particle); indices=False reads only the flag back: (did, None)."""
        idx = np.empty(self.P, dtype=np.int32) if indices else None
        did = C.c_int32()
        self._check(self._lib.rbpf_resample(self._h, float(u), None if idx is None else _ip(idx), C.byref(did)))
        return bool(did.value), idx

    def resample_async(self, u: float = float("nan")):
        """resample without reading the ancestor indices back (no host synchronisation)."""
        self._check(self._lib.rbpf_resample(self._h, float(u), None, None))

    # -- state ---------------------------------------------------------------------------------------
    def poses(self) -> np.ndarray:
        out = np.empty((self.P, 3))
        self._check(self._lib.rbpf_get_poses(self._h, _dp(out)))
        return out

    def covs(self) -> np.ndarray:
        out = np.empty((self.P, 3, 3))
        self._check(self._lib.rbpf_get_covs(self._h, _dp(out)))
        return out

    def weights(self) -> np.ndarray:
        out = np.empty(self.P)
        self._check(self._lib.rbpf_get_weights(self._h, _dp(out)))
        return out

    def set_state(self, poses=None, covs=None, weights=None):
        p = None if poses is None else _f64(np.broadcast_to(poses, (self.P, 3)))
        c = None if covs is None else _f64(np.broadcast_to(covs, (self.P, 3, 3)))
        w = None if weights is None else _f64(np.broadcast_to(weights, (self.P,)))
        self._check(self._lib.rbpf_set_state(self._h, None if p is None else _dp(p),
                                             None if c is None else _dp(c), None if w is None else _dp(w)))

    def tiles(self, particle: int) -> List[Tuple[Tuple[float, float], np.ndarray]]:
        """[(centre_xy, cells int8 [dim, dim] indexed [x][y])] of one particle, lattice order."""
        n = C.c_int32()
        self._check(self._lib.rbpf_get_tile_count(self._h, particle, C.byref(n)))
        out = []
        for k in range(n.value):
            c = np.empty(2)
            cells = np.empty((self.dim, self.dim), dtype=np.int8)
            self._check(self._lib.rbpf_get_tile(self._h, particle, k, _dp(c), cells.ctypes.data_as(C.POINTER(C.c_int8))))
            out.append(((float(c[0]), float(c[1])), cells))
        return out

    def set_tile(self, particle: int, centre, cells: np.ndarray):
        cells = np.ascontiguousarray(cells, dtype=np.int8)
        if cells.shape != (self.dim, self.dim):
            raise ValueError("tile must be [dim, dim] int8")
        self._check(self._lib.rbpf_set_tile(self._h, particle, float(centre[0]), float(centre[1]),
                                            cells.ctypes.data_as(C.POINTER(C.c_int8))))

    # -- map loading and localization (include/rbpf_hip.h: rbpf_load_map, rbpf_set_map_updates) --------------------------
    def load_map(self, raster, particle: Optional[int] = None):
        """Writes the int8 lattice values `raster.cells` (a MapRaster, as render_map or mapio.read_occupancy_map give it)
        into `particle`'s map, or into every particle's (None).  Cells inside the raster's box are replaced, every other
        cell keeps its value; missing tiles come from the pool.  `cells` is a numpy array, or an int8 torch tensor on the
        engine's device (read on the GPU, in torch's stream order).  All or nothing: on an error no map changes."""
        cfg = self.cfg
        for name, have, want in (("cell_size", raster.cell_size, cfg.cell_size), ("quantum", raster.quantum, cfg.quantum),
                                 ("tile_len", raster.tile_len, float(cfg.tile_len_m)), ("dim", raster.dim, self.dim)):
            if abs(float(have) - float(want)) > 1e-9 * abs(float(want)):
                raise ValueError(f"raster {name} = {have!r} differs from the engine's {want!r}")
        if raster.cells is None:
            raise ValueError("the raster has no int8 cells (a whole-filter render has prob / occ_frac): convert them with "
                             "thesis_amd.mapio.cells_from_probability first")
        p = -1 if particle is None else int(particle)
        cells, shape = self._int8_cells(raster.cells, "raster", "[nx][ny]")
        b = np.array([raster.x0, raster.x0 + shape[0], raster.y0, raster.y0 + shape[1]], dtype=np.int32)
        out = self._outputs(False)
        out.adopt(cells)
        flags = _lib.RBPF_LOAD_DEVICE_IN if hasattr(cells, "data_ptr") else 0
        with out:                                        # (an empty box writes nothing; the library only checks the box)
            self._check(self._lib.rbpf_load_map(self._h, p, _ip(b), out.ptr(cells), flags))

    # -- map placement (include/rbpf_hip.h: rbpf_place_map; thesis_amd/mapio.py: SourceMap) ----------------
    PLACE_MODES = {"replace": _lib.RBPF_PLACE_REPLACE, "known": _lib.RBPF_PLACE_KNOWN, "add": _lib.RBPF_PLACE_ADD}

    def _place_inputs(self, src, box, samples):
        """The arguments place_map and warp_map share: (cells, their shape, input flag, pose, box, its shape, samples)."""
        from .mapio import placed_box
        cfg = self.cfg
        if abs(float(src.quantum) - float(cfg.quantum)) > 1e-9 * abs(float(cfg.quantum)):
            raise ValueError(f"source quantum = {src.quantum!r} differs from the engine's {cfg.quantum!r}")
        cells, shape = self._int8_cells(src.cells, "source", "[nsx][nsy]")
        cell = float(cfg.tile_len_m) / self.dim
        b, oshape = _box4(box, lambda: placed_box(src, cell, self.dim, int(cfg.lattice_radius)))
        if samples is None:
            samples = min(8, max(2, int(np.ceil(2.0 * cell / float(src.cell_size)))))
        pose = _f64([float(v) for v in src.origin])
        if pose.shape != (3,):
            raise ValueError("source origin must be (x, y, yaw)")
        return cells, shape, _lib.RBPF_PLACE_DEVICE_IN if hasattr(cells, "data_ptr") else 0, pose, b, oshape, int(samples)

    def place_map(self, src, particle: Optional[int] = None, box=None, samples: Optional[int] = None, mode: str = "replace"):
        """Resamples the map `src` (a mapio.SourceMap: any cell size, origin and yaw; e.g. mapio.read_map_image, or
        mapio.source_from_raster of a render) onto the engine's cells and merges it into `particle`'s map, or into every
        particle's (None), each with its own old cells.  `box` = (x0, x1, y0, y1) in mosaic cells, default
        mapio.placed_box(src, ...); `samples` per axis and cell (1 .. 8), default min(8, max(2, ceil(2 cell / src cell))):
        a cell takes the largest source value any of its samples meets.  `mode`: "replace" (covered cells take the
        resampled value), "known" (only where that value is not 0) or "add" (log-odds fusion: old + new, clamped).  Cells
        the source does not cover keep their values.  `src.cells` is a numpy array, or an int8 torch tensor on the
        engine's device.  All or nothing: on an error no map changes.  Returns the box."""
        if mode not in self.PLACE_MODES:
            raise ValueError(f"unknown mode {mode!r}")
        cells, shape, flags, pose, b, _, S = self._place_inputs(src, box, samples)
        out = self._outputs(False)
        out.adopt(cells)
        with out:
            self._check(self._lib.rbpf_place_map(self._h, -1 if particle is None else int(particle), _ip(b), out.ptr(cells), shape[0],
                                                 shape[1], float(src.cell_size), _dp(pose), S, self.PLACE_MODES[mode], flags, None, None))
        return tuple(int(x) for x in b)

    def warp_map(self, src, box=None, samples: Optional[int] = None, device: bool = False):
        """What place_map would write, without writing it: (warped, covered, box) with `warped` int8 and `covered` uint8
        rasters [x1-x0, y1-y0] of `box` (covered: some sample of the cell met the source; warped: the largest source value
        met, 0 where none).  No engine state changes.  device=True: torch tensors on the engine's device, ready for work
        on torch's current stream."""
        cells, shape, flags, pose, b, oshape, S = self._place_inputs(src, box, samples)
        out = self._outputs(device)
        out.adopt(cells)
        warped, covered = out.empty(oshape, "int8"), out.empty(oshape, "uint8")
        flags |= _lib.RBPF_PLACE_DRY | (_lib.RBPF_PLACE_DEVICE_OUT if device else 0)
        with out:
            self._check(self._lib.rbpf_place_map(self._h, -1, _ip(b), out.ptr(cells), shape[0], shape[1], float(src.cell_size), _dp(pose),
                                                 S, _lib.RBPF_PLACE_REPLACE, flags, out.ptr(warped), out.ptr(covered)))
        return warped, covered, tuple(int(x) for x in b)

    @property
    def map_updates(self) -> bool:
        """True (default): every scan update writes the maps.  False: localization in the maps as they are; the NaN
        branch's weight is taken on the unchanged map and the random streams advance as with updates on."""
        on = C.c_int32()
        self._check(self._lib.rbpf_get_map_updates(self._h, C.byref(on)))
        return bool(on.value)

    def map_update_workgroups(self) -> int:
        """Workgroups the event-walk map kernel was launched with in the last map update (0: it did not run)."""
        n = C.c_int32()
        self._check(self._lib.rbpf_get_map_update_workgroups(self._h, C.byref(n)))
        return int(n.value)

    @map_updates.setter
    def map_updates(self, on: bool):
        self._check(self._lib.rbpf_set_map_updates(self._h, int(bool(on))))

    # -- checkpoint (a portable replacement of the reference's shelve pickles, main.py:183-210) ----
    CHECKPOINT_VERSION = 1

    def save_checkpoint(self, path: str):
        """Everything needed to continue the run bit-identically, as one compressed .npz: configuration, particle
        state, the position of the random streams and every tile (cropped to its non-zero box); with tracking on also the
        trajectory log (track_state, track_records), so that a continued run has the trajectories of an uninterrupted one."""
        import json
        su, rd = C.c_uint64(), C.c_uint64()
        self._check(self._lib.rbpf_get_rng_state(self._h, C.byref(su), C.byref(rd)))
        owner, centre, box, chunks = [], [], [], []
        for p in range(self.P):
            for c, cells in self.tiles(p):
                xs, ys = np.nonzero(cells)
                b = (0, 0, 0, 0) if len(xs) == 0 else (int(xs.min()), int(xs.max()) + 1, int(ys.min()), int(ys.max()) + 1)
                owner.append(p); centre.append(c); box.append(b)
                chunks.append(cells[b[0]:b[1], b[2]:b[3]].ravel())
        cfg = {k: (list(getattr(self.cfg, k)) if k == "vel_noise" else getattr(self.cfg, k)) for k, _ in self.cfg._fields_}
        np.savez_compressed(path, version=np.array(self.CHECKPOINT_VERSION), config=np.array(json.dumps(cfg)),
                            poses=self.poses(), covs=self.covs(), weights=self.weights(),
                            rng_state=np.array([su.value, rd.value], dtype=np.uint64), map_updates=np.array(int(self.map_updates)),
                            tile_owner=np.array(owner, dtype=np.int32), tile_centre=np.array(centre, dtype=np.float64).reshape(-1, 2),
                            tile_box=np.array(box, dtype=np.int32).reshape(-1, 4),
                            tile_cells=np.concatenate(chunks) if chunks else np.empty(0, dtype=np.int8),
                            **(self._track_export() or {}))

    @classmethod
    def from_checkpoint(cls, path: str, device: int = 0) -> "ParticleEngine":
        import json
        with np.load(path, allow_pickle=False) as d:
            if int(d["version"]) != cls.CHECKPOINT_VERSION:
                raise ValueError("unknown checkpoint version")
            cfg = json.loads(str(d["config"]))
            skip = {"n_particles", "n_samples", "max_beams", "cell_size", "tile_len_m", "lattice_radius", "pool_tiles", "device", "seed"}
            over = {k: (tuple(v) if k == "vel_noise" else v) for k, v in cfg.items() if k not in skip}
            e = cls(cfg["n_particles"], n_samples=cfg["n_samples"], max_beams=cfg["max_beams"], cell_size=cfg["cell_size"],
                    tile_len_m=cfg["tile_len_m"], lattice_radius=cfg["lattice_radius"], pool_tiles=cfg["pool_tiles"],
                    device=device, seed=cfg["seed"], **over)
            e.set_state(d["poses"], d["covs"], d["weights"])
            e._check(e._lib.rbpf_set_rng_state(e._h, int(d["rng_state"][0]), int(d["rng_state"][1])))
            e.map_updates = bool(int(d["map_updates"])) if "map_updates" in d.files else True   # absent in older checkpoints
            off = 0
            for p, c, b in zip(d["tile_owner"], d["tile_centre"], d["tile_box"]):
                n = int((b[1] - b[0]) * (b[3] - b[2]))
                cells = np.zeros((e.dim, e.dim), dtype=np.int8)
                cells[b[0]:b[1], b[2]:b[3]] = d["tile_cells"][off:off + n].reshape(b[1] - b[0], b[3] - b[2])
                off += n
                e.set_tile(int(p), c, cells)
            if "track_records" in d.files:               # absent in older checkpoints and without tracking: no log
                e._track_import(d["track_state"], d["track_records"])
        return e

    # -- map read-out (include/rbpf_hip.h: rbpf_map_extent, rbpf_render_map; thesis_amd/mapio.py) -----------------------
    def map_extent(self, particle: Optional[int] = None) -> Optional[Tuple[int, int, int, int]]:
        """(x0, x1, y0, y1), half-open, in mosaic cells: the smallest box holding the written cells of every tile of
        `particle`, or of all particles (None); None when there is none."""
        box = np.empty(4, dtype=np.int32)
        self._check(self._lib.rbpf_map_extent(self._h, -1 if particle is None else int(particle), _ip(box)))
        return None if box[0] == box[1] else tuple(int(b) for b in box)

    def render_map(self, particle=None, box=None, weights=None, device: bool = False,
                   fields=("prob", "occ_frac")) -> "MapRaster":
        """A dense raster of one particle's map (`particle` an index, or "best": the first argmax of weights()) or of the
        whole filter (None).  `box` = (x0, x1, y0, y1) in mosaic cells, default map_extent(particle).  The whole filter
        gives the weighted mean occupancy probability `prob` and the weight share `occ_frac` that calls a cell occupied
        (`fields` picks them); `weights`: None (uniform), P values, or "resample" (resample_weights of weights()).
        device=True: torch tensors on the engine's device, ready for work on torch's current stream."""
        from .mapio import MapRaster, resample_weights
        p = self._particle(particle)
        w = None
        if isinstance(weights, str):
            if weights != "resample":
                raise ValueError(f"unknown weights {weights!r}")
            w = resample_weights(self.weights())
        elif weights is not None:
            w = _f64(weights)
            if w.shape != (self.P,):
                raise ValueError(f"weights must have shape ({self.P},)")
        b, shape = _box4(box, lambda: self.map_extent(None if p < 0 else p) or (0, 0, 0, 0))
        want = [p >= 0, p < 0 and "prob" in fields, p < 0 and "occ_frac" in fields]
        out = self._outputs(device)
        outs = [out.empty(shape, d) if k else None for k, d in zip(want, ("int8", "float32", "float32"))]
        if not (device and b[1] >= b[0] and b[3] >= b[2] and shape[0] * shape[1] == 0):   # an empty tensor has no data pointer
            with out:
                self._check(self._lib.rbpf_render_map(self._h, p, _ip(b), None if w is None else _dp(w),
                                                      _lib.RBPF_RENDER_DEVICE_OUT if device else 0, *map(out.ptr, outs)))
        return MapRaster(x0=int(b[0]), y0=int(b[2]), cell_size=float(self.cfg.cell_size), quantum=float(self.cfg.quantum),
                         dim=self.dim, tile_len=float(self.cfg.tile_len_m), cells=outs[0], prob=outs[1], occ_frac=outs[2])

    # -- scan casting (include/rbpf_hip.h: rbpf_cast_scans; thesis_amd/datasets/mapsim.py) ------------------------------------
    def cast_scans(self, poses, angles, particle=None, max_range: Optional[float] = None, device: bool = False,
                   return_status: bool = False):
        """What a lidar with beam directions `angles` [B] (sensor frame) would see from `poses` [N, 3] (or [3]) in a
        particle's map: `particle` an index, "best" (the first argmax of weights()) or None (pose n in particle n's map,
        N == P; e.g. poses()).  Returns ranges [N, B] in metres, max_range (default cfg.weight_max_range) where nothing
        occupied was met; with return_status also status [N, B] uint8 (1 hit, 0 none within max_range, 2 left the tile
        lattice).  device=True: torch tensors on the engine's device, ready for work on torch's current stream."""
        p = self._particle(particle)
        ps, a = _poses_angles(poses, angles)
        shape = (ps.shape[0], a.shape[0])
        mr = float(self.cfg.weight_max_range if max_range is None else max_range)
        out = self._outputs(device)
        r = out.empty(shape, "float64")
        st = out.empty(shape, "uint8") if return_status else None
        with out:
            self._check(self._lib.rbpf_cast_scans(self._h, p, _dp(ps), shape[0], _dp(a), shape[1], mr,
                                                  _lib.RBPF_CAST_DEVICE_OUT if device else 0, out.ptr(r), out.ptr(st)))
        return (r, st) if return_status else r

    # -- view gain (include/rbpf_hip.h: rbpf_view_gain; thesis_amd/explore.py) ---------------------------------
    def view_gain(self, poses, angles, particle="best", max_range: Optional[float] = None, table=None, device: bool = False):
        """What a scan with beam directions `angles` [B] taken at `poses` [N, 3] (or [3]) would observe in a particle's map:
        the set of distinct cells its rays test (the rays of cast_scans), reduced against the map.  `particle`: an index,
        "best" (the first argmax of weights()), or None: every pose in EVERY particle's map.  Returns ViewGain(gain int64,
        seen int32, unknown int32), each [N], or [P, N] for particle=None: the number of cells seen, how many of them are
        unknown (lattice value 0), and the sum of table[v - vmin] over them.  `max_range` defaults to cfg.max_ray_m, the
        range the map update draws; `table` (one int in 0 .. 2^20 per lattice value) to explore.entropy_table(cfg), with
        which gain / 65536 reads as bits.  device=True: torch tensors on the engine's device, ready for work on torch's
        current stream."""
        p = self._particle(particle)
        ps, a = _poses_angles(poses, angles)
        tab = self._value_table(table)
        shape = (ps.shape[0],) if p >= 0 else (self.P, ps.shape[0])
        mr = float(self.cfg.max_ray_m if max_range is None else max_range)
        out = self._outputs(device)
        outs = [out.empty(shape, d) for d in ("int64", "int32", "int32")]
        with out:
            self._check(self._lib.rbpf_view_gain(self._h, p, _dp(ps), ps.shape[0], _dp(a), a.shape[0], mr, _ip(tab),
                                                 _lib.RBPF_GAIN_DEVICE_OUT if device else 0, *map(out.ptr, outs)))
        return ViewGain(*outs)

    # -- scan checks (include/rbpf_hip.h: rbpf_check_scans; thesis_amd/sensor.py) --------------------------------
    def check_scans(self, poses, ranges, angles, particle=None, max_range: Optional[float] = None, min_range: float = 0.0,
                    tol: Optional[float] = None, model=None, device: bool = False, return_classes: bool = False,
                    return_votes: bool = False):
        """How well measured scans agree with a particle's map: `ranges` [B] (one scan, checked at every pose) or [N, B] (scan n at
        pose n) in metres, NaN, inf, 0 and negatives allowed, with beam directions `angles` [B], at `poses` [N, 3] (or [3]).
        `particle`: an index, "best" (the first argmax of weights()) or None (pose n in particle n's map, N == P; e.g. poses()).
        Every beam walks the ray of cast_scans up to its measured end plus `tol` metres (default two cells) and falls into one of
        the classes sensor.SKIP .. sensor.CLEAR; `model` (default sensor.beam_model(cfg)) prices them.  A beam at or beyond
        `max_range` (default cfg.weight_max_range) is a no-return beam, one below `min_range` is skipped.  Returns
        sensor.ScanCheck(cost int64 [N], counts int32 [N, 8], classes uint8 [N, B] with return_classes, votes int32 [B, 8] with
        return_votes, else None).  device=True: torch tensors on the engine's device, ready for work on torch's current stream."""
        from . import sensor
        p = self._particle(particle)
        ps, a = _poses_angles(poses, angles)
        rg = _f64(ranges)
        if rg.ndim == 1:
            rg = rg.reshape(1, -1)
        N, B = ps.shape[0], a.shape[0]
        if rg.ndim != 2 or rg.shape[1] != B or rg.shape[0] not in (1, N):
            raise ValueError("ranges must be [B] or [N, B] for poses [N, 3] and angles [B]")
        m = sensor.beam_model(self.cfg) if model is None else model
        hit = np.ascontiguousarray(m.hit_tab, dtype=np.int32)
        cc = np.ascontiguousarray(m.class_cost, dtype=np.int32)
        if hit.shape != (2 * int(m.half_bins) + 1,) or cc.shape != (8,):
            raise ValueError("model.hit_tab must have 2 * half_bins + 1 entries and model.class_cost 8")
        cell = float(self.cfg.tile_len_m) / self.dim
        mr = float(self.cfg.weight_max_range if max_range is None else max_range)
        out = self._outputs(device)
        outs = [out.empty((N,), "int64"), out.empty((N, 8), "int32"), out.empty((N, B), "uint8") if return_classes else None,
                out.empty((B, 8), "int32") if return_votes else None]
        with out:
            self._check(self._lib.rbpf_check_scans(self._h, p, _dp(ps), N, _dp(rg), rg.shape[0], _dp(a), B, mr, float(min_range),
                                                   2.0 * cell if tol is None else float(tol), _ip(hit), int(m.half_bins),
                                                   int(m.bins_per_cell), _ip(cc), _lib.RBPF_SCANS_DEVICE_OUT if device else 0,
                                                   *map(out.ptr, outs)))
        return sensor.ScanCheck(*outs, scale=int(m.scale))

    # -- travel cost (include/rbpf_hip.h: rbpf_travel_cost; thesis_amd/plan.py) ---------------------------------
    def travel_cost(self, starts, goals=None, particle="best", box=None, radius_m: float = 0.0, clear_max: Optional[int] = None,
                    through_unknown: bool = False, device: bool = False):
        """Travel cost from `starts` [n, 2] (or [2]; metres, further columns such as a heading are ignored) to every cell of
        `box` = (x0, x1, y0, y1) in mosaic cells (default map_extent of the particle, or of all particles with particle=None)
        in a particle's map, walls inflated by `radius_m`: inflate = floor(radius_m * cells per metre * 5) chamfer units, and a
        cell carries the robot if it is known free (with through_unknown: not occupied) and its clearance exceeds inflate.
        `particle`: an index or "best" (the first argmax of weights()): returns plan.Travel with cost int32 and clearance uint16
        rasters [x1-x0, y1-y0] (cost in chamfer units, 5 per axial step and 7 per diagonal one, -1 unreachable; clearance capped
        at `clear_max`, default and at least inflate + 1) and goal_cost [n_goals] for `goals` [n, 2].  particle=None: goal_cost
        [P, n_goals] only, every goal in every particle's map; starts are then one point, or P points (start n in particle n's
        map, e.g. poses()).  plan.path_to walks a path down the field, plan.cost_metres converts.  device=True: torch tensors
        on the engine's device (clearance as int16), ready for work on torch's current stream."""
        from .plan import Travel
        p = self._particle(particle)
        s = _f64(starts)
        if s.ndim == 1:
            s = s.reshape(1, -1)
        if s.ndim != 2 or s.shape[1] < 2:
            raise ValueError("starts must be [n, 2] (or [2])")
        s = np.ascontiguousarray(s[:, :2])
        g = None
        if goals is not None:
            g = _f64(goals)
            if g.ndim == 1:
                g = g.reshape(1, -1)
            if g.ndim != 2 or g.shape[1] < 2:
                raise ValueError("goals must be [n, 2] (or [2])")
            g = np.ascontiguousarray(g[:, :2])
        if p < 0 and g is None:
            raise ValueError("particle=None computes goal costs only: give goals")
        b, shape = _box4(box, lambda: self.map_extent(None if p < 0 else p) or (0, 0, 0, 0))
        inv = self.dim / float(self.cfg.tile_len_m)
        inflate = int(np.floor(float(radius_m) * inv * 5.0))
        cmax = max(inflate + 1, inflate + 1 if clear_max is None else int(clear_max))
        gshape = None if g is None else ((g.shape[0],) if p >= 0 else (self.P, g.shape[0]))
        out = self._outputs(device)
        outs = [out.empty(shape, "int32") if p >= 0 else None,
                out.empty(shape, "uint16", device_dtype="int16") if p >= 0 else None,       # torch has no arithmetic on uint16
                out.empty(gshape, "int32") if g is not None else None]
        flags = (_lib.RBPF_TRAVEL_DEVICE_OUT if device else 0) | (_lib.RBPF_TRAVEL_THROUGH_UNKNOWN if through_unknown else 0)
        rounds = C.c_int32(0)
        with out:
            self._check(self._lib.rbpf_travel_cost(self._h, p, _ip(b), _dp(s), s.shape[0], None if g is None else _dp(g),
                                                   0 if g is None else g.shape[0], inflate, cmax, flags, *map(out.ptr, outs),
                                                   C.byref(rounds)))
        return Travel(outs[0], outs[1], outs[2], int(rounds.value), tuple(int(x) for x in b), float(self.cfg.tile_len_m) / self.dim,
                      inv, inflate, cmax)

    def travel_stats(self) -> Dict[str, int]:
        """How the last travel_cost went: relaxation rounds, block runs (workgroups that had work), and the (particle, block)
        pairs a sweep of everything would run in every round."""
        out = (C.c_uint64 * 3)()
        self._check(self._lib.rbpf_travel_stats(self._h, out))
        return {"rounds": int(out[0]), "block_runs": int(out[1]), "blocks": int(out[2])}

    # -- path checks (include/rbpf_hip.h: rbpf_check_paths; thesis_amd/plan.py) ------------------------------------
    def check_paths(self, paths, particle="best", radius_m: float = 0.0, clear_max: Optional[int] = None, through_unknown: bool = False,
                    start_exempt: bool = False, own: bool = False, device: bool = False):
        """Walks `paths` cell by cell through a particle's map and tests every step: `paths` is [K, M, 2+] (metres; further
        columns are ignored) or a list of K arrays [m_k, 2+].  A step is blocked if its cell is not known free (with
        through_unknown: is occupied) or its clearance does not exceed inflate = floor(radius_m * cells per metre * 5), or if it is
        diagonal and cuts a corner; start_exempt: the cell of a path's first waypoint always carries the robot.  `particle`: an
        index, "best" (the first argmax of weights()), or None: every path in EVERY particle's map, results [P, K].  own=True
        (particle=None only): `paths` is [P, K, M, 2+] and the paths of group p are checked in particle p's map alone, e.g.
        rollouts from every particle's own pose.  Returns plan.PathCheck(first_blocked, first_unknown, min_clearance, n_unknown,
        steps, cell, inflate, clear_max): int32 [K] or [P, K]; steps is numpy int32 [K] ([P, K] with own).  min_clearance is
        capped at `clear_max` (default and at least inflate + 1).  device=True: torch tensors on the engine's device, ready for
        work on torch's current stream (steps stays numpy)."""
        from .plan import PathCheck
        p = self._particle(particle)
        if own:
            if p >= 0:
                raise ValueError("own=True needs particle=None")
            a = _f64(paths)
            if a.ndim != 4 or a.shape[0] != self.P or a.shape[3] < 2:
                raise ValueError("with own=True paths must be [P, K, M, 2+]")
            lead, plist = a.shape[:2], list(a.reshape((-1,) + a.shape[2:]))
        else:
            plist = list(paths) if isinstance(paths, (list, tuple)) else list(_f64(paths))
            lead = (len(plist),)
        plist = [_f64(q) for q in plist]
        if not plist or any(q.ndim != 2 or q.shape[1] < 2 or q.shape[0] < 1 for q in plist):
            raise ValueError("paths must be [K, M, 2+] or a list of [m, 2+] arrays, K >= 1 and every m >= 1")
        xy = np.ascontiguousarray(np.concatenate([q[:, :2] for q in plist]))
        start = np.zeros(len(plist) + 1, dtype=np.int32)
        np.cumsum([q.shape[0] for q in plist], out=start[1:])
        inv = self.dim / float(self.cfg.tile_len_m)
        inflate = int(np.floor(float(radius_m) * inv * 5.0))
        cmax = max(inflate + 1, inflate + 1 if clear_max is None else int(clear_max))
        shape = lead if p >= 0 or own else (self.P,) + lead
        steps = np.zeros(len(plist), dtype=np.int32)
        out = self._outputs(device)
        res = out.empty(shape + (4,), "int32")
        flags = ((_lib.RBPF_PATHS_DEVICE_OUT if device else 0) | (_lib.RBPF_PATHS_THROUGH_UNKNOWN if through_unknown else 0)
                 | (_lib.RBPF_PATHS_START_EXEMPT if start_exempt else 0) | (_lib.RBPF_PATHS_OWN if own else 0))
        with out:
            self._check(self._lib.rbpf_check_paths(self._h, p, _dp(xy), _ip(start), len(plist), inflate, cmax, flags, out.ptr(res), _ip(steps)))
        return PathCheck(res[..., 0], res[..., 1], res[..., 2], res[..., 3], steps.reshape(lead), float(self.cfg.tile_len_m) / self.dim,
                         inflate, cmax)

    # -- rollout checks (include/rbpf_hip.h: rbpf_check_rollouts; thesis_amd/plan.py) ----------------------------
    def check_rollouts(self, poses, templates, particle=None, radius_m: float = 0.0, clear_max: Optional[int] = None,
                       through_unknown: bool = False, start_exempt: bool = False, device: bool = False):
        """The same motion templates driven from every pose, placed on the GPU and checked as check_paths checks a path:
        `templates` is [K, M, 2+] (metres in the robot's frame, e.g. plan.arc_templates; further columns are ignored) or a list of
        K arrays [m_k, 2+] of 1 .. 128 waypoints, `poses` is [N, 3] (or [3]).  `particle`: an index, "best" (the first argmax of
        weights()) or None (pose p in particle p's map, N == P; e.g. poses()).  radius_m, clear_max, through_unknown and
        start_exempt are check_paths's.  The rollout of template k from pose n is plan.place_templates(poses, templates)[n, k]:
        check_paths of that gives the same numbers, but builds and uploads N * K * M points to do so.  A pose from which a
        template could leave the tile lattice is refused (RbpfError, which names it).  Returns plan.PathCheck with every field, steps too, [N, K].
        device=True: torch tensors on the engine's device, steps among them, ready for work on torch's current stream."""
        from .plan import PathCheck
        p = self._particle(particle)
        ps = _f64(poses)
        if ps.ndim == 1:
            ps = ps.reshape(1, -1)
        if ps.ndim != 2 or ps.shape[1] != 3 or ps.shape[0] < 1:
            raise ValueError("poses must be [N, 3] (or [3]), N >= 1")
        tlist = [_f64(q) for q in (list(templates) if isinstance(templates, (list, tuple)) else list(_f64(templates)))]
        if not tlist or any(q.ndim != 2 or q.shape[1] < 2 or q.shape[0] < 1 for q in tlist):
            raise ValueError("templates must be [K, M, 2+] or a list of [m, 2+] arrays, K >= 1 and every m >= 1")
        xy = np.ascontiguousarray(np.concatenate([q[:, :2] for q in tlist]))
        start = np.zeros(len(tlist) + 1, dtype=np.int32)
        np.cumsum([q.shape[0] for q in tlist], out=start[1:])
        inv = self.dim / float(self.cfg.tile_len_m)
        inflate = int(np.floor(float(radius_m) * inv * 5.0))
        cmax = max(inflate + 1, inflate + 1 if clear_max is None else int(clear_max))
        shape = (ps.shape[0], len(tlist))
        out = self._outputs(device)
        res, steps = out.empty(shape + (4,), "int32"), out.empty(shape, "int32")
        flags = ((_lib.RBPF_PATHS_DEVICE_OUT if device else 0) | (_lib.RBPF_PATHS_THROUGH_UNKNOWN if through_unknown else 0)
                 | (_lib.RBPF_PATHS_START_EXEMPT if start_exempt else 0))
        with out:
            self._check(self._lib.rbpf_check_rollouts(self._h, p, _dp(ps), ps.shape[0], _dp(xy), _ip(start), len(tlist), inflate, cmax, flags,
                                                      out.ptr(res), out.ptr(steps)))
        return PathCheck(res[..., 0], res[..., 1], res[..., 2], res[..., 3], steps, float(self.cfg.tile_len_m) / self.dim, inflate, cmax)

    # -- local map (include/rbpf_hip.h: rbpf_local_map; thesis_amd/local.py) ---------------------------------------
    def local_map(self, poses=None, particle=None, size_m: float = 6.4, cell: Optional[float] = None, samples: int = 2,
                  weights="resample", offset=(0.0, 0.0), crops: bool = False, device: bool = False):
        """What is round the robot, in the robot's frame, fused over the particles: a window of n x n cells of `cell` metres
        (default: the engine's), n = ceil(size_m / cell), cut out of the map of every pose's particle with the pose at its
        centre (moved by `offset` = (ahead, left) metres: a look-ahead window) and x forward, then summed with integer weights.
        `poses` is [N, 3] (or [3]); None: poses().  `particle`: None (pose p in particle p's map, N == P), an index, or "best"
        (the first argmax of weights()).  A cell of a cut is the largest of samples x samples map values inside it: a wall
        that crosses the cell keeps it.  `weights`: "resample" (resample_weights of weights(), as estimate() uses), "uniform" /
        None, or N non-negative values; they pass through local.quantise_weights.  Returns local.LocalMap: occ_w, free_w,
        unknown_w, sum_wv [n, n] int64 and, with crops=True, every pose's own cut [N, n, n] int8.  device=True: torch tensors
        on the engine's device, ready for work on torch's current stream."""
        from .local import LocalMap, quantise_weights
        from .mapio import resample_weights
        p = self._particle(particle)
        ps = _f64(self.poses() if poses is None else poses)
        if ps.ndim == 1:
            ps = ps.reshape(1, -1)
        if ps.ndim != 2 or ps.shape[1] != 3 or ps.shape[0] < 1:
            raise ValueError("poses must be [N, 3] (or [3]), N >= 1")
        N = ps.shape[0]
        cs = float(self.cfg.cell_size if cell is None else cell)
        if not (np.isfinite(cs) and cs > 0.0 and np.isfinite(float(size_m)) and float(size_m) > 0.0):
            raise ValueError("size_m and cell must be finite and > 0")
        n = max(1, int(np.ceil(float(size_m) / cs - 1e-9)))          # 6.4 / 0.05 is 128 whichever way the quotient rounds
        off = _f64(offset).reshape(-1)
        if off.shape != (2,):
            raise ValueError("offset must be (ahead, left) in metres")
        if weights is None or (isinstance(weights, str) and weights == "uniform"):
            wq, total = None, N
        else:
            if isinstance(weights, str):
                if weights != "resample":
                    raise ValueError(f"unknown weights {weights!r}")
                w = resample_weights(self.weights())
            else:
                w = _f64(weights).reshape(-1)
            if w.shape != (N,):
                raise ValueError(f"weights must have shape ({N},): one for every pose")
            wq = np.ascontiguousarray(quantise_weights(w))
            total = int(wq.sum(dtype=np.uint64))
        out = self._outputs(device)
        fused = out.empty((n, n, 4), "int64")
        cr = out.empty((N, n, n), "int8") if crops else None
        with out:
            self._check(self._lib.rbpf_local_map(self._h, p, _dp(ps), N, None if wq is None else wq.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 n, cs, int(samples), _dp(off), _lib.RBPF_LOCAL_DEVICE_OUT if device else 0,
                                                 out.ptr(fused), out.ptr(cr)))
        return LocalMap(occ_w=fused[..., 0], free_w=fused[..., 1], unknown_w=fused[..., 2], sum_wv=fused[..., 3], total=total, cell=cs,
                        offset=(float(off[0]), float(off[1])), crops=cr)

    # -- footprint checks (include/rbpf_hip.h: rbpf_check_footprints; thesis_amd/plan.py) -------------------------
    def check_footprints(self, poses, templates, headings, footprint, particle=None, radius_m: float = 0.0, clear_max: Optional[int] = None,
                         through_unknown: bool = False, exempt_cells: Optional[int] = None, device: bool = False):
        """check_rollouts for a robot that is no disc: every step of every rollout tests, besides its centre cell (not known free,
        or clearance <= inflate = floor(radius_m * cells per metre * 5): radius_m is the INSCRIBED radius here), the cells an
        oriented footprint covers there.  `poses` [N, 3] (or [3]) and `templates` ([K, M, 2+] or a list of [m_k, 2+], 1 .. 128
        waypoints) are check_rollouts's; `headings` is [K, M] or a list of K arrays [m_k]: the robot's heading at each waypoint
        in the robot's frame (plan.arc_headings goes with plan.arc_templates, plan.path_headings with a world path placed at the
        pose (0, 0, 0)); `footprint` is a plan.Footprint (plan.footprint_table of the robot's outline, cut for this engine's cell
        size).  A step on a waypoint tests the heading bin of every waypoint it stands on - a turn on the spot sweeps the corners -
        and a step between two waypoints that of the nearer one.  `particle`: an index or "best": every pose in that map, [N, K];
        None: pose p in particle p's map (N == P), or one pose in EVERY particle's map (N == 1), [P, K].  exempt_cells: cells
        within this Chebyshev distance of a rollout's first cell block nothing (the robot is where it is); None: no exemption.
        Returns plan.PathCheck as check_rollouts does, min_clearance and steps equal to its; first_unknown and n_unknown count the
        steps at which the centre or a covered cell is unknown.  device=True: torch tensors on the engine's device."""
        from .plan import PathCheck, heading_bins
        p = self._particle(particle)
        ps = _f64(poses)
        if ps.ndim == 1:
            ps = ps.reshape(1, -1)
        if ps.ndim != 2 or ps.shape[1] != 3 or ps.shape[0] < 1:
            raise ValueError("poses must be [N, 3] (or [3]), N >= 1")
        tlist = [_f64(q) for q in (list(templates) if isinstance(templates, (list, tuple)) else list(_f64(templates)))]
        if not tlist or any(q.ndim != 2 or q.shape[1] < 2 or q.shape[0] < 1 for q in tlist):
            raise ValueError("templates must be [K, M, 2+] or a list of [m, 2+] arrays, K >= 1 and every m >= 1")
        hlist = [_f64(q).reshape(-1) for q in (list(headings) if isinstance(headings, (list, tuple)) else list(_f64(headings)))]
        if len(hlist) != len(tlist) or any(a.shape[0] != q.shape[0] for a, q in zip(hlist, tlist)):
            raise ValueError("headings must hold one heading for every waypoint of every template")
        H = int(footprint.H)
        spans = np.ascontiguousarray(footprint.spans, dtype=np.int32).reshape(-1, 3)
        offsets = np.ascontiguousarray(footprint.offsets, dtype=np.int32).reshape(-1)
        if offsets.shape[0] != H + 1 or (H >= 1 and int(offsets[-1]) != spans.shape[0]):
            raise ValueError("footprint.offsets must be [H + 1] and end at the number of spans")
        if abs(float(footprint.cell) - float(self.cfg.tile_len_m) / self.dim) > 1e-9 * float(footprint.cell):
            raise ValueError("the footprint table was cut for another cell size")
        xy = np.ascontiguousarray(np.concatenate([q[:, :2] for q in tlist]))
        tbin = np.ascontiguousarray(heading_bins(np.concatenate(hlist), H))
        start = np.zeros(len(tlist) + 1, dtype=np.int32)
        np.cumsum([q.shape[0] for q in tlist], out=start[1:])
        inv = self.dim / float(self.cfg.tile_len_m)
        inflate = int(np.floor(float(radius_m) * inv * 5.0))
        cmax = max(inflate + 1, inflate + 1 if clear_max is None else int(clear_max))
        shape = (ps.shape[0] if p >= 0 else self.P, len(tlist))
        out = self._outputs(device)
        res, steps = out.empty(shape + (4,), "int32"), out.empty(shape, "int32")
        flags = (_lib.RBPF_PATHS_DEVICE_OUT if device else 0) | (_lib.RBPF_PATHS_THROUGH_UNKNOWN if through_unknown else 0)
        with out:
            self._check(self._lib.rbpf_check_footprints(self._h, p, _dp(ps), ps.shape[0], _dp(xy), _ip(tbin), _ip(start), len(tlist), _ip(spans),
                                                        _ip(offsets), H, inflate, cmax, -1 if exempt_cells is None else int(exempt_cells), flags,
                                                        out.ptr(res), out.ptr(steps)))
        return PathCheck(res[..., 0], res[..., 1], res[..., 2], res[..., 3], steps, float(self.cfg.tile_len_m) / self.dim, inflate, cmax)

    # -- frontier regions (include/rbpf_hip.h: rbpf_frontier_regions; thesis_amd/explore.py) ----------------------
    def frontier_regions(self, particle="best", box=None, clearance_cells: int = 4, min_size: int = 1, max_regions: int = 64,
                         labels: bool = True, device: bool = False):
        """The frontier of a particle's map as regions: the known-free cells of `box` = (x0, x1, y0, y1) in mosaic cells (default
        map_extent of the particle, or of all particles with particle=None) that touch an unknown cell and have no occupied cell
        within `clearance_cells` on either axis, joined into 8-connected regions.  `particle`: an index or "best" (the first argmax
        of weights()): returns explore.Frontiers(label, regions, counts, box, cell) with label int32 [x1-x0, y1-y0] (the smallest
        dx * ny + dy of the cell's region, -1 off the frontier; None with labels=False), regions a structured array [max_regions]
        with the fields explore.REGION_FIELDS (the regions of at least `min_size` cells, largest first, ties to the smaller label;
        every field -1 past the last) and counts int32 [3]: frontier cells, regions, regions in the table.  particle=None: every
        particle in its own map, regions [P, max_regions], counts [P, 3], no label.  device=True: torch tensors on the engine's
        device (regions as int64 [..., 10]), ready for work on torch's current stream."""
        from .explore import Frontiers, REGION_DTYPE
        p = self._particle(particle)
        b, shape = _box4(box, lambda: self.map_extent(None if p < 0 else p) or (0, 0, 0, 0))
        K = int(max_regions)
        lead = () if p >= 0 else (self.P,)
        out = self._outputs(device)
        outs = [out.empty(shape, "int32") if labels and p >= 0 else None, out.empty(lead + (max(K, 0), 10), "int64"),
                out.empty(lead + (3,), "int32")]
        with out:
            self._check(self._lib.rbpf_frontier_regions(self._h, p, _ip(b), int(clearance_cells), int(min_size), K,
                                                        _lib.RBPF_FRONTIER_DEVICE_OUT if device else 0, *map(out.ptr, outs)))
        regions = outs[1] if device else outs[1].view(REGION_DTYPE)[..., 0]
        return Frontiers(outs[0], regions, outs[2], tuple(int(x) for x in b), float(self.cfg.tile_len_m) / self.dim)

    def frontier_stats(self) -> Dict[str, int]:
        """How the last frontier_regions went: labelling rounds, block runs and (particle, block) pairs, as travel_stats."""
        out = (C.c_uint64 * 3)()
        self._check(self._lib.rbpf_frontier_stats(self._h, out))
        return {"rounds": int(out[0]), "block_runs": int(out[1]), "blocks": int(out[2])}

    # -- map scores (include/rbpf_hip.h: rbpf_score_maps; thesis_amd/mapeval.py) --------------------------------
    def score_maps(self, reference, particle=None, box=None, tol_cells: int = 1, table=None, device: bool = False):
        """How close the particles' maps are to `reference`: a MapRaster with int8 cells (its box is its own), an int8 array
        [x1-x0, y1-y0] with `box` = (x0, x1, y0, y1) in mosaic cells, or an int8 torch tensor on the engine's device with `box`
        (read on the GPU, in torch's stream order).  `particle`: None (every particle in its own map), an index or "best" (the
        first argmax of weights()).  Returns mapeval.MapScores: the 3 x 3 table n[class of the map][class of the reference] over
        the classes free, unknown, occupied; hit_m / hit_r, the occupied cells of the map / of the reference that have an
        occupied cell of the other side within `tol_cells` (0 .. 16) on either axis; l1, the sum of |v - r|; tab, the sum of
        table[v - vmin] over the box (`table` as view_gain's, default explore.entropy_table(cfg): tab / 65536 is the map's
        entropy in bits).  All exact integers; leading shape [P] with particle=None.  device=True: the raw int64 tensor
        [..., 13] on the engine's device (the fields in the order of include/rbpf_hip.h), ready for work on torch's current
        stream; mapeval.MapScores.from_fields reads it."""
        from .mapeval import MapScores
        p = self._particle(particle)
        cells = reference
        if hasattr(reference, "cells") and hasattr(reference, "x0"):      # a MapRaster
            if reference.cells is None:
                raise ValueError("the reference raster has no int8 cells (a whole-filter render has prob / occ_frac): "
                                 "mapeval.consensus converts them")
            if abs(float(reference.quantum) - float(self.cfg.quantum)) > 1e-9 * abs(float(self.cfg.quantum)):
                raise ValueError(f"reference quantum = {reference.quantum!r} differs from the engine's {self.cfg.quantum!r}")
            cells = reference.cells
            if box is None:
                box = (reference.x0, reference.x0 + int(cells.shape[0]), reference.y0, reference.y0 + int(cells.shape[1]))
        if box is None:
            raise ValueError("an array reference needs box = (x0, x1, y0, y1)")
        b, _ = _box4(box, None)
        shape = (int(b[1]) - int(b[0]), int(b[3]) - int(b[2]))           # not clamped: no reference fits a bad box
        cells, have = self._int8_cells(cells, "reference", "[nx][ny]")
        if tuple(have) != shape:
            raise ValueError(f"reference shape {tuple(have)} differs from the box's {shape}")
        tab = self._value_table(table)
        out = self._outputs(device)
        out.adopt(cells)
        fields = out.empty(((self.P,) if p < 0 else ()) + (_lib.RBPF_SCORE_FIELDS,), "int64")
        flags = (_lib.RBPF_SCORE_DEVICE_IN if hasattr(cells, "data_ptr") else 0) | (_lib.RBPF_SCORE_DEVICE_OUT if device else 0)
        with out:
            self._check(self._lib.rbpf_score_maps(self._h, p, _ip(b), out.ptr(cells), int(tol_cells), _ip(tab), flags, out.ptr(fields)))
        if device:
            return fields
        return MapScores.from_fields(fields, tuple(int(x) for x in b), int(tol_cells), float(self.cfg.quantum))

    # -- global localization (include/rbpf_hip.h: rbpf_locate_scan; thesis_amd/locate.py) ---------------------------------------
    def locate_scan(self, ranges, angles, particle="best", box=None, n_rot: int = 720, device: bool = False):
        """Scores the scan (`ranges` [B], `angles` [B], sensor frame) at every observed-free cell and each of `n_rot`
        headings of `box` = (x0, x1, y0, y1) in mosaic cells (default map_extent(particle)) in a particle's map:
        `particle` an index or "best" (the first argmax of weights()).  Returns (best, rot, box): int32 [x1-x0, y1-y0]
        rasters of the best score per cell and the smallest rotation index that attains it, -1 where no robot can stand
        (locate.hypotheses turns them into poses).  device=True: torch tensors on the engine's device, ready
        for work on torch's current stream."""
        p = self._particle(particle, allow_none=False)
        r, a = _f64(ranges), _f64(angles)
        if r.ndim != 1 or a.shape != r.shape:
            raise ValueError("ranges and angles must be 1-D and of equal length")
        b, shape = _box4(box, lambda: self.map_extent(p) or (0, 0, 0, 0))
        out = self._outputs(device)
        best, rot = out.empty(shape, "int32"), out.empty(shape, "int32")
        with out:
            self._check(self._lib.rbpf_locate_scan(self._h, p, _ip(b), _dp(r), _dp(a), r.shape[0], int(n_rot),
                                                   _lib.RBPF_LOCATE_DEVICE_OUT if device else 0, out.ptr(best), out.ptr(rot)))
        return best, rot, tuple(int(x) for x in b)

    def relocalize(self, ranges, angles, particle="best", k: int = 8, n_rot: int = 720, seed: int = 0, box=None,
                   nms_cells: int = 10):
        """Starts the filter anywhere in a known map: locate_scan, then locate.hypotheses, then set_state with the particles
        shared among the hypotheses in proportion to their scores (locate.seed_particles), covariances 0 and weights 1.
        Returns the hypotheses (locate.Hypotheses); the filter then runs as after any set_state."""
        from . import locate
        best, rot, box = self.locate_scan(ranges, angles, particle=particle, box=box, n_rot=n_rot)
        r = _f64(ranges)
        n_used = int(np.count_nonzero((r > float(self.cfg.match_min_range)) & (r < float(self.cfg.match_max_range))))
        cell = float(self.cfg.tile_len_m) / self.dim
        hyp = locate.hypotheses(best, rot, box, n_rot, cell, k=k, nms_cells=nms_cells, n_used=n_used)
        if len(hyp.poses) == 0:
            raise ValueError("the box holds no observed-free cell: nothing to relocalize in")
        self.set_state(poses=locate.seed_particles(hyp, self.P, cell, n_rot, seed), covs=0.0, weights=1.0)
        return hyp

    # -- alignment of a map of unknown pose (include/rbpf_hip.h: rbpf_align_points; thesis_amd/align.py) --------
    def align_points(self, occ_xy, free_xy=None, particle="best", box=None, n_rot: int = 720, rot_window=None,
                     device: bool = False):
        """Scores a point set of unknown pose - `occ_xy` [n, 2] occupied and `free_xy` [m, 2] free points, metres in a frame
        of their own - at every cell of `box` = (x0, x1, y0, y1) in mosaic cells (default map_extent(particle)) and every
        rotation of `rot_window` = (r_begin, r_count) out of `n_rot` (default all) in a particle's map: `particle` an index
        or "best" (the first argmax of weights()).  score = sum of F over the occupied points - 2 * the free points that land
        on an occupied cell.  Returns (best, rot, box): int32 [x1-x0, y1-y0] rasters of the best score per
        cell and the smallest rotation index of the window that attains it.  device=True: torch tensors on the engine's
        device, ready for work on torch's current stream."""
        p = self._particle(particle, allow_none=False)
        o = _f64(occ_xy)
        f = _f64(np.empty((0, 2)) if free_xy is None else free_xy)
        if o.ndim != 2 or o.shape[1] != 2 or f.ndim != 2 or f.shape[1] != 2:
            raise ValueError("occ_xy and free_xy must be [n, 2]")
        b, shape = _box4(box, lambda: self.map_extent(p) or (0, 0, 0, 0))
        r_begin, r_count = (0, int(n_rot)) if rot_window is None else (int(rot_window[0]), int(rot_window[1]))
        out = self._outputs(device)
        best, rot = out.empty(shape, "int32"), out.empty(shape, "int32")
        with out:
            self._check(self._lib.rbpf_align_points(self._h, p, _ip(b), _dp(o), o.shape[0], _dp(f) if f.shape[0] else None, f.shape[0],
                                                    int(n_rot), r_begin, r_count, _lib.RBPF_ALIGN_DEVICE_OUT if device else 0,
                                                    out.ptr(best), out.ptr(rot)))
        return best, rot, tuple(int(x) for x in b)

    def align_map(self, src, particle="best", k: int = 4, n_rot: int = 360, refine: int = 8, box=None):
        """Finds where the map `src` (a mapio.SourceMap whose frame is unknown) fits a particle's map: its occupied and free
        cells become a point set (align.points_from_source), a coarse align_points pass over `box` (default
        map_extent(particle)) at `n_rot` rotations gives up to `k` hypotheses, and a fine pass at n_rot * refine rotations
        (one coarse step either way, 5 x 5 cells) sharpens each.  Returns locate.Hypotheses, best first: poses[n] is the
        rigid transform for src.moved, e.g. place_map(src.moved(hyp.poses[0]), mode="add")."""
        from . import align
        p = self._particle(particle, allow_none=False)
        if box is None:
            box = self.map_extent(p)
            if box is None:
                raise ValueError("the particle's map is empty: nothing to align to")
        lo = -int(self.cfg.lattice_radius) * self.dim - self.dim // 2
        limits = (lo, lo + (2 * int(self.cfg.lattice_radius) + 1) * self.dim)

        def search(occ_xy, free_xy, bx, nr, r_begin, r_count):
            return self.align_points(occ_xy, free_xy, particle=p, box=bx, n_rot=nr, rot_window=(r_begin, r_count))[:2]
        return align.align_map(search, src, float(self.cfg.occupied_threshold), float(self.cfg.tile_len_m) / self.dim, box, limits,
                               k=k, n_rot=n_rot, refine=refine)

    # -- pose estimate and trajectory log (include/rbpf_hip.h: rbpf_estimate, rbpf_track_*; thesis_amd/trajectory.py) --
    WEIGHT_MODES = {"uniform": _lib.RBPF_W_UNIFORM, "resample": _lib.RBPF_W_RESAMPLE}

    def _weights_arg(self, weights):
        """(mode, array kept alive or None) of a `weights` argument: "resample", "uniform" or None (uniform), or P values."""
        if weights is None:
            return _lib.RBPF_W_UNIFORM, None
        if isinstance(weights, str):
            if weights not in self.WEIGHT_MODES:
                raise ValueError(f"unknown weights {weights!r}")
            return self.WEIGHT_MODES[weights], None
        w = _f64(weights)
        if w.shape != (self.P,):
            raise ValueError(f"weights must have shape ({self.P},)")
        return _lib.RBPF_W_GIVEN, w

    def estimate(self, weights="resample") -> Estimate:
        """The filter's pose estimate, computed on the device: weighted mean pose (circular mean heading), covariance, mean
        resultant length, effective sample size and the heaviest particle.  `weights`: "resample" (resample_weights of
        weights(), the distribution the resample draws from), "uniform" / None, or P non-negative values.  A particle with
        weight 0 or a non-finite pose or weight is left out.  Needs no tracking; two calls on the same state agree bit for bit."""
        mode, w = self._weights_arg(weights)
        f, i = np.empty(_lib.RBPF_EST_F64), np.empty(_lib.RBPF_EST_I32, dtype=np.int32)
        self._check(self._lib.rbpf_estimate(self._h, mode, None if w is None else _dp(w), _dp(f), _ip(i)))
        return Estimate(pose=f[0:3].copy(), cov=_cov_from_rows(f), resultant=float(f[9]), n_eff=float(f[11]), best=int(i[0]),
                        n_used=int(i[1]), weight_sum=float(f[10]))

    def pose_modes(self, bin_xy: float = 0.5, heading_bins: int = 36, max_modes: int = 8, weights="resample", labels: bool = False,
                   device: bool = False) -> Modes:
        """The modes of the particle cloud, clustered on the device: connected components of the occupied bins of a lattice of
        bin_xy metres and 2 pi / heading_bins (26-neighbourhood, cyclic heading), heaviest first, one estimate per mode
        (Modes; `weights` as estimate()).  While the filter is multimodal - after relocalize(), in a symmetric building -
        estimate() averages hypotheses; this tells them apart, and locate.converged(modes) says when one is left.  Needs no
        tracking, changes nothing.  device=True: torch tensors on the engine's device, ready for work on torch's current stream."""
        mode, w = self._weights_arg(weights)
        bxy, n_th, K = float(bin_xy), int(heading_bins), int(max_modes)
        Kc = min(max(K, 0), _lib.RBPF_MODES_MAX)          # bad parameters are the library's to refuse
        out = self._outputs(device)
        info, f, i = out.empty(4, "int64"), out.empty((Kc, _lib.RBPF_EST_F64), "float64"), out.empty((Kc, _lib.RBPF_EST_I32), "int32")
        lab = out.empty(self.P, "int32") if labels else None
        with out:
            self._check(self._lib.rbpf_pose_modes(self._h, mode, None if w is None else _dp(w), bxy, n_th, K,
                                                  _lib.RBPF_MODES_DEVICE_OUT if device else 0, *map(out.ptr, (info, f, i, lab))))
        k = Kc if device else min(int(info[0]), Kc)
        f, i = f[:k], i[:k]
        return Modes(count=info[0] if device else int(info[0]), bins=info[1] if device else int(info[1]),
                     used=info[2] if device else int(info[2]), poses=f[:, 0:3], covs=_cov_from_rows(f), share=f[:, 13], size=i[:, 1],
                     mode_bins=i[:, 2], root=i[:, 3], best=i[:, 0], resultant=f[:, 9], n_eff=f[:, 11], weight_sum=f[:, 10], labels=lab)

    def trajectory_modes(self, bin_xy: float = 0.5, heading_bins: int = 36, max_modes: int = 4, weights="resample", t0: int = 0,
                         t1: Optional[int] = None) -> TrajectoryModes:
        """The smoothed form of pose_modes, the companion of trajectory_summary: per record the modes of the poses the current
        particles' ancestors had there, with the FINAL weights.  Where n_alive of the summary says how many lineages survive,
        count says where along the path they still disagree by more than a bin.  P <= 65536."""
        if t1 is None:
            t1 = self.track_info()["n_records"]
        mode, w = self._weights_arg(weights)
        bxy, n_th, K = float(bin_xy), int(heading_bins), int(max_modes)
        T, Kc = max(int(t1) - int(t0), 0), min(max(K, 0), _lib.RBPF_MODES_MAX)
        info, f, i = np.empty((T, 4), dtype=np.int64), np.empty((T, Kc, _lib.RBPF_EST_F64)), np.empty((T, Kc, _lib.RBPF_EST_I32), dtype=np.int32)
        vp = lambda a: C.c_void_p(a.ctypes.data or 1)
        self._check(self._lib.rbpf_track_modes(self._h, int(t0), int(t1), mode, None if w is None else _dp(w), bxy, n_th, K, vp(info), vp(f), vp(i)))
        return TrajectoryModes(count=info[:, 0].copy(), share=f[:, :, 13].copy(), poses=f[:, :, 0:3].copy(), size=i[:, :, 1].copy())

    def track(self, capacity: int, imu: bool = False, scan: bool = True):
        """Starts the trajectory log on the device: room for `capacity` records of every particle's pose and parent (28 bytes per
        particle and record), record 0 from the current state.  scan=True: every scan_update / scan_update_end records;
        imu=True: every imu_update too; record() adds one at any time.  Nothing is read back while the filter runs.  Off by
        default; untrack() frees the log."""
        flags = (_lib.RBPF_TRACK_IMU if imu else 0) | (_lib.RBPF_TRACK_SCAN if scan else 0)
        self._check(self._lib.rbpf_track_begin(self._h, int(capacity), flags))

    def untrack(self):
        self._check(self._lib.rbpf_track_end(self._h))

    def record(self):
        """One record of the current state; an RbpfError (RBPF_ENOMEM) when the log is full."""
        self._check(self._lib.rbpf_track_record(self._h))

    def track_info(self) -> Dict[str, int]:
        """{"n_records", "capacity", "dropped" (records a full log refused), "imu", "scan"}; an RbpfError with tracking off."""
        n, cap, dr, fl = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint32()
        self._check(self._lib.rbpf_track_info(self._h, C.byref(n), C.byref(cap), C.byref(dr), C.byref(fl)))
        return {"n_records": n.value, "capacity": cap.value, "dropped": dr.value, "imu": bool(fl.value & _lib.RBPF_TRACK_IMU),
                "scan": bool(fl.value & _lib.RBPF_TRACK_SCAN)}

    def lineage(self, particles=None, t0: int = 0, t1: Optional[int] = None, poses: bool = True, device: bool = False):
        """Where the current particles come from: (idx, pose) with idx int32 [t1-t0, n], the index in record t of the ancestor of
        current particle particles[k] (None: all P), and pose float64 [t1-t0, n, 3], that ancestor's recorded pose (None with
        poses=False).  t1 defaults to the number of records.  device=True: torch tensors on the engine's device, ready for
        work on torch's current stream."""
        if t1 is None:
            t1 = self.track_info()["n_records"]
        pl = None
        if particles is not None:
            pl = np.ascontiguousarray(particles, dtype=np.int32).reshape(-1)
        n = self.P if pl is None else len(pl)
        T = max(int(t1) - int(t0), 0)                     # a bad range is the library's to refuse
        out = self._outputs(device)
        idx = out.empty((T, n), "int32")
        pose = out.empty((T, n, 3), "float64") if poses else None
        with out:
            self._check(self._lib.rbpf_track_lineage(self._h, int(t0), int(t1), None if pl is None else _ip(pl), 0 if pl is None else len(pl),
                                                     out.ptr(idx), out.ptr(pose), _lib.RBPF_TRACK_DEVICE_OUT if device else 0))
        return idx, pose

    def trajectory(self, particle="best") -> np.ndarray:
        """[T, 3]: the recorded poses of the ancestors of one current particle (an index, or "best": estimate().best), one row
        per record."""
        if isinstance(particle, str) and particle == "best":
            particle = self.estimate().best
        return self.lineage([self._particle(particle, allow_none=False)])[1][:, 0, :]

    def trajectory_summary(self, weights="resample", t0: int = 0, t1: Optional[int] = None) -> TrajectorySummary:
        """The smoothed trajectory: per record the estimate (as estimate(), `weights` likewise) over the poses the current
        particles' ancestors had there, weighted with the FINAL weights, and n_alive, the number of distinct ancestors
        (trajectory.coalescence finds where the lineages merge).  P <= 65536."""
        if t1 is None:
            t1 = self.track_info()["n_records"]
        mode, w = self._weights_arg(weights)
        T = max(int(t1) - int(t0), 0)
        f, i = np.empty((T, _lib.RBPF_EST_F64)), np.empty((T, _lib.RBPF_EST_I32), dtype=np.int32)
        self._check(self._lib.rbpf_track_summary(self._h, int(t0), int(t1), mode, None if w is None else _dp(w), _dp(f), _ip(i)))
        return _summary_from_rows(f, i)

    def filtered_trajectory(self, t0: int = 0, t1: Optional[int] = None) -> TrajectorySummary:
        """The filtered trajectory: the estimate each record stored when it was written (weights "resample" of that moment);
        n_alive is -1."""
        if t1 is None:
            t1 = self.track_info()["n_records"]
        T = max(int(t1) - int(t0), 0)
        f, i = np.empty((T, _lib.RBPF_EST_F64)), np.empty((T, _lib.RBPF_EST_I32), dtype=np.int32)
        self._check(self._lib.rbpf_track_filtered(self._h, int(t0), int(t1), _dp(f), _ip(i)))
        return _summary_from_rows(f, i)

    def _track_export(self) -> Optional[Dict[str, np.ndarray]]:
        """The log as checkpoint entries, or None with tracking off."""
        n, cap, dr, fl = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint32()
        if self._lib.rbpf_track_info(self._h, C.byref(n), C.byref(cap), C.byref(dr), C.byref(fl)) != 0:
            return None
        blob = np.empty(n.value * int(self._lib.rbpf_track_record_bytes(self._h)) + 4 * self.P, dtype=np.uint8)
        self._check(self._lib.rbpf_track_export(self._h, 0, n.value, C.c_void_p(blob.ctypes.data)))
        return {"track_state": np.array([n.value, cap.value, fl.value], dtype=np.int64), "track_records": blob}

    def _track_import(self, state, blob):
        n, cap, fl = (int(x) for x in state)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        if blob.size != n * int(self._lib.rbpf_track_record_bytes(self._h)) + 4 * self.P:
            raise ValueError("the checkpoint's trajectory log does not fit this engine")
        self._check(self._lib.rbpf_track_begin(self._h, cap, fl))
        self._check(self._lib.rbpf_track_import(self._h, n, C.c_void_p(blob.ctypes.data)))

    # -- map building (include/rbpf_hip.h: rbpf_build_map; thesis_amd/rebuild.py) ------------------------------
    def build_map(self, poses, ranges, angles, cell_size: Optional[float] = None, box=None, min_range: float = 0.0,
                  max_range: Optional[float] = None, device: bool = False, into: Optional[BuiltMap] = None) -> BuiltMap:
        """The map that the scans `ranges` [N, B] (beam directions `angles` [B]) draw from the sensor poses `poses` [N, 3]: per
        cell of `box` = (x0, x1, y0, y1), in how many scans a beam returned from it (hits) and in how many a beam passed or ended
        in it (seen), int32 [x1-x0, y1-y0].  No particle's map is read.  `cell_size` is any size in metres (cells per metre =
        1 / cell_size); None is the engine's own dim / tile_len, and the cells are then those of render_map.  `box` defaults to
        the smallest box holding every pose's window, floor(x * cells per metre) -+ (ceil(max_range * cells per metre) + 2) on
        each axis.  Beams shorter than `min_range` or NaN are skipped, beams longer than `max_range` (default cfg.max_ray_m) are
        free to max_range and hit nothing.  `into`: an earlier BuiltMap of the same geometry, added to in place (a long log in
        chunks).  device=True: torch tensors on the engine's device, ready for work on torch's current stream."""
        ps, rg, a = _scan_batch(poses, ranges, angles)
        inv = self.dim / float(self.cfg.tile_len_m) if cell_size is None else 1.0 / float(cell_size)
        cs = float(self.cfg.cell_size) if cell_size is None else float(cell_size)
        mr = float(self.cfg.max_ray_m if max_range is None else max_range)
        if into is not None:
            if box is not None and tuple(int(q) for q in box) != (into.x0, into.x0 + into.hits.shape[0], into.y0, into.y0 + into.hits.shape[1]):
                raise ValueError("box differs from the box of `into`")
            if into.cells_per_m != inv or into.hits.shape != into.seen.shape:
                raise ValueError("`into` was built at another cell size")
            box = (into.x0, into.x0 + into.hits.shape[0], into.y0, into.y0 + into.hits.shape[1])
            device = not isinstance(into.hits, np.ndarray)
        b4, shape = _box4(box, lambda: self.build_box(ps, inv, mr))
        flags = (_lib.RBPF_BUILD_DEVICE_OUT if device else 0) | (_lib.RBPF_BUILD_ACCUMULATE if into is not None else 0)
        out = self._outputs(device)
        if into is None:
            outs = [out.empty(shape, "int32") for _ in range(2)]
        else:
            outs = [out.adopt(into.hits), out.adopt(into.seen)]           # tensors were last written in torch's stream order
            if device and any(o.dtype != out.torch.int32 or not o.is_contiguous() or o.device != out.dev for o in outs):
                raise ValueError("`into` must hold contiguous int32 tensors on the engine's device")
            if not device and any(o.dtype != np.int32 or not o.flags.c_contiguous or not o.flags.writeable for o in outs):
                raise ValueError("`into` must hold contiguous, writeable int32 arrays")
        with out:
            self._check(self._lib.rbpf_build_map(self._h, _dp(ps), ps.shape[0], _dp(rg), _dp(a), a.shape[0], inv, _ip(b4), float(min_range),
                                                 mr, flags, *map(out.ptr, outs)))
        return BuiltMap(outs[0], outs[1], int(b4[0]), int(b4[2]), cs, inv)

    @staticmethod
    def build_box(poses, cells_per_m: float, max_range: float) -> Tuple[int, int, int, int]:
        """build_map's default box (x0, x1, y0, y1): the smallest one holding the window of every pose, the cells within
        ceil(max_range * cells_per_m) + 2 of floor(x * cells_per_m) on each axis."""
        ps = _f64(poses).reshape(-1, 3)
        if not (len(ps) and np.all(np.isfinite(ps)) and np.isfinite(max_range * cells_per_m)):
            raise ValueError("poses, cell size and max_range must be finite")
        m = int(np.ceil(max_range * cells_per_m)) + 2
        fx, fy = np.floor(ps[:, 0] * cells_per_m), np.floor(ps[:, 1] * cells_per_m)
        return (int(fx.min()) - m, int(fx.max()) + m + 1, int(fy.min()) - m, int(fy.max()) + m + 1)

    # -- pose refinement (include/rbpf_hip.h: rbpf_refine_poses; thesis_amd/refine.py) --------------------------
    def refine_poses(self, poses, ranges, angles, particle="best", substeps: int = 4, window: int = 12, rotations: int = 10,
                     rot_step: float = 0.004363323129985824, min_range: Optional[float] = None, max_range: Optional[float] = None,
                     return_scores: bool = False, device: bool = False) -> RefineResult:
        """The pose near each guess `poses` [N, 3] that fits the scan `ranges` [N, B] (beam directions `angles` [B]) best in a
        particle's map: `particle` an index or "best" (the first argmax of weights()).  Every translation of -window .. window
        steps of cell_size / substeps on each axis and every rotation of -rotations .. rotations steps of `rot_step` radians
        (default 0.25 degrees) is scored by the sum of F = occ + dil at the end cells of the beams with min_range < range <
        max_range (defaults cfg.match_min_range, cfg.match_max_range); ties go to the smallest rotation, then the shortest
        translation, so a guess that is already best comes back bit for bit.  A [3] pose with a [B] scan is N = 1.
        return_scores: the whole score volume as well.  max_range is limited by the window that fits one workgroup's LDS
        (refine_max_range).  device=True: torch tensors on the engine's device, ready for work on torch's current stream."""
        p = self._particle(particle, allow_none=False)
        ps, rg, a = _scan_batch(poses, ranges, angles)
        n, nw, nk = ps.shape[0], 2 * int(window) + 1, 2 * int(rotations) + 1
        lo = float(self.cfg.match_min_range if min_range is None else min_range)
        hi = float(self.cfg.match_max_range if max_range is None else max_range)
        out = self._outputs(device)
        outs = [out.empty((n, 3), "float64"), out.empty((n, 6), "int32"),
                out.empty((n, max(nk, 0), max(nw, 0), max(nw, 0)), "int32") if return_scores else None]   # a bad window is the library's to refuse
        with out:
            self._check(self._lib.rbpf_refine_poses(self._h, p, _dp(ps), n, _dp(rg), _dp(a), a.shape[0], lo, hi, int(substeps),
                                                    int(window), int(rotations), float(rot_step), *map(out.ptr, outs),
                                                    _lib.RBPF_REFINE_DEVICE_OUT if device else 0))
        n6 = outs[1]
        return RefineResult(outs[0], n6[:, 0:3], n6[:, 3], n6[:, 4], n6[:, 5], outs[2], int(substeps),
                            float(rot_step), float(self.cfg.cell_size))

    def refine_max_range(self, substeps: int = 4, window: int = 12) -> float:
        """The largest max_range refine_poses admits at this cell size for a window of `window` steps of cell_size / substeps:
        ceil(max_range * cells per metre) + ceil(window / substeps) + 2 <= 367 (include/rbpf_hip.h, the window limit)."""
        return self.match_max_range(None, substeps, window)

    # -- pair matching (include/rbpf_hip.h: rbpf_match_pairs; thesis_amd/loops.py) -------------------------------
    def match_pairs(self, poses, ranges, angles, pairs, guesses=None, cell_size: Optional[float] = None, substeps: int = 1,
                    window: int = 16, rotations: int = 20, rot_step: float = 0.008726646259971648, min_range: Optional[float] = None,
                    max_range: Optional[float] = None, return_scores: bool = False, device: bool = False) -> PairResult:
        """Where the query scan of each pair sits among the pair's reference scans: `pairs` [M, 3] = (q, r0, r1) matches scan q
        of `ranges` [N, B] (beam directions `angles` [B]) against the scans r0 .. r1 - 1 drawn at their poses `poses` [N, 3].  No
        particle's map is read: the run's end points are the map, as occ + dil over cells of `cell_size` metres (None: the
        engine's tile_len / dim).  `guesses` [M, 3] are the guessed poses of the queries (None: poses[q]).  The search is
        refine_poses's: every translation of -window .. window steps of cell_size / substeps and every rotation of -rotations ..
        rotations steps of `rot_step` radians (default 0.5 degrees) round the guess, beams with min_range < range < max_range
        (defaults cfg.match_min_range, cfg.match_max_range), the same tie order, so a guess that is already best comes back bit
        for bit.  A [3] triple is M = 1.  return_scores: the whole score volume as well.  max_range is limited as in
        refine_poses (match_max_range).  device=True: torch tensors on the engine's device, ready for work on torch's current
        stream."""
        ps, rg, a = _scan_batch(poses, ranges, angles)
        pr = np.ascontiguousarray(pairs, dtype=np.int32)
        if pr.ndim == 1:
            pr = pr.reshape(1, -1)
        if pr.ndim != 2 or pr.shape[1] != 3:
            raise ValueError("pairs must be [M, 3]")
        m = pr.shape[0]
        gs = None
        if guesses is not None:
            gs = _f64(guesses).reshape(-1, 3) if np.ndim(guesses) == 1 else _f64(guesses)
            if gs.shape != (m, 3):
                raise ValueError("guesses must be [M, 3]")
        inv = self.dim / float(self.cfg.tile_len_m) if cell_size is None else 1.0 / float(cell_size)
        cs = float(self.cfg.cell_size) if cell_size is None else float(cell_size)
        nw, nk = 2 * int(window) + 1, 2 * int(rotations) + 1
        lo = float(self.cfg.match_min_range if min_range is None else min_range)
        hi = float(self.cfg.match_max_range if max_range is None else max_range)
        out = self._outputs(device)
        outs = [out.empty((m, 3), "float64"), out.empty((m, 8), "int32"),
                out.empty((m, max(nk, 0), max(nw, 0), max(nw, 0)), "int32") if return_scores else None]   # a bad window is the library's to refuse
        with out:
            self._check(self._lib.rbpf_match_pairs(self._h, _dp(ps), ps.shape[0], _dp(rg), _dp(a), a.shape[0], _ip(pr), m,
                                                   None if gs is None else _dp(gs), inv, lo, hi, int(substeps), int(window), int(rotations),
                                                   float(rot_step), *map(out.ptr, outs), _lib.RBPF_PAIRS_DEVICE_OUT if device else 0))
        m8 = outs[1]
        return PairResult(outs[0], m8[:, 0:3], m8[:, 3], m8[:, 4], m8[:, 5], m8[:, 6], outs[2], int(substeps),
                          float(rot_step), cs)

    def match_max_range(self, cell_size: Optional[float] = None, substeps: int = 1, window: int = 16) -> float:
        """The largest max_range match_pairs admits at `cell_size` (None: the engine's) for a window of `window` steps of
        cell_size / substeps: refine_max_range's limit at that cell size."""
        reach = int(self._lib.rbpf_refine_max_reach(int(substeps), int(window)))
        if reach < 0:
            raise ValueError("substeps must be 1, 2, 4, 8 or 16 and 0 <= window <= 32")
        inv = self.dim / float(self.cfg.tile_len_m) if cell_size is None else 1.0 / float(cell_size)
        most = reach / inv
        return float(np.nextafter(most, 0.0)) if np.ceil(most * inv) > reach else most

    # -- places by appearance (include/rbpf_hip.h: rbpf_describe_scans, rbpf_match_places; thesis_amd/loops.py) ---
    def describe_scans(self, ranges, angles, rings: int = 24, min_range: Optional[float] = None, max_range: Optional[float] = None,
                       device: bool = False) -> ScanDescriptors:
        """What each scan looks like from where it was taken: `ranges` [N, B] (beam directions `angles` [B]) become polar
        occupancy images of `rings` rings (1 .. 32) between 0 and max_range and 64 sectors of 5.625 degrees, one 64-bit word a
        ring, bit j sector j, from the beams with min_range < range < max_range (defaults cfg.match_min_range,
        cfg.match_max_range).  A [B] scan is N = 1.  match_places compares them.  device=True: torch tensors on the engine's
        device, ready for work on torch's current stream, the words as int64 (torch has no arithmetic on uint64; the bits are
        the same)."""
        rg, a = _f64(ranges), _f64(angles)
        if rg.ndim == 1:
            rg = rg.reshape(1, -1)
        if a.ndim != 1 or rg.ndim != 2 or rg.shape[1] != a.shape[0]:
            raise ValueError("angles must be [B] and ranges [N, B]")
        n, r = rg.shape[0], int(rings)
        lo = float(self.cfg.match_min_range if min_range is None else min_range)
        hi = float(self.cfg.match_max_range if max_range is None else max_range)
        out = self._outputs(device)
        desc = out.empty((n, max(r, 0)), "uint64", device_dtype="int64")       # a bad ring count is the library's to refuse
        info = out.empty((n, 2), "int32")
        with out:
            self._check(self._lib.rbpf_describe_scans(self._h, _dp(rg), n, _dp(a), a.shape[0], lo, hi, r, out.ptr(desc), out.ptr(info),
                                                      _lib.RBPF_PLACES_DEVICE_OUT if device else 0))
        return ScanDescriptors(desc, info[:, 0], info[:, 1])

    def match_places(self, queries, refs=None, ref_limit=None, k: int = 4, device: bool = False) -> PlaceMatches:
        """Which references look like each query, and how they are turned: `queries` [Q, R] and `refs` [N, R] (None: the
        queries themselves) are descriptors of describe_scans, each a uint64 array, the int64 tensor of a
        describe_scans(device=True) or the ScanDescriptors itself, so a run's table never leaves the GPU.  Every query is
        scored against every reference r < ref_limit[q] (int [Q], None: all) at all 64 turns: the score counts the query's
        bits on the reference's bits and again on their 3 x 3 dilation.  Per query the `k` (1 .. 16) references of largest
        score^2 / weight come back best first, ties to the smaller r, each with its best turn `shift`: the query's heading is
        the reference's minus shift * 2 pi / 64.  device=True: torch tensors on the engine's device, ready for work on torch's
        current stream."""
        def table(t):
            t = t.desc if isinstance(t, ScanDescriptors) else t
            if hasattr(t, "data_ptr"):
                torch, dev = _torch_device(self.cfg)
                if t.dtype != torch.int64 or t.dim() != 2 or t.device != dev:
                    raise ValueError("a descriptor tensor must be [N, R] int64 on the engine's device")
                return t.contiguous()
            t = np.asarray(t)
            if t.ndim == 1:
                t = t.reshape(1, -1)
            if t.ndim != 2 or t.dtype.kind not in "iu" or t.dtype.itemsize != 8:
                raise ValueError("descriptors must be [N, R] uint64")
            return np.ascontiguousarray(t).view(np.uint64)
        qd = table(queries)
        rd = qd if refs is None else table(refs)
        if qd.shape[1] != rd.shape[1]:
            raise ValueError(f"queries have {qd.shape[1]} rings, references {rd.shape[1]}")
        nq, nr, k = int(qd.shape[0]), int(rd.shape[0]), int(k)
        lim = None
        if ref_limit is not None:
            lim = np.ascontiguousarray(ref_limit, dtype=np.int32)
            if lim.shape != (nq,):
                raise ValueError("ref_limit must be [Q]")
        flags = _lib.RBPF_PLACES_DEVICE_OUT if device else 0
        if hasattr(qd, "data_ptr") or hasattr(rd, "data_ptr"):       # one table is on the GPU: the other goes there too
            torch, dev = _torch_device(self.cfg)
            up = lambda t: t if hasattr(t, "data_ptr") else torch.from_numpy(t.view(np.int64)).to(dev)
            qd, rd = up(qd), (None if rd is qd else up(rd))
            rd = qd if rd is None else rd
            flags |= _lib.RBPF_PLACES_DEVICE_IN
        out = self._outputs(device)
        out.adopt(qd)
        out.adopt(rd)
        kk = min(max(k, 0), _lib.RBPF_PLACES_MAX_K)          # a bad k is the library's to refuse
        qk4, q2 = out.empty((nq, kk, 4), "int32"), out.empty((nq, 2), "int32")
        with out:
            self._check(self._lib.rbpf_match_places(self._h, out.ptr(qd), nq, out.ptr(rd), nr, int(qd.shape[1]),
                                                    None if lim is None else _ip(lim), k, out.ptr(qk4), out.ptr(q2), flags))
        return PlaceMatches(qk4[..., 0], qk4[..., 1], qk4[..., 2], qk4[..., 3], q2[:, 0], q2[:, 1])

    # -- score surface (include/rbpf_hip.h: rbpf_score_surface; thesis_amd/loops.py) -----------------------------
    @staticmethod
    def surface_exclusion(window: int, rotations: int) -> Tuple[int, int]:
        """score_surface's default exclusion box (translation steps, rotation steps): a quarter of the window's full width
        on each axis, ceil(window / 2) and ceil(rotations / 2), at least 1.  A convention, not a tuned value."""
        return max(1, -(-int(window) // 2)), max(1, -(-int(rotations) // 2))

    def score_surface(self, scores, drop=None, drop_fraction: float = 0.05, exclude=None, peaks: int = 2,
                      device: bool = False) -> ScoreSurface:
        """What a score volume says beyond its best candidate: the `peaks` (1 .. 8) best candidates that lie outside one
        another's exclusion boxes, and for each the plateau of candidates within `drop` of it inside its box: size, weight
        and first and second moments in exact integers.  `scores` is a RefineResult or PairResult that carries its volume
        (return_scores=True; numpy, or device tensors from device=True), or a bare int32 [N, 2R+1, 2W+1, 2W+1] array or
        tensor; a volume on the GPU is read where it is.  `drop` [N] (or one number): with a result and None it is
        floor(drop_fraction * 2 n_used); with a bare volume and None it is 0.  `exclude` = (translation steps, rotation
        steps) defaults to surface_exclusion(W, R).  device=True: torch tensors on the engine's device, ready for work on
        torch's current stream."""
        res = scores if hasattr(scores, "scores") and hasattr(scores, "n_used") else None      # a RefineResult or a PairResult
        vol = scores.scores if res is not None else scores
        if vol is None:
            raise ValueError("the result carries no score volume: ask for return_scores=True")
        dev_in = hasattr(vol, "data_ptr")
        if dev_in:
            torch, dev = _torch_device(self.cfg)
            if vol.dtype != torch.int32 or vol.dim() != 4 or vol.device != dev:
                raise ValueError("a score tensor must be [N, 2R+1, 2W+1, 2W+1] int32 on the engine's device")
            vol = vol.contiguous()
        else:
            vol = np.asarray(vol)
            if vol.ndim != 4 or vol.dtype != np.int32:
                raise ValueError("scores must be [N, 2R+1, 2W+1, 2W+1] int32")
            vol = np.ascontiguousarray(vol)
        n, nk, nw = int(vol.shape[0]), int(vol.shape[1]), int(vol.shape[2])
        if nk % 2 != 1 or nw % 2 != 1 or int(vol.shape[3]) != nw:
            raise ValueError("scores must be [N, 2R+1, 2W+1, 2W+1]")
        R, W = nk // 2, nw // 2
        if drop is None:
            if res is not None:
                used = ScoreSurface._host(res.n_used).astype(np.int64)
                drop = np.floor(float(drop_fraction) * (2 * used).astype(np.float64))
            else:
                drop = 0
        dr = np.array(np.broadcast_to(np.asarray(drop), (n,)), dtype=np.int32)       # a copy: contiguous and writeable
        ex_t, ex_r = self.surface_exclusion(W, R) if exclude is None else (int(exclude[0]), int(exclude[1]))
        k = int(peaks)
        kk = min(max(k, 0), 8)                               # a bad count is the library's to refuse
        dr_in = torch.from_numpy(dr).to(dev) if dev_in else dr
        out = self._outputs(device)
        out.adopt(vol)
        out.adopt(dr_in)
        rec, cnt = out.empty((n, kk, 16), "int64"), out.empty((n,), "int32")
        flags = (_lib.RBPF_SURFACE_DEVICE_IN if dev_in else 0) | (_lib.RBPF_SURFACE_DEVICE_OUT if device else 0)
        with out:
            self._check(self._lib.rbpf_score_surface(self._h, out.ptr(vol), n, R, W, out.ptr(dr_in), ex_t, ex_r, k, out.ptr(rec),
                                                     out.ptr(cnt), flags))
        dr_out = out.torch.from_numpy(dr).to(out.dev) if device else dr
        steps = (int(res.substeps), float(res.rot_step), float(res.cell_size)) if res is not None else (None, None, None)
        return ScoreSurface.from_records(rec, cnt, dr_out, *steps)

    def get_odds_at(self, particle: int, xy) -> Tuple[np.ndarray, np.ndarray]:
        pts = _f64(xy).reshape(-1, 2)
        vals = np.empty(len(pts))
        none = np.empty(len(pts), dtype=np.uint8)
        self._check(self._lib.rbpf_get_odds_at(self._h, particle, _dp(pts), len(pts), _dp(vals),
                                               none.ctypes.data_as(C.POINTER(C.c_uint8))))
        return vals, none.astype(bool)


def match_scan(engine: ParticleEngine, curr_xy, ref_xy, guess, cells_per_m: int, pose_range):
    """Stateless twin of the reference's engine seam ``matchScanCustom(curr, ref, guess, cells_per_m,
    pose_range, nargout=3)`` (hybridmap.py:244-251): returns (pose[3], cov[3,3], score); a failed match
    has NaN covariance and score 0 (matchScanCustom.m:25-28)."""
    cu, rf = _f64(curr_xy).reshape(-1, 2), _f64(ref_xy).reshape(-1, 2)
    g, pr = _f64(guess).reshape(3), _f64(pose_range).reshape(3)
    pose, cov, score = np.empty(3), np.empty((3, 3)), C.c_double()
    engine._check(engine._lib.rbpf_match_scan(engine._h, _dp(cu), len(cu), _dp(rf), len(rf), _dp(g), int(cells_per_m),
                                              _dp(pr), _dp(pose), _dp(cov), C.byref(score)))
    return pose, cov, score.value
