"""A plain NumPy model of the trajectory log and the estimate row (kernels_track.hip).

TrackModel records, composes and walks one particle at a time, in the manner of ParticleFilter.trajectory; lineage_chunked is the
three-stage scan over chunks of 64 records the kernels run, as a second implementation.  estimate_row sums with math.fsum (the
correctly rounded sum), est_tolerance is the bound a float64 summation of the same terms may differ by."""
import math

import numpy as np

CHUNK = 64
W_UNIFORM, W_RESAMPLE, W_GIVEN = 0, 1, 2
TWO_PI = 6.283185307179586


def resample_weights(w):
    """mapio.resample_weights (main.py:52-56): -inf -> 0, then |min| onto every non-zero value if the minimum is negative."""
    w = np.array(w, dtype=np.float64)
    w[w == -np.inf] = 0.0
    if len(w) and np.nanmin(w) < 0:
        w[w != 0] += abs(np.nanmin(w))
    return w


def effective_weights(raw, mode, given=None):
    if mode == W_UNIFORM:
        return np.ones(len(raw))
    if mode == W_GIVEN:
        return np.array(given, dtype=np.float64)
    return resample_weights(raw)


def wrap(a):
    d = math.remainder(a, TWO_PI)
    return d + TWO_PI if d <= -math.pi else d


def _terms(poses, w):
    """The contributing particles' (w, x, y, theta)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    keep = np.isfinite(w) & (w > 0) & np.isfinite(poses).all(axis=1)
    return [(float(w[j]), float(poses[j, 0]), float(poses[j, 1]), float(poses[j, 2])) for j in np.nonzero(keep)[0]]


def estimate_row(poses, raw, mode=W_RESAMPLE, given=None, n_alive=-1):
    """(f64 [16], i32 [4]) of include/rbpf_hip.h, every sum a math.fsum of the float64 terms the kernel adds."""
    raw = np.asarray(raw, dtype=np.float64)
    t = _terms(poses, effective_weights(raw, mode, given))
    f, i = np.zeros(16), np.array([int(np.argmax(raw)), len(t), n_alive, 0], dtype=np.int32)
    W = math.fsum(w for w, *_ in t)
    if not W > 0:
        f[:12] = np.nan
        return f, i
    mx, my = math.fsum(w * x for w, x, _, _ in t) / W, math.fsum(w * y for w, _, y, _ in t) / W
    S, Cc = math.fsum(w * math.sin(th) for w, _, _, th in t), math.fsum(w * math.cos(th) for w, _, _, th in t)
    mth = math.atan2(S, Cc)
    d = [(w, x - mx, y - my, wrap(th - mth)) for w, x, y, th in t]
    pairs = ((1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
    f[0:3] = mx, my, mth
    f[3:9] = [math.fsum(q[0] * (q[a] * q[b]) for q in d) / W for a, b in pairs]
    f[9], f[10], f[11] = math.hypot(S, Cc) / W, W, W * W / math.fsum(w * w for w, *_ in t)
    return f, i


def est_tolerance(poses, raw, mode=W_RESAMPLE, given=None):
    """[12] how far a float64 evaluation may lie from estimate_row: 4 P 2^-53 max |a_i| over the summands a_i of each value (the
    summands of a mean are w_i x_i / W, of a covariance w_i d_i d_j / W); mth gets 8 * 2^-52 more for the device's sincos and
    atan2 and is bounded through the summands of S / (R W) and C / (R W); R, W and n_eff likewise through their own summands."""
    raw = np.asarray(raw, dtype=np.float64)
    t = _terms(poses, effective_weights(raw, mode, given))
    P, tol = len(raw), np.zeros(12)
    if not t:
        return tol
    u = 4.0 * P * 2.0 ** -53
    f, _ = estimate_row(poses, raw, mode, given)
    W = f[10]
    w, x, y, th = (np.array(c) for c in zip(*t))
    tol[0], tol[1] = u * np.max(np.abs(w * x)) / W, u * np.max(np.abs(w * y)) / W
    RW = max(f[9] * W, np.finfo(float).tiny)
    tol[2] = u * np.max(w) / RW + 8 * 2.0 ** -52
    d = np.stack([x - f[0], y - f[1], np.array([wrap(a - f[2]) for a in th])])
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        tol[3 + k] = u * np.max(np.abs(w * d[a] * d[b])) / W
    tol[9] = u * np.max(w) / W + 8 * 2.0 ** -52
    tol[10] = u * np.max(w)
    tol[11] = 3 * u * f[11]
    return tol


class TrackModel:
    """The log: record(poses, weights) and resample(ancestors) as the engine is driven; lineage() walks it."""

    def __init__(self, poses, weights):
        self.P = len(poses)
        self.poses, self.parent, self.weights = [], [], []
        self.pending = np.arange(self.P, dtype=np.int32)
        self.record(poses, weights)

    def row(self, t):
        """The estimate row record t stored: RBPF_W_RESAMPLE of the weights of that moment."""
        return estimate_row(self.poses[t], self.weights[t], W_RESAMPLE)

    def resample(self, idx):
        """A resample that happened, with ancestors idx: composes onto pending."""
        self.pending = self.pending[np.asarray(idx)]

    def record(self, poses, weights):
        self.poses.append(np.array(poses, dtype=np.float64).reshape(self.P, 3))
        self.parent.append(self.pending.copy())
        self.weights.append(np.array(weights, dtype=np.float64))
        self.pending = np.arange(self.P, dtype=np.int32)

    @property
    def n(self):
        return len(self.poses)

    def lineage(self, particles=None, t0=0, t1=None):
        """(idx [t1-t0, n], pose [t1-t0, n, 3]): one particle at a time, one record at a time."""
        t1 = self.n if t1 is None else t1
        particles = range(self.P) if particles is None else particles
        idx = np.empty((t1 - t0, len(particles)), dtype=np.int32)
        for k, p in enumerate(particles):
            cur = int(self.pending[p])
            for t in range(self.n - 1, t0 - 1, -1):
                if t < t1:
                    idx[t - t0, k] = cur
                if t > 0:
                    cur = int(self.parent[t][cur])
        pose = np.stack([self.poses[t][idx[t - t0]] for t in range(t0, t1)]) if t1 > t0 else np.empty((0, len(particles), 3))
        return idx, pose

    def summary(self, raw, mode=W_RESAMPLE, given=None, t0=0, t1=None):
        """[(f64 row, i32 row)] per record of [t0, t1): the smoothed estimate with the final weights, and n_alive."""
        idx, pose = self.lineage(None, t0, t1)
        return [estimate_row(pose[k], raw, mode, given, n_alive=len(np.unique(idx[k]))) for k in range(len(idx))]


def lineage_chunked(parent, pending, particles=None, t0=0, t1=None, chunk=CHUNK):
    """The kernels' three stages over a parent table [N][P] (parent[0] unused) and pending [P]: (1) per chunk above the first,
    the map from the index at its last record to the index at the last record of the chunk before; (2) one chain over the chunks
    from the walked particles; (3) per chunk, the walk down from its start."""
    parent, pending = np.asarray(parent), np.asarray(pending)
    N, P = parent.shape
    t1 = N if t1 is None else t1
    particles = np.arange(P) if particles is None else np.asarray(particles)
    c0, c1 = t0 // chunk, (N - 1) // chunk
    comp = {}
    for c in range(c0 + 1, c1 + 1):                            # stage 1
        cur = np.arange(P)
        for t in range(min(c * chunk + chunk, N) - 1, c * chunk - 1, -1):
            cur = parent[t][cur]
        comp[c] = cur
    start = {c1: pending[particles]}                           # stage 2
    for c in range(c1, c0, -1):
        start[c - 1] = comp[c][start[c]]
    idx = np.empty((t1 - t0, len(particles)), dtype=np.int32)
    for c in range(c0, (t1 - 1) // chunk + 1):                 # stage 3
        a, b = max(c * chunk, t0), min(c * chunk + chunk, N)
        cur = start[c]
        for t in range(b - 1, a - 1, -1):
            if t < t1:
                idx[t - t0] = cur
            if t > a:
                cur = parent[t][cur]
    return idx
