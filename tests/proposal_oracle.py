"""A plain NumPy / float64 model of the proposal of a scan update (Robot.map_update robot.py:73-114).

Test infrastructure only.  Written from the specification, not from the kernels:

  counters   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), counter
             {global particle id, sample k, stream, block}, key = (low, high) half of the 64-bit seed; `stream` is the number
             of scan updates the handle has finished (rbpf_get_rng_state), block 0 and 1
  uniforms   a block's words (x0, x1) and (x2, x3) give one uniform each: the 53-bit integer x_even * 2^21 + (x_odd >> 11),
             plus one, times 2^-53 - in (0, 1], every value exact in float64
  normals    Box-Muller: r = sqrt(-2 ln u_a), phi = 2 pi u_b; z0 = r cos phi and z1 = r sin phi of block 0, z2 = r cos phi
             of block 1
  samples    g = mean + A z with A A^T = the positive part of the matcher covariance
  pdf        scipy.stats.multivariate_normal.pdf(..., allow_singular=True): eigenvalues above eps = 1e6 * 2^-52 * max|w|
             are kept (pseudo-inverse, pseudo-determinant, rank), pdf = exp(log c - |(g - mean) U|^2 / 2),
             log c = -(rank * log(2 pi) + sum of log kept) / 2; robot.py:87 multiplies by 10
  moments    robot.py:89-108 as sequential float64 sums in the reference's order (oracle.rbpf_oracle.proposal_moments is
             the same in longdouble)
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # the two multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # the key's Weyl increments (golden ratio, sqrt(3) - 1)
EPS0 = 1e6 * 2.0 ** -52                                 # scipy's _eigvalsh_to_eps factor for float64
LOG_2PI = float(np.log(2 * np.pi))


def philox4x32_10(counter4, key2):
    """Ten rounds of Philox4x32.  `counter4`: four words, `key2`: two; Python ints, or uint64 arrays of one shape (the
    words are then arrays).  Returns the four output words (ints, or uint64 arrays holding 32-bit values)."""
    arrays = any(isinstance(x, np.ndarray) for x in list(counter4) + list(key2))
    if arrays:
        c = [np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in counter4]
        k = [np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in key2]
        m32, s32 = np.uint64(M32), np.uint64(32)
        for _ in range(10):
            p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]      # 32 x 32 -> 64 bits: no overflow
            c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
            k = [(k[0] + np.uint64(PHILOX_W0)) & m32, (k[1] + np.uint64(PHILOX_W1)) & m32]
        return c
    c = [int(x) & M32 for x in counter4]
    k = [int(x) & M32 for x in key2]
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + PHILOX_W0) & M32, (k[1] + PHILOX_W1) & M32]
    return c


def u01(hi32, lo32):
    """A uniform in (0, 1] from two 32-bit words: (hi32 * 2^21 + (lo32 >> 11) + 1) * 2^-53 (exact in float64)."""
    if isinstance(hi32, np.ndarray) or isinstance(lo32, np.ndarray):
        m = (np.asarray(hi32, dtype=np.uint64) << np.uint64(21)) + (np.asarray(lo32, dtype=np.uint64) >> np.uint64(11))
        return (m.astype(np.float64) + 1.0) * 2.0 ** -53
    return (float((int(hi32) << 21) + (int(lo32) >> 11)) + 1.0) * 2.0 ** -53


def normals3(seed, stream, gid, k) -> np.ndarray:
    """The three standard normals of sample `k` of the particle with global id `gid` in scan update `stream`.  Scalars give
    [3]; `gid` and `k` may be integer arrays of one shape S, giving S + (3,)."""
    key = (int(seed) & M32, (int(seed) >> 32) & M32)
    if isinstance(gid, np.ndarray) or isinstance(k, np.ndarray):
        gid, k = np.broadcast_arrays(np.asarray(gid).astype(np.int64).astype(np.uint64) & np.uint64(M32),
                                     np.asarray(k).astype(np.uint64))
        st = np.full(gid.shape, int(stream) & M32, dtype=np.uint64)
        blocks = [philox4x32_10([gid, k, st, np.full(gid.shape, b, dtype=np.uint64)],
                                [np.uint64(key[0]), np.uint64(key[1])]) for b in (0, 1)]
    else:
        blocks = [philox4x32_10([int(gid) & M32, int(k), int(stream) & M32, b], key) for b in (0, 1)]
    r0, phi0 = np.sqrt(-2.0 * np.log(u01(blocks[0][0], blocks[0][1]))), 2.0 * np.pi * u01(blocks[0][2], blocks[0][3])
    r1, phi1 = np.sqrt(-2.0 * np.log(u01(blocks[1][0], blocks[1][1]))), 2.0 * np.pi * u01(blocks[1][2], blocks[1][3])
    return np.stack([r0 * np.cos(phi0), r0 * np.sin(phi0), r1 * np.cos(phi1)], axis=-1)


# ---- the frame -----------------------------------------------------------------------------------------------------------
class Frame(NamedTuple):
    U: np.ndarray      # [3, 3]: maha = |(g - mean) U|^2
    A: np.ndarray      # [3, 3]: g = mean + A z
    log_c: float
    rank: int


def frame_from_cov(cov) -> Frame:
    """The LAPACK route (numpy.linalg.eigh, what scipy's _PSD runs) to the frame of a covariance."""
    cov = np.asarray(cov, dtype=np.float64)
    w, v = np.linalg.eigh(cov)
    eps = EPS0 * float(np.max(np.abs(w)))
    keep = w > eps
    inv = np.where(keep, 1.0 / np.where(keep, w, 1.0), 0.0)
    pos = np.where(w > 0, w, 0.0)
    rank = int(np.count_nonzero(keep))
    return Frame(U=v * np.sqrt(inv), A=v * np.sqrt(pos), log_c=-0.5 * (rank * LOG_2PI + float(np.sum(np.log(w[keep])))), rank=rank)


def pdf10(g, mean, U, log_c) -> np.ndarray:
    """robot.py:87: the density of the samples `g` [K, 3] times 10."""
    t = (np.atleast_2d(g) - np.asarray(mean)) @ np.asarray(U)
    return np.exp(log_c - 0.5 * np.sum(t * t, axis=-1)) * 10


class Truth(NamedTuple):
    """A covariance built from a known eigen-system: what every frame of it must reproduce, whatever its column order
    and signs."""
    cov: np.ndarray        # float64, as handed to the filter
    pos_part: np.ndarray   # V diag(max(lam, 0)) V^T
    pinv: np.ndarray       # V diag(1 / lam over the kept) V^T
    log_c: float
    rank: int
    lam_max: float
    kappa: float           # lam_max / smallest kept eigenvalue (1 for rank 0)


def truth_from_eigen(V, lam, cov=None) -> Truth:
    """V [3, 3] orthonormal columns, lam [3].  cov = V diag(lam) V^T in longdouble, rounded to float64 and symmetrised (or
    the given float64 matrix, for a variant of it)."""
    Vl, ll = np.asarray(V, dtype=np.longdouble), np.asarray(lam, dtype=np.longdouble)
    if cov is None:
        c = ((Vl * ll) @ Vl.T).astype(np.float64)
        cov = 0.5 * (c + c.T)
    lam_max = float(np.max(np.abs(ll)))
    keep = ll > np.longdouble(EPS0) * np.max(np.abs(ll))
    inv = np.where(keep, 1 / np.where(keep, ll, 1), 0)
    pos = np.where(ll > 0, ll, 0)
    rank = int(np.count_nonzero(keep))
    log_c = float(-0.5 * (rank * np.log(2 * np.longdouble(np.pi)) + np.sum(np.log(ll[keep]))))
    kappa = float(lam_max / np.min(ll[keep])) if rank else 1.0
    return Truth(cov=np.asarray(cov, dtype=np.float64), pos_part=((Vl * pos) @ Vl.T).astype(np.float64),
                 pinv=((Vl * inv) @ Vl.T).astype(np.float64), log_c=log_c, rank=rank, lam_max=lam_max, kappa=kappa)


def frame_rank(U) -> int:
    """Kept eigenvalues of a frame: the non-zero columns of U."""
    return int(np.count_nonzero(np.any(np.asarray(U) != 0.0, axis=0)))


def frame_deviation(truth: Truth, U, A, log_c) -> Tuple[float, float, float]:
    """The frame-free quantities of a frame against the truth, each relative: max|A A^T - cov+| / lam_max,
    max|U U^T - pinv| / max|pinv|, |log c - truth| / max(1, |truth|).  (A zero matrix has nothing to divide by: absolute.)"""
    U, A = np.asarray(U, dtype=np.longdouble), np.asarray(A, dtype=np.longdouble)
    dA = float(np.max(np.abs(A @ A.T - truth.pos_part))) / (truth.lam_max if truth.lam_max > 0 else 1.0)
    pm = float(np.max(np.abs(truth.pinv)))
    dU = float(np.max(np.abs(U @ U.T - truth.pinv))) / (pm if pm > 0 else 1.0)
    dC = abs(float(log_c) - truth.log_c) / max(1.0, abs(truth.log_c))
    return dA, dU, dC


def frame_floor(truth: Truth) -> float:
    """What rounding the covariance to float64 alone may cost a frame-free quantity: 64 * 2^-53 * lam_max / lam_min,kept."""
    return 64 * 2.0 ** -53 * truth.kappa


# ---- the covariance list of tests/test_gpu_proposal.py (and of the CPU checks of the model) --------------------------------
def rotation(seed: int, mixing: bool = False) -> np.ndarray:
    """A random rotation from a seeded generator (QR of a Gaussian matrix, longdouble Gram-Schmidt polish); mixing = True
    redraws until every entry is at least 0.25 in magnitude: every column mixes all three axes strongly."""
    rng = np.random.Generator(np.random.PCG64(seed))
    while True:
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        if not mixing or np.min(np.abs(q)) >= 0.25:
            break
    v = q.astype(np.longdouble)
    for j in range(3):                                   # orthonormal to longdouble precision
        for i in range(j):
            v[:, j] -= (v[:, i] @ v[:, j]) * v[:, i]
        v[:, j] /= np.sqrt(v[:, j] @ v[:, j])
    return v


def covariance_cases():
    """[(name, Truth)]: every covariance the proposal tests feed, with its constructed eigen-system."""
    I3 = np.eye(3, dtype=np.longdouble)
    out = [("matcher scale, correlated", truth_from_eigen(rotation(11, True), [2.5e-3, 1e-3, 1e-5])),
           ("two equal", truth_from_eigen(rotation(12), [1e-4, 1e-4, 1e-5])),
           ("three equal, rotated", truth_from_eigen(rotation(13), [1e-4, 1e-4, 1e-4])),
           ("three equal, diagonal", truth_from_eigen(I3, [1e-4, 1e-4, 1e-4])),
           ("wide spread", truth_from_eigen(rotation(14), [1e-2, 1e-7, 1e-11])),
           ("above the cut-off", truth_from_eigen(rotation(15), [1e-3, 1e-6, 2e-3 * EPS0])),
           ("below the cut-off", truth_from_eigen(rotation(15), [1e-3, 1e-6, 0.5e-3 * EPS0]))]
    V = rotation(16, True)                               # rank 2: B B^T of a 3 x 2 matrix, the dropped eigenvalue exactly 0
    lam = np.array([2e-3, 4e-4, 0.0], dtype=np.longdouble)
    B = V[:, :2] * np.sqrt(lam[:2])
    c = (B @ B.T).astype(np.float64)
    out.append(("rank 2", truth_from_eigen(V, lam, cov=0.5 * (c + c.T))))
    out.append(("rank 1", truth_from_eigen(rotation(17), [1e-3, 0.0, 0.0])))
    out.append(("zero", truth_from_eigen(I3, [0.0, 0.0, 0.0])))
    out.append(("tiny negative", truth_from_eigen(rotation(18), [1e-3, 1e-4, -1e-15])))
    t = out[0][1]                                        # asymmetric by one ulp in one off-diagonal pair
    c = t.cov.copy()
    c[0, 2] = np.nextafter(c[0, 2], np.inf)
    out.append(("asymmetric by an ulp", t._replace(cov=c)))
    return out


# ---- moments -------------------------------------------------------------------------------------------------------------
def sequential_moments(g, w):
    """robot.py:89-108 in float64, every sum sequential over the samples in the reference's order.  Returns
    (mean [3], sigma [3, 3], weight increment)."""
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K = len(w)
    min_w = np.min(w)
    kw = (w - min_w) + 1e-2
    mean, norm = np.zeros(3), np.float64(0.0)
    for i in range(K):
        mean = mean + g[i] * kw[i]
        norm = norm + kw[i]
    mean = mean / norm
    sigma = np.zeros((3, 3))
    for i in range(K):
        d = g[i] + (-mean)
        sigma = sigma + np.outer(d, d) * kw[i]
    sigma = sigma / norm
    return mean, sigma, norm + min_w * K
