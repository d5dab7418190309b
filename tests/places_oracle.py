"""NumPy restatement of the place-recognition specification (include/rbpf_hip.h: rbpf_describe_scans and
rbpf_match_places), written from the specification and not from the kernels: a descriptor is a boolean image [N, R, 64], a turn is
np.roll along the sector axis, a score is a sum of ANDs.  The GPU tests compare bit for bit with it."""
import math
from typing import NamedTuple

import numpy as np

from tests.pairs_oracle import OracleEngine as PairsOracleEngine

# the turns in tie order: the smaller min(s, 64 - s), then the smaller s
TURNS = np.array(sorted(range(64), key=lambda s: (min(s, 64 - s), s)))


def to_bits(desc) -> np.ndarray:
    """uint64 [N, R] -> bool [N, R, 64], bit j of a word at [..., j]."""
    d = np.asarray(desc).astype(np.uint64)
    return ((d[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def to_words(bits) -> np.ndarray:
    """bool [N, R, 64] -> uint64 [N, R]."""
    return (np.asarray(bits).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def sectors(angles) -> np.ndarray:
    return (np.floor(np.asarray(angles, dtype=np.float64) * (32.0 / math.pi)).astype(np.int64)) & 63


def describe(ranges, angles, rings, min_range, max_range):
    """(desc uint64 [N, R], info int32 [N, 2] = {n_used, n_bits})."""
    r = np.asarray(ranges, dtype=np.float64).reshape(-1, len(np.atleast_1d(angles)))
    R = int(rings)
    sec = sectors(angles)
    per_m = float(R) / float(max_range)
    bits = np.zeros((len(r), R, 64), dtype=bool)
    info = np.zeros((len(r), 2), dtype=np.int32)
    for n, row in enumerate(r):
        with np.errstate(invalid="ignore"):
            used = (min_range < row) & (row < max_range)
        ring = np.minimum(np.floor(row[used] * per_m).astype(np.int64), R - 1)
        bits[n, ring, sec[used]] = True
        info[n] = int(used.sum()), int(bits[n].sum())
    return to_words(bits), info


def dilate(bits) -> np.ndarray:
    """D' of bool [N, R, 64]: 3 x 3, sectors circular, rings clipped."""
    b = np.asarray(bits, dtype=bool)
    wide = b | np.roll(b, 1, axis=-1) | np.roll(b, -1, axis=-1)
    out = wide.copy()
    out[:, 1:] |= wide[:, :-1]
    out[:, :-1] |= wide[:, 1:]
    return out


def scores(q_desc, r_desc) -> np.ndarray:
    """int64 [Q, N, 64]: score(q, r, s) for every turn s."""
    qb, rb = to_bits(q_desc), to_bits(r_desc)
    field = rb.astype(np.float32) + dilate(rb).astype(np.float32)         # sums stay below 2^24: exact in float32
    qf = qb.reshape(len(qb), -1).astype(np.float32)
    out = np.empty((len(qb), len(rb), 64), dtype=np.int64)
    for s in range(64):
        out[:, :, s] = np.rint(qf @ np.roll(field, s, axis=-1).reshape(len(rb), -1).T).astype(np.int64)   # roll moves bit j to j + s
    return out


def match_places(q_desc, r_desc, ref_limit, k):
    """(out_qk4 int32 [Q, k, 4], out_q2 int32 [Q, 2]).  The rank v^2 / w is compared as a float64 quotient: v^2 w' < 2^37, so two
    different quotients differ by more than 2^-48 of their size and equal ones round alike; the order is the exact one."""
    qd, rd = np.asarray(q_desc).astype(np.uint64), np.asarray(r_desc).astype(np.uint64)
    Q, N = len(qd), len(rd)
    sc = scores(qd, rd)[:, :, TURNS]
    first = np.argmax(sc, axis=2)                                         # the first maximum in tie order
    v = np.take_along_axis(sc, first[:, :, None], axis=2)[:, :, 0]
    s = TURNS[first]
    rb = to_bits(rd)
    w = rb.sum(axis=(1, 2)) + dilate(rb).sum(axis=(1, 2))
    limit = np.full(Q, N) if ref_limit is None else np.asarray(ref_limit, dtype=np.int64)
    out4 = np.zeros((Q, int(k), 4), dtype=np.int32)
    out4[:, :, 0] = -1
    out2 = np.zeros((Q, 2), dtype=np.int32)
    out2[:, 0] = to_bits(qd).sum(axis=(1, 2))
    for q in range(Q):
        ok = np.flatnonzero((np.arange(N) < limit[q]) & (w > 0) & (v[q] > 0))
        order = ok[np.lexsort((ok, -(v[q, ok].astype(np.float64) ** 2 / w[ok])))][:int(k)]
        out4[q, :len(order)] = np.stack([order, s[q, order], v[q, order], w[order]], axis=1)
        out2[q, 1] = len(order)
    return out4, out2


class Descriptors(NamedTuple):
    """What ParticleEngine.describe_scans returns (thesis_amd.engine.ScanDescriptors), from the oracle."""
    desc: np.ndarray
    n_used: np.ndarray
    n_bits: np.ndarray


def as_matches(out4, out2):
    from thesis_amd.engine import PlaceMatches
    return PlaceMatches(out4[..., 0], out4[..., 1], out4[..., 2], out4[..., 3], out2[:, 0], out2[:, 1])


class OracleEngine(PairsOracleEngine):
    """pairs_oracle.OracleEngine with describe_scans and match_places from this oracle: thesis_amd/loops.py's appearance path
    without a GPU."""

    def describe_scans(self, ranges, angles, rings=24, min_range=None, max_range=None, device=False):
        lo = self.min_range if min_range is None else float(min_range)
        hi = self.max_range if max_range is None else float(max_range)
        desc, info = describe(ranges, angles, rings, lo, hi)
        return Descriptors(desc, info[:, 0], info[:, 1])

    def match_places(self, queries, refs=None, ref_limit=None, k=4, device=False):
        q = queries.desc if isinstance(queries, Descriptors) else queries
        r = q if refs is None else refs.desc if isinstance(refs, Descriptors) else refs
        return as_matches(*match_places(q, r, ref_limit, k))
