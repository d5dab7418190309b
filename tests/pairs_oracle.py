"""Scalar / NumPy restatement of the pair-matching specification (include/rbpf_hip.h: rbpf_match_pairs), written
from the specification and not from the kernels.  The field of a pair is a dictionary of the cells its reference beams hit, every
one of them, however far away; every read of the search is asserted to lie inside the window, which is why the kernel may drop
the far ones.  Scores are integers and the poses are formed by the same single float64 operations, so the GPU tests compare bit
for bit.  Every cosine and sine comes from math.cos / math.sin, the libm the library's host code calls."""
import math
from typing import NamedTuple

import numpy as np

from tests.refine_oracle import SUBSTEPS, tie_order, window_reach


def used_points(ranges, angles, min_range, max_range):
    """(bx, bx) float64 [n_used]: r cos a, r sin a of the beams with min_range < r < max_range, in beam order."""
    bx, by = [], []
    for r, a in zip(ranges, angles):
        r, a = float(r), float(a)
        if min_range < r < max_range:
            bx.append(r * math.cos(a))
            by.append(r * math.sin(a))
    return np.array(bx, dtype=np.float64), np.array(by, dtype=np.float64)


def hit_cells(poses, ranges, angles, r0, r1, inv, min_range, max_range):
    """(H, n_ref): the dictionary {(HX, HY): beams} of the cells the used beams of scans r0 .. r1 - 1 hit, and their number."""
    H, n_ref = {}, 0
    for n in range(r0, r1):
        px, py, pth = (float(q) for q in poses[n])
        c, s = math.cos(pth), math.sin(pth)
        bx, by = used_points(ranges[n], angles, min_range, max_range)
        hx = np.floor((px + (c * bx - s * by)) * inv).astype(np.int64)
        hy = np.floor((py + (s * bx + c * by)) * inv).astype(np.int64)
        for cell in zip(hx.tolist(), hy.tolist()):
            H[cell] = H.get(cell, 0) + 1
        n_ref += len(bx)
    return H, n_ref


def field_at(H, X, Y):
    """F(X, Y) = occ + dil of the hit cells H, anywhere in the plane."""
    return int((X, Y) in H) + int(any((X + da, Y + db) in H for da in (-1, 0, 1) for db in (-1, 0, 1)))


def match_one(poses, ranges, angles, pair, guess, inv, min_range, max_range, S, W, R, rot_step):
    """One pair {q, r0, r1}; guess None: poses[q].  Returns (pose [3], m8 [8] = i, j, k, best score, score(0, 0, 0), n_used,
    n_ref, 0; scores int32 [2R+1][2W+1][2W+1])."""
    assert S in SUBSTEPS and 0 <= W <= 32 and 0 <= R <= 100
    q, r0, r1 = (int(v) for v in pair)
    assert 0 <= q < len(poses) and 0 <= r0 < r1 <= len(poses)
    s = S.bit_length() - 1
    invS = inv * S
    gx, gy, gth = (float(v) for v in (poses[q] if guess is None else guess))
    H, n_ref = hit_cells(poses, ranges, angles, r0, r1, inv, min_range, max_range)
    bx, by = used_points(ranges[q], angles, min_range, max_range)
    X0, Y0 = math.floor(gx * inv), math.floor(gy * inv)
    Mw = window_reach(max_range, inv, W, S)
    g = Mw + 1                                           # one ring more: what the dilation of the window's border cells reads
    occ = np.zeros((2 * g + 1, 2 * g + 1), dtype=np.int32)
    for (X, Y) in H:                                     # all of H is the field; only this much of it can be read
        if abs(X - X0) <= g and abs(Y - Y0) <= g:
            occ[X - X0 + g, Y - Y0 + g] = 1
    p = np.pad(occ, 1)
    dil = np.zeros_like(occ)
    for da in range(3):
        for db in range(3):
            dil |= p[da:da + occ.shape[0], db:db + occ.shape[1]]
    F = occ + dil                                        # exact for |X - X0|, |Y - Y0| <= Mw; the ring itself is not to be read
    nw = 2 * W + 1
    scores = np.zeros((2 * R + 1, nw, nw), dtype=np.int32)
    shift = np.arange(-W, W + 1, dtype=np.int64)
    for k in range(-R, R + 1):
        th = gth + float(k) * rot_step
        ck, sk = math.cos(th), math.sin(th)
        PX = np.floor((gx + (ck * bx - sk * by)) * invS).astype(np.int64)
        PY = np.floor((gy + (sk * bx + ck * by)) * invS).astype(np.int64)
        EX = (PX[:, None] + shift[None, :]) >> s         # [n_used][2W+1]
        EY = (PY[:, None] + shift[None, :]) >> s
        assert np.all(np.abs(EX - X0) <= Mw) and np.all(np.abs(EY - Y0) <= Mw), "the window bound"
        scores[k + R] = F[(EX - X0 + g)[:, :, None], (EY - Y0 + g)[:, None, :]].sum(axis=0)
    best = None
    for k, i, j in tie_order(W, R):
        sc = int(scores[k + R, i + W, j + W])
        if best is None or sc > best[3]:
            best = (i, j, k, sc)
    i, j, k, sc = best
    out = np.array([gx + float(i) / invS, gy + float(j) / invS, gth + float(k) * rot_step], dtype=np.float64)
    m8 = np.array([i, j, k, sc, int(scores[R, W, W]), len(bx), n_ref, 0], dtype=np.int32)
    return out, m8, scores


def match_pairs(poses, ranges, angles, pairs, guesses, inv, min_range, max_range, S, W, R, rot_step):
    """All pairs: (poses [M, 3] float64, m8 [M, 8] int32, scores [M, 2R+1, 2W+1, 2W+1] int32)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(len(poses), -1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    out = [match_one(poses, ranges, angles, p, None if guesses is None else guesses[m], inv, min_range, max_range, S, W, R, rot_step)
           for m, p in enumerate(pairs)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def score_scalar(poses, ranges, angles, pair, guess, inv, min_range, max_range, S, i, j, k, rot_step):
    """score(i, j, k) of one pair by loops in plain Python over the whole dictionary: no window anywhere."""
    q, r0, r1 = (int(v) for v in pair)
    H, _ = hit_cells(poses, ranges, angles, r0, r1, inv, min_range, max_range)
    gx, gy, gth = (float(v) for v in (poses[q] if guess is None else guess))
    invS = inv * S
    th = gth + float(k) * rot_step
    ck, sk = math.cos(th), math.sin(th)
    total = 0
    for r, a in zip(ranges[q], angles):
        r, a = float(r), float(a)
        if not (min_range < r < max_range):
            continue
        bx, by = r * math.cos(a), r * math.sin(a)
        px = math.floor((gx + (ck * bx - sk * by)) * invS)
        py = math.floor((gy + (sk * bx + ck * by)) * invS)
        total += field_at(H, (px + i) // S, (py + j) // S)
    return total


class OracleResult(NamedTuple):
    """What ParticleEngine.match_pairs returns (thesis_amd.engine.PairResult), from the oracle."""
    poses: np.ndarray
    index: np.ndarray
    score: np.ndarray
    score_guess: np.ndarray
    n_used: np.ndarray
    n_ref: np.ndarray
    scores: object
    substeps: int
    rot_step: float
    cell_size: float


class OracleEngine:
    """A stand-in for ParticleEngine whose match_pairs is this oracle (tests of thesis_amd/loops.py without a GPU).  It has
    the configuration loops.py reads, and of the trajectory log and the map building what close_loops calls: `path` [T, 3]
    is every particle's trajectory, and build_map records its poses and returns an empty BuiltMap."""

    def __init__(self, cell_size=0.05, min_range=0.3, max_range=11.0, path=None):
        import types
        self.cell_size, self.min_range, self.max_range = float(cell_size), float(min_range), float(max_range)
        self.cfg = types.SimpleNamespace(cell_size=self.cell_size, tile_len_m=40, match_min_range=self.min_range, match_max_range=self.max_range,
                                         max_ray_m=self.max_range)
        self.dim = int(round(40.0 / self.cell_size))
        self.path = None if path is None else np.array(path, dtype=np.float64)
        self.calls, self.built_at = [], []

    def track_info(self):
        return {"n_records": len(self.path)}

    def trajectory(self, particle="best"):
        return self.path.copy()

    def build_box(self, poses, cells_per_m, max_range):
        return (0, 1, 0, 1)

    def build_map(self, poses, ranges, angles, cell_size=None, box=None, into=None, **kw):
        from thesis_amd.engine import BuiltMap
        self.built_at.append(np.array(poses))
        cs = self.cell_size if cell_size is None else float(cell_size)
        return BuiltMap(np.zeros((1, 1), np.int32), np.zeros((1, 1), np.int32), 0, 0, cs, 1.0 / cs)

    def match_pairs(self, poses, ranges, angles, pairs, guesses=None, cell_size=None, substeps=1, window=16, rotations=20,
                    rot_step=math.radians(0.5), min_range=None, max_range=None, return_scores=False, device=False):
        cs = self.cell_size if cell_size is None else float(cell_size)
        lo = self.min_range if min_range is None else float(min_range)
        hi = self.max_range if max_range is None else float(max_range)
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 3)
        self.calls.append(len(pairs))
        p, m8, sc = match_pairs(poses, ranges, angles, pairs, guesses, 1.0 / cs, lo, hi, int(substeps), int(window), int(rotations), float(rot_step))
        return OracleResult(p, m8[:, 0:3], m8[:, 3], m8[:, 4], m8[:, 5], m8[:, 6], sc if return_scores else None, int(substeps), float(rot_step), cs)
