"""Scalar / NumPy restatement of the pose-refinement specification (include/rbpf_hip.h: rbpf_refine_poses),
written from the specification and not from the kernel.  Scores are integers and the poses are formed by the same single
float64 operations, so the GPU tests compare bit for bit.  Every cosine and sine comes from math.cos / math.sin, the libm the
library's host code calls; sub-cell coordinates are int64."""
import functools
import math

import numpy as np

from tests.locate_oracle import field, window

SUBSTEPS = (1, 2, 4, 8, 16)


@functools.lru_cache(maxsize=None)
def tie_order(W, R):
    """Candidates (k, i, j) in the order ties are broken: |k|, then i^2 + j^2, then (k, i, j)."""
    c = [(abs(k), i * i + j * j, k, i, j) for k in range(-R, R + 1) for i in range(-W, W + 1) for j in range(-W, W + 1)]
    c.sort()
    return [(k, i, j) for _, _, k, i, j in c]


def window_reach(max_range, inv, W, S):
    """Mw: no end cell of a scan lies farther from the guess's cell on either axis."""
    return int(math.ceil(max_range * inv)) + -(-W // S) + 2


def refine_one(cells, x0, y0, pose, ranges, angles, inv, quantum, occupied_threshold, min_range, max_range, S, W, R, rot_step):
    """One scan.  cells[X - x0][Y - y0]: int8 lattice values of a rendered map, 0 outside the raster.  Returns (pose [3],
    n6 [6] = i, j, k, best score, score(0, 0, 0), n_used; scores int32 [2R+1][2W+1][2W+1])."""
    assert S in SUBSTEPS and 0 <= W <= 32 and 0 <= R <= 100
    s = S.bit_length() - 1
    invS = inv * S
    gx, gy, gth = (float(q) for q in pose)
    bx, by = [], []
    for r, a in zip(ranges, angles):
        r, a = float(r), float(a)
        if min_range < r < max_range:
            bx.append(r * math.cos(a))
            by.append(r * math.sin(a))
    bx, by = np.array(bx, dtype=np.float64), np.array(by, dtype=np.float64)
    X0, Y0 = math.floor(gx * inv), math.floor(gy * inv)
    Mw = window_reach(max_range, inv, W, S)
    g = Mw + 1                                           # one ring more: the dilation of the outermost cells read
    F = field(window(cells, x0, y0, X0 - g, X0 + g + 1, Y0 - g, Y0 + g + 1), quantum, occupied_threshold).astype(np.int32)
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
        scores[k + R] = F[(EX - X0 + g)[:, :, None], (EY - Y0 + g)[:, None, :]].sum(axis=0)      # [n_used][i][j] summed over the beams
    best = None
    for k, i, j in tie_order(W, R):
        sc = int(scores[k + R, i + W, j + W])
        if best is None or sc > best[3]:
            best = (i, j, k, sc)
    i, j, k, sc = best
    out = np.array([gx + float(i) / invS, gy + float(j) / invS, gth + float(k) * rot_step], dtype=np.float64)
    n6 = np.array([i, j, k, sc, int(scores[R, W, W]), len(bx)], dtype=np.int32)
    return out, n6, scores


def refine(cells, x0, y0, poses, ranges, angles, inv, quantum, occupied_threshold, min_range, max_range, S, W, R, rot_step):
    """All scans: (poses [N, 3] float64, n6 [N, 6] int32, scores [N, 2R+1, 2W+1, 2W+1] int32)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(len(poses), -1)
    out = [refine_one(cells, x0, y0, p, r, angles, inv, quantum, occupied_threshold, min_range, max_range, S, W, R, rot_step)
           for p, r in zip(poses, ranges)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def score_scalar(cells, x0, y0, pose, ranges, angles, inv, quantum, occupied_threshold, min_range, max_range, S, i, j, k, rot_step):
    """score(i, j, k) of one scan by loops in plain Python."""
    rows = cells.tolist()

    def occ(a, b):
        u, w = a - x0, b - y0
        v = rows[u][w] if 0 <= u < len(rows) and 0 <= w < len(rows[0]) else 0
        return 1 if v * quantum > occupied_threshold else 0

    def F(a, b):
        return occ(a, b) + max(occ(a + da, b + db) for da in (-1, 0, 1) for db in (-1, 0, 1))

    gx, gy, gth = (float(q) for q in pose)
    invS = inv * S
    th = gth + float(k) * rot_step
    ck, sk = math.cos(th), math.sin(th)
    total = 0
    for r, a in zip(ranges, angles):
        r, a = float(r), float(a)
        if not (min_range < r < max_range):
            continue
        bx, by = r * math.cos(a), r * math.sin(a)
        px = math.floor((gx + (ck * bx - sk * by)) * invS)
        py = math.floor((gy + (sk * bx + ck * by)) * invS)
        total += F((px + i) // S, (py + j) // S)
    return total
