"""NumPy restatement of the score-surface specification (include/rbpf_hip.h: rbpf_score_surface), written from
the specification and not from the kernel.  Python integers and int64 arrays throughout; the order of the candidates is
tests.refine_oracle.tie_order's, so no key is packed here."""
import functools

import numpy as np

from tests.refine_oracle import tie_order


@functools.lru_cache(maxsize=None)
def tie_rank(W, R):
    """int64 [2R+1][2W+1][2W+1]: the place of candidate (k, i, j) in tie_order(W, R), 0 first."""
    order = np.array(tie_order(W, R), dtype=np.int64)                    # rows (k, i, j)
    rank = np.empty((2 * R + 1, 2 * W + 1, 2 * W + 1), dtype=np.int64)
    rank[order[:, 0] + R, order[:, 1] + W, order[:, 2] + W] = np.arange(len(order), dtype=np.int64)
    rank.setflags(write=False)
    return rank


def surface_one(V, drop, ex_t, ex_r, K):
    """One item: V int [2R+1][2W+1][2W+1].  Returns (records int64 [K][16], count)."""
    V = np.asarray(V).astype(np.int64)
    nk, nw = V.shape[0], V.shape[1]
    assert V.shape == (nk, nw, nw) and nk % 2 == 1 and nw % 2 == 1 and 1 <= K <= 8
    R, W, drop = nk // 2, nw // 2, int(drop)
    assert 0 <= R <= 100 and 0 <= W <= 32 and 0 <= drop <= 32768 and 0 <= ex_t <= 64 and 0 <= ex_r <= 200
    assert V.min() >= 0 and V.max() <= 32768
    rank = tie_rank(W, R)
    ncand = V.size
    merit = V * ncand + (ncand - 1 - rank)               # larger score first, then the earlier place in tie_order
    kk, ii, jj = np.meshgrid(np.arange(-R, R + 1), np.arange(-W, W + 1), np.arange(-W, W + 1), indexing="ij")
    free = np.ones(V.shape, dtype=bool)
    rec = np.zeros((K, 16), dtype=np.int64)
    count = 0
    for p in range(K):
        if not free.any():
            break
        flat = int(np.argmax(np.where(free, merit, -1)))
        qk, qi, qj = np.unravel_index(flat, V.shape)
        kp, ip, jp, sp = int(qk) - R, int(qi) - W, int(qj) - W, int(V[qk, qi, qj])
        di, dj, dk = ii - ip, jj - jp, kk - kp
        box = (np.abs(di) <= ex_t) & (np.abs(dj) <= ex_t) & (np.abs(dk) <= ex_r)
        T = free & box & (V >= sp - drop)
        assert T[qk, qi, qj]
        w = (V - (sp - drop) + 1)[T]
        a, b, c = di[T], dj[T], dk[T]
        sums = [len(w), w.sum(), (w * a).sum(), (w * b).sum(), (w * c).sum(), (w * a * a).sum(), (w * a * b).sum(), (w * a * c).sum(),
                (w * b * b).sum(), (w * b * c).sum(), (w * c * c).sum()]
        assert int(w.min()) >= 1 and int(w.max()) <= drop + 1
        # the int64 sums cannot have wrapped: their bound in Python integers
        assert int(w.max()) * max(4 * W * W, 4 * R * R, 1) * len(w) < 2 ** 63
        rec[p] = [ip, jp, kp, sp] + [int(s) for s in sums] + [0]
        free &= ~box
        count += 1
    return rec, count


def surface(V, drop=None, ex_t=0, ex_r=0, K=2):
    """All items: V [N][2R+1][2W+1][2W+1]; drop [N] or None (0).  Returns (records int64 [N][K][16], count int32 [N])."""
    V = np.asarray(V)
    assert V.ndim == 4
    drop = np.zeros(len(V), dtype=np.int64) if drop is None else np.asarray(drop, dtype=np.int64).reshape(len(V))
    out = [surface_one(V[n], drop[n], ex_t, ex_r, K) for n in range(len(V))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)
