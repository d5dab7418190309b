"""A plain NumPy / Python model of the pose modes (include/rbpf_hip.h, rbpf_pose_modes; kernels_modes.hip).

Bins as specified (one IEEE multiplication and a floor each), components by breadth-first search over a dict of bins, q and Q as
Python ints, rows through track_oracle.estimate_row with the effective weights of the members in the RBPF_W_GIVEN form, best fixed
up to the members' first raw argmax.  components_uf is a second implementation of the components (union-find over the bins)."""
from collections import Counter, deque

import numpy as np

from tests import track_oracle as T

TWO_PI = 6.283185307179586


def bins_of(poses, w, bin_xy, n_th):
    """(contributing [P] bool, bins [P, 3] int64: ix, iy, it; rows of the others are 0)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    inv, kth = 1.0 / float(bin_xy), float(n_th) / TWO_PI
    with np.errstate(invalid="ignore", over="ignore"):
        f = poses * np.array([inv, inv, kth])
        ok = np.isfinite(w) & (w > 0) & np.isfinite(poses).all(axis=1)
        ok &= (np.abs(f[:, 0]) < 2.0 ** 23) & (np.abs(f[:, 1]) < 2.0 ** 23) & (np.abs(f[:, 2]) < 2.0 ** 40)
    b = np.zeros((len(poses), 3), dtype=np.int64)
    b[ok] = np.floor(f[ok]).astype(np.int64)
    b[ok, 2] %= n_th                                          # Python's modulo: non-negative
    return ok, b


def neighbours(b, n_th):
    """The up to 26 bins adjacent to bin b (itself left out)."""
    out = set()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dt in (-1, 0, 1):
                out.add((b[0] + dx, b[1] + dy, (b[2] + dt) % n_th))
    out.discard(tuple(b))
    return out


def adjacent(a, b, n_th):
    d = abs(a[2] - b[2]) % n_th
    return abs(a[0] - b[0]) <= 1 and abs(a[1] - b[1]) <= 1 and min(d, n_th - d) <= 1


def components_bfs(bins, n_th):
    """{bin: root} over a dict {bin: smallest particle index in it}: the root of a component is the smallest of its bins' values."""
    comp = {}
    for start in bins:
        if start in comp:
            continue
        seen, todo = {start}, deque([start])
        while todo:
            for nb in neighbours(todo.popleft(), n_th):
                if nb in bins and nb not in seen:
                    seen.add(nb); todo.append(nb)
        root = min(bins[b] for b in seen)
        for b in seen:
            comp[b] = root
    return comp


def components_uf(bins, n_th):
    """The same by union-find with path halving, all pairs of bins tested with `adjacent`."""
    keys = list(bins)
    up = list(range(len(keys)))

    def find(i):
        while up[i] != i:
            up[i] = up[up[i]]
            i = up[i]
        return i

    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            if adjacent(keys[i], keys[j], n_th):
                a, b = find(i), find(j)
                if a != b:
                    up[max(a, b)] = min(a, b)
    root = {}
    for i, k in enumerate(keys):
        r = find(i)
        root[r] = min(root.get(r, bins[k]), bins[k])
    return {k: root[find(i)] for i, k in enumerate(keys)}


def bin_dict(ok, b):
    bins = {}
    for j in np.nonzero(ok)[0]:
        bins.setdefault(tuple(int(v) for v in b[j]), int(j))   # ascending j: the first is the smallest
    return bins


def unused_row():
    f = np.zeros(16)
    f[:12] = np.nan
    return f, np.array([-1, 0, 0, -1], dtype=np.int32)


def pose_modes(poses, raw, mode, given, bin_xy, n_th, K, components=components_bfs):
    """(info [4] Python ints, rows_f [K, 16], rows_i [K, 4], label [P], members: the index arrays of the K rows' modes)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    raw = np.asarray(raw, dtype=np.float64)
    w = T.effective_weights(raw, mode, given)
    ok, b = bins_of(poses, w, bin_xy, n_th)
    bins = bin_dict(ok, b)
    comp = components(bins, n_th)
    label = np.full(len(poses), -1, dtype=np.int32)
    for j in np.nonzero(ok)[0]:
        label[j] = comp[tuple(int(v) for v in b[j])]
    rows_f, rows_i, members = np.zeros((K, 16)), np.zeros((K, 4), dtype=np.int32), []
    for k in range(K):
        rows_f[k], rows_i[k] = unused_row()
    if not ok.any():
        return [0, 0, 0, 0], rows_f, rows_i, label, members
    wmax = np.max(w[ok])
    q = np.zeros(len(poses), dtype=object)
    for j in np.nonzero(ok)[0]:
        q[j] = int(np.floor((w[j] / wmax) * 4294967296.0))
    roots = sorted(set(comp.values()))
    Q = {r: sum(int(q[j]) for j in np.nonzero(label == r)[0]) for r in roots}
    Q_total = sum(Q.values())
    nb = Counter(comp.values())
    order = sorted(roots, key=lambda r: (-Q[r], r))
    for k, r in enumerate(order[:K]):
        mem = np.nonzero(label == r)[0]
        w_mem = np.zeros(len(poses))
        w_mem[mem] = w[mem]
        f, i = T.estimate_row(poses, raw, T.W_GIVEN, w_mem)
        f[12], f[13] = float(Q[r]), float(Q[r]) / float(Q_total)
        i[0], i[2], i[3] = mem[first_argmax(raw[mem])], nb[r], r
        assert i[1] == len(mem)
        rows_f[k], rows_i[k] = f, i
        members.append(mem)
    return [len(roots), len(bins), int(ok.sum()), Q_total], rows_f, rows_i, label, members


def first_argmax(x):
    return int(np.argmax(x))                                  # a NaN counts as the largest, the first wins


def row_tolerance(poses, raw, mode, given, mem):
    """track_oracle.est_tolerance of a row's members: the set with everyone else's weight 0."""
    w = T.effective_weights(np.asarray(raw, dtype=np.float64), mode, given)
    w_mem = np.zeros(len(w))
    w_mem[mem] = w[mem]
    return T.est_tolerance(poses, raw, T.W_GIVEN, w_mem)
