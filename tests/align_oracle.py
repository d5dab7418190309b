"""NumPy restatement of the alignment specification (include/rbpf_hip.h: rbpf_align_points), written from the
specification and not from the kernels.  Scores are integers, so the GPU tests compare bit for bit.  Field, window and the
libm conventions are those of tests/locate_oracle.py: every cosine and sine comes from math.cos / math.sin, the products and
sums are single IEEE float64 operations.

`align` is the definition (one shifted-slice add per rotation and point), `align_scalar` the same for one cell in plain
loops.  `align_fft` computes the same integers as a correlation of the field with the histogram of the offsets: what makes
a whole-map search with tens of thousands of points affordable on the host.  Its sums are exact integers below 2^17 and
float64 FFTs of these sizes err by far less than 0.5, which it asserts before rounding; tests/test_align_oracle.py pins it to
`align`."""
import math

import numpy as np

from tests.locate_oracle import TWO_PI, field, window


def offsets(pxy, n_rot, r_begin, r_count, inv):
    """(u, w) int64 [r_count][n]: the cell offset of every point from the cell its frame's origin stands in."""
    pxy = np.asarray(pxy, dtype=np.float64).reshape(-1, 2)
    px, py = pxy[:, 0], pxy[:, 1]
    u = np.empty((r_count, len(px)), dtype=np.int64)
    w = np.empty((r_count, len(px)), dtype=np.int64)
    for q in range(r_count):
        th = ((r_begin + q) * TWO_PI) / n_rot
        c, s = math.cos(th), math.sin(th)
        u[q] = np.floor(0.5 + (c * px - s * py) * inv)
        w[q] = np.floor(0.5 + (s * px + c * py) * inv)
    return u, w


def _planes(cells, x0, y0, box, g, quantum, occupied_threshold):
    """(F, occ) uint8 over the box grown by g cells; g is one ring more than the largest offset, for the dilation."""
    bx0, bx1, by0, by1 = box
    wnd = window(cells, x0, y0, bx0 - g, bx1 + g, by0 - g, by1 + g)
    occ = (wnd.astype(np.float64) * quantum > occupied_threshold).astype(np.uint8)
    return field(wnd, quantum, occupied_threshold), occ


def _reduce(score_of, r_begin, r_count, shape):
    best = np.full(shape, np.iinfo(np.int32).min, dtype=np.int32)
    rot = np.full(shape, -1, dtype=np.int32)
    for q in range(r_count):
        s = score_of(q)
        better = s > best                                # strictly: the smallest r that attains the maximum is kept
        best[better] = s[better]
        rot[better] = r_begin + q
    return best, rot


def _setup(cells, x0, y0, box, occ_xy, free_xy, n_rot, r_begin, r_count, inv, quantum, occupied_threshold):
    box = tuple(int(q) for q in box)
    occ_xy = np.asarray(occ_xy, dtype=np.float64).reshape(-1, 2)
    free_xy = np.zeros((0, 2)) if free_xy is None else np.asarray(free_xy, dtype=np.float64).reshape(-1, 2)
    uo, wo = offsets(occ_xy, n_rot, r_begin, r_count, inv)
    uf, wf = offsets(free_xy, n_rot, r_begin, r_count, inv)
    m = max(int(np.abs(a).max()) if a.size else 0 for a in (uo, wo, uf, wf))
    g = m + 1
    F, occ = _planes(cells, x0, y0, box, g, quantum, occupied_threshold)
    return box, (uo, wo, uf, wf), g, F, occ


def align(cells, x0, y0, box, occ_xy, free_xy, n_rot, r_begin, r_count, inv, quantum, occupied_threshold):
    """cells[X - x0][Y - y0]: int8 lattice values of a rendered map, 0 outside the raster.  Returns (best, rot): int32
    [x1-x0][y1-y0] rasters over `box` for the rotations r_begin .. r_begin + r_count - 1 of n_rot."""
    box, (uo, wo, uf, wf), g, F, occ = _setup(cells, x0, y0, box, occ_xy, free_xy, n_rot, r_begin, r_count, inv, quantum,
                                              occupied_threshold)
    nx, ny = box[1] - box[0], box[3] - box[2]

    def score_of(q):
        s = np.zeros((nx, ny), dtype=np.int32)
        for k in range(uo.shape[1]):
            i, j = g + int(uo[q, k]), g + int(wo[q, k])
            s += F[i:i + nx, j:j + ny]
        for k in range(uf.shape[1]):
            i, j = g + int(uf[q, k]), g + int(wf[q, k])
            s -= 2 * occ[i:i + nx, j:j + ny].astype(np.int32)
        return s
    return _reduce(score_of, r_begin, r_count, (nx, ny))


def _fast_len(n):
    """The smallest 2^a 3^b 5^c >= n."""
    while True:
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def align_fft(cells, x0, y0, box, occ_xy, free_xy, n_rot, r_begin, r_count, inv, quantum, occupied_threshold):
    """`align`, computed per rotation as correlate(F, histogram of the occupied offsets) - 2 correlate(occ, histogram of the
    free offsets) through one inverse FFT."""
    box, (uo, wo, uf, wf), g, F, occ = _setup(cells, x0, y0, box, occ_xy, free_xy, n_rot, r_begin, r_count, inv, quantum,
                                              occupied_threshold)
    nx, ny = box[1] - box[0], box[3] - box[2]
    shape = (_fast_len(F.shape[0]), _fast_len(F.shape[1]))     # X + i <= nx - 1 + 2 g < shape: the circular sum never wraps
    fF = np.fft.rfft2(F.astype(np.float64), shape)
    fO = np.fft.rfft2(occ.astype(np.float64), shape)

    def hist(u, w):
        h = np.zeros(shape)
        np.add.at(h, (g + u, g + w), 1.0)
        return np.conj(np.fft.rfft2(h))

    def score_of(q):
        acc = fF * hist(uo[q], wo[q])
        if uf.shape[1]:
            acc -= 2.0 * (fO * hist(uf[q], wf[q]))
        c = np.fft.irfft2(acc, shape)[:nx, :ny]
        s = np.rint(c)
        assert np.abs(c - s).max() < 0.25, "FFT error too large to round to the exact integer"
        return s.astype(np.int32)
    return _reduce(score_of, r_begin, r_count, (nx, ny))


def align_scalar(cells, x0, y0, X, Y, occ_xy, free_xy, n_rot, r_begin, r_count, inv, quantum, occupied_threshold):
    """(best, rot) of the one cell (X, Y), by loops over rotations and points in plain Python."""
    rows = cells.tolist()

    def v(a, b):
        i, j = a - x0, b - y0
        return rows[i][j] if 0 <= i < len(rows) and 0 <= j < len(rows[0]) else 0

    def occ(a, b):
        return 1 if v(a, b) * quantum > occupied_threshold else 0

    def F(a, b):
        return occ(a, b) + max(occ(a + da, b + db) for da in (-1, 0, 1) for db in (-1, 0, 1))

    def cell_of(c, s, px, py):
        return X + math.floor(0.5 + (c * px - s * py) * inv), Y + math.floor(0.5 + (s * px + c * py) * inv)

    po = [(float(p[0]), float(p[1])) for p in np.asarray(occ_xy, dtype=np.float64).reshape(-1, 2)]
    pf = [] if free_xy is None else [(float(p[0]), float(p[1])) for p in np.asarray(free_xy, dtype=np.float64).reshape(-1, 2)]
    best, rot = None, -1
    for r in range(r_begin, r_begin + r_count):
        th = (r * TWO_PI) / n_rot
        c, s = math.cos(th), math.sin(th)
        hits = sum(F(*cell_of(c, s, px, py)) for px, py in po)
        clash = sum(occ(*cell_of(c, s, px, py)) for px, py in pf)
        score = hits - 2 * clash
        if best is None or score > best:
            best, rot = score, r
    return best, rot
