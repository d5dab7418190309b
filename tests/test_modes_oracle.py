"""The model of the pose modes (tests/modes_oracle.py) against itself and by hand, and the host helpers that read a
Modes result (thesis_amd/locate.py: converged, kld_size).  No GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import modes_oracle as M
from tests import track_oracle as T
from thesis_amd import locate


def random_cloud(rng, P):
    """1 .. 12 Gaussian blobs plus scattered singletons, headings anywhere."""
    n_blobs = int(rng.integers(1, 13))
    centres = rng.uniform(-8.0, 8.0, size=(n_blobs, 3))
    centres[:, 2] = rng.uniform(-7.0, 7.0, size=n_blobs)
    which = rng.integers(0, n_blobs, size=P)
    poses = centres[which] + rng.normal(scale=[0.3, 0.3, 0.15], size=(P, 3))
    lone = rng.random(P) < 0.1
    poses[lone] = rng.uniform(-20.0, 20.0, size=(int(lone.sum()), 3))
    return poses


def test_union_find_components_equal_the_breadth_first_search():
    for seed in range(200):
        rng = np.random.default_rng(seed)
        P = int(rng.integers(1, 120))
        poses = random_cloud(rng, P)
        n_th = int(rng.choice([1, 2, 3, 4, 8, 36]))
        bin_xy = float(rng.choice([0.25, 0.5, 1.0]))
        ok, b = M.bins_of(poses, np.ones(P), bin_xy, n_th)
        bins = M.bin_dict(ok, b)
        assert M.components_bfs(bins, n_th) == M.components_uf(bins, n_th), seed
        a = M.pose_modes(poses, np.ones(P), T.W_UNIFORM, None, bin_xy, n_th, 8)
        c = M.pose_modes(poses, np.ones(P), T.W_UNIFORM, None, bin_xy, n_th, 8, components=M.components_uf)
        assert a[0] == c[0] and np.array_equal(a[3], c[3]) and np.array_equal(a[2], c[2])
        assert a[0][3] == a[0][2] << 32                       # uniform weights: q = 2^32 each


def labels(poses, bin_xy=1.0, n_th=36, w=None):
    poses = np.asarray(poses, dtype=np.float64)
    w = np.ones(len(poses)) if w is None else np.asarray(w, dtype=np.float64)
    return M.pose_modes(poses, w, T.W_GIVEN, w, bin_xy, n_th, 4)[3].tolist()


def test_adjacency_hand_cases():
    step = T.TWO_PI / 36
    # floor, not truncation: -0.01 lies in bin -1, next to bin 0; two bins further on is a mode of its own
    ok, b = M.bins_of([[-0.01, 0.5, 0.0]], np.ones(1), 1.0, 36)
    assert b[0].tolist() == [-1, 0, 0]
    assert labels([[-0.01, 0.5, 0.1], [0.01, 0.5, 0.1], [2.01, 0.5, 0.1]]) == [0, 0, 2]
    # a diagonal step in all three coordinates joins; two bins apart in one does not
    assert labels([[0.5, 0.5, 0.5 * step], [1.5, -0.5, 1.5 * step]]) == [0, 0]
    assert labels([[0.5, 0.5, 0.5 * step], [2.5, 0.5, 0.5 * step]]) == [0, 1]
    assert labels([[0.5, 0.5, 0.5 * step], [0.5, 0.5, 2.5 * step]]) == [0, 1]
    # the heading seam, and headings far outside (-pi, pi]
    assert labels([[0.5, 0.5, math.pi - 0.01], [0.5, 0.5, -math.pi + 0.01]]) == [0, 0]
    kth = 36.0 / T.TWO_PI
    ok, b = M.bins_of([[0, 0, 7.0], [0, 0, -9.0]], np.ones(2), 1.0, 36)
    assert b[:, 2].tolist() == [math.floor(7.0 * kth) % 36, math.floor(-9.0 * kth) % 36] == [4, 20]
    # n_th <= 3: every heading is adjacent to every other; n_th = 4 separates opposite bins
    for n_th in (1, 2, 3):
        assert labels([[0.5, 0.5, 0.1], [0.5, 0.5, 3.0], [0.5, 0.5, -2.0]], n_th=n_th) == [0, 0, 0]
    assert labels([[0.5, 0.5, 0.1], [0.5, 0.5, 3.2]], n_th=4) == [0, 1]
    assert labels([[0.5, 0.5, 0.1], [0.5, 0.5, 1.7]], n_th=4) == [0, 0]
    # who contributes: weight 0, a NaN pose, a bin index out of range
    assert labels([[0.5, 0.5, 0], [0.5, 0.5, 0], [np.nan, 0, 0], [2.0 ** 23, 0, 0], [0.5, 0.5, 0]], w=[0, 1, 1, 1, 1]) == [-1, 1, -1, -1, 1]
    assert M.adjacent((0, 0, 0), (1, -1, 35), 36) and not M.adjacent((0, 0, 0), (0, 0, 2), 36) and not M.adjacent((0, 0, 0), (2, 0, 0), 36)


def test_order_and_rows_of_the_model():
    poses = np.array([[0.1, 0.1, 0.0], [5.1, 5.1, 1.0], [0.2, 0.2, 0.0], [5.2, 5.2, 1.0], [9.0, 9.0, 2.0]])
    info, f, i, lab, mem = M.pose_modes(poses, np.ones(5), T.W_UNIFORM, None, 0.5, 36, 2)
    assert info == [3, 3, 5, 5 << 32] and lab.tolist() == [0, 1, 0, 1, 4]
    assert i.tolist() == [[0, 2, 1, 0], [1, 2, 1, 1]]         # equal Q: the smaller root first; the third mode gets no row
    assert f[0, 12] == 2.0 * 2 ** 32 and f[0, 13] == 0.4 and f[0, 0] == pytest.approx(0.15)
    given = np.array([1.0, 2.0, 1.0, 2.0, 2.0 ** -40])
    info, f, i, lab, mem = M.pose_modes(poses, np.ones(5), T.W_GIVEN, given, 0.5, 36, 3)
    assert [r[3] for r in i] == [1, 0, 4] and f[2, 12] == 0.0 and i[2].tolist() == [4, 1, 1, 4]   # q = 0 is still a member
    assert info[3] == (2 << 32) + (2 << 31)
    info, f, i, lab, mem = M.pose_modes(poses, np.full(5, -np.inf), T.W_RESAMPLE, None, 0.5, 36, 2)
    assert info == [0, 0, 0, 0] and np.isnan(f[:, :12]).all() and i.tolist() == [[-1, 0, 0, -1]] * 2 and (lab == -1).all()


def test_kld_size():
    for k, eps, z in ((2, 0.05, 2.326), (10, 0.05, 2.326), (100, 0.05, 2.326), (1000, 0.01, 1.645), (37, 0.1, 3.0)):
        a = 2.0 / (9.0 * (k - 1))
        want = math.ceil((k - 1) / (2.0 * eps) * (1.0 - a + math.sqrt(a) * z) ** 3)
        assert locate.kld_size(k, eps, z) == want
    assert locate.kld_size(0) == locate.kld_size(1) == 1
    assert locate.kld_size(2) < locate.kld_size(20) < locate.kld_size(200)


def test_converged():
    m = lambda count, share: SimpleNamespace(count=count, share=np.array(share))
    assert not locate.converged(m(0, []))
    assert locate.converged(m(1, [1.0])) and locate.converged(m(3, [0.95, 0.03, 0.02]))
    assert not locate.converged(m(2, [0.9, 0.1])) and locate.converged(m(2, [0.9, 0.1]), share=0.9)
