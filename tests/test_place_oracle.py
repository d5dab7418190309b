"""Properties of the map-placement oracle (tests/place_oracle.py) that need no GPU: the cases in which the
resampling rule must reduce to a copy, a repeat or a block maximum, what lies outside the source, and the merge modes."""
import numpy as np
import pytest

from tests import place_oracle as po

CS = 0.05


def rand_src(rng, shape):
    return rng.integers(-30, 31, size=shape).astype(np.int8)


@pytest.mark.parametrize("S", range(1, 9))
def test_same_grid_is_a_copy(S):
    rng = np.random.Generator(np.random.PCG64(S))
    src = rand_src(rng, (37, 23))
    x0, y0 = -11, 140
    w, c = po.warp(src, CS, (x0 * CS, y0 * CS, 0.0), (x0, x0 + 37, y0, y0 + 23), CS, S)
    assert w.dtype == np.int8 and c.dtype == np.uint8
    assert np.array_equal(w, src) and np.all(c == 1)


@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_coarser_source_is_repeated(S):
    rng = np.random.Generator(np.random.PCG64(10 + S))
    src = rand_src(rng, (19, 31))
    x0, y0 = 6, -48
    w, c = po.warp(src, 2 * CS, (x0 * CS, y0 * CS, 0.0), (x0, x0 + 38, y0, y0 + 62), CS, S)
    assert np.array_equal(w, np.repeat(np.repeat(src, 2, axis=0), 2, axis=1)) and np.all(c == 1)


def test_finer_source_is_the_block_maximum():
    rng = np.random.Generator(np.random.PCG64(20))
    src = rand_src(rng, (40, 26))
    x0, y0 = -7, 3
    w, c = po.warp(src, CS / 2, (x0 * CS, y0 * CS, 0.0), (x0, x0 + 20, y0, y0 + 13), CS, 2)
    assert np.array_equal(w, src.reshape(20, 2, 13, 2).max(axis=(1, 3))) and np.all(c == 1)


def test_outside_the_source_is_uncovered_and_zero():
    rng = np.random.Generator(np.random.PCG64(21))
    src = rand_src(rng, (10, 10)) | 1                       # no zero in the source
    w, c = po.warp(src, CS, (0.0, 0.0, 0.0), (-5, 15, -5, 15), CS, 2)
    inside = np.zeros((20, 20), dtype=bool)
    inside[5:15, 5:15] = True
    assert np.array_equal(c.astype(bool), inside) and np.all(w[~inside] == 0) and np.array_equal(w[5:15, 5:15], src)
    w, c = po.warp(src, CS, (100.0, 100.0, 0.3), (-5, 15, -5, 15), CS, 3)       # a box that misses the source
    assert not c.any() and not w.any()


def test_quarter_turn_transposes():
    # yaw = pi/2: source x runs along world +y, source y along world -x.  The origin is an eighth of a cell off the grid, so that
    # no sample lies on a source cell boundary, where the rounding of cos(pi/2) = 6e-17 would decide.
    rng = np.random.Generator(np.random.PCG64(22))
    src = rand_src(rng, (8, 5))
    ox, oy = 5 * CS + CS / 8, -3 * CS + CS / 8
    w, c = po.warp(src, CS / 2, (ox, oy, np.pi / 2), (-1, 7, -4, 3), CS, 2)
    # world point (x, y) -> u = (y - oy) / sc, w = (ox - x) / sc
    want = np.zeros((8, 7), dtype=np.int16) - 128
    cov = np.zeros((8, 7), dtype=bool)
    for ix, X in enumerate(range(-1, 7)):
        for iy, Y in enumerate(range(-4, 3)):
            for a in (0.25, 0.75):
                for b in (0.25, 0.75):
                    u = int(np.floor(((Y + b) * CS - oy) / (CS / 2)))
                    v = int(np.floor((ox - (X + a) * CS) / (CS / 2)))
                    if 0 <= u < 8 and 0 <= v < 5:
                        cov[ix, iy] = True
                        want[ix, iy] = max(want[ix, iy], src[u, v])
    assert cov.any() and not cov.all()
    assert np.array_equal(c.astype(bool), cov) and np.array_equal(w, np.where(cov, want, 0))


def test_a_wall_survives_any_sampling():
    """A one-cell wall of a 0.03 m source crosses every 0.05 m cell it touches: with S = 4 (sample pitch 0.0125 m, less than
    half a source cell) no destination cell along it is left free."""
    src = np.full((200, 200), -30, np.int8)
    src[:, 100] = 30
    w, c = po.warp(src, 0.03, (-3.0, -3.0, 0.4), (-80, 80, -80, 80), CS, 4)
    assert c.any()
    # walk the wall's centre line in the world and look its cells up
    t = np.linspace(0.05, 5.95, 4000)
    cx, cy = np.cos(0.4), np.sin(0.4)
    wx = -3.0 + cx * t - cy * (100.5 * 0.03)
    wy = -3.0 + cy * t + cx * (100.5 * 0.03)
    X, Y = np.floor(wx / CS).astype(int) + 80, np.floor(wy / CS).astype(int) + 80
    ok = (X >= 0) & (X < 160) & (Y >= 0) & (Y < 160)
    assert ok.sum() > 1000 and np.all(w[X[ok], Y[ok]] == 30)


def test_merge_modes():
    old = np.array([[-30, -5, 0, 7, 30, 12]], dtype=np.int8)
    wrp = np.array([[10, 0, -4, 30, 5, -30]], dtype=np.int8)
    cov = np.array([[1, 1, 1, 0, 1, 1]], dtype=np.uint8)
    assert po.merge(old, wrp, cov, po.REPLACE, -30, 30).tolist() == [[10, 0, -4, 7, 5, -30]]
    assert po.merge(old, wrp, cov, po.KNOWN, -30, 30).tolist() == [[10, -5, -4, 7, 5, -30]]
    assert po.merge(old, wrp, cov, po.ADD, -30, 30).tolist() == [[-20, -5, -4, 7, 30, -18]]
    assert po.merge(np.array([[-28, 29]], np.int8), np.array([[-30, 30]], np.int8), np.ones((1, 2), np.uint8), po.ADD, -30, 30).tolist() == [[-30, 30]]
    with pytest.raises(ValueError):
        po.merge(old, wrp, cov, 3, -30, 30)


def test_resample_agrees_with_warp_on_the_lattice():
    rng = np.random.Generator(np.random.PCG64(23))
    src = rand_src(rng, (50, 60))
    pose = (-0.613, 0.277, 0.3)
    w, c = po.warp(src, 0.03, pose, (-20, 30, -10, 45), CS, 2)
    w2, c2 = po.resample(src, 0.03, pose, (50, 55), CS, (-20 * CS, -10 * CS, 0.0), 2)
    assert np.mean(w != w2) < 0.01 and np.mean(c != c2) < 0.01        # the same rule; only the rounding of a sample may differ
