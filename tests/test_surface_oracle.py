"""tests/surface_oracle.py against volumes whose peaks and sums are worked out by hand here, and against the
best-candidate loop of tests/pairs_oracle.match_one.  No GPU."""
import numpy as np

from tests import surface_oracle as so
from tests.refine_oracle import tie_order


def put(V, i, j, k, value):
    R, W = V.shape[0] // 2, V.shape[1] // 2
    V[k + R, i + W, j + W] = value


def record(i, j, k, s, size, w, first=(0, 0, 0), second=(0, 0, 0, 0, 0, 0)):
    return [i, j, k, s, size, w, *first, *second, 0]


def test_single_spike():
    V = np.zeros((3, 5, 5), dtype=np.int32)              # R = 1, W = 2
    put(V, 1, -1, 1, 10)
    rec, count = so.surface_one(V, 0, 1, 1, 2)
    assert count == 2
    # peak 0 is the spike; nothing else reaches 10 - 0, so the plateau is the spike alone with weight 1
    assert rec[0].tolist() == record(1, -1, 1, 10, 1, 1)
    # box 0 is i in 0 .. 2, j in -2 .. 0, k in 0 .. 1.  The rest is 0 everywhere, so peak 1 is the first of the tie order outside it:
    # (0, 0, 0) lies inside, then i^2 + j^2 = 1 at k = 0 in the order (i, j) = (-1, 0), (0, -1), ..: (-1, 0) has |i - 1| = 2: free.
    # Its box is i in -2 .. 0, j in -1 .. 1, k in -1 .. 1: 27 cells, of which (i = 0, j in {-1, 0}, k in {0, 1}) belong to box 0:
    # 23 cells of weight 1.  With di = i + 1, dj = j, dk = k the full box sums to 0 in every odd moment and the four missing
    # cells have di = 1, dj in {-1, 0}, dk in {0, 1}:
    #   sum di = 0 - 4 = -4, sum dj = 0 - (-2) = 2, sum dk = 0 - 2 = -2
    #   sum di^2 = 18 - 4 = 14, sum dj^2 = 18 - 2 = 16, sum dk^2 = 18 - 2 = 16
    #   sum di dj = 0 - (-2) = 2, sum di dk = 0 - 2 = -2, sum dj dk = 0 - (-1) = 1
    assert rec[1].tolist() == record(-1, 0, 0, 0, 23, 23, (-4, 2, -2), (14, 2, -2, 16, 1, 16))


def test_equal_spikes_come_in_tie_order():
    V = np.zeros((3, 3, 3), dtype=np.int32)              # R = 1, W = 1
    for i, j, k in [(0, 0, 1), (1, 0, 0), (0, -1, 0), (-1, 0, 0)]:
        put(V, i, j, k, 7)
    rec, count = so.surface_one(V, 0, 0, 0, 4)
    assert count == 4
    # the smaller |k| first; at k = 0 and i^2 + j^2 = 1 the lexicographically smaller (k, i, j)
    assert rec[:, :4].tolist() == [[-1, 0, 0, 7], [0, -1, 0, 7], [1, 0, 0, 7], [0, 0, 1, 7]]
    assert np.all(rec[:, 4:6] == 1) and not rec[:, 6:].any()


def test_ridge_along_i():
    V = np.zeros((1, 7, 7), dtype=np.int32)              # R = 0, W = 3
    V[0, :, 3] = 5                                       # j = 0, every i
    rec, count = so.surface_one(V, 0, 3, 0, 2)
    # the box of peak (0, 0, 0) is the whole volume: one peak; its plateau is the ridge, di = -3 .. 3, weight 1:
    # sum di^2 = 2 (1 + 4 + 9) = 28
    assert count == 1 and not rec[1].any()
    assert rec[0].tolist() == record(0, 0, 0, 5, 7, 7, second=(28, 0, 0, 0, 0, 0))
    # drop 2: the floor is 3, the zeros stay out, every ridge cell weighs 5 - 3 + 1 = 3
    rec, _ = so.surface_one(V, 2, 3, 0, 2)
    assert rec[0].tolist() == record(0, 0, 0, 5, 7, 21, second=(84, 0, 0, 0, 0, 0))
    # drop 5: the floor is 0 and the whole volume is the plateau: ridge cells weigh 6, the other 42 cells 1.
    # sum w = 42 + 42 = 84; sum w di^2 = 6 * 28 + 6 columns * 28 = 336; sum w dj^2 = 7 rows * 28 = 196 (the ridge has dj = 0)
    rec, _ = so.surface_one(V, 5, 3, 0, 2)
    assert rec[0].tolist() == record(0, 0, 0, 5, 49, 84, second=(336, 0, 0, 196, 0, 0))


def test_constant_volume():
    V = np.full((3, 5, 5), 4, dtype=np.int32)            # R = 1, W = 2
    rec, count = so.surface_one(V, 0, 1, 0, 3)
    assert count == 3
    # peak 0 is (0, 0, 0); its box |i|, |j| <= 1 at k = 0 is its plateau: 9 cells, sum di^2 = sum dj^2 = 6
    assert rec[0].tolist() == record(0, 0, 0, 4, 9, 9, second=(6, 0, 0, 6, 0, 0))
    # outside it the tie order goes on at k = 0 with i^2 + j^2 = 4: (i, j) = (-2, 0) first.  Its box i in -3 .. -1, j in -1 .. 1
    # is clipped at i = -2 and has lost i = -1 to box 0: 3 cells with dj = -1, 0, 1
    assert rec[1].tolist() == record(-2, 0, 0, 4, 3, 3, second=(0, 0, 0, 2, 0, 0))
    # then (0, -2): its box j in -3 .. -1 is clipped at j = -2 and has lost j = -1 to box 0: 3 cells with di = -1, 0, 1
    assert rec[2].tolist() == record(0, -2, 0, 4, 3, 3, second=(2, 0, 0, 0, 0, 0))
    # every later peak is the first of the tie order outside the boxes before it, whatever the shape
    V = np.full((5, 7, 7), 9, dtype=np.int32)            # R = 2, W = 3
    ex_t, ex_r = 1, 1
    rec, count = so.surface_one(V, 0, ex_t, ex_r, 8)
    assert count == 8
    found = []
    for p in range(8):
        want = next((i, j, k) for k, i, j in tie_order(3, 2)
                    if not any(abs(i - a) <= ex_t and abs(j - b) <= ex_t and abs(k - c) <= ex_r for a, b, c in found))
        assert tuple(rec[p, :3]) == want
        found.append(want)
    assert found[0] == (0, 0, 0)


def test_exclusion_over_the_whole_volume_leaves_one_peak():
    rng = np.random.Generator(np.random.PCG64(3))
    V = rng.integers(0, 50, size=(3, 5, 5)).astype(np.int32)
    rec, count = so.surface_one(V, 3, 4, 2, 8)
    assert count == 1 and not rec[1:].any() and rec[0, 3] == V.max()


def test_peak_0_is_the_best_of_the_matchers_own_loop():
    """tests/pairs_oracle.match_one picks its best by walking tie_order and keeping the first strictly larger score."""
    rng = np.random.Generator(np.random.PCG64(11))
    for R, W, top in [(0, 0, 5), (2, 3, 3), (4, 1, 2), (1, 5, 40), (3, 2, 1)]:
        for _ in range(4):
            V = rng.integers(0, top + 1, size=(2 * R + 1, 2 * W + 1, 2 * W + 1)).astype(np.int32)   # few values: many ties
            best = None
            for k, i, j in tie_order(W, R):
                sc = int(V[k + R, i + W, j + W])
                if best is None or sc > best[3]:
                    best = (i, j, k, sc)
            rec, count = so.surface_one(V, 0, 1, 1, 2)
            assert tuple(rec[0, :4]) == best and count >= 1


def test_peak_0_is_match_ones_result_on_its_own_volume():
    from tests import surface_scenes as scenes
    for scene in (scenes.corridor(), scenes.room(), scenes.room((0.5, 0.3))):
        _, m8, V = scenes.oracle_volume(scene)
        rec, _ = so.surface_one(V, 5, 2, 2, 2)
        assert rec[0, :4].tolist() == m8[:4].tolist()


def test_invariants_on_random_volumes():
    rng = np.random.Generator(np.random.PCG64(5))
    V = rng.integers(0, 200, size=(4, 7, 9, 9)).astype(np.int32)
    rec, count = so.surface(V, drop=[0, 7, 30, 200], ex_t=2, ex_r=1, K=5)
    for n in range(4):
        c = int(count[n])
        assert c >= 1 and np.all(np.diff(rec[n, :c, 3]) <= 0)            # scores do not increase over the peaks
        assert np.all(rec[n, :c, 4] >= 1) and np.all(rec[n, :c, 5] >= rec[n, :c, 4])   # the peak is in its plateau; sum w >= |T|
        assert not rec[n, c:].any()
