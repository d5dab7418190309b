"""The NumPy model of the trajectory log (tests/track_oracle.py) that tests/test_gpu_track.py leans on: the chunked three-stage
scan equals the walk of one particle at a time, and the fsum estimate row meets hand cases.  No GPU."""
import math

import numpy as np
import pytest

from tests import track_oracle as T


def random_log(rng, P, N, merge=0.5):
    """A TrackModel of N records driven at random: 0, 1 or 2 resamples between records, some of them collapsing lineages."""
    m = T.TrackModel(rng.normal(size=(P, 3)), np.ones(P))
    for _ in range(N - 1):
        for _ in range(int(rng.integers(0, 3))):
            idx = np.sort(rng.integers(0, P, size=P)) if rng.random() < merge else rng.permutation(P)
            m.resample(idx.astype(np.int32))
        m.record(rng.normal(size=(P, 3)), np.ones(P))
    for _ in range(int(rng.integers(0, 3))):                   # resamples after the last record stay pending
        m.resample(np.sort(rng.integers(0, P, size=P)).astype(np.int32))
    return m


@pytest.mark.parametrize("P", [1, 2, 63, 65, 300])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 3 * 64 + 5])
def test_chunked_scan_equals_the_walk(P, N):
    rng = np.random.default_rng(1000 * P + N)
    m = random_log(rng, P, N)
    parent = np.stack(m.parent)
    want, _ = m.lineage()
    assert np.array_equal(T.lineage_chunked(parent, m.pending), want)
    some = rng.integers(0, P, size=min(P, 7))
    assert np.array_equal(T.lineage_chunked(parent, m.pending, particles=some), m.lineage(list(some))[0])
    for t0, t1 in ((0, 1), (N // 3, N // 3 + 1), (N // 2, N), (max(N - 70, 0), max(N - 3, 1)), (min(66, N - 1), N)):
        if 0 <= t0 < t1 <= N:
            assert np.array_equal(T.lineage_chunked(parent, m.pending, t0=t0, t1=t1), m.lineage(None, t0, t1)[0]), (t0, t1)
    for chunk in (1, 3, 64, 1000):                              # the result does not depend on the chunk length
        assert np.array_equal(T.lineage_chunked(parent, m.pending, chunk=chunk), want)


def test_lineage_follows_a_known_genealogy():
    m = T.TrackModel(np.zeros((4, 3)), np.ones(4))
    m.resample([0, 0, 2, 3])
    m.resample([1, 1, 1, 3])                                    # two resamples compose: current 0, 1, 2 all come from 0
    m.record(np.ones((4, 3)), np.ones(4))
    m.record(2 * np.ones((4, 3)), np.ones(4))                   # none in between: the identity
    m.resample([3, 3, 3, 3])                                    # after the last record
    idx, pose = m.lineage()
    assert idx.tolist() == [[3, 3, 3, 3], [3, 3, 3, 3], [3, 3, 3, 3]]
    m.pending = np.arange(4, dtype=np.int32)
    assert m.lineage()[0].tolist() == [[0, 0, 0, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert [len(np.unique(r)) for r in m.lineage()[0]] == [2, 4, 4]
    assert np.array_equal(m.lineage()[1][2], 2 * np.ones((4, 3)))


def test_estimate_all_particles_equal():
    f, i = T.estimate_row(np.tile([1.5, -2.0, 0.3], (9, 1)), np.ones(9), T.W_UNIFORM)
    assert np.allclose(f[0:3], [1.5, -2.0, 0.3], rtol=0, atol=1e-15)
    assert np.allclose(f[3:9], 0, atol=1e-30) and abs(f[9] - 1) < 1e-15
    assert f[10] == 9 and abs(f[11] - 9) < 1e-12 and list(f[12:]) == [0, 0, 0, 0]
    assert i.tolist() == [0, 9, -1, 0]


def test_estimate_heading_mean_across_the_cut():
    """Two particles at +-(pi - 0.01): the mean heading is pi, not 0, and the spread is 0.01, not pi."""
    poses = np.array([[0, 0, math.pi - 0.01], [0, 0, -(math.pi - 0.01)]])
    f, _ = T.estimate_row(poses, np.ones(2), T.W_UNIFORM)
    assert abs(abs(f[2]) - math.pi) < 1e-15
    assert abs(f[8] - 1e-4) < 1e-15 and abs(f[9] - math.cos(0.01)) < 1e-15


def test_estimate_one_survivor():
    w = np.full(5, -np.inf)
    w[3] = -7.0                                                 # -inf -> 0; the minimum -7 is added to the non-zero one: 0
    f, i = T.estimate_row(np.arange(15.0).reshape(5, 3), w)
    assert np.isnan(f[:12]).all() and i.tolist() == [3, 0, -1, 0]
    w[3] = 2.0
    f, i = T.estimate_row(np.arange(15.0).reshape(5, 3), w)
    assert f[0:2].tolist() == [9.0, 10.0] and abs(T.wrap(f[2] - 11.0)) < 1e-15 and i.tolist() == [3, 1, -1, 0]
    assert np.allclose(f[3:9], 0, atol=1e-30) and f[10] == 2.0 and f[11] == 1.0


def test_estimate_no_weight():
    f, i = T.estimate_row(np.zeros((3, 3)), np.zeros(3))
    assert np.isnan(f[:12]).all() and list(f[12:]) == [0, 0, 0, 0] and i.tolist() == [0, 0, -1, 0]


def test_estimate_leaves_out_bad_particles_and_shifts_negative_weights():
    poses = np.array([[1.0, 0, 0], [np.nan, 0, 0], [3.0, 0, 0], [5.0, 0, 0]])
    f, i = T.estimate_row(poses, np.array([-2.0, 4.0, 0.0, 2.0]))          # resample weights: 0, 6, 0, 4; particle 1 is NaN
    assert i.tolist() == [1, 1, -1, 0] and f[0] == 5.0 and f[10] == 4.0
    f, i = T.estimate_row(poses, np.ones(4), T.W_GIVEN, given=[1.0, 1.0, 1.0, 2.0])
    assert i[1] == 3 and f[0] == (1 + 3 + 10) / 4 and f[10] == 4.0
    assert np.all(T.est_tolerance(poses, np.ones(4), T.W_GIVEN, given=[1.0, 1.0, 1.0, 2.0])[:2] < 1e-14)
