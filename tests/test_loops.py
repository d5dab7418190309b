"""thesis_amd/loops.py without a GPU: candidate pairs, the bookkeeping of match() over a stand-in engine whose match_pairs is
the oracle of tests/pairs_oracle.py, the pose-graph relaxation on graphs whose answer is known, and close_loops' identity."""
import math

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds
from tests.locate_oracle import asym_room
from tests.pairs_oracle import OracleEngine
from thesis_amd import loops, rebuild


def test_candidates_gap_radius_order_and_clipping():
    x = np.concatenate([np.arange(10) * 1.0, [2.1, 0.2, 7.0, 3.5]])          # scans 0 .. 9 walk out, 10 .. 13 come back to places
    poses = np.stack([x, np.zeros(14), np.zeros(14)], axis=1)
    got = loops.candidates(poses, min_gap=3, radius=0.5, half_run=2)
    # q = 10 (x 2.1): r < 10 - 3 - 2 = 5, nearest 2 (0.1 away); q = 11 (x 0.2): r < 6, nearest 0: the run is clipped at 0;
    # q = 12 (x 7.0): r < 7, so scan 7 itself is too recent and scan 6 is 1 m away: none; q = 13 (x 3.5): 3 and 4 tie: the smaller
    assert got.dtype == np.int32 and got.tolist() == [[10, 0, 5], [11, 0, 3], [13, 1, 6]]
    assert loops.candidates(poses, 3, 1.0, half_run=2, per_query=2).tolist() == [[10, 0, 5], [10, 1, 6], [11, 0, 3], [11, 0, 4], [12, 4, 9],
                                                                                   [13, 1, 6], [13, 2, 7]]
    assert loops.candidates(poses, 3, 0.5, half_run=2, stride=10).tolist() == [[10, 0, 5]]
    none = loops.candidates(poses, 20, 5.0)
    assert none.shape == (0, 3) and none.dtype == np.int32
    assert loops.candidates(poses, 0, 0.0, half_run=0).tolist() == [[12, 7, 8]]            # scan 12 stands where scan 7 stood
    with pytest.raises(ValueError):
        loops.candidates(poses, 3, 1.0, stride=0)


@pytest.fixture(scope="module")
def walk():
    """Eighteen scans of 121 beams in the asymmetric room: the sensor walks 1.6 m along x and backs up beside its track.
    (poses, scans, angles)."""
    cells, x0, y0 = asym_room(0.05)
    ang = np.linspace(-0.75 * math.pi, 0.75 * math.pi, 121)
    xs = np.concatenate([np.arange(9) * 0.2, 1.6 - np.arange(9) * 0.2])
    poses = np.stack([xs - 1.0, np.where(np.arange(18) < 9, 1.5, 1.6), np.where(np.arange(18) < 9, 0.1, 0.2)], axis=1)
    lo, hi = lattice_bounds(800, 3)
    scans = np.stack([cast(cells, x0, y0, lo, hi, 20.0, 0.1, 1.0, p, ang, 12.0)[0] for p in poses])
    return poses, scans, ang


SEARCH = dict(window=6, rotations=4, rot_step=math.radians(1.0))


def test_match_bookkeeping_and_chunking(walk, monkeypatch):
    truth, scans, ang = walk
    drift = truth.copy()
    drift[9:] += [0.15, -0.1, 0.03]                      # the way back has drifted: three cells, two cells, three steps
    pairs = loops.candidates(drift, min_gap=4, radius=0.5, half_run=2)
    assert pairs[:, 0].tolist() == [12, 13, 14, 15, 16, 17] and pairs[-1].tolist() == [17, 0, 4]      # r = 1: its run is clipped at 0
    e = OracleEngine()
    whole = loops.match(e, drift, scans, ang, pairs, **SEARCH)
    assert e.calls == [6]
    assert whole.q.tolist() == pairs[:, 0].tolist() and whole.r.tolist() == ((pairs[:, 1] + pairs[:, 2]) // 2).tolist()
    res = e.match_pairs(drift, scans, ang, pairs, **SEARCH)
    assert np.array_equal(whole.fraction, res.score / (2.0 * res.n_used)) and np.array_equal(whole.fraction_guess, res.score_guess / (2.0 * res.n_used))
    assert np.allclose(whole.z, loops.relative(np.concatenate([drift, res.poses]), whole.r, 18 + np.arange(6)), atol=1e-15)
    # the matches undo the drift: seen from the run's middle scan, the query sits where the truth has it, to a cell and a step
    want = loops.relative(truth, whole.r, whole.q)
    assert np.all(whole.accepted) and np.abs(whole.z - want)[:, :2].max() < 0.08 and np.abs(whole.z - want)[:, 2].max() < 0.02
    # acceptance: the fraction, the gain over the guess unless the guess stayed, the number of beams
    assert not loops.match(e, drift, scans, ang, pairs, accept=1.01, **SEARCH).accepted.any()
    assert not loops.match(e, drift, scans, ang, pairs, min_used=122, **SEARCH).accepted.any()
    settled = drift.copy()
    settled[pairs[:, 0]] = res.poses                     # every query where its match put it: the runs hold none of them
    at_truth = loops.match(e, settled, scans, ang, pairs, gain=0.5, **SEARCH)
    assert np.all(at_truth.accepted) and np.all(at_truth.fraction == at_truth.fraction_guess)      # already best: gain does not apply
    assert not loops.match(e, drift, scans, ang, pairs, gain=0.99, **SEARCH).accepted.any()
    # chunks: a scratch limit that admits four pairs a call gives the same edges
    per = loops.pairs_per_call(e, 18, 121, limit=1 << 30, **SEARCH)
    fixed = 18 * (32 + 8 * 121) + 16 * 121 + 4096
    assert per == ((1 << 30) - fixed) // (112 + 32 * 9 + (2 * 228 + 1) * 17 * 8)
    monkeypatch.setattr(loops, "SCRATCH_BYTES", fixed + 4 * (112 + 32 * 9 + (2 * 228 + 1) * 17 * 8) + 5)
    e.calls.clear()
    parts = loops.match(e, drift, scans, ang, pairs, **SEARCH)
    assert e.calls == [4, 2]
    for a, b in zip(parts, whole):
        assert np.array_equal(a, b)
    empty = loops.match(e, drift, scans, ang, np.zeros((0, 3), np.int32), **SEARCH)
    assert empty.z.shape == (0, 3) and empty.accepted.shape == (0,)
    with pytest.raises(ValueError):
        loops.match(e, drift, scans, ang, pairs, device=True)


def graph(rng, n=30, extra=12):
    truth = np.cumsum(rng.uniform(-1.0, 1.0, (n, 3)) * [0.5, 0.5, 0.4], axis=0)
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    more = np.array([sorted(rng.choice(n, 2, replace=False)) for _ in range(extra)])
    ij = np.concatenate([chain, more])
    return truth, ij


def test_relax_on_consistent_edges_returns_the_truth():
    rng = np.random.Generator(np.random.PCG64(3))
    truth, ij = graph(rng)
    z = loops.relative(truth, ij[:, 0], ij[:, 1])
    for trial in range(3):
        start = truth + rng.normal(0.0, 1.0, truth.shape) * [0.1, 0.1, 0.05]
        start[0] = truth[0]                              # pose 0 is held
        out = loops.relax(start, ij, z, 0.05, rng.uniform(0.005, 0.02, len(ij)))
        assert np.abs(out - truth).max() < 1e-9, trial
    assert loops.relax(truth, ij, z, 0.05, 0.01).tobytes() != b"" and np.abs(loops.relax(truth, ij, z, 0.05, 0.01) - truth).max() < 1e-12
    assert loops.relax(truth, np.zeros((0, 2), int), np.zeros((0, 3)), 1.0, 1.0).tobytes() == truth.tobytes()
    with pytest.raises(ValueError):
        loops.relax(truth, [[0, 0]], [[0.0, 0.0, 0.0]], 1.0, 1.0)


def test_relax_closes_a_square_with_a_heading_bias():
    """A 10 m square walked in 40 steps of 1 m; the odometry's heading is off by 0.01 rad a step, so dead reckoning ends
    2.678 m from where the walk ends.  Four true loop edges join the last four poses to the first four.  Measured: the end
    point's error falls to 0.0217 m, 0.0081 of the dead-reckoned one, and the mean pose error from 1.191 m to 0.085 m: the
    loop edges pin the end and the relaxation spreads the bias along the path.  The result depends on the sparse solver only
    in its last bits; the assertions leave a factor of six on the end point (0.05) and of seven on the mean (0.5), so that
    they say what the feature is for, the ends meet and the path follows, and not which digits this machine printed."""
    n = 41
    truth = np.zeros((n, 3))
    for k in range(1, n):
        th = truth[k - 1, 2]
        truth[k] = truth[k - 1] + [math.cos(th), math.sin(th), (math.pi / 2 if k % 10 == 0 else 0.0)]
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    odo = loops.relative(truth, chain[:, 0], chain[:, 1]) + [0.0, 0.0, 0.01]
    dead = np.zeros((n, 3))
    for k in range(1, n):
        c, s = math.cos(dead[k - 1, 2]), math.sin(dead[k - 1, 2])
        dead[k] = dead[k - 1] + [c * odo[k - 1, 0] - s * odo[k - 1, 1], s * odo[k - 1, 0] + c * odo[k - 1, 1], odo[k - 1, 2]]
    loop = np.stack([np.arange(4), np.arange(37, 41)], axis=1)
    ij = np.concatenate([chain, loop])
    z = np.concatenate([odo, loops.relative(truth, loop[:, 0], loop[:, 1])])
    st = np.concatenate([np.full(n - 1, 0.02), np.full(4, 0.05)])
    sh = np.concatenate([np.full(n - 1, 0.005), np.full(4, 0.01)])
    out = loops.relax(dead, ij, z, st, sh)
    err = lambda p: np.hypot(p[:, 0] - truth[:, 0], p[:, 1] - truth[:, 1])
    before, after = err(dead), err(out)
    print("end point: %.4f m -> %.4f m (ratio %.4f); mean: %.4f m -> %.4f m" % (before[-1], after[-1], after[-1] / before[-1], before.mean(), after.mean()))
    assert before[-1] > 2.0 and after[-1] < 0.05 * before[-1] and after.mean() < 0.5 * before.mean()


def test_close_loops_without_an_accepted_edge_is_the_identity(walk):
    truth, scans, ang = walk
    path = np.concatenate([np.zeros((1, 3)), truth + [0.0123456789, -0.0987654321, 0.001]])      # record 0 holds no scan
    e = OracleEngine(path=path)
    log = rebuild.ScanLog()
    for k, r in enumerate(scans):
        log.append(k + 1, r)
    out = loops.close_loops(e, log, ang, min_gap=4, radius=0.5, half_run=2, accept=1.01, rounds=3, **SEARCH)
    assert out.poses.tobytes() == path[1:].tobytes() and out.records.tolist() == list(range(1, 19))
    assert out.rounds == [loops.LoopRound(7, 0, 0.0)] and len(out.edges.q) == 7 and not out.edges.accepted.any()
    assert len(e.built_at) == 1 and e.built_at[0].tobytes() == path[1:].tobytes() and out.built.cell_size == 0.05
    # and with the drift of the way back, the loop edges pull it home
    drift = path.copy()
    drift[10:] += [0.15, -0.1, 0.03]
    e2 = OracleEngine(path=drift)
    closed = loops.close_loops(e2, log, ang, min_gap=4, radius=0.5, half_run=2, **SEARCH)
    assert closed.rounds[0].pairs == 6 and closed.rounds[0].accepted == 6 and closed.rounds[0].moved > 0.05
    d = lambda p: np.hypot(*(p[9:, :2] - path[10:, :2]).T).mean()
    assert d(closed.poses) < 0.5 * d(drift[1:]) and closed.poses[0].tobytes() == drift[1].tobytes()
    given = loops.close_loops(e2, log, ang, poses=path[1:], min_gap=4, radius=0.5, half_run=2, accept=1.01, **SEARCH)
    assert given.poses.tobytes() == path[1:].tobytes()
    with pytest.raises(ValueError):
        loops.close_loops(e2, log, ang, poses=path[:5])
