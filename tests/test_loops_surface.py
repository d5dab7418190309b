"""thesis_amd/loops.py with score surfaces, without a GPU: relax() with an information matrix per edge against the sigma path and
against a dense Gauss-Newton written here, edge_information, match_informed and close_loops(information="surface") over a
stand-in engine whose match_pairs and score_surface are the oracles of tests/pairs_oracle.py and tests/surface_oracle.py."""
import math

import numpy as np
import pytest

from tests import surface_oracle as so
from tests import surface_scenes as scenes
from tests.pairs_oracle import OracleEngine
from tests.test_loops import SEARCH, graph, walk  # noqa: F401  (walk is a fixture)
from thesis_amd import loops, rebuild
from thesis_amd.engine import ParticleEngine, ScoreSurface


class SurfaceEngine(OracleEngine):
    """OracleEngine whose score_surface is the oracle; match_pairs notes whether the device was asked for."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.device_calls, self.surface_calls = [], []

    def match_pairs(self, *a, **kw):
        self.device_calls.append((kw.get("device", False), kw.get("return_scores", False)))
        return super().match_pairs(*a, **kw)

    def score_surface(self, scores, drop=None, drop_fraction=0.05, exclude=None, peaks=2, device=False):
        V = scores.scores
        if drop is None:
            drop = np.floor(float(drop_fraction) * (2 * np.asarray(scores.n_used, dtype=np.int64)).astype(np.float64)).astype(np.int32)
        ex = ParticleEngine.surface_exclusion(V.shape[2] // 2, V.shape[1] // 2) if exclude is None else exclude
        self.surface_calls.append((len(V), tuple(ex), peaks, device))
        rec, cnt = so.surface(V, drop, int(ex[0]), int(ex[1]), peaks)
        return ScoreSurface.from_records(rec, cnt, np.asarray(drop, dtype=np.int32), scores.substeps, scores.rot_step, scores.cell_size)


def dense_relax(poses, ij, z, info, iterations=30):
    """Gauss-Newton on sum e^T info e with dense normal equations, full information matrices, pose 0 held."""
    x = np.array(poses, dtype=np.float64)
    n = len(x)
    for _ in range(iterations):
        H, g = np.zeros((3 * n, 3 * n)), np.zeros(3 * n)
        for (i, j), zz, L in zip(ij, z, info):
            c, s = math.cos(x[i, 2]), math.sin(x[i, 2])
            dx, dy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
            th = x[j, 2] - x[i, 2] - zz[2]
            e = np.array([c * dx + s * dy - zz[0], -s * dx + c * dy - zz[1], (th + math.pi) % (2 * math.pi) - math.pi])
            J = np.zeros((3, 3 * n))
            J[:, 3 * i:3 * i + 3] = [[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0.0, 0.0, -1.0]]
            J[:, 3 * j:3 * j + 3] = [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]
            H += J.T @ L @ J
            g += J.T @ L @ e
        step = np.linalg.solve(H[3:, 3:], -g[3:])
        x[1:] += step.reshape(-1, 3)
        if np.abs(step).max() < 1e-13:
            break
    return x


def noisy_graph(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    truth, ij = graph(rng, n=14, extra=6)
    z = loops.relative(truth, ij[:, 0], ij[:, 1]) + rng.normal(0.0, 1.0, (len(ij), 3)) * [0.03, 0.03, 0.01]   # edges that disagree
    start = truth + rng.normal(0.0, 1.0, truth.shape) * [0.05, 0.05, 0.02]
    return rng, start, ij, z


def test_relax_with_diagonal_information_is_relax_with_sigmas():
    rng, start, ij, z = noisy_graph(21)
    st, sh = rng.uniform(0.02, 0.08, len(ij)), rng.uniform(0.005, 0.02, len(ij))
    info = np.zeros((len(ij), 3, 3))
    info[:, 0, 0] = info[:, 1, 1] = st ** -2.0
    info[:, 2, 2] = sh ** -2.0
    a, b = loops.relax(start, ij, z, st, sh), loops.relax(start, ij, z, information=info)
    assert np.abs(a - b).max() < 1e-9 and np.abs(a - start).max() > 1e-3


def test_relax_with_full_information_is_the_dense_solver():
    rng, start, ij, z = noisy_graph(22)
    A = rng.normal(0.0, 1.0, (len(ij), 3, 3))
    info = A @ np.transpose(A, (0, 2, 1)) + 0.5 * np.eye(3)
    info *= np.array([20.0, 20.0, 100.0])[:, None] * np.array([20.0, 20.0, 100.0])[None, :]      # metres and radians of a pose graph
    got, want = loops.relax(start, ij, z, information=info), dense_relax(start, ij, z, info)
    assert np.abs(got - want).max() < 1e-9
    diag = info * np.eye(3)
    assert np.abs(loops.relax(start, ij, z, information=diag) - got).max() > 1e-4                # the off-diagonal terms matter
    with pytest.raises(ValueError):
        loops.relax(start, ij, z, information=info[:-1])
    with pytest.raises(ValueError):
        loops.relax(start, ij, z, information=-info)
    with pytest.raises(ValueError):
        loops.relax(start, ij, z)


def flat_surface(n, second=(0, 0, 0, 0, 0, 0), weight=1, cell=0.1, rot_step=0.01):
    """A surface of n items whose best peak's plateau has the given second moments (sum w d d^T, in steps) and weight."""
    rec = np.zeros((n, 2, 16), dtype=np.int64)
    rec[:, 0, 3:6] = [100, max(1, weight), weight]
    rec[:, 0, 9:15] = second
    return ScoreSurface.from_records(rec, np.ones(n, np.int32), np.zeros(n, np.int32), 1, rot_step, cell)


def test_edge_information_of_a_lone_peak_is_the_fixed_information():
    info = loops.edge_information(flat_surface(3), [0.0, 1.0, -2.5], (0.05, 0.01))
    assert np.array_equal(info, np.broadcast_to(np.diag([1.0 / 0.05 ** 2, 1.0 / 0.05 ** 2, 1.0 / 0.01 ** 2]), (3, 3, 3)))


def test_edge_information_turns_the_plateau_into_the_frame_of_the_reference():
    # a plateau of weight 10 with sum w di^2 = 1000 steps^2: 100 steps^2 = 1 m^2 along world x, nothing else
    surf = flat_surface(2, second=(1000, 0, 0, 0, 0, 0), weight=10)
    assert np.allclose(surf.second_moment(0)[0], np.diag([1.0, 0.0, 0.0]))
    info = loops.edge_information(surf, [0.0, math.pi / 2], (0.05, 0.01))
    fixed = np.array([400.0, 400.0, 10000.0])
    # heading 0: the frame's x is world x; heading 90 degrees: world x is the frame's -y
    assert np.allclose(info[0], np.diag([1.0 / (0.0025 + 1.0), 400.0, 10000.0]), rtol=1e-12, atol=1e-9)
    assert np.allclose(info[1], np.diag([400.0, 1.0 / (0.0025 + 1.0), 10000.0]), rtol=1e-12, atol=1e-9)
    for m in info:                                       # never more than the fixed information: fixed - info is positive semi-definite
        assert np.linalg.eigvalsh(np.diag(fixed) - m).min() > -1e-9


def test_a_weak_direction_lets_the_odometry_win_there():
    """Eleven poses 1 m apart along x, consistent odometry, and one loop edge 0 -> 10 whose measurement is off by 0.5 m along
    the path and 0.2 m across it."""
    n = 11
    truth = np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)], axis=1)
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    ij = np.concatenate([chain, [[0, n - 1]]])
    z = np.concatenate([loops.relative(truth, chain[:, 0], chain[:, 1]), [[10.5, 0.2, 0.0]]])
    odo = np.diag([0.02 ** -2.0, 0.02 ** -2.0, 0.005 ** -2.0])
    fixed = loops.edge_information(flat_surface(1), [0.0])
    weak = loops.edge_information(flat_surface(1, second=(1000, 0, 0, 0, 0, 0), weight=10), [0.0])      # 1 m^2 along the path
    out = {}
    for name, last in (("fixed", fixed), ("weak", weak)):
        info = np.concatenate([np.broadcast_to(odo, (n - 1, 3, 3)), last])
        out[name] = loops.relax(truth, ij, z, information=info)
        assert np.abs(out[name] - dense_relax(truth, ij, z, info)).max() < 1e-9
    along = {k: v[-1, 0] - 10.0 for k, v in out.items()}
    across = {k: v[-1, 1] for k, v in out.items()}
    # the end pose moves less along the path, and across it as the dense solver says (above), which is as far as before:
    # the two directions couple only through the headings, a few hundredths of a radian here
    assert 0.0 < along["weak"] < 0.1 * along["fixed"] and along["fixed"] > 0.05
    assert across["fixed"] > 0.01 and abs(across["weak"] - across["fixed"]) < 0.1 * across["fixed"]
    # the sigma path is the fixed information
    assert np.abs(loops.relax(truth, ij, z, [0.02] * (n - 1) + [0.05], [0.005] * (n - 1) + [0.01]) - out["fixed"]).max() < 1e-9


def test_max_ambiguity_refuses_the_centred_room_and_keeps_the_other():
    centred, off = scenes.room(), scenes.room((0.5, 0.3))
    e = SurfaceEngine()
    found = {}
    for name, (poses, ranges, angles, pair, search) in (("centred", centred), ("off", off)):
        plain = loops.match(e, poses, ranges, angles, pair, **search)
        free = loops.match_informed(e, poses, ranges, angles, pair, **search)
        tight = loops.match_informed(e, poses, ranges, angles, pair, max_ambiguity=0.7, **search)
        for a, b in zip(plain, free.edges):
            assert np.array_equal(a, b)                  # with None the edges are match()'s
        assert plain.accepted.tolist() == [True]
        found[name] = (free.ambiguity[0], bool(tight.edges.accepted[0]))
        assert tight.ambiguity[0] == free.ambiguity[0] and tight.information.shape == (1, 3, 3)
    # the oracle's runner-up a quarter turn away: 157 / 168 = 0.935 at the centre, 80 / 173 = 0.462 off it
    assert found["centred"][0] > 0.7 > found["off"][0]
    assert found["centred"][1] is False and found["off"][1] is True
    assert e.device_calls.count((True, True)) == 4 and e.surface_calls[0] == (1, (2, 10), 2, False)


def test_match_informed_batches_like_match(walk, monkeypatch):  # noqa: F811
    truth, scans, ang = walk
    drift = truth.copy()
    drift[9:] += [0.15, -0.1, 0.03]
    pairs = loops.candidates(drift, min_gap=4, radius=0.5, half_run=2)
    e = SurfaceEngine()
    whole = loops.match_informed(e, drift, scans, ang, pairs, **SEARCH)
    assert e.calls == [6] and len(whole.surface.count) == 6 and whole.information.shape == (6, 3, 3)
    per_plain, per = loops.pairs_per_call(e, 18, 121, **SEARCH), loops.pairs_per_call(e, 18, 121, scores=True, **SEARCH)
    field = 112 + 32 * 9 + (2 * 228 + 1) * 17 * 8
    fixed = 18 * (32 + 8 * 121) + 16 * 121 + 4096
    assert per_plain == ((1 << 30) - fixed) // field and per == ((1 << 30) - fixed) // (field + 4 * 9 * 13 * 13)
    monkeypatch.setattr(loops, "SCRATCH_BYTES", fixed + 4 * (field + 4 * 9 * 13 * 13) + 5)
    e.calls.clear()
    parts = loops.match_informed(e, drift, scans, ang, pairs, **SEARCH)
    assert e.calls == [4, 2]
    for a, b in zip(parts.edges, whole.edges):
        assert np.array_equal(a, b)
    assert np.array_equal(parts.information, whole.information) and np.array_equal(parts.ambiguity, whole.ambiguity)
    for a, b in zip(parts.surface[:6], whole.surface[:6]):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        loops.match_informed(e, drift, scans, ang, pairs, device=True, **SEARCH)
    empty = loops.match_informed(e, drift, scans, ang, np.zeros((0, 3), np.int32), **SEARCH)
    assert empty.information.shape == (0, 3, 3) and empty.edges.accepted.shape == (0,)


def logged(walk_):
    truth, scans, ang = walk_
    path = np.concatenate([np.zeros((1, 3)), truth + [0.0123456789, -0.0987654321, 0.001]])      # record 0 holds no scan
    drift = path.copy()
    drift[10:] += [0.15, -0.1, 0.03]
    log = rebuild.ScanLog()
    for k, r in enumerate(scans):
        log.append(k + 1, r)
    return drift, log, ang, scans


def test_close_loops_with_lone_peaks_is_close_loops_with_fixed_sigmas(walk):  # noqa: F811
    drift, log, ang, _ = logged(walk)
    kw = dict(min_gap=4, radius=0.5, half_run=2, **SEARCH)
    fixed = loops.close_loops(SurfaceEngine(path=drift), log, ang, **kw)
    # an exclusion box of one candidate: every plateau is its peak alone
    lone = loops.close_loops(SurfaceEngine(path=drift), log, ang, information="surface", exclude=(0, 0), **kw)
    assert fixed.rounds[0].accepted == 6 and lone.rounds[0].accepted == 6
    assert np.abs(lone.poses - fixed.poses).max() < 1e-9
    # with the plateaus of the default box the loop edges weigh less, never more: the poses move, and no farther than before
    e = SurfaceEngine(path=drift)
    soft = loops.close_loops(e, log, ang, information="surface", **kw)
    assert soft.rounds[0].accepted == 6 and 0.0 < soft.rounds[0].moved <= fixed.rounds[0].moved + 1e-9
    assert e.device_calls == [(True, True)]
    with pytest.raises(ValueError):
        loops.close_loops(e, log, ang, max_ambiguity=0.5, **kw)
    with pytest.raises(ValueError):
        loops.close_loops(e, log, ang, information="learned", **kw)
    refused = loops.close_loops(SurfaceEngine(path=drift), log, ang, information="surface", max_ambiguity=0.0, **kw)
    # every pair here has a runner-up with a positive score: none survives a bound of 0, and the poses come back as they went in
    assert refused.rounds[0] == loops.LoopRound(6, 0, 0.0) and refused.poses.tobytes() == drift[1:].tobytes()


def test_close_loops_by_default_is_what_it_was(walk):  # noqa: F811
    """The default path is match() and relax() on sigmas, composed as before: the same poses bit for bit."""
    drift, log, ang, scans = logged(walk)
    e = SurfaceEngine(path=drift)
    out = loops.close_loops(e, log, ang, min_gap=4, radius=0.5, half_run=2, **SEARCH)
    assert e.device_calls == [(False, False)] and not e.surface_calls
    cur = drift[1:]
    n = len(cur)
    pairs = loops.candidates(cur, 4, 0.5, half_run=2)
    edges = loops.match(OracleEngine(), cur, scans, ang, pairs, **SEARCH)
    ok = edges.accepted
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    ij = np.concatenate([chain, np.stack([edges.r[ok], edges.q[ok]], axis=1)])
    z = np.concatenate([loops.relative(cur, chain[:, 0], chain[:, 1]), edges.z[ok]])
    st = np.concatenate([np.full(n - 1, 0.02), np.full(int(ok.sum()), 0.05)])
    sh = np.concatenate([np.full(n - 1, 0.005), np.full(int(ok.sum()), 0.01)])
    assert out.poses.tobytes() == loops.relax(cur, ij, z, st, sh).tobytes()
