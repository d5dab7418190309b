"""Pair matching on the GPU (rbpf_match_pairs, kernels_pairs.hip) against the NumPy oracle of tests/pairs_oracle.py: the whole
score volume, out_m8 and out_pose_m3 bit for bit.  Then what the call leaves alone, its device outputs, its argument checks, and
thesis_amd/loops.py on a run.  No accuracy is asserted here: the GPU result is the oracle's, and tests/test_pairs_oracle.py and
tests/test_loops.py carry the accuracy claims."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds
from tests.locate_oracle import asym_room
from tests.pairs_oracle import OracleEngine, match_pairs as oracle_pairs
from tests.test_gpu_locate import engine, load_room, rng_state
from tests.test_pairs_oracle import border_case

pytestmark = pytest.mark.gpu

STEP = math.radians(0.5)
LO, HI = 0.3, 11.0


def gpu(e, poses, ranges, angles, pairs, guesses=None, cell=0.05, lo=LO, hi=HI, S=1, W=6, R=3, step=STEP, **kw):
    return e.match_pairs(poses, ranges, angles, pairs, guesses=guesses, cell_size=cell, substeps=S, window=W, rotations=R, rot_step=step,
                         min_range=lo, max_range=hi, return_scores=True, **kw)


def oracle(poses, ranges, angles, pairs, guesses=None, cell=0.05, lo=LO, hi=HI, S=1, W=6, R=3, step=STEP):
    return oracle_pairs(poses, ranges, angles, pairs, guesses, 1.0 / cell, lo, hi, S, W, R, step)


def assert_same(res, want, what=""):
    poses, m8, scores = want
    got8 = np.concatenate([res.index, res.score[:, None], res.score_guess[:, None], res.n_used[:, None], res.n_ref[:, None]], axis=1)
    assert res.scores.shape == scores.shape and res.scores.dtype == np.int32, (what, res.scores.shape, scores.shape)
    bad = res.scores != scores
    if bad.any():
        k = tuple(int(q) for q in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: scores differ in {int(bad.sum())} of {bad.size} candidates; first [m, k, i, j] = {k}: got {res.scores[k]}, oracle {scores[k]}")
    assert np.array_equal(got8, m8[:, :7]), (what, got8[np.any(got8 != m8[:, :7], axis=1)][:4], m8[np.any(got8 != m8[:, :7], axis=1)][:4])
    assert res.poses.dtype == np.float64 and res.poses.tobytes() == poses.tobytes(), (what, res.poses - poses)


def both(e, poses, ranges, angles, pairs, what, guesses=None, **kw):
    res = gpu(e, poses, ranges, angles, pairs, guesses, **kw)
    assert_same(res, oracle(poses, ranges, angles, pairs, guesses, **kw), what)
    return res


@pytest.fixture(scope="module")
def scene():
    """Twenty scans of 61 beams in the asymmetric room, cast by the CPU oracle: scans 0 .. 17 along a walk and back beside it,
    scan 18 a hundred metres away, scan 19 without a used beam.  Ranges that are not used stand in queries and references.
    Twelve pairs with runs of 1, 3 and 20, and a guess for each."""
    cells, x0, y0 = asym_room(0.05)
    ang = np.linspace(-0.75 * math.pi, 0.75 * math.pi, 61)
    xs = np.concatenate([np.arange(9) * 0.2, 1.6 - np.arange(9) * 0.2])
    poses = np.stack([xs - 1.0, np.where(np.arange(18) < 9, 1.5, 1.6), np.where(np.arange(18) < 9, 0.1, 0.2)], axis=1)
    lo, hi = lattice_bounds(800, 3)
    scans = np.stack([cast(cells, x0, y0, lo, hi, 20.0, 0.1, 1.0, p, ang, 12.0)[0] for p in poses])
    poses = np.concatenate([poses, [[100.3, -99.2, 1.0], [0.0, 1.5, 0.0]]])
    scans = np.concatenate([scans, scans[4:5], np.full((1, 61), np.nan)])
    scans[2, :9] = [np.nan, np.inf, -np.inf, 0.0, -2.0, 0.3, 11.0, 0.2999, 11.0001]      # none of them is used in (0.3, 11)
    scans[12, :9] = scans[2, :9]
    scans[14, ::2] = 30.0
    pairs = np.array([[12, 3, 6], [13, 2, 5], [12, 2, 3], [14, 0, 20], [17, 0, 1], [19, 0, 3], [10, 19, 20], [11, 18, 19],
                      [4, 3, 6], [16, 0, 20], [2, 12, 15], [15, 14, 15]], dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(12))
    guesses = poses[pairs[:, 0]] + rng.uniform(-1.0, 1.0, (12, 3)) * [0.2, 0.2, 0.03]
    guesses[8] = poses[4]                                # the self-match: scan 4 in its own run, at its own pose
    return poses, scans, ang, pairs, guesses


@pytest.fixture(scope="module")
def eng():
    e = engine(2)
    load_room(e, particle=1)                             # a map nothing here may read
    yield e
    e.close()


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,W,R", [(1, 16, 4), (1, 3, 2), (2, 7, 1), (4, 12, 3), (8, 12, 2), (16, 9, 3), (4, 0, 4), (4, 6, 0), (2, 0, 0),
                                   (1, 32, 1), (4, 1, 100)])
def test_a_batch_of_twelve_pairs(eng, scene, S, W, R):
    poses, scans, ang, pairs, guesses = scene
    res = both(eng, poses, scans, ang, pairs, f"S {S}, W {W}, R {R}", guesses, S=S, W=W, R=R)
    n_used = np.sum((scans > LO) & (scans < HI), axis=1)
    assert res.n_used.tolist() == n_used[pairs[:, 0]].tolist() and res.n_used[5] == 0 and res.n_used[0] <= 61 - 9
    assert res.n_ref.tolist() == [int(n_used[a:b].sum()) for _, a, b in pairs] and res.n_ref[6] == 0
    for m in (5, 6, 7):                                  # a query without a used beam, a run without one, a run outside the window
        assert res.index[m].tolist() == [0, 0, 0] and res.score[m] == 0 and not res.scores[m].any() and res.poses[m].tobytes() == guesses[m].tobytes()
    assert res.index[8].tolist() == [0, 0, 0] and res.score[8] == res.score_guess[8] == 2 * res.n_used[8] and res.poses[8].tobytes() == poses[4].tobytes()
    assert np.all(res.score <= 2 * res.n_used) and np.all(res.score >= res.score_guess) and res.score.max() > 60
    assert (res.substeps, res.rot_step, res.cell_size) == (S, STEP, 0.05)


@pytest.mark.parametrize("cell", [0.1, 0.037])
def test_other_cell_sizes(eng, scene, cell):
    poses, scans, ang, pairs, guesses = scene
    res = both(eng, poses, scans, ang, pairs, f"cell {cell}", guesses, cell=cell, S=2, W=5, R=2)
    assert res.cell_size == cell and res.score[8] == 2 * res.n_used[8] and res.score.max() > 60
    # None is the engine's own tile_len / dim
    own = eng.match_pairs(poses, scans, ang, pairs, guesses, substeps=2, window=5, rotations=2, min_range=LO, max_range=HI, return_scores=True)
    assert_same(own, oracle(poses, scans, ang, pairs, guesses, S=2, W=5, R=2), "the engine's cell size")


def test_reference_points_one_cell_outside_the_window(eng):
    poses, scans, ang, pair, Mw = border_case()
    res = both(eng, poses, scans, ang, [pair], "the window's border", lo=0.01, hi=2.0, S=1, W=4, R=0, step=0.0)
    assert res.index.tolist() == [[0, 3, 0]] and res.score[0] == 2 and res.n_ref[0] == 12 and res.scores[0, 0, 8, 4] == 2


def test_launch_shapes_and_guesses_agree(eng, scene, monkeypatch):
    """RBPF_PAIRS_KPW sets the rotations a workgroup takes (a batch this small gets one each); a pair alone gives its row of
    the batch; no guess is the query's own pose as the guess."""
    poses, scans, ang, pairs, guesses = scene
    kw = dict(S=4, W=12, R=10)
    monkeypatch.delenv("RBPF_PAIRS_KPW", raising=False)
    whole = gpu(eng, poses, scans, ang, pairs, guesses, **kw)
    want = oracle(poses, scans, ang, pairs, guesses, **kw)
    assert_same(whole, want, "one rotation per workgroup")
    for kpw in ("5", "2", "16"):                         # 21 rotations in runs of 5, 2 and 16
        monkeypatch.setenv("RBPF_PAIRS_KPW", kpw)
        assert_same(gpu(eng, poses, scans, ang, pairs, guesses, **kw), want, f"{kpw} rotations per workgroup")
    monkeypatch.delenv("RBPF_PAIRS_KPW")
    for m in (0, 3, 8, 11):
        alone = gpu(eng, poses, scans, ang, pairs[m], guesses[m], **kw)
        assert np.array_equal(alone.scores[0], whole.scores[m]) and alone.poses.tobytes() == whole.poses[m].tobytes()
        assert alone.index.tolist() == [whole.index[m].tolist()] and alone.n_ref[0] == whole.n_ref[m] and alone.n_used[0] == whole.n_used[m]
    null = gpu(eng, poses, scans, ang, pairs, None, **kw)
    given = gpu(eng, poses, scans, ang, pairs, poses[pairs[:, 0]], **kw)
    assert_same(null, oracle(poses, scans, ang, pairs, None, **kw), "no guesses")
    for name in ("poses", "index", "score", "score_guess", "n_used", "n_ref", "scores"):
        assert np.array_equal(getattr(null, name), getattr(given, name)), name
    # more tasks than lanes (65 x 9 per rotation) and more beams than the table holds: several passes, several chunks
    monkeypatch.setenv("RBPF_PAIRS_KPW", "3")
    many = np.tile(scans, (1, 25))[:, :1500]
    a_many = np.linspace(-math.pi, math.pi, 1500, endpoint=False)
    both(eng, poses, many, a_many, pairs[:2], "3 rotations per workgroup, 1500 beams, W 32", guesses[:2], hi=6.0, S=2, W=32, R=2)


def test_the_window_limit_at_0025(eng, scene):
    from thesis_amd.engine import RbpfError
    poses, scans, ang, pairs, guesses = scene
    # 16384 + (2 Mw + 1) WW 8 <= 163776 bytes admits Mw <= 367 = ceil(max_range * 40) + ceil(W / S) + 2
    for S, W, reach in ((1, 16, 349), (4, 12, 362), (1, 0, 365), (1, 32, 333)):
        m = eng.match_max_range(0.025, S, W)
        assert abs(m - reach / 40.0) < 1e-12 and math.ceil(m * 40.0) == reach
    most = eng.match_max_range(0.025, 1, 16)
    res = both(eng, poses, scans, ang, pairs[[0, 3, 8]], "0.025 m at the limit", guesses[[0, 3, 8]], cell=0.025, hi=most, S=1, W=16, R=1)
    assert res.score.min() > 0 and res.n_used.tolist() == [int(np.sum((scans[q] > LO) & (scans[q] < most))) for q in (12, 14, 4)]
    for beyond in (most + 1e-9, 11.0):
        with pytest.raises(RbpfError) as err:
            eng.match_pairs(poses, scans, ang, pairs, cell_size=0.025, max_range=beyond)
        assert err.value.code == -1 and "8.72" in str(err.value) and "349" in str(err.value)    # 8.725 * 40 rounds above 349: the float below it


# ---- 2. device outputs --------------------------------------------------------------------------------------------------------------
def test_device_outputs_equal_host_outputs(eng, scene):
    torch = pytest.importorskip("torch")
    from thesis_amd import _lib
    poses, scans, ang, pairs, guesses = scene
    kw = dict(S=4, W=4, R=2)
    host = gpu(eng, poses, scans, ang, pairs, guesses, **kw)
    dev = gpu(eng, poses, scans, ang, pairs, guesses, device=True, **kw)
    assert isinstance(dev.poses, torch.Tensor) and dev.poses.device.type == "cuda" and dev.poses.dtype == torch.float64
    assert dev.scores.dtype == torch.int32 and dev.index.shape == (12, 3)
    for name in ("poses", "index", "score", "score_guess", "n_used", "n_ref", "scores"):
        assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(host, name)), name
    # poisoned buffers: nothing outside the outputs is written; out_pose_m3 alone and out_m8 alone are both admitted
    pad, n = 64, 12
    bp = torch.full((3 * n + 2 * pad,), -77.0, dtype=torch.float64, device=dev.poses.device)
    b8 = torch.full((8 * n + 2 * pad,), -77, dtype=torch.int32, device=dev.poses.device)
    torch.cuda.synchronize()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    p, r, g = np.ascontiguousarray(poses), np.ascontiguousarray(scans), np.ascontiguousarray(guesses)
    for po, mo in ((C.c_void_p(bp.data_ptr() + 8 * pad), None), (None, C.c_void_p(b8.data_ptr() + 4 * pad))):
        rc = eng._lib.rbpf_match_pairs(eng._h, dp(p), 20, dp(r), dp(ang), 61, ip(pairs), n, dp(g), 20.0, LO, HI, 4, 4, 2, STEP, po, mo, None,
                                       _lib.RBPF_PAIRS_DEVICE_OUT)
        assert rc == 0
    eng.synchronize()
    tp, t8 = bp.cpu().numpy(), b8.cpu().numpy()
    assert np.all(tp[:pad] == -77.0) and np.all(tp[-pad:] == -77.0) and tp[pad:-pad].tobytes() == host.poses.tobytes()
    assert np.all(t8[:pad] == -77) and np.all(t8[-pad:] == -77)
    m8 = t8[pad:-pad].reshape(n, 8)
    assert np.array_equal(m8[:, :3], host.index) and np.array_equal(m8[:, 3], host.score) and np.array_equal(m8[:, 6], host.n_ref) and not m8[:, 7].any()


# ---- 3. arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    P, NB, N, M = 3, 16, 4, 2
    e = engine(P, lattice_radius=1)
    ang = np.linspace(-2.0, 2.0, NB)
    rg = np.tile(np.linspace(1.0, 6.0, NB), (N, 1))
    poses = np.array([[0.5, 0.4, 0.3], [-1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [0.3, 0.3, 3.0]])
    pairs = np.array([[3, 0, 2], [2, 1, 2]], dtype=np.int32)
    guess = np.array([[0.4, 0.3, 2.9], [0.1, 0.0, 0.1]])
    out_p, out_8, out_s = np.full((M, 3), -7.0), np.full((M, 8), -9, np.int32), np.full((M, 3, 5, 5), -11, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(p=poses, n=N, r=rg, a=ang, nb=NB, pr=pairs, m=M, g=guess, inv=20.0, lo=0.3, hi=11.0, S=4, W=2, R=1, step=STEP, op=out_p, o8=out_8,
             sc=out_s, flags=0):
        return e._lib.rbpf_match_pairs(e._h, dp(p), n, dp(r), dp(a), nb, ip(pr), m, dp(g), inv, lo, hi, S, W, R, step, vp(op), vp(o8), vp(sc), flags)

    def with_(arr, k, val):
        out = arr.copy()
        out[k] = val
        return out
    far = 2.0 ** 30 / (20.0 * 4)                          # (|coordinate| + max_range) * invS + W reaches 2^30
    cases = dict(no_poses=dict(p=None), no_ranges=dict(r=None), no_angles=dict(a=None), no_pairs=dict(pr=None), no_outputs=dict(op=None, o8=None),
                 no_scans=dict(n=0), neg_scans=dict(n=-1), no_pairs_n=dict(m=0), neg_pairs=dict(m=-1), no_beams=dict(nb=0), many_beams=dict(nb=16385),
                 huge=dict(n=2 ** 27, nb=16), substeps_0=dict(S=0), substeps_3=dict(S=3), substeps_32=dict(S=32), window_neg=dict(W=-1),
                 window_33=dict(W=33), rot_neg=dict(R=-1), rot_101=dict(R=101), step_neg=dict(step=-0.01), step_nan=dict(step=np.nan),
                 step_inf=dict(step=np.inf), nan_pose=dict(p=with_(poses, (1, 2), np.nan)), inf_pose=dict(p=with_(poses, (2, 0), np.inf)),
                 nan_guess=dict(g=with_(guess, (1, 2), np.nan)), inf_guess=dict(g=with_(guess, (0, 1), -np.inf)),
                 nan_angle=dict(a=with_(ang, 15, np.nan)), inf_angle=dict(a=with_(ang, 5, -np.inf)), min_neg=dict(lo=-0.1), min_nan=dict(lo=np.nan),
                 max_zero=dict(hi=0.0), max_neg=dict(hi=-1.0), max_inf=dict(hi=np.inf), max_nan=dict(hi=np.nan), inv_zero=dict(inv=0.0),
                 inv_neg=dict(inv=-20.0), inv_nan=dict(inv=np.nan), inv_inf=dict(inv=np.inf), far_guess=dict(g=with_(guess, (1, 0), far)),
                 far_reference=dict(p=with_(poses, (1, 1), -far)), far_query_no_guess=dict(p=with_(poses, (3, 0), far), g=None),
                 q_high=dict(pr=with_(pairs, (0, 0), N)), q_neg=dict(pr=with_(pairs, (1, 0), -1)), r0_neg=dict(pr=with_(pairs, (0, 1), -1)),
                 run_empty=dict(pr=with_(pairs, (1, 2), 1)), run_backwards=dict(pr=with_(pairs, (0, 2), 0)), r1_high=dict(pr=with_(pairs, (0, 2), N + 1)),
                 flags=dict(flags=2), flags_high=dict(flags=1 << 31), window_limit=dict(hi=e.match_max_range(0.05, 4, 2) + 0.05))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert np.all(out_p == -7.0) and np.all(out_8 == -9) and np.all(out_s == -11), name
    # a far pose that no pair's run holds is not looked at; NaN and infinite ranges are data
    assert call(p=with_(poses, (2, 0), far), pr=with_(pairs, (1, 0), 3)) == 0
    assert call(r=with_(with_(rg, (3, 3), np.nan), (2, 0), np.inf)) == 0 and out_8[:, 5].tolist() == [NB - 1, NB - 1] and out_8[:, 6].tolist() == [2 * NB, NB]
    out_p[...], out_8[...], out_s[...] = -7.0, -9, -11
    # between the two halves of a scan update
    e.set_scan(rg[0], ang)
    e.map_update(np.zeros((P, 3)))
    e.imu_update("velocity", np.array([0.1, 0.0, 0.0]), 1000.0)
    e.set_scan(rg[1], ang)
    e.scan_update_begin(adj=False)
    assert call() == _lib.RBPF_ESTATE
    assert np.all(out_p == -7.0) and np.all(out_8 == -9) and np.all(out_s == -11)
    e.scan_update_end()
    assert call() == 0 and np.all(out_8[:, 5] == NB) and np.all(out_8[:, 7] == 0)
    # more than 4 GiB of scratch: 2^17 fields of 63 KiB
    big = 1 << 17
    assert call(pr=np.tile(pairs[:1], (big, 1)), m=big, g=None, sc=None, op=None, o8=np.zeros((big, 8), np.int32)) == _lib.RBPF_ENOMEM
    e.close()


# ---- 4. read-only ---------------------------------------------------------------------------------------------------------------------
def test_matches_interleaved_in_a_run_change_nothing():
    from thesis_amd.datasets import synthetic
    P, N, NB = 16, 6, 1081
    ang, ranges, odo, truth = synthetic.make_log(N + 1, NB)
    plain, mixed = engine(P, seed=11), engine(P, seed=11)
    for e in (plain, mixed):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))
    for k in range(N):
        for e in (plain, mixed):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            if e is mixed:
                e.match_pairs(truth[:k + 2], ranges[:k + 2], ang, [[k + 1, 0, k + 1]], window=4, rotations=2)
            e.scan_update(adj=False)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)                             # an explicit u: the duplicate groups after it are used by the next match
            if e is mixed:
                e.match_pairs(truth[:k + 2], ranges[:k + 2], ang, [[0, 1, k + 2], [k + 1, 0, 1]], substeps=2, window=3, rotations=1, return_scores=True)
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    assert np.array_equal(mixed.render_map(3, box=box).cells, plain.render_map(3, box=box).cells)
    assert mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    assert rng_state(mixed) == rng_state(plain)
    plain.close(); mixed.close()


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
class OverOracle:
    """The engine with match_pairs replaced by the oracle."""

    def __init__(self, e):
        self._e = e
        self._o = OracleEngine(float(e.cfg.cell_size), float(e.cfg.match_min_range), float(e.cfg.match_max_range))

    def __getattr__(self, name):
        return getattr(self._e, name)

    def match_pairs(self, *a, **kw):
        return self._o.match_pairs(*a, **kw)


def test_close_loops_on_a_small_loop_equals_the_run_over_the_oracle():
    from thesis_amd import loops
    from thesis_amd.datasets import mapsim, synthetic
    from thesis_amd.slam import ParticleFilter
    room = engine(1, seed=5)
    load_room(room)
    ang = synthetic.beam_angles(121)
    steps = 78                                           # a circle of 1 m radius in 63 steps of 0.1 m, and a quarter more
    truth = synthetic.circle_trajectory(steps, radius=1.0, speed=1.0) + np.array([0.33, 0.41, 0.0])
    _, ranges, odo, _ = mapsim.make_log(room, 0, truth, ang)
    room.close()
    pf = ParticleFilter(32, ang, seed=5, history="device", keep_scans=True)
    pf.map_update(ranges[0])
    for k in range(steps):
        pf.imu_update(odo[k], 1000.0)
        pf.map_update(ranges[k + 1])
        pf.resample()
    e = pf.engine
    args = dict(min_gap=40, radius=0.5, half_run=2, window=8, rotations=4, rot_step=math.radians(1.0), max_range=8.0, build_args=dict(max_range=8.0))
    got = loops.close_loops(e, pf.scans, ang, **args)
    want = loops.close_loops(OverOracle(e), pf.scans, ang, **args)
    assert got.rounds == want.rounds and got.rounds[0].pairs > 8
    for a, b in zip(got.edges, want.edges):
        assert np.array_equal(a, b)
    assert got.poses.tobytes() == want.poses.tobytes() and got.records.tolist() == pf.scans.records
    assert np.array_equal(got.built.hits, want.built.hits) and np.array_equal(got.built.seen, want.built.seen)
    print(f"closed loop: {got.rounds[0].pairs} pairs, {got.rounds[0].accepted} accepted, largest move {got.rounds[0].moved:.4f} m; "
          f"fractions {np.round(got.edges.fraction, 2).tolist()}")
    pf.close()
