"""The proposal of a scan update WITHOUT explicit guesses - the path every step of the product runs - pinned to a model.

propose_prep_kernel (Jacobi eigen-decomposition, scipy's _PSD cut-off, pseudo-inverse, log c), propose_samples_kernel
(Philox4x32-10, Box-Muller, the sampling matrix, pdf * 10, the single-precision look-up frame and its home-tile offsets)
and propose_weight_kernel (look-ups, moments) are read back through ParticleEngine.proposal (rbpf_get_proposal) and
compared with tests/proposal_oracle.py - a NumPy model anchored on the CPU by tests/test_proposal_oracle.py - and with
oracle.rbpf_oracle.  Reference: Robot.map_update robot.py:73-114.
GPU only:  python -m pytest tests -m gpu"""
import ctypes as C

import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests import proposal_oracle as po
from tests.helpers import oracle_map_from_dump

pytestmark = pytest.mark.gpu

Q = 0.1
TILE = 40
CASES = po.covariance_cases()


@pytest.fixture(scope="module")
def eng_mod():
    from thesis_amd import engine
    return engine


@pytest.fixture(scope="module")
def room_scan():
    from thesis_amd.datasets import synthetic
    ang = synthetic.beam_angles(361, np.pi)
    return synthetic.cast_scan((0, 0, 0), ang, None), ang


def _rng_stream(e):
    su, rd = C.c_uint64(), C.c_uint64()
    e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(su), C.byref(rd)))
    return su.value


def _set_global_ids(e, ids):
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    e._check(e._lib.rbpf_set_global_ids(e._h, ids.ctypes.data_as(C.POINTER(C.c_int32))))


def _match_rows(means, covs):
    return np.array([np.concatenate([m, np.asarray(c).ravel(), [100.0]]) for m, c in zip(means, covs)])


def _room_engine(eng_mod, room_scan, P, K, **kw):
    """P particles that have drawn the synthetic room once from the origin (the rng stream is then 1, not 0)."""
    r, ang = room_scan
    e = eng_mod.ParticleEngine(P, n_samples=K, max_beams=len(r), **kw)
    e.set_scan(r, ang)
    e.map_update(np.zeros((P, 3)))
    return e


def _home_offsets(mean, dim):
    """off_x, off_y of the look-up frame from the ORACLE's tile arithmetic (hybridmap.py:193-200)."""
    return tuple(dim // 2 - int(round(orc.map_centre_1d(float(v), TILE) / TILE)) * dim for v in mean[:2])


def _check_samples(pr, z_want, dim):
    """One particle's samples against the model, given the normals it should have drawn (None: explicit guesses)."""
    K = len(pr.g)
    A, U, mean = pr.A, pr.U, pr.mean
    if z_want is not None:
        z = z_want
        g_want = mean + ((A[:, 0] * z[:, 0:1] + A[:, 1] * z[:, 1:2]) + A[:, 2] * z[:, 2:3])
        tol = 4 * 2.0 ** -53 * (np.abs(mean) + np.abs(z) @ np.abs(A).T) + np.max(np.sum(np.abs(A), axis=1)) * 1e-13
        err = np.abs(pr.g - g_want)
        assert np.all(err <= tol), f"samples off by up to {np.max(err / tol):.3g} x the bound"
    # robot.py:87 with the device's own U and g, in the device's order of operations (no fused multiply-adds)
    d = pr.g - mean
    t = (d[:, 0:1] * U[0] + d[:, 1:2] * U[1]) + d[:, 2:3] * U[2]
    maha = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
    want = np.exp(pr.log_c - 0.5 * maha) * 10
    rel = np.abs(pr.motion_pr - want) / np.where(want > 0, want, 1.0)
    assert np.all(rel <= 4 * 2.0 ** -52 * (8 + abs(pr.log_c) + maha)), f"motion probability off by {rel.max():.3g}"
    assert np.all(np.abs(pr.cos - np.cos(pr.g[:, 2])) <= 2 * np.spacing(np.abs(np.cos(pr.g[:, 2]))))
    assert np.all(np.abs(pr.sin - np.sin(pr.g[:, 2])) <= 2 * np.spacing(np.abs(np.sin(pr.g[:, 2]))))
    inv_cs = float(dim) / float(TILE)
    off_x, off_y = _home_offsets(mean, dim)
    f32 = np.stack([pr.cos * inv_cs, pr.sin * inv_cs, pr.g[:, 0] * inv_cs + float(off_x), pr.g[:, 1] * inv_cs + float(off_y)], axis=1).astype(np.float32)
    assert f32.shape == (K, 4) and np.array_equal(f32.view(np.uint32), pr.frame_f32.view(np.uint32)), "single-precision look-up frame"


# ---------------------------------------------------------------------------------------------------
# the frame: eigen-decomposition, cut-off, pseudo-inverse, log c
# ---------------------------------------------------------------------------------------------------
def test_read_out_needs_a_scan_update_first(eng_mod, room_scan):
    e = _room_engine(eng_mod, room_scan, 2, 30)
    with pytest.raises(eng_mod.RbpfError) as err:
        e.proposal(0)
    assert err.value.code == -4                                         # RBPF_ESTATE
    e.scan_update(match_override=_match_rows([[0.0, 0.0, 0.0]] * 2, [CASES[0][1].cov] * 2))
    assert e.proposal(1).raw_w is None
    e.set_proposal_capture(True)                                        # turned on after the update: nothing was captured
    with pytest.raises(eng_mod.RbpfError) as err:
        e.proposal(0)
    assert err.value.code == -4
    e.close()


def test_frame_of_every_covariance(eng_mod, room_scan):
    """One particle per covariance of proposal_oracle.covariance_cases().  The read-back frame (U, A, log c) against the
    constructed eigen-system through the frame-free quantities A A^T, U U^T, log c only; rank and the bad flag exact.
    Tolerance per case: 16 x the deviation of the LAPACK route (numpy eigh, scipy's _PSD arithmetic) on the same matrix, or
    the floor 64 * 2^-53 * lam_max / lam_min,kept where that is larger.  Yardsticks measured on the CPU (dA, dU, dC; floor):
      matcher scale, correlated  3.8e-16 4.5e-15 0        1.8e-12      below the cut-off     3.9e-16 9.6e-14 6.3e-15  7.1e-12
      two equal                  3.5e-16 8.9e-16 1.5e-16  7.1e-14      rank 2                5.2e-16 9.2e-16 1.7e-16  3.6e-14
      three equal, rotated       9.4e-16 4.1e-16 0        7.1e-15      rank 1                3.0e-16 7.5e-16 0        7.1e-15
      three equal, diagonal      6.3e-18 0       0        7.1e-15      zero                  0       0       0        7.1e-15
      wide spread                2.4e-16 9.0e-09 2.2e-10  7.1e-06      tiny negative         7.4e-16 4.2e-16 1.4e-16  7.1e-14
      above the cut-off          3.5e-16 2.5e-07 5.8e-09  1.6e-05      asymmetric by an ulp  3.8e-16 4.5e-15 0        1.8e-12
    (LAPACK stays below the floor on every case - tests/test_proposal_oracle.py asserts that - so the floor decides but for two
    entries of 1.5e-14 and 1.2e-14.)  The kernel's Jacobi sweeps measured: at or below LAPACK's figures on the ill-conditioned
    cases (wide spread dU 5.3e-10, dC 1.3e-11; above the cut-off dU 7.5e-08, dC 1.7e-09), within 2 x elsewhere.
    Then the samples drawn from each frame: pdf * 10 from the device's own U and g, and for the zero matrix every sample the
    mean itself, every pdf * 10 = 10, log c = 0."""
    P, K = len(CASES), 30
    e = _room_engine(eng_mod, room_scan, P, K)
    rng = np.random.Generator(np.random.PCG64(3))
    means = rng.uniform(-0.5, 0.5, size=(P, 3)) * [1, 1, 0.2]
    stream = _rng_stream(e)
    e.scan_update(match_override=_match_rows(means, [t.cov for _, t in CASES]))
    for p, (name, truth) in enumerate(CASES):
        pr = e.proposal(p)
        assert not pr.bad, name
        assert np.array_equal(pr.mean, means[p])
        assert po.frame_rank(pr.U) == truth.rank, f"{name}: rank"
        lap = po.frame_from_cov(truth.cov)
        yard = po.frame_deviation(truth, lap.U, lap.A, lap.log_c)
        dev = po.frame_deviation(truth, pr.U, pr.A, pr.log_c)
        tol = [max(16 * y, po.frame_floor(truth)) for y in yard]
        print(f"{name:28s} dA {dev[0]:.2e} dU {dev[1]:.2e} dC {dev[2]:.2e}   tol {tol[0]:.2e} {tol[1]:.2e} {tol[2]:.2e}")
        assert all(d <= t for d, t in zip(dev, tol)), f"{name}: A A^T, U U^T, log c off by {dev}, allowed {tol}"
        _check_samples(pr, po.normals3(42, stream, np.full(K, p), np.arange(K)), e.dim)
        if truth.rank == 0:
            assert pr.log_c == 0.0 and np.all(pr.motion_pr == 10.0) and np.all(pr.g == means[p])
            assert np.all(pr.U == 0) and np.all(pr.A == 0)
    e.close()


def test_nan_and_indefinite_covariances_keep_the_state(eng_mod, room_scan):
    """A NaN covariance takes robot.py:73-78.  An indefinite one - an eigenvalue below -eps, for which the reference's scipy
    call raises - takes the same branch: flagged, nothing proposed, the pose kept, every number finite.  The
    ordinary particles between them are untouched by their neighbours: their samples are the model's."""
    P, K = 5, 30
    e = _room_engine(eng_mod, room_scan, P, K)
    start = np.array([[0.02 * p, -0.01 * p, 0.005 * p] for p in range(P)])
    e.set_state(poses=start, weights=1.0)
    good = CASES[0][1].cov
    V = po.rotation(21, True)
    indef = po.truth_from_eigen(V, [1e-3, 1e-4, -1e-4]).cov
    barely = po.truth_from_eigen(V, [1e-3, 1e-4, -1e-15]).cov          # round-off, not indefinite: dropped, rank 2
    covs = [good, np.full((3, 3), np.nan), barely, indef, good]
    means = start + [0.01, -0.02, 0.003]
    stream = _rng_stream(e)
    e.scan_update(match_override=_match_rows(means, covs))
    poses, cv, w = e.poses(), e.covs(), e.weights()
    assert np.all(np.isfinite(poses)) and np.all(np.isfinite(cv)) and np.all(np.isfinite(w))
    for p in range(P):
        pr = e.proposal(p)
        assert pr.bad == (p in (1, 3))
        if pr.bad:
            assert np.array_equal(poses[p], start[p])                   # no pose appended
        else:
            _check_samples(pr, po.normals3(42, stream, np.full(K, p), np.arange(K)), e.dim)
            assert po.frame_rank(pr.U) == (2 if p == 2 else 3)
            assert not np.array_equal(poses[p], start[p])
    # both flagged particles got the same treatment: weight += 1 + the log-odds under the scan at the kept pose
    assert w[1] > 1.0 and w[3] > 1.0
    e.close()


# ---------------------------------------------------------------------------------------------------
# the sampler: counters, Box-Muller, g = mean + A z
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [42, 2 ** 63 + 5])
@pytest.mark.parametrize("K", [1, 7, 30, 32])
def test_samples_are_the_models(eng_mod, room_scan, K, seed):
    """Three consecutive scan updates of 64 particles, each with a covariance of the list: every sample of every particle is
    mean + A_dev z with z = normals3(seed, stream, global id, k) of the model and the read-back A_dev - the frame's freedom
    (column order, signs) is the kernel's, the normals are not.  The stream is rbpf_get_rng_state before the update; the
    global ids are the default (the particle index) in the first update, then 1000 + 3 p with one id above 2^31.
      |g_dev - g_want| <= 4 * 2^-53 * (|mean| + sum |A| |z|) + |A|_inf * 1e-13
    (1e-13: r <= sqrt(2 * 53 * ln 2) = 8.57, an angle error <= 2^-50, ten-fold margin.)"""
    P = 64
    e = _room_engine(eng_mod, room_scan, P, K, seed=seed)
    rng = np.random.Generator(np.random.PCG64(K))
    covs = [CASES[p % len(CASES)][1].cov for p in range(P)]
    gid = np.arange(P, dtype=np.int64)
    streams = []
    for step in range(3):
        if step == 1:
            gid = 1000 + 3 * np.arange(P, dtype=np.int64)
            gid[17] = 2 ** 31 + 9
            _set_global_ids(e, gid.astype(np.uint32).view(np.int32))
        means = rng.uniform(-0.3, 0.3, size=(P, 3)) * [1, 1, 0.2]
        streams.append(_rng_stream(e))
        e.scan_update(match_override=_match_rows(means, covs))
        z = po.normals3(seed, streams[-1], gid[:, None], np.arange(K)[None, :])     # [P, K, 3]
        for p in range(P):
            pr = e.proposal(p)
            assert not pr.bad and np.array_equal(pr.mean, means[p])
            _check_samples(pr, z[p], e.dim)
    assert streams == [1, 2, 3]                                          # (the room was drawn once before)
    e.close()


# ---------------------------------------------------------------------------------------------------
# the home tile of the look-up frame: propose_samples_kernel's offsets against weight_beams' home_tile()
# ---------------------------------------------------------------------------------------------------
def _seam_poses(cs):
    h = cs / 2
    out = [("tile (-1, 0)", (-36.7, 2.1), []), ("tile (1, -1)", (37.3, -34.5), [])]
    for s in (-h, h):
        out.append((f"x seam {s:+.4f}", (20 + s, 1.3), [(0, 0), (40, 0)]))
        out.append((f"-x seam {s:+.4f}", (-20 + s, -2.2), [(0, 0), (-40, 0)]))
        out.append((f"y seam {s:+.4f}", (1.7, 20 + s), [(0, 0), (0, 40)]))
        for s2 in (-h, h):
            out.append((f"corner {s:+.4f} {s2:+.4f}", (20 + s, 20 + s2), [(0, 0), (40, 0), (0, 40), (40, 40)]))
    return out


@pytest.mark.parametrize("cs", [0.05, 0.025])
def test_raw_weights_with_the_matcher_pose_off_the_origin_tile(eng_mod, room_scan, cs):
    """The matcher pose in tiles (-1, 0) and (1, -1), and half a cell on either side of a tile seam on x (both signs), on y and
    at a corner; dim 800 and 1600; each pose once with the tiles behind the seam present and once with the home tile alone.
    The captured raw weights w_k against orc.generate_sample_weight on the oracle's copy of the map, with the read-back
    samples and motion probabilities, at the relative 1e-12 of tests/test_gpu_weighting.py: the sums are integers, a look-up
    frame shifted by a tile is a gross mismatch.  That file's measure |w - want| / max(1, |want|) is written for motion
    probabilities of 0.5 .. 2; here they are pdf * 10 = 1e5, and where 1 + sum comes out as 0 in quanta the oracle's float64
    multiples of 0.1 leave 1e-15 * 1e5 (1.0e-11 measured at dim 1600).  So the probability is taken out of the measure:
    |w - obs * pr| <= 1e-12 * max(1, |obs|) * pr with obs = 1 + the oracle's sum - the same 1e-12 at any scale of pr.
    The frame itself is compared bit for bit with the oracle's tile arithmetic."""
    r, ang = room_scan
    sx, sy = orc.scan_xy(r, ang)
    poses = _seam_poses(cs)
    P, K = 2 * len(poses), 30
    dim = int(round(TILE / cs))
    e = eng_mod.ParticleEngine(P, n_samples=K, max_beams=len(r), cell_size=cs, pool_tiles=P * 5 + 2)
    assert e.dim == dim
    rng = np.random.Generator(np.random.PCG64(dim))
    centres = [(0, 0), (40, 0), (-40, 0), (0, 40), (40, 40), (40, -40)]
    cells = {c: rng.integers(-30, 31, size=(dim, dim)).astype(np.int8) for c in centres}
    dump = {"m_centres": np.array(centres, dtype=np.float64), "m_offs": [0], "m_xs": [], "m_ys": [], "m_vals": []}
    for c in centres:                                                    # a golden-style dump of the full set, for the oracle
        xs, ys = np.nonzero(cells[c])
        dump["m_xs"].append(xs); dump["m_ys"].append(ys); dump["m_vals"].append(cells[c][xs, ys] * Q)
        dump["m_offs"].append(dump["m_offs"][-1] + len(xs))
    for k in ("m_xs", "m_ys", "m_vals"):
        dump[k] = np.concatenate(dump[k])
    full = oracle_map_from_dump(dump, "m_", cs)
    by_centre = {(float(t.cx), float(t.cy)): t for t in full.tiles}
    means, tiles_of = [], []
    for p in range(P):
        name, xy, behind = poses[p // 2]
        home = tuple(orc.map_centre_1d(v, TILE) for v in xy)
        mine = {home} | (set(behind) if p % 2 == 0 else set())
        for c in sorted(mine):
            e.set_tile(p, c, cells[c])
        means.append([xy[0], xy[1], rng.uniform(-np.pi, np.pi)])
        tiles_of.append(mine)
    assert sorted(c for c, _ in e.tiles(0)) == sorted((float(a), float(b)) for a, b in tiles_of[0] | {(0, 0)})
    e.set_scan(r, ang)
    e.set_state(poses=np.array(means))
    e.set_proposal_capture(True)
    stream = _rng_stream(e)
    e.scan_update_begin(match_override=_match_rows(means, [CASES[0][1].cov] * P))
    worst = 0.0
    for p in range(P):
        pr = e.proposal(p)
        assert not pr.bad
        _check_samples(pr, po.normals3(42, stream, np.full(K, p), np.arange(K)), dim)
        hm = orc.OracleHybridMap(cs)
        hm.tiles = [by_centre[(float(a), float(b))] for a, b in sorted(tiles_of[p])]
        obs = np.asarray(orc.generate_sample_weight(hm, pr.g, sx, sy, np.ones(K)), dtype=np.float64)   # 1 + the sum of log-odds
        err = float(np.max(np.abs(pr.raw_w - obs * pr.motion_pr) / (np.maximum(1.0, np.abs(obs)) * pr.motion_pr)))
        assert err < 1e-12, f"{poses[p // 2][0]} ({'tiles behind' if p % 2 == 0 else 'home only'}): raw weights off by {err:.3g}"
        worst = max(worst, err)
    print(f"dim {dim}: worst raw-weight deviation {worst:.3g}")
    e.close()


# ---------------------------------------------------------------------------------------------------
# moments on the device-sampled path (robot.py:89-114)
# ---------------------------------------------------------------------------------------------------
def _check_moments(e, p, pr, w_before):
    """Pose, covariance and weight increment of particle p from the read-back samples and captured raw weights: the
    longdouble oracle at the project's tolerances, the float64 sequential model at 8 x ITS deviation from the oracle."""
    pose, cov, w = e.poses()[p], e.covs()[p], e.weights()[p]
    m_ld, s_ld, t_ld = orc.proposal_moments(pr.g, pr.raw_w.astype(np.longdouble))
    m_ld, s_ld, t_ld = np.asarray(m_ld, dtype=np.float64), np.asarray(s_ld, dtype=np.float64), float(t_ld)
    np.testing.assert_allclose(pose, m_ld, rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(cov, s_ld, rtol=1e-5, atol=1e-14)
    np.testing.assert_allclose(w, t_ld + w_before, rtol=1e-9)
    m, s, t = po.sequential_moments(pr.g, pr.raw_w)
    own = (np.max(np.abs(m - m_ld)), np.max(np.abs(s - s_ld)), abs((t + w_before) - (t_ld + w_before)))
    dev = (np.max(np.abs(pose - m)), np.max(np.abs(cov - s)), abs(w - (t + w_before)))
    print(f"particle {p}: float64 model vs longdouble {own[0]:.2e} {own[1]:.2e} {own[2]:.2e}   device vs float64 model {dev[0]:.2e} {dev[1]:.2e} {dev[2]:.2e}")
    assert all(d <= 8 * o for d, o in zip(dev, own)), f"device vs sequential float64 model {dev}, model vs longdouble {own}"


@pytest.mark.parametrize("K", [1, 30])
def test_moments_of_device_drawn_samples(eng_mod, room_scan, K):
    """Six particles, the first six covariances of the list.  Measured on the MI355X, absolute (pose, covariance, weight):
    the float64 model deviates from the longdouble oracle by up to 1.1e-16, 1.7e-18 and one ulp of the weight (9.8e-4 on
    1e13, where log c is large); the device reproduces the float64 model bit for bit (0, 0, 0) for K = 30 and K = 1.
    K = 1: the shifted weight and the norm are exactly 1e-2, the weight increment w_0 + 1e-2.  The covariance is 0 in exact
    arithmetic; the reference's own operations give d_i d_j with d = g - (g * 1e-2) / 1e-2, two roundings of g: at most
    2^-104 |g_i g_j| (7.7e-34 measured), which is what is asserted beside the bit-equality with the model."""
    P = 6
    e = _room_engine(eng_mod, room_scan, P, K)
    e.set_proposal_capture(True)
    rng = np.random.Generator(np.random.PCG64(40 + K))
    means = rng.uniform(-0.2, 0.2, size=(P, 3)) * [1, 1, 0.2]
    e.set_state(weights=np.arange(1.0, P + 1.0))
    e.scan_update(match_override=_match_rows(means, [CASES[p][1].cov for p in range(P)]))
    for p in range(P):
        pr = e.proposal(p)
        assert pr.raw_w is not None and np.all(np.isfinite(pr.raw_w))
        _check_moments(e, p, pr, float(p + 1))
        if K == 1:
            assert np.all(np.abs(e.covs()[p]) <= 2.0 ** -104 * np.outer(np.abs(pr.g[0]), np.abs(pr.g[0])))
            np.testing.assert_allclose(e.weights()[p] - (p + 1), pr.raw_w[0] + 1e-2, rtol=1e-12)
    e.close()


def test_moments_when_every_pdf_is_zero(eng_mod, room_scan):
    """Explicit guesses a metre off a 1e-5 covariance: every pdf is exactly 0, every raw weight 0, the shifted weights all
    1e-2 - the pose is the plain mean of the guesses and the weight increment 30 * 1e-2."""
    P, K = 2, 30
    e = _room_engine(eng_mod, room_scan, P, K)
    e.set_proposal_capture(True)
    rng = np.random.Generator(np.random.PCG64(50))
    g = np.array([1.0, -1.0, 0.1]) + rng.normal(0, [0.05, 0.05, 0.01], size=(P, K, 3))
    e.scan_update(match_override=_match_rows(np.zeros((P, 3)), [np.diag([1e-5, 1e-5, 1e-6])] * P), guesses=g)
    for p in range(P):
        pr = e.proposal(p)
        assert np.array_equal(pr.g, g[p]) and np.all(pr.motion_pr == 0.0) and np.all(pr.raw_w == 0.0)
        _check_samples(pr, None, e.dim)
        _check_moments(e, p, pr, 1.0)
        np.testing.assert_allclose(e.weights()[p], 1.0 + K * 1e-2, rtol=1e-14)
    e.close()


# ---------------------------------------------------------------------------------------------------
# the read-out is an observer
# ---------------------------------------------------------------------------------------------------
def test_capture_changes_nothing(eng_mod):
    """Two engines run the same three steps of the whole pipeline (built-in matcher, device-drawn proposal, map update,
    resample), one with capture on: poses, covariances, weights, counters, rng state and a rendered map are equal."""
    from thesis_amd.datasets import synthetic
    P, B = 32, 361
    ang = synthetic.beam_angles(B, np.pi)
    truth = [(0.0, 0.0, 0.0), (0.05, 0.01, 0.01), (0.1, 0.02, 0.02), (0.15, 0.03, 0.03)]
    scans = [synthetic.cast_scan(t, ang, np.random.Generator(np.random.PCG64(60 + i))) for i, t in enumerate(truth)]
    out = []
    for capture in (False, True):
        e = eng_mod.ParticleEngine(P, max_beams=B)
        e.set_proposal_capture(capture)
        e.set_scan(scans[0], ang)
        e.map_update(np.zeros((P, 3)))
        for i in range(1, 4):
            e.imu_update("velocity", [0.5, 0.1, 0.1], 1000.0)
            e.set_scan(scans[i], ang)
            e.scan_update()
            e.resample(0.37)
        if capture:
            assert e.proposal(3).raw_w is not None
        su, rd = C.c_uint64(), C.c_uint64()
        e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(su), C.byref(rd)))
        ctr = {k: v for k, v in e.counters().items() if not k.startswith("ms_")}
        out.append((e.poses(), e.covs(), e.weights(), ctr, (su.value, rd.value), e.render_map(particle=5).cells))
        e.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and a[4] == b[4] == (4, a[4][1])
    assert np.array_equal(a[5], b[5]) and a[5].size > 0
