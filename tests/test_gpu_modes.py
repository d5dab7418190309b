"""Pose modes on the GPU (rbpf_pose_modes, rbpf_track_modes, kernels_modes.hip) against the model of
tests/modes_oracle.py: info, labels, the int rows, Q and the share exactly, the estimate slots within track_oracle.est_tolerance of
the members.  Shapes: the smallest at which each phase of the kernel can go wrong.

est_tolerance bounds the error of the sums.  For a set whose contributing particles share one heading theta it is 0 for c_thth, while
the device's mean heading atan2(w sin theta, w cos theta) may miss theta by an ulp; tests/test_gpu_track.py meets the same corner
only at P = 1.  The hand-made clouds here stay out of it by construction: a mode that gets a row holds two different headings, or
stands at heading 0, where sin, cos and atan2 are exact in every libm."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import modes_oracle as M
from tests import track_oracle as T
from tests.test_gpu_cast import engine, load_room16, rng_state
from tests.test_gpu_track import forcing_weights, host, same_bits, state_engine
from tests.test_modes_oracle import random_cloud

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -4, -1
TWO_PI = T.TWO_PI
vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def raw_modes(e, mode, given, bin_xy, n_th, K, rows=True, label=True):
    """rbpf_pose_modes with host outputs: (info [4], rows_f [K, 16], rows_i [K, 4], label [P])."""
    info, f, i = np.full(4, -7, dtype=np.int64), np.full((K, 16), -7.0), np.full((K, 4), -7, dtype=np.int32)
    lab = np.full(e.P, -7, dtype=np.int32)
    g = None if given is None else np.ascontiguousarray(given, dtype=np.float64)
    rc = e._lib.rbpf_pose_modes(e._h, mode, dp(g), float(bin_xy), n_th, K, 0, vp(info), vp(f) if rows else None, vp(i) if rows else None,
                                vp(lab) if label else None)
    assert rc == 0, e._lib.rbpf_last_error(e._h)
    return info, f, i, lab


def assert_modes(got, want, poses, raw, mode, given, what):
    """got = (info, f, i, label) of the device, want = modes_oracle.pose_modes(...)."""
    info, f, i, lab = got
    w_info, w_f, w_i, w_lab, members = want
    assert info.tolist() == w_info, (what, info.tolist(), w_info)
    assert np.array_equal(lab, w_lab), what
    assert np.array_equal(i, w_i), (what, i.tolist(), w_i.tolist())
    assert np.array_equal(f[:, 12:], w_f[:, 12:]), (what, f[:, 12:14], w_f[:, 12:14])       # Q, share, 0, 0: exact
    assert np.array_equal(np.isnan(f), np.isnan(w_f)), what
    worst = 0.0
    for k, mem in enumerate(members):
        tol = M.row_tolerance(poses, raw, mode, given, mem)
        err = np.abs(f[k, :12] - w_f[k, :12])
        err[2] = abs(T.wrap(f[k, 2] - w_f[k, 2]))
        worst = max([worst] + [err[c] / tol[c] for c in range(12) if tol[c] > 0])
        assert (err <= tol).all(), (what, k, np.nonzero(err > tol)[0].tolist(), err, tol)
    print(f"{what}: largest |device - fsum| / bound = {worst:.3g}")


def check(e, poses, raw, mode, given, bin_xy, n_th, K, what):
    e.set_state(poses=poses, weights=raw)
    got = raw_modes(e, mode, given, bin_xy, n_th, K)
    want = M.pose_modes(poses, raw, mode, given, bin_xy, n_th, K)
    assert_modes(got, want, poses, raw, mode, given, what)
    return got, want


# ---- 1. population sizes, all three weight modes --------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 513, 1000, 4097])
def test_random_clouds_equal_the_model(P):
    rng = np.random.default_rng(31 * P)
    e = state_engine(P)
    poses = random_cloud(rng, P)
    raw = rng.uniform(-30.0, 30.0, size=P)
    if P >= 63:
        raw[[3, 17]], raw[[5, 40]] = -np.inf, 0.0
    given = rng.uniform(0.0, 2.0, size=P)
    given[0] = 0.0 if P > 1 else 1.0
    for mode, g in ((T.W_RESAMPLE, None), (T.W_UNIFORM, None), (T.W_GIVEN, given)):
        got, want = check(e, poses, raw, mode, g, 0.5, 36, 8, f"cloud P={P} mode={mode}")
        again = raw_modes(e, mode, g, 0.5, 36, 8)
        assert all(same_bits(a, b) for a, b in zip(got, again))                         # identical bits from call to call
        only_info = raw_modes(e, mode, g, 0.5, 36, 8, rows=False, label=False)
        assert same_bits(only_info[0], got[0]) and (only_info[1] == -7).all() and (only_info[3] == -7).all()
    if P >= 513:
        assert want[0][0] > 8                                                               # more modes than rows
    e.close()


# ---- 2. who contributes ------------------------------------------------------------------------------------------------------------
def test_non_contributing_particles():
    P = 12
    e = state_engine(P)
    poses = np.tile([0.2, 0.3, 0.0], (P, 1))
    raw = np.ones(P)
    poses[1, 0], poses[2, 1], poses[3, 2] = np.nan, np.inf, -np.inf
    raw[4], raw[5] = 0.0, -np.inf
    poses[6, 0] = 2.0 ** 23 * 0.5                              # |x inv| = 2^23
    poses[7, 1] = -(2.0 ** 23) * 0.5
    poses[8, 2] = 2.0 ** 40 / (36 / TWO_PI) * 1.001            # |theta kth| >= 2^40
    poses[9, 0] = (2.0 ** 23 - 1) * 0.5                        # the last bin that counts: a mode of its own
    (info, f, i, lab), _ = check(e, poses, raw, T.W_RESAMPLE, None, 0.5, 36, 4, "non-contributing")
    assert lab.tolist() == [0, -1, -1, -1, -1, -1, -1, -1, -1, 9, 0, 0] and info.tolist()[:3] == [2, 2, 4]
    e.close()
    e = state_engine(3)
    (info, f, i, lab), _ = check(e, [[1, 1, 1], [np.nan, 0, 0], [2, 2, 0]], [0.0, 1.0, 5.0], T.W_RESAMPLE, None, 0.5, 36, 2, "P=3, one contributes")
    assert info.tolist() == [1, 1, 1, 1 << 32] and lab.tolist() == [-1, -1, 2] and i.tolist() == [[2, 1, 1, 2], [-1, 0, 0, -1]]
    e.close()
    e = state_engine(4)
    (info, f, i, lab), _ = check(e, np.zeros((4, 3)), np.full(4, -np.inf), T.W_RESAMPLE, None, 0.5, 36, 3, "P=4, none contributes")
    assert info.tolist() == [0, 0, 0, 0] and (lab == -1).all() and i.tolist() == [[-1, 0, 0, -1]] * 3
    assert np.isnan(f[:, :12]).all() and (f[:, 12:] == 0).all()
    e.close()


# ---- 3. bins and adjacency by hand --------------------------------------------------------------------------------------------------
def labels_of(e, poses, bin_xy=1.0, n_th=36):
    P, n = e.P, len(poses)
    full = np.full((P, 3), np.nan)                             # the particles the case does not use contribute nothing
    full[:n] = poses
    full[n:2 * n] = np.asarray(poses) + [0.0, 0.0, 1e-3]       # a twin in the same bin: no mode of one heading alone (see the module's docstring)
    (info, f, i, lab), _ = check(e, full, np.ones(P), T.W_UNIFORM, None, bin_xy, n_th, 4, f"hand case {np.asarray(poses).tolist()}")
    assert lab[n:2 * n].tolist() == lab[:n].tolist()
    return lab[:n].tolist()


def test_floor_diagonals_and_headings():
    e = state_engine(256)                                      # six particles of the set contribute: the bound is the set's, 4 P 2^-53
    step = TWO_PI / 36
    assert labels_of(e, [[-0.01, 0.5, 0.1], [0.01, 0.5, 0.1], [2.01, 0.5, 0.1]]) == [0, 0, 2]      # floor, not truncation
    assert labels_of(e, [[0.5, 0.5, 0.5 * step], [1.5, -0.5, 1.5 * step]]) == [0, 0]               # (1, -1, 1) joins
    assert labels_of(e, [[0.5, 0.5, 0.5 * step], [2.5, 0.5, 0.5 * step]]) == [0, 1]                # (2, 0, 0) does not
    assert labels_of(e, [[0.5, 0.5, 0.5 * step], [0.5, 0.5, 2.5 * step]]) == [0, 1]                # (0, 0, 2) does not
    assert labels_of(e, [[0.5, 0.5, math.pi - 0.01], [0.5, 0.5, -math.pi + 0.01]]) == [0, 0]       # across the seam
    # theta = 7.0 and -9.0 land in the bins of the formula: next to 4 and 20, apart from their second neighbours
    kth = 36 / TWO_PI
    assert [math.floor(7.0 * kth) % 36, math.floor(-9.0 * kth) % 36] == [4, 20]
    assert labels_of(e, [[0.5, 0.5, 7.0], [0.5, 0.5, 5.5 * step], [0.5, 0.5, 7.5 * step]]) == [0, 0, 2]
    assert labels_of(e, [[0.5, 0.5, -9.0], [0.5, 0.5, 19.5 * step], [0.5, 0.5, 22.5 * step]]) == [0, 0, 2]
    for n_th in (1, 2, 3):
        assert labels_of(e, [[0.5, 0.5, 0.1], [0.5, 0.5, 3.0], [0.5, 0.5, -2.0]], n_th=n_th) == [0, 0, 0]
    assert labels_of(e, [[0.5, 0.5, 0.1], [0.5, 0.5, 1.7]], n_th=4) == [0, 0]
    assert labels_of(e, [[0.5, 0.5, 0.1], [0.5, 0.5, 3.2]], n_th=4) == [0, 1]                       # opposite bins stay apart
    e.close()


# ---- 4. a long thin component ---------------------------------------------------------------------------------------------------------
def test_snake_and_ring_are_one_mode():
    P = 600
    rng = np.random.default_rng(5)
    order = np.concatenate([1 + rng.permutation(P - 1), [0]])   # order[k]: the particle in bin k; particle 0 sits at the far end
    e = state_engine(P)
    k = np.arange(P)
    snake = np.zeros((P, 3))
    snake[order] = np.stack([k + 0.5, (k // 3) % 2 + 0.5, np.zeros(P)], axis=1)
    (info, f, i, lab), _ = check(e, snake, np.ones(P), T.W_UNIFORM, None, 1.0, 36, 2, "snake")
    assert info.tolist() == [1, P, P, P << 32] and (lab == 0).all() and i[0].tolist() == [0, P, P, 0]
    ring = np.zeros((P, 3))
    ring[order] = np.stack([np.full(P, 0.5), np.full(P, 0.5), (k + 0.5) * (TWO_PI / P) - math.pi], axis=1)
    lean = 1.0 + np.cos(ring[:, 2])                            # weights that give the ring a mean heading: uniform ones leave it to rounding
    (info, f, i, lab), _ = check(e, ring, np.ones(P), T.W_GIVEN, lean, 1.0, P, 2, "ring")
    assert info.tolist()[:3] == [1, P, P] and (lab == 0).all() and i[0].tolist() == [0, P, P, 0]
    open_ring = ring.copy()
    open_ring[order[[100, 400]], 0] = 9.5                      # two bins moved away: two arcs, one of them across the seam, and two lone bins
    (info, f, i, lab), _ = check(e, open_ring, np.ones(P), T.W_GIVEN, lean, 1.0, P, 2, "cut ring")
    assert info.tolist()[:3] == [4, P, P] and sorted(i[:, 1].tolist()) == [299, 299] and 0 in i[:, 3].tolist()
    e.close()


# ---- 5. the bin table ---------------------------------------------------------------------------------------------------------------
def test_table_stress():
    P = 4097
    e = state_engine(P)
    rng = np.random.default_rng(9)
    one_bin = np.tile([0.1, 0.1, 0.01], (P, 1)) + rng.uniform(0, 0.05, size=(P, 3)) * [1, 1, 0.1]
    (info, f, i, lab), _ = check(e, one_bin, np.ones(P), T.W_UNIFORM, None, 0.5, 36, 2, "one bin")
    assert info.tolist() == [1, 1, P, P << 32] and f[0, 13] == 1.0
    a = rng.permutation(P)
    apart = np.stack([2.0 * (a % 65) + 0.5, 2.0 * (a // 65) + 0.5, np.zeros(P)], axis=1)
    raw = rng.uniform(1.0, 2.0, size=P)                        # distinct Q: the order is the weights'
    for K in (1, 64):
        (info, f, i, lab), _ = check(e, apart, raw, T.W_RESAMPLE, None, 1.0, 36, K, f"all apart K={K}")
        assert info.tolist()[:3] == [P, P, P] and np.array_equal(lab, np.arange(P))
        assert i[:, 3].tolist() == np.argsort(-raw, kind="stable")[:K].tolist()
    e.close()
    P = 300
    e = state_engine(P)
    j = np.arange(P)                                           # keys that differ in `it` alone: every second heading bin, two particles each
    only_it = np.stack([np.full(P, 0.5), np.full(P, 0.5), (2 * (j // 2) + 0.3 + 0.4 * (j % 2)) * (TWO_PI / 4096)], axis=1)
    (info, f, i, lab), _ = check(e, only_it, np.ones(P), T.W_UNIFORM, None, 1.0, 4096, 64, "heading bins only")
    assert info.tolist()[:3] == [P // 2, P // 2, P] and i[:, 3].tolist() == list(range(0, 128, 2))
    e.close()


# ---- 6. the order ----------------------------------------------------------------------------------------------------------------------
def test_order_is_exact():
    P = 9
    e = state_engine(P)
    poses = np.array([[5.1, 5.1, 1.0]] * 4 + [[0.1, 0.1, 0.0]] * 4 + [[9.1, 9.1, 2.0]])
    poses += np.linspace(0, 0.02, P)[:, None]
    poses[8, 2] = 0.0
    (info, f, i, lab), _ = check(e, poses, np.ones(P), T.W_UNIFORM, None, 0.5, 36, 3, "equal counts")
    assert i[:, 3].tolist() == [0, 4, 8] and f[:, 12].tolist() == [4.0 * 2 ** 32, 4.0 * 2 ** 32, 2.0 ** 32]   # the tie falls to the root
    given = np.array([1.0] * 4 + [1.5] * 4 + [2.0 ** -40])
    (info, f, i, lab), _ = check(e, poses, np.ones(P), T.W_GIVEN, given, 0.5, 36, 3, "flipped by weights")
    assert i[:, 3].tolist() == [4, 0, 8]
    assert i[2].tolist() == [8, 1, 1, 8] and f[2, 12] == 0.0 and f[2, 13] == 0.0 and f[2, 0] == poses[8, 0]   # w / wmax < 2^-32: a member with q = 0
    e.close()


# ---- 7. what the feature is for --------------------------------------------------------------------------------------------------------
def test_two_hypotheses_are_told_apart():
    from thesis_amd import locate
    P = 200
    rng = np.random.default_rng(2)
    e = state_engine(P)
    poses = np.concatenate([[-10.0, 0.0, 0.0] + rng.normal(scale=[0.1, 0.1, 0.02], size=(120, 3)),
                            [10.0, 0.0, math.pi] + rng.normal(scale=[0.1, 0.1, 0.02], size=(80, 3))])
    poses = poses[rng.permutation(P)]
    left = poses[:, 0] < 0
    raw = rng.uniform(1.0, 2.0, size=P)
    e.set_state(poses=poses, weights=raw)
    est = e.estimate()
    assert np.min(np.hypot(*(poses[:, :2] - est.pose[:2]).T)) > 5.0            # the mean is a pose where no particle stands
    m = e.pose_modes(labels=True)
    assert (m.count, m.bins > 2, m.used) == (2, True, P) and m.size.tolist() == [120, 80]
    assert np.array_equal(m.labels == m.root[0], left) and abs(m.share.sum() - 1.0) < 1e-15
    for k, side in enumerate((left, ~left)):
        alone = e.estimate(np.where(side, raw, 0.0))           # estimate() over the blob alone: the same sums, the same bits
        got = m.estimate(k)
        assert same_bits(got.pose, alone.pose) and same_bits(got.cov, alone.cov) and got.n_used == alone.n_used
        assert (got.resultant, got.n_eff, got.weight_sum) == (alone.resultant, alone.n_eff, alone.weight_sum)
        assert got.best == int(np.nonzero(side)[0][np.argmax(raw[side])])
    assert not locate.converged(m) and locate.kld_size(m.bins) > locate.kld_size(1) == 1
    e.set_state(weights=np.where(left, raw, -np.inf))
    m = e.pose_modes()
    assert m.count == 1 and m.size.tolist() == [120] and m.share.tolist() == [1.0] and locate.converged(m) and m.labels is None
    e.close()


def test_relocalize_seeding_gives_one_mode_a_hypothesis():
    from thesis_amd import locate
    from thesis_amd.slam import ParticleFilter
    P = 64
    hyp = locate.Hypotheses(poses=np.array([[1.05, 2.05, 0.5], [-7.95, 3.05, 2.0], [4.05, -6.95, 4.0]]), scores=np.array([50, 30, 20]),
                            cells=np.zeros((3, 3), dtype=np.int64), n_used=None)
    e = state_engine(P)
    e.set_state(poses=locate.seed_particles(hyp, P, 0.1, 720, seed=4), weights=1.0)
    m = e.pose_modes(weights="uniform")
    sizes = locate.allot(hyp.scores, P)
    assert m.count == 3 and m.size.tolist() == sizes.tolist() == sorted(sizes.tolist(), reverse=True)
    assert np.abs(m.poses[:, :2] - hyp.poses[:, :2]).max() < 0.05 and m.root.tolist() == [0, int(sizes[0]), int(sizes[0] + sizes[1])]
    assert not locate.converged(m)
    e.close()
    pf = ParticleFilter(4, np.linspace(-1.0, 1.0, 16))
    assert pf.pose_modes(bin_xy=1.0, max_modes=2).count == 1    # ParticleFilter passes through to its engine
    pf.close()


# ---- 8. the smoothed form ---------------------------------------------------------------------------------------------------------------
def track_modes_raw(e, t0, t1, mode, given, bin_xy, n_th, K, outs=(True, True, True)):
    n = t1 - t0
    info, f, i = np.full((n, 4), -7, dtype=np.int64), np.full((n, K, 16), -7.0), np.full((n, K, 4), -7, dtype=np.int32)
    g = None if given is None else np.ascontiguousarray(given, dtype=np.float64)
    rc = e._lib.rbpf_track_modes(e._h, t0, t1, mode, dp(g), float(bin_xy), n_th, K, *(vp(a) if on else None for a, on in zip((info, f, i), outs)))
    assert rc == 0, e._lib.rbpf_last_error(e._h)
    return info, f, i


def drive_log(e, rng, n_records, resamples, headings):
    """The pattern of test_gpu_track.drive: track(), then n_records - 1 records of a random walk with resamples(t) resamples
    (forced or suppressed) in front of record t.  headings = 0 keeps every heading at 0: behind a resample the particles of a mode
    may all continue one ancestor, one heading (the module's docstring)."""
    P, spread = e.P, float(e.cfg.resample_spread)
    scale = np.array([1.0, 1.0, headings])
    poses, w = rng.normal(scale=3.0, size=(P, 3)) * scale, np.ones(P)
    e.set_state(poses=poses, weights=w)
    e.track(n_records)
    m = T.TrackModel(poses, w)
    for t in range(1, n_records):
        for _ in range(resamples(t)):
            forced = rng.random() < 0.7
            w = forcing_weights(rng, P, spread) if forced else np.full(P, float(rng.uniform(-5, 5)))
            e.set_state(weights=w)
            did, idx = e.resample(float(rng.random()))
            assert did == forced
            if did:
                m.resample(idx)
                poses, w = poses[idx], np.ones(P)
        poses = poses + rng.normal(scale=0.1, size=(P, 3)) * scale
        e.set_state(poses=poses)
        e.record()
        m.record(poses, w)
    return m


@pytest.mark.parametrize("P", [65, 300])
def test_trajectory_modes_gather_the_headings_through_the_lineage(P):
    N, K = 70, 2
    rng = np.random.default_rng(13 * P)
    e = state_engine(P)
    m = drive_log(e, rng, N, lambda t: int(t in (N - 40, N - 10)), headings=1.0)
    raw = rng.uniform(-5.0, 30.0, size=P)
    e.set_state(weights=raw)
    idx, lin_pose = m.lineage()
    assert 1 < len(np.unique(idx[0])) < P                      # lineages merged, and more than one is left: one wide bin holds them all
    info, f, i = track_modes_raw(e, 0, N, T.W_RESAMPLE, None, 1000.0, 1, K)
    for t in range(N):
        want = M.pose_modes(lin_pose[t], raw, T.W_RESAMPLE, None, 1000.0, 1, K)
        assert_modes((info[t], f[t], i[t], want[3]), want, lin_pose[t], raw, T.W_RESAMPLE, None, f"record {t} P={P}")
    assert info[:, 0].tolist() == [1] * N
    e.close()


@pytest.mark.parametrize("P", [2, 65, 300])
def test_trajectory_modes_equal_the_model_on_the_lineage_poses(P):
    N, K = 3 * 64 + 5, 4
    rng = np.random.default_rng(11 * P)
    e = state_engine(P)
    m = drive_log(e, rng, N, lambda t: t % 3, headings=0.0)   # none, one, two
    raw = rng.uniform(-5.0, 30.0, size=P)
    e.set_state(weights=raw)
    lin_pose = m.lineage()[1]
    want = [M.pose_modes(lin_pose[t], raw, T.W_RESAMPLE, None, 1.0, 8, K) for t in range(N)]
    info, f, i = track_modes_raw(e, 0, N, T.W_RESAMPLE, None, 1.0, 8, K)
    for t in range(N):
        assert_modes((info[t], f[t], i[t], want[t][3]), want[t], lin_pose[t], raw, T.W_RESAMPLE, None, f"record {t} P={P}")
    tm = e.trajectory_modes(bin_xy=1.0, heading_bins=8, max_modes=K)
    assert tm.count.tolist() == [w[0][0] for w in want] and same_bits(tm.share, f[:, :, 13]) and same_bits(tm.poses, f[:, :, 0:3])
    assert same_bits(tm.size, i[:, :, 1])
    for t0, t1 in ((0, 1), (N - 1, N), (N // 3, 2 * N // 3 + 1), (70, N), (N - 70, N - 3), (5, 60)):      # start and end inside a chunk
        sub = track_modes_raw(e, t0, t1, T.W_RESAMPLE, None, 1.0, 8, K)
        assert same_bits(sub[0], info[t0:t1]) and same_bits(sub[1], f[t0:t1]) and same_bits(sub[2], i[t0:t1]), (t0, t1)
    for budget in (1, 160000):                                 # one record a slab; 29 at P = 65 and 7 at P = 300, the last slab ragged
        os.environ["RBPF_MODES_SLAB_BYTES"] = str(budget)
        try:
            slabbed = track_modes_raw(e, 2, N - 1, T.W_RESAMPLE, None, 1.0, 8, K)
        finally:
            del os.environ["RBPF_MODES_SLAB_BYTES"]
        assert same_bits(slabbed[0], info[2:N - 1]) and same_bits(slabbed[1], f[2:N - 1]) and same_bits(slabbed[2], i[2:N - 1]), budget
    part = track_modes_raw(e, 3, 9, T.W_RESAMPLE, None, 1.0, 8, K, outs=(True, False, False))          # any output may be left out
    assert same_bits(part[0], info[3:9]) and (part[1] == -7.0).all() and (part[2] == -7).all()
    given = rng.uniform(0.0, 2.0, size=P)
    for mode, g in ((T.W_UNIFORM, None), (T.W_GIVEN, given)):
        got = track_modes_raw(e, 60, 70, mode, g, 1.0, 8, K)
        for t in range(60, 70):
            w = M.pose_modes(lin_pose[t], raw, mode, g, 1.0, 8, K)
            assert_modes((got[0][t - 60], got[1][t - 60], got[2][t - 60], w[3]), w, lin_pose[t], raw, mode, g, f"record {t} P={P} mode={mode}")
    e.close()


def test_one_mode_from_the_coalescence_record_back():
    P = 65
    rng = np.random.default_rng(8)
    e = state_engine(P)
    poses = rng.normal(scale=3.0, size=(P, 3))
    e.set_state(poses=poses, weights=1.0)
    e.track(70)
    for _ in range(2):
        poses = poses + rng.normal(scale=0.5, size=(P, 3))
        e.set_state(poses=poses)
        e.record()
    one = np.zeros(P)
    one[P // 2] = 1000.0                                       # every particle continues particle P // 2 from record 2 back
    e.set_state(weights=one)
    did, idx = e.resample(0.37)
    assert did
    poses = poses[idx]
    for _ in range(66):                                        # across a chunk border
        poses = poses + rng.normal(scale=0.5, size=(P, 3))
        e.set_state(poses=poses)
        e.record()
    narrow = e.trajectory_modes(bin_xy=0.05, heading_bins=360, weights="uniform")
    assert narrow.count[:3].tolist() == [1, 1, 1] and narrow.size[:3, 0].tolist() == [P] * 3 and (narrow.count[3:] > 1).all()
    assert e.trajectory_summary("uniform").n_alive.tolist() == [1, 1, 1] + [P] * 66
    wide = e.trajectory_modes(bin_xy=1000.0, heading_bins=1, weights="uniform")
    assert wide.count.tolist() == [1] * 69 and (wide.share[:, 0] == 1.0).all() and np.isnan(wide.poses[:, 1:]).all()
    e.close()


# ---- 9. determinism and device outputs ----------------------------------------------------------------------------------------------------
def test_device_outputs_equal_the_host_outputs():
    import torch
    P = 513
    rng = np.random.default_rng(4)
    e = state_engine(P)
    e.set_state(poses=random_cloud(rng, P), weights=rng.uniform(-30.0, 30.0, size=P))
    a, b = e.pose_modes(labels=True), e.pose_modes(labels=True)
    assert all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    d = e.pose_modes(labels=True, device=True)                 # written in stream order: nothing was read back to form it
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in d)
    k = a.count if a.count < 8 else 8
    assert (int(d.count), int(d.bins), int(d.used)) == (a.count, a.bins, a.used) and same_bits(host(d.labels), a.labels)
    for name in ("poses", "covs", "share", "size", "mode_bins", "root", "best", "resultant", "n_eff", "weight_sum"):
        assert same_bits(host(getattr(d, name))[:k], np.asarray(getattr(a, name))), name
    assert d.labels.dtype == torch.int32 and d.poses.shape == (8, 3) and e.pose_modes(device=True).labels is None
    e.close()


# ---- 10. nothing else changes ----------------------------------------------------------------------------------------------------------------
def test_no_engine_state_changes():
    e = engine(16, max_beams=61, seed=3)
    load_room16(e)
    rng = np.random.default_rng(1)
    e.set_state(poses=rng.normal(scale=2.0, size=(16, 3)), weights=rng.uniform(-3, 3, size=16))
    e.track(4)
    e.record()

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.track_info(), e.render_map(3).cells, e.lineage()[1])

    before = state()
    e.pose_modes(labels=True)
    e.pose_modes(weights=np.ones(16), device=True)
    e.trajectory_modes()
    after = state()
    for x, y in zip(before, after):
        assert same_bits(x, y) if isinstance(x, np.ndarray) else x == y
    e.close()


# ---- 11. argument checks -------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_alone():
    P, K = 8, 4
    e = state_engine(P)
    info, f, i, lab = np.full((4, 4), -7, dtype=np.int64), np.full((4, K, 16), -7.0), np.full((4, K, 4), -7, dtype=np.int32), np.full(P, -7, dtype=np.int32)
    w = np.ones(P)

    def pm(mode=1, weights=None, bin_xy=0.5, n_th=36, K=K, flags=0, outs=(info, f, i, lab)):
        return e._lib.rbpf_pose_modes(e._h, mode, dp(weights), float(bin_xy), n_th, K, flags, *(vp(o) for o in outs))

    def tm(t0=0, t1=4, mode=1, weights=None, bin_xy=0.5, n_th=36, K=K, outs=(info, f, i)):
        return e._lib.rbpf_track_modes(e._h, t0, t1, mode, dp(weights), float(bin_xy), n_th, K, *(vp(o) for o in outs))

    assert tm() == ESTATE and b"tracking is off" in e._lib.rbpf_last_error(e._h)
    e.track(6)
    for _ in range(3):
        e.record()
    neg, nan, inf = w.copy(), w.copy(), w.copy()
    neg[2], nan[3], inf[4] = -1.0, np.nan, np.inf
    bad = [pm(outs=(None, f, i, lab)), pm(outs=(info, None, i, lab)), pm(outs=(info, f, None, lab)),
           pm(mode=3), pm(mode=-1), pm(mode=2), pm(mode=1, weights=w), pm(mode=2, weights=neg), pm(mode=2, weights=nan), pm(mode=2, weights=inf),
           pm(bin_xy=0.0), pm(bin_xy=-1.0), pm(bin_xy=np.nan), pm(bin_xy=np.inf), pm(n_th=0), pm(n_th=4097), pm(K=0), pm(K=65), pm(flags=2),
           tm(outs=(None, None, None)), tm(mode=3), tm(mode=2), tm(mode=0, weights=w), tm(mode=2, weights=neg), tm(mode=2, weights=nan),
           tm(bin_xy=0.0), tm(bin_xy=np.nan), tm(n_th=0), tm(n_th=4097), tm(K=0), tm(K=65),
           tm(-1, 2), tm(2, 2), tm(3, 2), tm(0, 5)]
    assert bad == [EINVAL] * len(bad)
    assert (info == -7).all() and (f == -7.0).all() and (i == -7).all() and (lab == -7).all()
    assert pm() == 0 and tm() == 0 and pm(mode=2, weights=w, outs=(info, None, None, None)) == 0 and (info != -7).all()
    e.untrack()
    assert tm() == ESTATE
    e.close()
