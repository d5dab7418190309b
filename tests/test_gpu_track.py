"""The trajectory log and the pose estimate on the GPU (rbpf_track_*, rbpf_estimate, kernels_track.hip) against
the NumPy model of tests/track_oracle.py: lineage indices and gathered poses bit for bit, n_alive / best / n_used exactly, the
estimate rows within the bound derived from the test's own inputs; then the recording hooks, the full log, what tracking leaves
alone, the argument checks, ParticleFilter(history="device") against history="host", and checkpoints."""
import ctypes as C

import numpy as np
import pytest

from tests import track_oracle as T
from tests.test_gpu_cast import engine, load_room16

pytestmark = pytest.mark.gpu

ESTATE, EINVAL, ENOMEM = -4, -1, -2
PS = [1, 2, 63, 64, 65, 300, 1025]           # one lane, the sides of a wave, a ragged last wave, more than the 512 / 1024 lanes of a workgroup
TS = [1, 2, 63, 64, 65, 3 * 64 + 5]          # the sides of a chunk, several chunks with a ragged last one


def state_engine(P, **kw):
    """An engine whose state the test sets itself: no scans, one tile per particle."""
    return engine(P, cs=0.1, pool_tiles=P + 8, max_beams=16, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def forcing_weights(rng, P, spread):
    """Weights whose spread passes the resample trigger, with zeros and negatives among them."""
    w = rng.uniform(-50.0, 50.0, size=P)
    hi = int(rng.integers(0, P))
    lo = (hi + 1 + int(rng.integers(0, P - 1))) % P            # P >= 2
    w[hi], w[lo] = spread + 100.0, min(w.min(), 0.0)
    return w


def drive(e, rng, n_records, capacity=None):
    """track(), then n_records - 1 records with random poses and 0, 1 or 2 resamples (forced or suppressed) in front of each,
    and 0 .. 2 resamples behind the last.  The model is driven with the ancestors the resamples report."""
    P, spread = e.P, float(e.cfg.resample_spread)
    poses, w = rng.normal(scale=3.0, size=(P, 3)), np.ones(P)
    e.set_state(poses=poses, weights=w)
    e.track(capacity or n_records)
    m = T.TrackModel(poses, w)

    def resamples(k):
        nonlocal poses, w
        for _ in range(k):
            forced = P > 1 and rng.random() < 0.7
            w = forcing_weights(rng, P, spread) if forced else np.full(P, float(rng.uniform(-5, 5)))
            e.set_state(weights=w)
            did, idx = e.resample(float(rng.random()))
            assert did == forced
            if did:
                m.resample(idx)
                poses, w = poses[idx], np.ones(P)

    for t in range(1, n_records):
        resamples(t % 3)                                       # none, one, two
        poses = poses + rng.normal(scale=0.1, size=(P, 3))
        e.set_state(poses=poses)
        e.record()
        m.record(poses, w)
    resamples(int(rng.integers(0, 3)))
    return m, poses, w


# ---- 1. lineage and poses by equality ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", TS)
@pytest.mark.parametrize("P", PS)
def test_lineage_and_poses_equal_the_model(P, N):
    rng = np.random.default_rng(100 * P + N)
    e = state_engine(P)
    m, _, _ = drive(e, rng, N)
    assert e.track_info() == {"n_records": N, "capacity": N, "dropped": 0, "imu": False, "scan": True}
    want_idx, want_pose = m.lineage()
    assert np.array_equal(T.lineage_chunked(np.stack(m.parent), m.pending), want_idx)       # the model's two implementations
    idx, pose = e.lineage()
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx) and same_bits(pose, want_pose)
    idx_only, none = e.lineage(poses=False)
    assert none is None and np.array_equal(idx_only, want_idx)
    some = [int(p) for p in rng.integers(0, P, size=min(P, 5))] + [P - 1]
    wi, wp = m.lineage(some)
    idx, pose = e.lineage(some)
    assert np.array_equal(idx, wi) and same_bits(pose, wp)
    assert same_bits(e.trajectory(some[0]), wp[:, 0, :])
    didx, dpose = e.lineage(some, device=True)
    assert np.array_equal(host(didx), wi) and same_bits(host(dpose), wp)
    didx, dpose = e.lineage(device=True)
    assert np.array_equal(host(didx), want_idx) and same_bits(host(dpose), want_pose)
    for t0, t1 in ((0, 1), (N - 1, N), (N // 3, 2 * N // 3 + 1), (min(70, N - 1), N), (max(N - 70, 0), max(N - 3, 1)), (5, min(60, N))):
        if 0 <= t0 < t1 <= N:                                  # sub-ranges that start and end inside a chunk
            wi, wp = m.lineage(None, t0, t1)
            idx, pose = e.lineage(t0=t0, t1=t1)
            assert np.array_equal(idx, wi) and same_bits(pose, wp), (t0, t1)
            idx, pose = e.lineage(some, t0=t0, t1=t1)
            assert np.array_equal(idx, wi[:, some]) and same_bits(pose, wp[:, some]), (t0, t1)
    e.close()


# ---- 2. n_alive, best, n_used by equality ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 65, 300])
def test_n_alive_and_coalescence(P):
    from thesis_amd import trajectory
    rng = np.random.default_rng(P)
    e = state_engine(P)
    poses = rng.normal(size=(P, 3))
    e.set_state(poses=poses, weights=1.0)
    e.track(70)
    m = T.TrackModel(poses, np.ones(P))
    w = np.ones(P)

    def resample(weights):
        nonlocal poses
        e.set_state(weights=weights)
        did, idx = e.resample(0.37)
        assert did
        m.resample(idx)
        poses = poses[idx]

    def record():
        e.record(); m.record(poses, w)

    for _ in range(2):
        resample(forcing_weights(rng, P, 200.0))
        record()
    one = np.zeros(P)
    one[P // 2] = 1000.0                                       # every new particle continues particle P // 2
    resample(one)
    for _ in range(66):                                        # across a chunk border
        record()
    s = e.trajectory_summary("uniform")
    want = m.summary(np.ones(P), T.W_UNIFORM)
    assert s.n_alive.tolist() == [i[2] for _, i in want] == [1, 1, 1] + [P] * 66
    assert s.best.tolist() == [0] * 69 and s.n_used.tolist() == [P] * 69
    assert trajectory.coalescence(s) == 2 and trajectory.coalescence(e.filtered_trajectory()) == -1
    e.close()


# ---- 3. estimate rows within the derived tolerance -------------------------------------------------------------------------------
def assert_row(got_f, got_i, want, tol, what):
    wf, wi = want
    assert list(got_i) == list(wi), (what, list(got_i), list(wi))
    assert np.array_equal(np.isnan(got_f), np.isnan(wf)), what
    err = np.abs(got_f[:12] - wf[:12])
    err[2] = abs(T.wrap(got_f[2] - wf[2])) if np.isfinite(wf[2]) else 0.0
    ratio = [err[k] / tol[k] for k in range(12) if tol[k] > 0 and np.isfinite(err[k])]
    print(f"{what}: largest |device - fsum| / bound = {max(ratio, default=0.0):.3g}")
    ok = np.isnan(wf[:12]) | (err <= tol)
    assert ok.all(), (what, np.nonzero(~ok)[0].tolist(), err, tol)
    assert list(got_f[12:]) == [0, 0, 0, 0]


def row_of(s, k):
    f = np.zeros(16)
    f[0:3], f[9], f[10], f[11] = s.pose[k], s.resultant[k], s.weight_sum[k], s.n_eff[k]
    f[3:9] = s.cov[k][[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    assert np.array_equal(s.cov[k], s.cov[k].T, equal_nan=True)
    return f, [s.best[k], s.n_used[k], s.n_alive[k], 0]


def est_row(est):
    f = np.zeros(16)
    f[0:3], f[9], f[10], f[11] = est.pose, est.resultant, est.weight_sum, est.n_eff
    f[3:9] = est.cov[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    return f, [est.best, est.n_used, -1, 0]


@pytest.mark.parametrize("P", PS)
def test_estimate_rows_within_the_derived_bound(P):
    rng = np.random.default_rng(7 * P)
    e = state_engine(P)
    poses = rng.normal(scale=4.0, size=(P, 3))
    poses[:, 2] = rng.uniform(-np.pi, np.pi, size=P)
    raw = rng.uniform(-30.0, 30.0, size=P)
    if P >= 63:
        raw[[3, 17]], raw[[5, 40]] = -np.inf, 0.0             # -inf, zeros and negatives
        poses[11, 1] = np.nan                                  # left out: n_used drops by one
    given = rng.uniform(0.0, 2.0, size=P)
    given[0] = 0.0 if P > 1 else 1.0
    e.set_state(poses=poses, weights=raw)
    for mode, arg, g in ((T.W_RESAMPLE, "resample", None), (T.W_UNIFORM, "uniform", None), (T.W_GIVEN, given, given)):
        want, tol = T.estimate_row(poses, raw, mode, g), T.est_tolerance(poses, raw, mode, g)
        est = e.estimate(arg)
        assert_row(*est_row(est), want, tol, f"estimate P={P} mode={mode}")
        again = e.estimate(arg)
        assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(est, again))     # identical bits from call to call
    if P >= 63:
        ok = np.isfinite(poses).all(axis=1)
        assert e.estimate("uniform").n_used == P - 1 == int(ok.sum())
        assert e.estimate("resample").best == int(np.argmax(raw))
    # the rows stored at record time, and the smoothed rows after two resamples
    e.track(3)
    m = T.TrackModel(poses, raw)
    if P > 1:
        e.set_state(weights=forcing_weights(rng, P, 200.0))
        did, idx = e.resample(0.61)
        assert did
        m.resample(idx)
        poses, raw = poses[idx], np.ones(P)
    poses = np.where(np.isfinite(poses), poses, 0.5) + rng.normal(scale=0.2, size=(P, 3))
    raw = rng.uniform(-30.0, 30.0, size=P)
    e.set_state(poses=poses, weights=raw)
    e.record()
    m.record(poses, raw)
    flt = e.filtered_trajectory()
    for t in range(2):
        assert_row(*row_of(flt, t), m.row(t), T.est_tolerance(m.poses[t], m.weights[t]), f"filtered P={P} t={t}")
    lin_pose = m.lineage()[1]
    for mode, arg, g in ((T.W_RESAMPLE, "resample", None), (T.W_UNIFORM, "uniform", None), (T.W_GIVEN, given, given)):
        s = e.trajectory_summary(arg)
        want = m.summary(raw, mode, g)
        for t in range(2):
            assert_row(*row_of(s, t), want[t], T.est_tolerance(lin_pose[t], raw, mode, g), f"summary P={P} t={t} mode={mode}")
        s2 = e.trajectory_summary(arg)
        assert all(same_bits(a, b) for a, b in zip(s, s2))
    e.close()


def test_estimate_hand_cases():
    e = state_engine(2)
    e.set_state(poses=[[0, 0, np.pi - 0.01], [0, 0, -(np.pi - 0.01)]], weights=1.0)
    est = e.estimate("uniform")
    assert abs(abs(est.pose[2]) - np.pi) < 1e-15 and abs(est.cov[2, 2] - 1e-4) < 1e-15     # the mean heading is pi, not 0
    e.set_state(weights=[-np.inf, -np.inf])
    est = e.estimate()
    assert np.isnan(est.pose).all() and np.isnan(est.cov).all() and np.isnan(est.n_eff) and est.n_used == 0 and est.best == 0
    e.set_state(poses=[[1, 2, 0.5], [7, 7, 7]], weights=[3.0, -np.inf])
    est = e.estimate()
    assert est.pose.tolist()[:2] == [1.0, 2.0] and abs(est.pose[2] - 0.5) < 1e-15 and est.n_used == 1 and est.n_eff == 1.0
    e.close()


# ---- 4. recording hooks -------------------------------------------------------------------------------------------------------
def small_engine(seed=3):
    e = engine(16, max_beams=61, seed=seed)
    load_room16(e)
    return e


def small_log(n):
    from thesis_amd.datasets import synthetic
    return synthetic.make_log(n, 61)


def test_recording_hooks():
    ang, ranges, odo, _ = small_log(6)
    e = small_engine()
    e.track(32, scan=True)
    n = lambda: e.track_info()["n_records"]
    assert n() == 1
    e.set_scan(ranges[0], ang)
    e.map_update()                                             # the test entries never record
    e.weight_samples(np.zeros((16, 4, 3)), np.ones((16, 4)))
    e.imu_update("velocity", odo[0], 1000.0)                   # imu=False
    assert n() == 1
    e.scan_update()
    assert n() == 2
    e.scan_update_begin(); e.scan_update_end()
    assert n() == 3
    e.resample(0.5)
    assert n() == 3
    assert same_bits(e.lineage(t0=2)[1][0], e.poses())         # the record holds bit copies, and a resample only moves them
    e.untrack()
    e.track(32, imu=True, scan=True)
    assert n() == 1 and e.track_info()["imu"]
    for k in range(1, 4):
        e.imu_update("velocity", odo[k], 1000.0)
        assert n() == 2 * k
        e.set_scan(ranges[k + 1], ang)
        e.scan_update()
        assert n() == 2 * k + 1
    e.untrack()
    e.track(8, imu=False, scan=False)
    e.imu_update("velocity", odo[4], 1000.0); e.scan_update()
    assert n() == 1
    e.close()


def test_resample_async_is_followed_without_a_host_read():
    ang, ranges, odo, _ = small_log(8)
    a, b = small_engine(), small_engine()
    for e in (a, b):
        e.track(32, imu=True, scan=True)
    for k in range(7):
        for e in (a, b):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            e.scan_update()
            w = e.weights()                                    # past the trigger on the odd steps, suppressed on the even ones
            w[1 + k % 5] += 300.0
            e.set_state(weights=w if k % 2 else 1.0)
        a.resample_async(0.3 + 0.1 * k)
        did, _ = b.resample(0.3 + 0.1 * k)
        assert did == bool(k % 2)
    (ia, pa), (ib, pb) = a.lineage(), b.lineage()
    assert np.array_equal(ia, ib) and same_bits(pa, pb) and len(ia) == 15
    assert any(len(np.unique(r)) < 16 for r in ia)             # lineages did merge
    a.close(); b.close()


# ---- 5. full log ---------------------------------------------------------------------------------------------------------------
def test_full_log_drops_implicit_records_and_refuses_explicit_ones():
    from thesis_amd.engine import RbpfError
    ang, ranges, odo, _ = small_log(5)
    e = small_engine()
    e.track(3, scan=True)
    for k in range(2):
        e.set_scan(ranges[k], ang)
        e.scan_update()
    before = e.lineage()
    assert e.track_info()["n_records"] == 3 and e.track_info()["dropped"] == 0
    e.set_scan(ranges[2], ang)
    e.scan_update()                                            # the fourth record: dropped, the call is fine
    info = e.track_info()
    assert (info["n_records"], info["capacity"], info["dropped"]) == (3, 3, 1)
    with pytest.raises(RbpfError) as err:
        e.record()
    assert err.value.code == ENOMEM and e.track_info()["dropped"] == 1
    after = e.lineage()
    assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1])
    e.close()


# ---- 6. off means off, and argument checks ---------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    from thesis_amd.engine import RbpfError
    try:
        fn(*a, **kw)
    except RbpfError as err:
        return err.code
    return 0


def test_track_calls_need_tracking_and_estimate_does_not():
    e = state_engine(8)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    for fn in (e.untrack, e.record, e.track_info, e.lineage, e.trajectory_summary, e.filtered_trajectory, lambda: e.lineage(t0=0, t1=1),
               lambda: e._check(e._lib.rbpf_track_export(e._h, 0, 0, C.c_void_p(buf.ctypes.data))),
               lambda: e._check(e._lib.rbpf_track_import(e._h, 1, C.c_void_p(buf.ctypes.data)))):
        assert code_of(fn) == ESTATE
    assert e.estimate().n_used == 8 and e._lib.rbpf_track_record_bytes(e._h) == (28 * 8 + 144 + 15) // 16 * 16
    e.track(4)
    assert code_of(e.track, 4) == ESTATE
    e.untrack()
    assert code_of(e.track_info) == ESTATE
    e.close()


def test_after_untrack_a_run_equals_one_that_never_tracked():
    ang, ranges, odo, _ = small_log(7)
    a, b = small_engine(), small_engine()
    a.track(4, imu=True, scan=True)
    a.record()
    a.untrack()
    for k in range(5):
        for e in (a, b):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            e.scan_update()
            if k in (1, 3):
                w = e.weights()
                w[2 + k] += 300.0
                e.set_state(weights=w)
            e.resample(0.25 + 0.1 * k)
    assert same_bits(a.poses(), b.poses()) and same_bits(a.weights(), b.weights()) and same_bits(a.covs(), b.covs())
    for p in range(16):
        ta, tb = a.tiles(p), b.tiles(p)
        assert [c for c, _ in ta] == [c for c, _ in tb] and all(np.array_equal(x, y) for (_, x), (_, y) in zip(ta, tb))
    assert a.counters()["resample_copies"] == b.counters()["resample_copies"] > 0
    a.close(); b.close()


def test_argument_checks_leave_the_outputs_alone():
    P = 8
    e = state_engine(P)
    e.track(6)
    for _ in range(3):
        e.record()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    src, gid = np.arange(P, dtype=np.int32), np.arange(P, dtype=np.int32)
    assert e._lib.rbpf_apply_resample_local(e._h, src.ctypes.data_as(ip), gid.ctypes.data_as(ip)) == ESTATE
    assert b"across ranks" in e._lib.rbpf_last_error(e._h)
    assert e._lib.rbpf_unpack_particles(e._h, None, 0, None, None) == ESTATE
    idx, pose = np.full((4, P), -7, dtype=np.int32), np.full((4, P, 3), -7.0)
    f, i = np.full((4, 16), -7.0), np.full((4, 4), -7, dtype=np.int32)
    w = np.ones(P)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    lin = lambda t0, t1, parts, n, flags=0: e._lib.rbpf_track_lineage(e._h, t0, t1, None if parts is None else parts.ctypes.data_as(ip), n,
                                                                    vp(idx), vp(pose), flags)
    bad_p = np.array([0, P], dtype=np.int32)
    for rc in (lin(-1, 2, None, 0), lin(2, 2, None, 0), lin(3, 2, None, 0), lin(0, 5, None, 0), lin(0, 4, bad_p, 2), lin(0, 4, bad_p, 0),
               lin(0, 4, None, 3), lin(0, 4, None, 0, 2), e._lib.rbpf_track_lineage(e._h, 0, 4, None, 0, None, None, 0),
               e._lib.rbpf_track_summary(e._h, 0, 5, 0, None, f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_track_summary(e._h, 0, 4, 3, None, f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_track_summary(e._h, 0, 4, 2, None, f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_track_summary(e._h, 0, 4, 0, w.ctypes.data_as(dp), f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_track_filtered(e._h, 1, 1, f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_track_filtered(e._h, 0, 5, f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_estimate(e._h, -1, None, f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_estimate(e._h, 2, (-w).ctypes.data_as(dp), f.ctypes.data_as(dp), i.ctypes.data_as(ip)),
               e._lib.rbpf_track_export(e._h, 2, 5, vp(pose)), e._lib.rbpf_track_import(e._h, 7, vp(pose)),
               e._lib.rbpf_track_import(e._h, 0, vp(pose))):
        assert rc == EINVAL
    assert (idx == -7).all() and (pose == -7.0).all() and (f == -7.0).all() and (i == -7).all()
    assert lin(0, 4, None, 0) == 0 and (idx[:, :] == np.arange(P)).all()
    # an import with a parent out of range is refused and replaces nothing
    nb = int(e._lib.rbpf_track_record_bytes(e._h))
    blob = np.zeros(4 * nb + 4 * P, dtype=np.uint8)
    assert e._lib.rbpf_track_export(e._h, 0, 4, vp(blob)) == 0
    bad = blob.copy()
    bad[nb + 24 * P + 128: nb + 24 * P + 132] = np.array([P], dtype=np.int32).view(np.uint8)
    assert e._lib.rbpf_track_import(e._h, 4, vp(bad)) == EINVAL
    assert e._lib.rbpf_track_import(e._h, 2, vp(np.concatenate([blob[:2 * nb], blob[4 * nb:]]))) == 0
    assert e.track_info()["n_records"] == 2 and np.array_equal(e.lineage()[0], np.tile(np.arange(P, dtype=np.int32), (2, 1)))
    assert e._lib.rbpf_track_begin(e._h, 4, 4) == ESTATE      # on already: the state decides first
    e.untrack()
    assert e._lib.rbpf_track_begin(e._h, 4, 4) == EINVAL and e._lib.rbpf_track_begin(e._h, 0, 0) == EINVAL
    e.close()


# ---- 7. ParticleFilter end to end ----------------------------------------------------------------------------------------------
def test_particle_filter_device_history_equals_host_history():
    from thesis_amd.datasets import synthetic
    from thesis_amd.slam import ParticleFilter, run_log
    period = 0.7
    angles, ranges, odo, _ = synthetic.make_log(40, 181, period=period)
    scan_times = (np.arange(41) * period * 1e4).astype(np.int64)
    odom_times = scan_times[1:] - 1
    out = []
    for history in ("host", "device"):
        pf = ParticleFilter(64, angles, motion_model="velocity", seed=5, history=history)
        res = run_log(pf, ranges, scan_times, odo, odom_times)
        out.append((res, [np.array(pf.trajectory(i)) for i in range(64)], np.array(pf.particles[3].x())))
        if history == "device":
            assert pf.engine.track_info()["n_records"] == len(out[0][1][0]) and pf._poses == []
        pf.close()
    (rh, th, xh), (rd, td, xd) = out
    assert rh.trace == rd.trace and rh.resamples == rd.resamples > 0 and rh.accepted == rd.accepted
    assert all(same_bits(a, b) for a, b in zip(th, td)) and same_bits(xh, xd) and len(th[0]) > 60
    assert len({a.tobytes() for a in th}) > 1                  # not all one path


def test_particle_filter_raises_when_the_log_ran_full():
    from thesis_amd.datasets import synthetic
    from thesis_amd.slam import ParticleFilter
    pf = ParticleFilter(4, synthetic.beam_angles(61), history="device", history_capacity=2)
    pf.imu_update([0.1, 0.0, 0.0], 1000.0)
    assert len(pf.trajectory(0)) == 2
    pf.imu_update([0.1, 0.0, 0.0], 1000.0)
    with pytest.raises(RuntimeError, match="ran full"):
        pf.trajectory(0)
    with pytest.raises(ValueError):
        ParticleFilter(4, synthetic.beam_angles(61), history="tape")
    pf.close()


# ---- 8. checkpoint -------------------------------------------------------------------------------------------------------------
def test_checkpoint_restores_the_log(tmp_path):
    from thesis_amd.engine import ParticleEngine
    ang, ranges, odo, _ = small_log(22)
    a = small_engine(seed=9)
    a.track(64, imu=True, scan=True)

    def step(e, k):
        e.imu_update("velocity", odo[k], 1000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update()
        if k % 4 == 1:
            w = e.weights()
            w[k % 16] += 300.0
            e.set_state(weights=w)
        e.resample_async()                                     # the internal uniform: part of the checkpointed stream state

    for k in range(10):
        step(a, k)
    path = str(tmp_path / "tracked.npz")
    a.save_checkpoint(path)
    b = ParticleEngine.from_checkpoint(path)
    assert b.track_info() == a.track_info() and a.track_info()["n_records"] == 21
    for k in range(10, 20):
        step(a, k); step(b, k)
    assert a.track_info() == b.track_info() and a.track_info()["n_records"] == 41
    (ia, pa), (ib, pb) = a.lineage(), b.lineage()
    assert np.array_equal(ia, ib) and same_bits(pa, pb) and same_bits(a.poses(), b.poses())
    assert all(same_bits(x, y) for x, y in zip(a.filtered_trajectory(), b.filtered_trajectory()))
    assert any(len(np.unique(r)) < 16 for r in ia)
    a.untrack()
    a.save_checkpoint(str(tmp_path / "plain.npz"))            # written without tracking: loads as before, no log
    c = ParticleEngine.from_checkpoint(str(tmp_path / "plain.npz"))
    assert code_of(c.track_info) == ESTATE and same_bits(c.poses(), a.poses())
    with np.load(str(tmp_path / "plain.npz")) as d:
        assert "track_records" not in d.files
    a.close(); b.close(); c.close()
