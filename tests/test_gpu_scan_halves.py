"""The front half of a scan step - matcher, NDT, proposal frame, samples, weighting - as two staggered half-batches on two
streams.  No kernel's arithmetic changes, so an engine created under RBPF_SCAN_HALVES=1 must leave every bit
where the same build leaves it under RBPF_SCAN_HALVES=0: poses, covariances, weights, every tile of every particle, the
resample's ancestors and every counter, after every step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CS, B, K = 0.05, 181, 30
NO_MS = ("ms_raycast", "ms_weight", "ms_match", "ms_resample", "ms_ndt", "stamps")
ENV = ("RBPF_SCAN_HALVES", "RBPF_MATCH_DEDUP", "RBPF_SKIP_DISCARDED", "RBPF_MAP_KERNEL", "RBPF_EV_RESIDENT", "RBPF_EV_GRID")


@pytest.fixture(scope="module")
def eng_mod():
    from thesis_amd import engine
    return engine


@pytest.fixture(scope="module")
def log181():
    from thesis_amd.datasets import synthetic
    return synthetic.make_log(8, n_beams=B)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def counts(e):
    return {k: v for k, v in e.counters().items() if k not in NO_MS}


def engine_pair(eng_mod, monkeypatch, P, env=(), **options):
    """(engine whose front half always runs as two half-batches, the single-stream reference): rbpf_create reads the environment"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    options.setdefault("cell_size", CS)
    options.setdefault("pool_tiles", 3 * P + 16)
    options.setdefault("resample_spread", 1.0)
    monkeypatch.setenv("RBPF_SCAN_HALVES", "1")
    e = eng_mod.ParticleEngine(P, max_beams=B, seed=7, **options)
    monkeypatch.setenv("RBPF_SCAN_HALVES", "0")
    ref = eng_mod.ParticleEngine(P, max_beams=B, seed=7, **options)
    monkeypatch.delenv("RBPF_SCAN_HALVES")
    return e, ref


def same(e, ref, what):
    for f in ("poses", "covs", "weights"):
        assert np.array_equal(bits(getattr(e, f)()), bits(getattr(ref, f)())), (what, f)
    for p in range(e.P):
        got, want = e.tiles(p), ref.tiles(p)
        assert [c for c, _ in got] == [c for c, _ in want], (what, p)
        for (c, a), (_, b) in zip(got, want):
            assert np.array_equal(a, b), (what, p, c, int(np.count_nonzero(a != b)))
    assert counts(e) == counts(ref), what


def whole(x, **kw):
    x.scan_update(**kw)


def begin_end(x, **kw):
    x.scan_update_begin(**kw)
    x.scan_update_end()


def drive(e, ref, log, steps, scan=whole, with_guesses=False, before_resample=None):
    """steps of the benchmark's loop body (imu / set_scan / scan_update / resample, its matcher cadence and previous-scan
    refresh) on both engines, everything compared after every step"""
    ang, ranges, odo, _ = log
    urng = np.random.Generator(np.random.PCG64(777))
    for x in (e, ref):
        x.set_scan(ranges[0], ang)
        x.map_update(np.zeros((x.P, 3)))
        x.refresh_last_scan(0)
    for k in range(steps):
        u = float(urng.random())
        adj = not (k % 5 < 2)
        g = None
        if with_guesses:
            g = ref.poses()[:, None, :] + np.random.Generator(np.random.PCG64(k)).normal(0, [0.02, 0.02, 0.005], size=(ref.P, K, 3))
        out = []
        for x in (e, ref):
            x.imu_update("velocity", odo[k], 1000.0)
            x.set_scan(ranges[k + 1], ang)
            scan(x, adj=adj, guesses=g)
            if before_resample is not None:
                before_resample(k, x)
            out.append(x.resample(u))
            if k % 5 == 0:
                x.refresh_last_scan(0)
        (did, idx), (did_r, idx_r) = out
        assert did == did_r and np.array_equal(idx, idx_r), k
        same(e, ref, f"step {k}")


# 1: the second half is empty, nothing may be launched for it; 2, 3: the smallest splits; 67, 130: the split lies inside a
# workgroup of the frame kernel (64 particles) and of the samples kernel (8 particles)
@pytest.mark.parametrize("P", [1, 2, 3, 67, 130])
def test_six_steps_equal_the_single_stream(eng_mod, monkeypatch, log181, P):
    e, ref = engine_pair(eng_mod, monkeypatch, P)
    drive(e, ref, log181, 6)
    c = e.counters()
    assert c["scan_updates"] == 7 and c["ndt_runs"] > 0
    e.close(); ref.close()


def test_without_the_ndt_stage(eng_mod, monkeypatch, log181):
    e, ref = engine_pair(eng_mod, monkeypatch, 67, ndt_refine=0)
    drive(e, ref, log181, 6)
    assert e.counters()["ndt_runs"] == 0
    e.close(); ref.close()


@pytest.mark.parametrize("dedup", ["1", "0"])
def test_duplicates_across_the_split_read_the_first_halfs_rows(eng_mod, monkeypatch, log181, dedup):
    """Nearly all weight on the last particle before the resample of step 1: its copies fill both halves and their
    representative is particle 0, so the second half's frame kernel reads a row the first half's matcher wrote."""
    P = 67
    e, ref = engine_pair(eng_mod, monkeypatch, P, (("RBPF_MATCH_DEDUP", dedup),))
    shared = {}

    def all_weight_on_the_last(k, x):
        shared[(k, x is e)] = x.counters()["match_shared"]
        if k == 1:
            w = np.full(P, 1e-3)
            w[-1] = 1e6
            x.set_state(weights=w)

    drive(e, ref, log181, 4, before_resample=all_weight_on_the_last)
    for is_e in (True, False):
        grown = shared[(2, is_e)] - shared[(1, is_e)]
        assert grown == (P - 1 if dedup == "1" else 0), (is_e, shared)
    e.close(); ref.close()


def test_nan_branch_in_both_halves(eng_mod, monkeypatch, log181):
    """A particle far from everything its map holds: the scan has no overlap with it, the match fails, the covariance is NaN
    and the particle keeps its pose (robot.py:73-78).  One such particle in each half."""
    P = 6
    ang, ranges, odo, _ = log181
    e, ref = engine_pair(eng_mod, monkeypatch, P, pool_tiles=8 * P)
    drive(e, ref, log181, 3)
    for x in (e, ref):
        x.imu_update("velocity", odo[3], 1000.0)
        poses = x.poses()
        poses[1] = [30.0, 30.0, 0.4]
        poses[4] = [-31.0, 29.0, -0.2]
        x.set_state(poses=poses)
        x.set_scan(ranges[4], ang)
        x.scan_update(adj=True)
        x.synchronize()
    same(e, ref, "NaN branch")
    got, near = e.poses(), [0, 2, 3, 5]
    assert np.array_equal(got[[1, 4]], poses[[1, 4]]) and not np.any(np.all(got[near] == poses[near], axis=1))
    assert np.all(e.weights() != 1.0)
    e.close(); ref.close()


def test_begin_end_path(eng_mod, monkeypatch, log181):
    e, ref = engine_pair(eng_mod, monkeypatch, 67)
    drive(e, ref, log181, 4, scan=begin_end)
    e.close(); ref.close()


def test_guesses_path(eng_mod, monkeypatch, log181):
    e, ref = engine_pair(eng_mod, monkeypatch, 67)
    drive(e, ref, log181, 4, with_guesses=True)
    e.close(); ref.close()


def test_profiled_families_take_the_single_stream_path(eng_mod, monkeypatch, log181):
    """Timing events of the match, ndt or weight family bracket one kernel's own duration: one entry a step."""
    e, ref = engine_pair(eng_mod, monkeypatch, 67)
    for x in (e, ref):
        x.set_profiling(True)
    drive(e, ref, log181, 4)
    for fam in ("match", "ndt", "weight"):
        ms = e.kernel_ms(fam)
        assert len(ms) == 4 and np.all(ms > 0), (fam, ms)
    e.close(); ref.close()


def test_borrowed_stream_carries_the_second_half(eng_mod, monkeypatch, log181):
    import torch
    e, ref = engine_pair(eng_mod, monkeypatch, 67)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        drive(e, ref, log181, 2)
        e.release_stream()
    same(e, ref, "after release_stream")
    e.close(); ref.close()
