"""The map update that rbpf_scan_update holds back for the resample behind it: rbpf_resample launches it
behind its plan, without the particles the plan discards.  The reference is the same build with RBPF_SKIP_DISCARDED=0 - the
same order of launches, nobody left out - and, for the NaN-covariance branch, the oracle."""
import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests.mapupdate_hidden import check_map_hidden, compare_hidden, read_hidden_of
from tests.test_gpu_parity import assert_tiles_equal, oracle_dump

pytestmark = pytest.mark.gpu

CS = 0.05
NO_MS = ("ms_raycast", "ms_weight", "ms_match", "ms_resample", "ms_ndt", "stamps")


@pytest.fixture(scope="module")
def eng_mod():
    from thesis_amd import engine
    return engine


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def counts(e):
    return {k: v for k, v in e.counters().items() if k not in NO_MS}


def engine_pair(eng_mod, monkeypatch, P, B, env=(), hold="1", **options):
    """(engine that leaves the discarded out, reference engine): rbpf_create reads the environment.  hold="1": held back at
    these small sizes too (by itself the library holds back above four particles per CU); None: the library's own choice."""
    for k in ("RBPF_MAP_KERNEL", "RBPF_EV_RESIDENT", "RBPF_EV_GRID", "RBPF_SKIP_DISCARDED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if hold is not None:
        monkeypatch.setenv("RBPF_SKIP_DISCARDED", hold)
    options.setdefault("cell_size", CS)
    options.setdefault("pool_tiles", 6 * P + 16)
    e = eng_mod.ParticleEngine(P, max_beams=B, **options)
    monkeypatch.setenv("RBPF_SKIP_DISCARDED", "0")
    ref = eng_mod.ParticleEngine(P, max_beams=B, **options)
    monkeypatch.delenv("RBPF_SKIP_DISCARDED")
    return e, ref


def same_state(e, ref, what):
    assert np.array_equal(bits(e.poses()), bits(ref.poses())), what
    assert np.array_equal(bits(e.covs()), bits(ref.covs())), what
    assert np.array_equal(bits(e.weights()), bits(ref.weights())), what
    assert e.counters()["tiles_in_use"] == ref.counters()["tiles_in_use"], what
    for p in (None, *range(e.P)):
        assert e.map_extent(p) == ref.map_extent(p), (what, p)


def same_maps(e, ref, what):
    for p in range(e.P):
        got, want = e.tiles(p), ref.tiles(p)
        assert [c for c, _ in got] == [c for c, _ in want], (what, p)
        for (c, a), (_, b) in zip(got, want):
            assert np.array_equal(a, b), (what, p, c, int(np.count_nonzero(a != b)))
    got, want = read_hidden_of(e, range(e.P)), read_hidden_of(ref, range(e.P))     # written boxes and occupancy words
    for p in range(e.P):
        compare_hidden(got[p], want[p], e.dim, f"{what}: particle {p}")


def without_offspring(idx, P):
    return P - len(np.unique(idx))


def drive(e, ref, log, steps, between=None):
    """steps of imu / set_scan / scan_update / [between] / resample on both engines, everything compared after every step.
    Returns the particles without offspring per step (0 where nothing was resampled)."""
    ang, ranges, odo, _ = log
    urng = np.random.Generator(np.random.PCG64(777))
    for x in (e, ref):
        x.set_scan(ranges[0], ang)
        x.map_update(np.zeros((x.P, 3)))
    dead = []
    for k in range(steps):
        u = float(urng.random())
        out = []
        for x in (e, ref):
            x.imu_update("velocity", odo[k], 1000.0)
            x.set_scan(ranges[k + 1], ang)
            x.scan_update()
            if between is not None:
                between(x)
            out.append(x.resample(u))
        (did, idx), (did_r, idx_r) = out
        assert did == did_r and np.array_equal(idx, idx_r), k
        same_state(e, ref, f"step {k}")
        dead.append(without_offspring(idx, e.P) if did else 0)
    return dead


@pytest.fixture(scope="module")
def log181():
    from thesis_amd.datasets import synthetic
    return synthetic.make_log(14, n_beams=181)


# (map kernel chain; RBPF_EV_GRID=5: the resident workgroups draw several positions of the list each)
CHAINS = {"default": (("RBPF_EV_GRID", "5"),), "ray": (("RBPF_MAP_KERNEL", "ray"),), "window": (("RBPF_MAP_KERNEL", "window"),),
          "workgroup_per_particle": (("RBPF_EV_RESIDENT", "0"),)}


@pytest.mark.parametrize("chain", list(CHAINS))
def test_ab_over_steps(eng_mod, monkeypatch, log181, chain):
    P = 48
    e, ref = engine_pair(eng_mod, monkeypatch, P, 181, CHAINS[chain], resample_spread=1.0)
    dead = drive(e, ref, log181, 12)
    same_maps(e, ref, chain)
    c, cr = e.counters(), ref.counters()
    print(chain, "without offspring per step", dead, "ray cells", c["ray_cells_visited"], cr["ray_cells_visited"])
    assert c["map_updates_skipped"] == sum(dead) and sum(1 for d in dead if d > 0) >= 3
    assert cr["map_updates_skipped"] == 0
    assert c["ray_cells_visited"] < cr["ray_cells_visited"]
    assert c["resample_copies"] == cr["resample_copies"] and c["scan_updates"] == cr["scan_updates"] == 13
    e.close(); ref.close()


def test_ab_one_window_fan_1081_beams(eng_mod, monkeypatch):
    from thesis_amd.datasets import synthetic
    P = 24
    e, ref = engine_pair(eng_mod, monkeypatch, P, 1081, resample_spread=1.0)
    dead = drive(e, ref, synthetic.make_log(12, n_beams=1081), 12)
    same_maps(e, ref, "1081 beams")
    c, cr = e.counters(), ref.counters()
    assert c["map_updates_skipped"] == sum(dead) and sum(1 for d in dead if d > 0) >= 3 and cr["map_updates_skipped"] == 0
    assert c["ray_cells_visited"] < cr["ray_cells_visited"] and c["window_fallbacks"] == cr["window_fallbacks"] == 0
    e.close(); ref.close()


def test_nan_branch_step_leaves_nobody_out_and_equals_the_oracle(eng_mod, monkeypatch):
    """The engine seam doubled as in test_gpu_parity's closed loop, resample right behind scan_update; in step 1 a particle is
    on the NaN-covariance branch: its weight changes after the map update, so the plan waits and nobody is left out."""
    from thesis_amd.datasets import synthetic
    for k in ("RBPF_MAP_KERNEL", "RBPF_EV_RESIDENT", "RBPF_EV_GRID", "RBPF_SKIP_DISCARDED"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RBPF_SKIP_DISCARDED", "1")
    P, K, B, T = 24, 30, 181, 4
    ang = synthetic.beam_angles(B, np.pi)
    rng = np.random.Generator(np.random.PCG64(2025))
    truth = np.array([0.2, -0.1, 0.05])
    e = eng_mod.ParticleEngine(P, max_beams=B, pool_tiles=8 * P, cell_size=CS)
    robots = [orc.OracleRobot(CS) for _ in range(P)]
    r0 = synthetic.cast_scan(truth, ang, rng)
    sx, sy = orc.scan_xy(r0, ang)
    e.set_scan(r0, ang)
    e.map_update(np.zeros((P, 3)))
    for rb in robots:
        rb.map.update((0.0, 0.0, 0.0), sx, sy)
    skipped = 0
    for t in range(T):
        # the spread past the trigger of main.py:50 before the step: the weights add up (robot.py:114)
        bump = np.zeros(P); bump[(5 * t) % P] = 260.0; bump[(5 * t + 3) % P] = -40.0
        e.set_state(weights=e.weights() + bump)
        for p, rb in enumerate(robots):
            rb.weight[-1] = rb.weight[-1] + bump[p]
        vel = np.array([0.4, 0.1, 0.08]) * (1 + 0.1 * rng.normal(size=3))
        e.imu_update("velocity", vel, 900.0)
        for rb in robots:
            rb.imu_update("velocity_fr101", vel, 900.0)
        truth = truth + np.array([0.036, 0.009, 0.0072])
        r = synthetic.cast_scan(truth, ang, rng)
        sx, sy = orc.scan_xy(r, ang)
        e.set_scan(r, ang)
        poses_in = e.poses()
        match, guesses = np.zeros((P, 13)), np.zeros((P, K, 3))
        for p in range(P):
            cov = np.diag([2e-4, 3e-4, 2e-5]) * (1 + 0.05 * p)
            mp = poses_in[p] + rng.normal(0, [0.01, 0.01, 0.003])
            match[p] = np.concatenate([mp, cov.ravel(), [100.0 + p]])
            guesses[p] = rng.multivariate_normal(mp, cov, K)
        if t == 1:
            match[2, 3:12] = np.nan                              # robot.py:73-78
        u = float(rng.random())
        e.scan_update(match_override=match, guesses=guesses)
        did, idx = e.resample(u)
        for p, rb in enumerate(robots):
            rb.map_update(sx, sy, (match[p, :3], match[p, 3:12].reshape(3, 3), match[p, 12]), guesses=guesses[p])
        did_ref, idx_ref = orc.resample_indices([rb.weight[-1] for rb in robots], u)
        assert did and did_ref and list(idx) == list(idx_ref), (t, idx, idx_ref)
        robots = orc.resample(robots, u)
        now = e.counters()["map_updates_skipped"]
        assert now - skipped == (0 if t == 1 else without_offspring(idx, P)), t
        assert t == 1 or now > skipped
        skipped = now
        np.testing.assert_allclose(e.poses(), [rb.pose() for rb in robots], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(e.weights(), [float(rb.weight[-1]) for rb in robots], rtol=1e-9)
    for p, rb in enumerate(robots):
        assert_tiles_equal(e, p, oracle_dump(rb.map), e.dim)
    for p, rb in enumerate(robots):                          # the update was launched late, by the resample: boxes and occupancy words
        check_map_hidden(e, p, rb.map, what="nan branch")
    e.close()


def test_the_library_holds_back_only_above_four_particles_per_cu(eng_mod, monkeypatch, log181):
    """Its own choice (RBPF_SKIP_DISCARDED unset): 32 particles are updated as ever, all counters equal the reference's; 1040
    (four per CU of the MI355X's 256 would be 1024) leave the discarded out, with equal ancestors, state and tile counts."""
    e, ref = engine_pair(eng_mod, monkeypatch, 32, 181, hold=None, resample_spread=1.0)
    assert sum(drive(e, ref, log181, 3)) > 0
    same_maps(e, ref, "32 particles")
    assert counts(e) == counts(ref) and e.counters()["map_updates_skipped"] == 0
    e.close(); ref.close()
    P = 1040
    e, ref = engine_pair(eng_mod, monkeypatch, P, 181, hold=None, resample_spread=1.0, cell_size=0.1, pool_tiles=2 * P + 16)
    ang, ranges, odo, _ = log181
    for x in (e, ref):
        x.set_scan(ranges[0], ang)
        x.map_update(np.zeros((P, 3)))
    dead = 0
    for k in range(3):
        out = []
        for x in (e, ref):
            x.imu_update("velocity", odo[k], 1000.0)
            x.set_scan(ranges[k + 1], ang)
            x.scan_update()
            out.append(x.resample(0.3 + 0.2 * k))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]), k
        dead += without_offspring(out[0][1], P) if out[0][0] else 0
        for f in ("poses", "covs", "weights"):
            assert np.array_equal(bits(getattr(e, f)()), bits(getattr(ref, f)())), (k, f)
    c, cr = e.counters(), ref.counters()
    assert c["map_updates_skipped"] == dead > 0 and cr["map_updates_skipped"] == 0 and c["tiles_in_use"] == cr["tiles_in_use"]
    for p in (0, 1, P // 2, P - 1):
        assert e.map_extent(p) == ref.map_extent(p)
        for (ca, a), (cb, b) in zip(e.tiles(p), ref.tiles(p)):
            assert ca == cb and np.array_equal(a, b), p
    e.close(); ref.close()


def test_no_trigger_leaves_nobody_out(eng_mod, monkeypatch, log181):
    e, ref = engine_pair(eng_mod, monkeypatch, 32, 181, resample_spread=1e12)
    assert drive(e, ref, log181, 2) == [0, 0]
    same_maps(e, ref, "no trigger")
    assert counts(e) == counts(ref) and e.counters()["map_updates_skipped"] == 0
    e.close(); ref.close()


@pytest.mark.parametrize("call", ["weights", "counters", "save_checkpoint", "set_profiling"])
def test_a_call_in_between_flushes_the_whole_update(eng_mod, monkeypatch, log181, tmp_path, call):
    between = {"weights": lambda x: x.weights(), "counters": lambda x: x.counters(),
               "save_checkpoint": lambda x: x.save_checkpoint(str(tmp_path / "ck.npz")),
               "set_profiling": lambda x: x.set_profiling(True)}[call]
    e, ref = engine_pair(eng_mod, monkeypatch, 32, 181, resample_spread=1.0)
    dead = drive(e, ref, log181, 3, between)
    same_maps(e, ref, call)
    assert sum(dead) > 0 and counts(e) == counts(ref) and e.counters()["map_updates_skipped"] == 0
    e.close(); ref.close()


def test_scan_update_as_the_last_call_updates_the_map(eng_mod, monkeypatch, log181):
    """Against the two halves called on their own, which hold nothing back."""
    e, ref = engine_pair(eng_mod, monkeypatch, 24, 181)
    ang, ranges, odo, _ = log181
    for x in (e, ref):
        x.set_scan(ranges[0], ang)
        x.map_update(np.zeros((x.P, 3)))
        x.imu_update("velocity", odo[0], 1000.0)
        x.set_scan(ranges[1], ang)
    e.scan_update()
    ref.scan_update_begin()
    ref.scan_update_end()
    e.synchronize(); ref.synchronize()
    same_maps(e, ref, "last call")
    same_state(e, ref, "last call")
    assert counts(e) == counts(ref) and e.counters()["scan_updates"] == 2
    e.close(); ref.close()


def test_on_device_history(monkeypatch, log181):
    from thesis_amd import slam
    ang, ranges, odo, _ = log181
    for k in ("RBPF_MAP_KERNEL", "RBPF_EV_RESIDENT", "RBPF_EV_GRID", "RBPF_SKIP_DISCARDED"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RBPF_SKIP_DISCARDED", "1")
    pf = slam.ParticleFilter(32, ang, cell_size=CS, history="device", resample_spread=1.0)
    monkeypatch.setenv("RBPF_SKIP_DISCARDED", "0")
    pr = slam.ParticleFilter(32, ang, cell_size=CS, history="device", resample_spread=1.0)
    monkeypatch.delenv("RBPF_SKIP_DISCARDED")
    for f in (pf, pr):
        f.engine.set_scan(ranges[0], ang)
        f.engine.map_update(np.zeros((32, 3)))
    for k in range(10):
        for f in (pf, pr):
            f.imu_update(odo[k], 1000.0)
            f.map_update(ranges[k + 1])
            f.resample(0.1 + 0.07 * k)
    assert pf.engine.track_info() == pr.engine.track_info() and pf.engine.track_info()["n_records"] >= 20   # an imu and a scan record per step
    (ia, pa), (ib, pb) = pf.engine.lineage(), pr.engine.lineage()
    assert np.array_equal(ia, ib) and np.array_equal(bits(pa), bits(pb))
    ta, tb = pf.engine._track_export(), pr.engine._track_export()          # every record whole: poses, the estimate's row from the weights, parents
    assert np.array_equal(ta["track_state"], tb["track_state"]) and np.array_equal(ta["track_records"], tb["track_records"])
    assert np.array_equal(bits(pf.engine.weights()), bits(pr.engine.weights()))
    assert pf.engine.counters()["map_updates_skipped"] > 0 and pr.engine.counters()["map_updates_skipped"] == 0
    pf.close(); pr.close()
