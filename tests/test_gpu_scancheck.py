"""Scan checks on the GPU (rbpf_check_scans, kernels_scancheck.hip) against the scalar oracle of tests/scancheck_oracle.py run on
the rendered maps: cost, counts, classes and votes exactly, for every ray.  Then what the call leaves alone, its device outputs,
its argument checks, and what it is for (thesis_amd/sensor.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import scancheck_oracle as so
from tests import scancheck_scenes as sc
from tests.cast_oracle import lattice_bounds

pytestmark = pytest.mark.gpu

B = 1081
KEYS = ("cost", "counts", "classes", "votes")


def engine(P, cs=0.05, **kw):
    from thesis_amd.engine import ParticleEngine
    kw.setdefault("pool_tiles", 8 * P + 16)
    kw.setdefault("max_beams", B)
    return ParticleEngine(P, cell_size=cs, **kw)


def raster(e, box, cells):
    from thesis_amd.mapio import MapRaster
    return MapRaster(x0=int(box[0]), y0=int(box[2]), cell_size=float(e.cfg.cell_size), quantum=float(e.cfg.quantum),
                     dim=e.dim, tile_len=float(e.cfg.tile_len_m), cells=cells)


def load_room(e, patch=True, particle=None):
    cells, x0, y0 = sc.known_room(patch)
    e.load_map(raster(e, (x0, x0 + cells.shape[0], y0, y0 + cells.shape[1]), cells), particle=particle)


def rendered(e, particles):
    """{p: (cells, x0, y0)} of render_map(p)."""
    out = {}
    for p in particles:
        m = e.render_map(p)
        out[p] = (m.cells, m.x0, m.y0)
    return out


def oracle(e, maps, poses, angles, ranges, max_range, min_range, tol, model):
    """tests/scancheck_oracle.check on rendered maps: maps(n) -> (cells, x0, y0) of the map pose n is checked in."""
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    return so.check(maps, lo, hi, e.dim / float(e.cfg.tile_len_m), float(e.cfg.quantum), float(e.cfg.occupied_threshold), poses, angles,
                    ranges, max_range, min_range, tol, model)


def assert_same(chk, want, what=""):
    got = dict(cost=chk.cost, counts=chk.counts, classes=chk.classes, votes=chk.votes)
    for k, dt in zip(KEYS, (np.int64, np.int32, np.uint8, np.int32)):
        g, w = got[k], want[k]
        assert g.dtype == dt and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = g != w
        if bad.any():
            i = tuple(int(q) for q in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {k} differs at {int(bad.sum())} of {bad.size} places; first {i}: got {g[i]}, oracle {w[i]}")


# ---- 1. the exact room, every class ------------------------------------------------------------------------------------------
BEST = 4                                 # the particle whose map holds the blocker, and the heaviest one


@pytest.fixture(scope="module")
def room():
    """Eight particles with the known room; particle BEST also holds the blocker and carries the most weight."""
    e = engine(8)
    load_room(e)
    x0, x1, y0, y1 = sc.BLOCKER_BOX
    e.load_map(raster(e, sc.BLOCKER_BOX, np.full((x1 - x0, y1 - y0), 30, np.int8)), particle=BEST)
    w = e.weights()
    w[BEST] += 1.0
    e.set_state(weights=w)
    maps = rendered(e, range(8))
    assert not np.array_equal(maps[BEST][0], maps[2][0]) and all(np.array_equal(maps[p][0], maps[2][0]) for p in (0, 1, 3, 5, 6, 7))
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    yield dict(e=e, maps=maps, lo=lo, hi=hi, model=sc.narrow_model())
    e.close()


@pytest.mark.parametrize("nb", sc.B_CASES)
def test_room_equals_the_oracle_in_every_class(room, nb):
    from thesis_amd.datasets import synthetic
    e, maps, model = room["e"], room["maps"], room["model"]
    assert e.dim / float(e.cfg.tile_len_m) == sc.INV and model.half_bins < sc.TOL * sc.INV * model.bins_per_cell
    ang = synthetic.beam_angles(nb)
    poses, paired = sc.all_poses(), sc.paired_poses()
    z = sc.measured_ranges(sc.true_ranges(*maps[2], room["lo"], room["hi"], poses, ang))
    zp = sc.measured_ranges(sc.true_ranges(*maps[2], room["lo"], room["hi"], paired, ang))
    kw = dict(max_range=sc.MAX_RANGE, min_range=sc.MIN_RANGE, tol=sc.TOL, model=model)
    okw = (sc.MAX_RANGE, sc.MIN_RANGE, sc.TOL, model)
    want = oracle(e, lambda n: maps[2], poses, ang, z, *okw)
    if nb >= 64:                         # the condition on the scene, on the oracle's output (tests/test_scancheck_oracle.py has it on the CPU)
        assert set(np.unique(want["classes"]).tolist()) == set(range(8))
        raw = so.raw_bins(want["d"], model)[want["classes"] == so.MATCH]
        assert (raw > model.half_bins).any() and (raw < -model.half_bins).any()
    full = dict(return_classes=True, return_votes=True)
    assert_same(e.check_scans(poses, z, ang, particle=2, **kw, **full), want, f"B {nb}, particle 2, a scan per pose")
    assert_same(e.check_scans(poses, z[1], ang, particle=2, **kw, **full), oracle(e, lambda n: maps[2], poses, ang, z[1], *okw),
                f"B {nb}, particle 2, one scan")
    assert_same(e.check_scans(poses, z, ang, particle="best", **kw, **full), oracle(e, lambda n: maps[BEST], poses, ang, z, *okw),
                f"B {nb}, best, a scan per pose")
    assert_same(e.check_scans(poses, z[3], ang, particle="best", **kw, **full), oracle(e, lambda n: maps[BEST], poses, ang, z[3], *okw),
                f"B {nb}, best, one scan")
    assert_same(e.check_scans(paired, zp, ang, particle=None, **kw, **full), oracle(e, lambda n: maps[n], paired, ang, zp, *okw),
                f"B {nb}, particle None, a scan per pose")
    assert_same(e.check_scans(paired, zp[0], ang, **kw, **full), oracle(e, lambda n: maps[n], paired, ang, zp[0], *okw),
                f"B {nb}, particle None, one scan")
    # cost and counts alone, and a single [3] pose with a [B] scan
    bare = e.check_scans(poses, z, ang, particle=2, **kw)
    assert bare.classes is None and bare.votes is None and np.array_equal(bare.cost, want["cost"]) and np.array_equal(bare.counts, want["counts"])
    one = e.check_scans(poses[5], z[5], ang, particle=2, return_classes=True, **kw)
    assert np.array_equal(one.classes, want["classes"][5:6]) and one.cost[0] == want["cost"][5]


def test_default_tolerance_and_model(room):
    from thesis_amd import sensor
    from thesis_amd.datasets import synthetic
    e, maps = room["e"], room["maps"]
    ang = synthetic.beam_angles(64)
    poses = sc.room_poses()
    z = sc.measured_ranges(sc.true_ranges(*maps[2], room["lo"], room["hi"], poses, ang), max_range=float(e.cfg.weight_max_range), min_range=0.0)
    got = e.check_scans(poses, z, ang, particle=2, return_classes=True, return_votes=True)
    model = sensor.beam_model(e.cfg)
    assert got.scale == model.scale == 65536
    assert_same(got, oracle(e, lambda n: maps[2], poses, ang, z, float(e.cfg.weight_max_range), 0.0, 2 * float(e.cfg.cell_size), model), "defaults")


# ---- 2. maps the engine built ----------------------------------------------------------------------------------------------------
def built_engine(P=16, steps=20, seed=11):
    from thesis_amd.datasets import synthetic
    ang, ranges, odo, truth = synthetic.make_log(steps + 1, B)
    e = engine(P, seed=seed)
    e.set_scan(ranges[0], ang)
    e.map_update(np.zeros((P, 3)))
    for k in range(steps):
        e.imu_update("velocity", odo[k], 1000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update(adj=False)
        if k in (5, 12):                                 # past the resample trigger: tiles are copied
            w = e.weights()
            w[1 + k % 3] += 250.0
            e.set_state(weights=w)
        e.resample()
    return e, ang, ranges[steps]


def test_built_maps_equal_the_oracle():
    from thesis_amd import sensor
    e, ang, scan = built_engine()
    P = e.P
    assert e.counters()["resample_copies"] > 0
    ang, scan = ang[::4], scan[::4]                       # every fourth beam of the current scan: 271, what the oracle walks in a second
    model = sensor.beam_model(e.cfg)
    full = dict(return_classes=True, return_votes=True)
    maps = rendered(e, range(P))
    assert any(not np.array_equal(maps[0][0], maps[p][0]) or maps[0][1:] != maps[p][1:] for p in range(1, P))
    poses = e.poses()
    mr, tol = float(e.cfg.weight_max_range), 2 * float(e.cfg.cell_size)
    want = oracle(e, lambda n: maps[n], poses, ang, scan, mr, 0.0, tol, model)
    assert_same(e.check_scans(poses, scan, ang, **full), want, "the current scan at every particle's pose")
    seen = set(np.unique(want["classes"]).tolist())
    rng = np.random.Generator(np.random.PCG64(31))
    k = int(np.argmax(e.weights()))
    fan = poses[k] + rng.normal(0, [1.5, 1.5, 1.0], size=(12, 3))
    noisy = e.cast_scans(fan, ang, particle=k, max_range=30.0) + rng.normal(0, 0.05, size=(12, len(ang)))
    noisy[:, 100:140] -= 1.5
    noisy[rng.random(noisy.shape) < 0.02] = np.inf
    for p in (k, (k + 5) % P):
        for z, what in ((scan, "the current scan"), (noisy, "a scan per pose")):
            want = oracle(e, lambda n: maps[p], fan, ang, z, 8.0, 0.2, tol, model)
            assert_same(e.check_scans(fan, z, ang, particle=p, max_range=8.0, min_range=0.2, **full), want, f"particle {p}, {what}")
            seen |= set(np.unique(want["classes"]).tolist())
    print("classes met in the built maps:", sorted(seen))
    assert {so.SHORT, so.NEW} <= seen and seen & {so.MISSING, so.CLEAR}
    e.close()


# ---- 3. what the call leaves alone -------------------------------------------------------------------------------------------------
def rng_state(e):
    a, b = C.c_uint64(), C.c_uint64()
    e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(a), C.byref(b)))
    return a.value, b.value


def test_a_check_changes_nothing():
    e, ang, scan = built_engine(P=8, steps=6)

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.render_map(0).cells, e.render_map(5).cells, e.map_extent())

    def same(a, b):
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    s0 = state()
    e.check_scans(e.poses(), scan, ang, return_classes=True, return_votes=True)
    e.check_scans(e.poses() + 0.3, scan[::6], ang[::6], particle=5, max_range=200.0, tol=0.5)
    same(state(), s0)
    e.close()


def test_checks_interleaved_in_a_run_change_nothing():
    from thesis_amd.datasets import synthetic
    P, N = 8, 6
    ang, ranges, odo, truth = synthetic.make_log(N + 1, B)
    plain, mixed = engine(P, seed=11), engine(P, seed=11)
    for e in (plain, mixed):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))
    for k in range(N):
        for e in (plain, mixed):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            if e is mixed:
                e.check_scans(e.poses(), ranges[k + 1], ang, return_votes=True)
            e.scan_update(adj=False)
            if e is mixed:
                e.check_scans(truth[:3], ranges[k + 1][::4], ang[::4], particle=k % P, return_classes=True)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)
            if e is mixed:
                e.check_scans(e.poses(), ranges[k + 1], ang)
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    assert rng_state(mixed) == rng_state(plain)
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    for p in (0, 3):
        assert np.array_equal(mixed.render_map(p, box=box).cells, plain.render_map(p, box=box).cells)
    assert mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    plain.close(); mixed.close()


# ---- 4. device outputs ---------------------------------------------------------------------------------------------------------------
def test_device_output_equals_host_output(room):
    torch = pytest.importorskip("torch")
    from thesis_amd.datasets import synthetic
    e, maps = room["e"], room["maps"]
    ang, poses = synthetic.beam_angles(361), sc.all_poses()
    z = sc.measured_ranges(sc.true_ranges(*maps[2], room["lo"], room["hi"], poses, ang))
    kw = dict(particle=1, max_range=sc.MAX_RANGE, min_range=sc.MIN_RANGE, model=room["model"], return_classes=True, return_votes=True)
    host = e.check_scans(poses, z, ang, **kw)
    dev = e.check_scans(poses, z, ang, device=True, **kw)
    again = e.check_scans(poses, z, ang, device=True, **kw)
    for k, dt in zip(KEYS, (torch.int64, torch.int32, torch.uint8, torch.int32)):
        d = getattr(dev, k)
        assert isinstance(d, torch.Tensor) and d.device.type == "cuda" and d.dtype == dt
        assert np.array_equal(d.cpu().numpy(), getattr(host, k)), k
        assert torch.equal(d, getattr(again, k)), k                       # two calls, identical bits
    assert len(np.unique(host.classes)) == 8
    assert np.array_equal(dev.matched(), host.matched()) and np.array_equal(dev.log_likelihood(), host.log_likelihood())
    bare = e.check_scans(poses, z[0], ang, device=True, particle=1, max_range=sc.MAX_RANGE, model=room["model"])
    assert bare.classes is None and bare.votes is None and bare.cost.shape == (len(poses),) and bare.counts.shape == (len(poses), 8)
    h2 = e.check_scans(poses, z[0], ang, particle=1, max_range=sc.MAX_RANGE, model=room["model"])
    assert np.array_equal(bare.cost.cpu().numpy(), h2.cost) and np.array_equal(bare.counts.cpu().numpy(), h2.counts)


# ---- 5. arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P, NB, HB = 4, 16, 3
    e = engine(P)
    load_room(e)
    ang = synthetic.beam_angles(NB)
    poses = np.zeros((P, 3))
    z = np.full((P, NB), 2.0)
    hit, cc = np.arange(2 * HB + 1, dtype=np.int32), np.arange(8, dtype=np.int32)
    cost, counts = np.full(P, -7, np.int64), np.full((P, 8), -7, np.int32)
    classes, votes = np.full((P, NB), 99, np.uint8), np.full((NB, 8), -7, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(particle=0, ps=poses, n=P, r=z, ns=P, a=ang, nb=NB, mr=30.0, mn=0.0, tol=0.1, ht=hit, hb=HB, bpc=4, c8=cc, flags=0, co=cost,
             cn=counts, cl=classes, vo=votes):
        return e._lib.rbpf_check_scans(e._h, particle, dp(ps), n, dp(r), ns, dp(a), nb, mr, mn, tol, ip(ht), hb, bpc, ip(c8), flags,
                                       vp(co), vp(cn), vp(cl), vp(vo))

    def untouched():
        return np.all(cost == -7) and np.all(counts == -7) and np.all(classes == 99) and np.all(votes == -7)
    bad_pose, inf_pose, bad_ang = poses.copy(), poses.copy(), ang.copy()
    bad_pose[2, 1] = np.nan
    inf_pose[0, 2] = -np.inf
    bad_ang[5] = np.inf
    neg_hit, big_hit, neg_cc, big_cc = hit.copy(), hit.copy(), cc.copy(), cc.copy()
    neg_hit[2 * HB], big_hit[0], neg_cc[7], big_cc[3] = -1, (1 << 20) + 1, -1, (1 << 20) + 1
    cases = dict(no_poses=dict(ps=None), no_ranges=dict(r=None), no_angles=dict(a=None), no_hit_tab=dict(ht=None), no_class_cost=dict(c8=None),
                 no_cost=dict(co=None), nan_pose=dict(ps=bad_pose), inf_theta=dict(ps=inf_pose), inf_angle=dict(a=bad_ang),
                 max_zero=dict(mr=0.0), max_neg=dict(mr=-1.0), max_inf=dict(mr=np.inf), max_nan=dict(mr=np.nan),
                 min_neg=dict(mn=-0.1), min_inf=dict(mn=np.inf), min_nan=dict(mn=np.nan),
                 tol_neg=dict(tol=-0.1), tol_inf=dict(tol=np.inf), tol_nan=dict(tol=np.nan),
                 half_bins_zero=dict(hb=0), half_bins_neg=dict(hb=-1), half_bins_high=dict(hb=4097),
                 bins_zero=dict(bpc=0), bins_high=dict(bpc=65), hit_neg=dict(ht=neg_hit), hit_big=dict(ht=big_hit),
                 class_neg=dict(c8=neg_cc), class_big=dict(c8=big_cc),
                 scans_two=dict(ns=2), scans_zero=dict(ns=0), scans_more=dict(ns=P + 1),
                 particle_high=dict(particle=P), particle_low=dict(particle=-2), count=dict(particle=-1, n=P - 1, ns=P - 1),
                 count_more=dict(particle=-1, ps=np.zeros((P + 1, 3)), n=P + 1, ns=1), no_beams=dict(nb=0), no_pose=dict(n=0, ns=1),
                 neg_poses=dict(n=-1, ns=-1), too_many_rays=dict(n=1 << 16, ns=1, nb=1 << 15), flags=dict(flags=2))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert untouched(), name
    # between the two halves of a scan update the maps are in flux
    e.set_scan(synthetic.cast_scan((0.0, 0.0, 0.0), synthetic.beam_angles(B), None), synthetic.beam_angles(B))
    e.scan_update_begin(adj=False)
    assert call() == _lib.RBPF_ESTATE and call(particle=-1) == _lib.RBPF_ESTATE and untouched()
    e.scan_update_end()
    assert call() == 0 and np.all(cost >= 0) and np.all(counts.sum(axis=1) == NB) and np.all(classes < 8) and np.all(votes.sum(axis=1) == P)
    cost[:] = -7; counts[:] = -7; classes[:] = 99; votes[:] = -7
    assert call(cn=None, cl=None, vo=None) == 0 and np.all(cost >= 0) and np.all(counts == -7) and np.all(classes == 99) and np.all(votes == -7)
    assert call(particle=-1, ns=1) == 0 and call(particle=-1) == 0
    with pytest.raises(ValueError):
        e.check_scans(np.zeros((2, 4)), z[0], ang)
    with pytest.raises(ValueError):
        e.check_scans(poses, z[:2], ang, particle=0)
    with pytest.raises(ValueError):
        e.check_scans(poses, z, ang, particle="worst")
    # more beams than max_beams, and no scan set: neither matters
    f = engine(2, max_beams=8)
    load_room(f)
    assert f.check_scans(np.zeros(3), np.full(100, 3.0), synthetic.beam_angles(100), particle=0).counts.sum() == 100
    e.close(); f.close()


# ---- 6. what it is for ---------------------------------------------------------------------------------------------------------------
def test_dynamic_beams_posterior_weights_and_lost():
    from thesis_amd import sensor
    from thesis_amd.datasets import synthetic
    nb = 271
    e = engine(4)
    load_room(e, patch=False)
    ang = synthetic.beam_angles(nb)
    true_pose = np.array([1.23, -2.2, 2.5])
    scan = synthetic.cast_scan(true_pose, ang, np.random.Generator(np.random.PCG64(3)))
    assert scan[100:140].min() > 2.0
    scan[100:140] -= 1.5                                  # somebody stands in the room
    moved = np.zeros(nb, bool)
    moved[100:140] = True
    chk = e.check_scans(true_pose, scan, ang, particle=0, max_range=30.0, return_classes=True, return_votes=True)
    assert np.array_equal(sensor.dynamic_beams(chk), moved)
    assert np.all(chk.classes[0][~moved] == sensor.MATCH) and chk.matched()[0] == (nb - 40) / nb
    r, a = sensor.keep(scan, ang, sensor.dynamic_beams(chk))
    assert len(r) == nb - 40 and e.check_scans(true_pose, r, a, particle=0, max_range=30.0).matched()[0] == 1.0
    # the true pose among seven displaced ones, chosen with the oracle: its cost is strictly the least
    room_map = rendered(e, [0])[0]
    model = sensor.beam_model(e.cfg)
    okw = (30.0, 0.0, 2 * float(e.cfg.cell_size), model)
    rng = np.random.Generator(np.random.PCG64(4))
    cost_true = oracle(e, lambda n: room_map, true_pose, ang, scan, *okw)["cost"][0]
    others = []
    for cand in true_pose + rng.normal(0, [0.4, 0.4, 0.15], size=(40, 3)):
        if len(others) < 7 and oracle(e, lambda n: room_map, cand, ang, scan, *okw)["cost"][0] > cost_true:
            others.append(cand)
    assert len(others) == 7
    poses = np.array(others[:3] + [true_pose] + others[3:])
    chk = e.check_scans(poses, scan, ang, particle=0, max_range=30.0, return_classes=True, return_votes=True)
    want = oracle(e, lambda n: room_map, poses, ang, scan, *okw)
    assert_same(chk, want, "the true pose among displaced ones")
    w = sensor.posterior_weights(chk)
    assert int(np.argmax(w)) == 3 and abs(w.sum() - 1.0) < 1e-12 and np.all(w[np.arange(8) != 3] < w[3])
    assert int(np.argmax(chk.log_likelihood())) == 3
    assert not sensor.lost(chk, weights=w)
    # from the wrong corner of the room the map does not explain the scan
    wrong = e.check_scans(np.array([-6.0, 6.0, -0.5]), scan, ang, particle=0, max_range=30.0)
    assert wrong.matched()[0] < 0.5 and sensor.lost(wrong)
    e.close()
