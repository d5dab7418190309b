"""Scan casting on the GPU (rbpf_cast_scans, kernels_cast.hip) against the scalar oracle of tests/cast_oracle.py run on the
rendered maps: ranges bit for bit, status exactly, for every ray.  Then what the call leaves alone, its device outputs, its
argument checks, and logs simulated in a map (datasets.mapsim)."""
import ctypes as C

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds, room16_cells

pytestmark = pytest.mark.gpu

B = 1081


def engine(P, cs=0.05, **kw):
    from thesis_amd.engine import ParticleEngine
    kw.setdefault("pool_tiles", 8 * P + 16)
    kw.setdefault("max_beams", B)
    return ParticleEngine(P, cell_size=cs, **kw)


def raster(e, box, cells):
    from thesis_amd.mapio import MapRaster
    return MapRaster(x0=int(box[0]), y0=int(box[2]), cell_size=float(e.cfg.cell_size), quantum=float(e.cfg.quantum),
                     dim=e.dim, tile_len=float(e.cfg.tile_len_m), cells=cells)


def load_room16(e, particle=None):
    cells, x0, y0 = room16_cells()
    e.load_map(raster(e, (x0, x0 + cells.shape[0], y0, y0 + cells.shape[1]), cells), particle=particle)
    return cells, x0, y0


def room_poses():
    from thesis_amd.datasets import synthetic
    return np.array(synthetic.circle_trajectory(40)[::8].tolist() + [[1.23, -2.2, 2.5], [-6.1, 6.3, -1.0]])


def oracle(e, p, poses, angles, max_range):
    """The oracle on render_map(p): (ranges [N, B], status [N, B], steps)."""
    m = e.render_map(p)
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    inv = e.dim / float(e.cfg.tile_len_m)
    out = [cast(m.cells, m.x0, m.y0, lo, hi, inv, float(e.cfg.quantum), float(e.cfg.occupied_threshold), q, angles, max_range)
           for q in np.asarray(poses, dtype=np.float64).reshape(-1, 3)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), sum(o[2] for o in out)


def assert_same(got, want, what=""):
    (r, st), (wr, wst) = got, want[:2]
    assert r.shape == wr.shape and st.shape == wst.shape and r.dtype == np.float64 and st.dtype == np.uint8
    bad = (np.ascontiguousarray(r).view(np.uint64) != np.ascontiguousarray(wr).view(np.uint64)) | (st != wst)
    if bad.any():
        k = tuple(int(q) for q in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} rays differ; first {k}: got {r[k]!r} / {st[k]}, "
                             f"oracle {wr[k]!r} / {wst[k]}")


# ---- 4. the exact room ---------------------------------------------------------------------------------------------------------
def test_room16_equals_the_oracle_and_the_analytic_room():
    from thesis_amd.datasets import synthetic
    e = engine(4)
    load_room16(e)
    ang, poses = synthetic.beam_angles(B), room_poses()
    got = e.cast_scans(poses, ang, particle=2, max_range=30.0, return_status=True)
    want = oracle(e, 2, poses, ang, 30.0)
    assert_same(got, want, "room16")
    assert np.all(got[1] == 1)
    ref = np.stack([synthetic.cast_scan(p, ang, None) for p in poses])
    d = np.abs(got[0] - ref)
    print(f"room16: max |cast - analytic| {d.max():.3g} m over {d.size} beams, {want[2] / d.size:.0f} steps per ray")
    assert np.all(d <= 1e-9)
    assert np.array_equal(e.cast_scans(poses[3], ang, particle=0, max_range=30.0), got[0][3:4])     # a single [3] pose
    e.close()


# ---- 5. maps the engine built ----------------------------------------------------------------------------------------------
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
    return e


def test_built_maps_equal_the_oracle():
    from thesis_amd.datasets import synthetic
    e = built_engine()
    P = e.P
    assert e.counters()["resample_copies"] > 0
    maps = [e.render_map(p, box=e.map_extent(None)).cells for p in range(P)]
    assert any(not np.array_equal(maps[0], m) for m in maps[1:])          # the particles hold different maps
    assert any((m > 10).any() for m in maps) and any((m < 0).any() for m in maps) and any(((m > 0) & (m <= 10)).any() for m in maps)
    ang = synthetic.beam_angles(271)
    poses = e.poses()
    got = e.cast_scans(poses, ang, return_status=True)                    # particle=None: pose n in particle n's map
    want_r, want_s = np.empty_like(got[0]), np.empty_like(got[1])
    for p in range(P):
        want_r[p], want_s[p] = (q[0] for q in oracle(e, p, poses[p], ang, float(e.cfg.weight_max_range))[:2])
    assert_same(got, (want_r, want_s), "particle=None")
    rng = np.random.Generator(np.random.PCG64(31))
    k = int(np.argmax(e.weights()))
    fan = poses[k] + rng.normal(0, [1.5, 1.5, 1.0], size=(12, 3))
    for p in (k, (k + 5) % P):
        got = e.cast_scans(fan, ang, particle=p, max_range=8.0, return_status=True)
        assert_same(got, oracle(e, p, fan, ang, 8.0), f"particle={p}")
        assert len(np.unique(got[1])) >= 2                                # hits, and beams that meet nothing within 8 m
    best = e.cast_scans(fan, ang, particle="best", max_range=8.0)
    assert np.array_equal(best, e.cast_scans(fan, ang, particle=k, max_range=8.0))
    e.close()


# ---- 6. geometry that leaves the home tile -----------------------------------------------------------------------------------
def seam_scene(dim, rng):
    """[(box, cells)]: sparse random rasters across the seams of tile (0, 0), at negative coordinates, mid-word offsets."""
    h = dim // 2
    out = []
    for b in [(h - 60, h + 50, h - 45, h + 40),               # the corner shared by four tiles
              (-h - 80, -h + 30, -h - 300, -h - 190),         # negative; the seam X = -h
              (-37, 55, -13, 71),                              # inside the home tile
              (3, 4, -h - 140, -h + 7)]:                       # one row across the seam Y = -h
        c = rng.integers(-30, 11, size=(b[1] - b[0], b[3] - b[2])).astype(np.int8)      # free: <= the threshold (10)
        hit = rng.random(c.shape) < 0.02
        c[hit] = rng.integers(11, 31, size=int(hit.sum())).astype(np.int8)
        out.append((b, c))
    return out


def seam_rays(dim, inv, rng):
    """[(poses, angles, max_range)]: origins over the tiles around (0, 0) - inside and outside the written boxes, and where
    there is no tile - with short, medium and lattice-leaving ranges."""
    h = dim // 2
    def origins(n):
        xy = rng.uniform(-h - 150, h + 150, size=(n, 2)) / inv
        return np.concatenate([xy, rng.uniform(-np.pi, np.pi, size=(n, 1))], axis=1)
    near = origins(10)
    near[:5, :2] = (rng.uniform(h - 70, h + 60, size=(5, 2))) / inv              # around the four-tile corner
    return [(near, rng.uniform(-np.pi, np.pi, 14), 6.0),
            (origins(8), rng.uniform(-np.pi, np.pi, 12), 20.0),
            (origins(4), rng.uniform(-np.pi, np.pi, 10), 500.0)]


@pytest.mark.parametrize("cs", [0.05, 0.1, 0.025])
def test_seams_missing_tiles_and_the_lattice_edge(cs):
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs))))
    e = engine(2, cs=cs, pool_tiles=24, lattice_radius=1)
    assert e.dim == int(round(40 / cs))
    for b, c in seam_scene(e.dim, rng):
        e.load_map(raster(e, b, c), particle=1)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)     # another map, which must not be seen
    inv = e.dim / float(e.cfg.tile_len_m)
    seen, steps, rays = set(), 0, 0
    for poses, ang, mr in seam_rays(e.dim, inv, rng):
        got = e.cast_scans(poses, ang, particle=1, max_range=mr, return_status=True)
        want = oracle(e, 1, poses, ang, mr)
        assert_same(got, want, f"cs {cs}, max_range {mr}")
        assert np.all(got[0][got[1] != 1] == mr)
        seen |= set(np.unique(got[1]).tolist())
        steps, rays = steps + want[2], rays + got[0].size
    print(f"cs {cs}: {rays} rays, {steps / rays:.0f} steps per ray, statuses {sorted(seen)}")
    assert seen == {0, 1, 2}
    e.close()


# ---- 7. thresholds -----------------------------------------------------------------------------------------------------------
def test_threshold_is_strict():
    e = engine(2)
    assert float(e.cfg.occupied_threshold) / float(e.cfg.quantum) == 10.0
    c = np.zeros((12, 3), np.int8)
    c[5] = 10                                            # exactly the threshold: free
    c[7] = -30
    c[9] = 11
    e.load_map(raster(e, (0, 12, -1, 2), c))
    inv = e.dim / float(e.cfg.tile_len_m)
    pose = np.array([[0.5 / inv, 0.5 / inv, 0.0]])
    got = e.cast_scans(pose, [0.0], particle=1, max_range=5.0, return_status=True)
    assert_same(got, oracle(e, 1, pose, [0.0], 5.0), "threshold")
    assert got[0][0, 0] == 8.5 / inv and got[1][0, 0] == 1
    e.close()


# ---- 8. read-only --------------------------------------------------------------------------------------------------------------
def rng_state(e):
    a, b = C.c_uint64(), C.c_uint64()
    e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(a), C.byref(b)))
    return a.value, b.value


def test_a_cast_changes_nothing():
    from thesis_amd.datasets import synthetic
    e = built_engine(P=8, steps=6)
    ang = synthetic.beam_angles(181)

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.render_map(0).cells, e.render_map(5).cells, e.map_extent())

    def same(a, b):
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    s0 = state()
    e.cast_scans(e.poses(), ang)
    e.cast_scans(e.poses() + 0.3, ang, particle=5, max_range=200.0, return_status=True)
    same(state(), s0)
    e.close()


def test_casts_interleaved_in_a_run_change_nothing():
    from thesis_amd.datasets import synthetic
    P, N = 16, 6
    ang, ranges, odo, truth = synthetic.make_log(N + 1, B)
    cang = synthetic.beam_angles(91)
    plain, mixed = engine(P, seed=11), engine(P, seed=11)
    for e in (plain, mixed):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))
    for k in range(N):
        for e in (plain, mixed):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            if e is mixed:
                e.cast_scans(e.poses(), cang)
            e.scan_update(adj=False)
            if e is mixed:
                e.cast_scans(truth[:3], cang, particle=k % P)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)                             # an explicit u: the duplicate groups after it are used by the next match
            if e is mixed:
                e.cast_scans(e.poses(), cang, device=False, return_status=True)
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    assert np.array_equal(mixed.render_map(3, box=box).cells, plain.render_map(3, box=box).cells)
    assert mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    plain.close(); mixed.close()


# ---- 9. device outputs ---------------------------------------------------------------------------------------------------------
def test_device_output_equals_host_output():
    torch = pytest.importorskip("torch")
    from thesis_amd.datasets import synthetic
    e = engine(4)
    load_room16(e)
    ang, poses = synthetic.beam_angles(361), room_poses()
    hr, hs = e.cast_scans(poses, ang, particle=1, max_range=9.0, return_status=True)
    dr, ds = e.cast_scans(poses, ang, particle=1, max_range=9.0, return_status=True, device=True)
    assert isinstance(dr, torch.Tensor) and dr.device.type == "cuda" and dr.dtype == torch.float64 and ds.dtype == torch.uint8
    assert np.array_equal(dr.cpu().numpy().view(np.uint64), hr.view(np.uint64)) and np.array_equal(ds.cpu().numpy(), hs)
    assert len(np.unique(hs)) == 2                       # hits and beams that run out at 9 m
    only = e.cast_scans(poses, ang, particle=1, max_range=9.0, device=True)
    assert torch.equal(only, dr)
    # on a borrowed stream that is torch's current one, no extra synchronisation is needed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = e.cast_scans(poses, ang, particle=1, max_range=9.0, return_status=True, device=True)
        total = d2[0].sum() + d2[1].sum()                # consumed by torch in stream order
        same = torch.equal(d2[0], dr) and torch.equal(d2[1], ds) and float(total) == float(dr.sum() + ds.sum())
        e.release_stream()
    assert same
    e.close()


# ---- 10. arguments -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P, NB = 4, 16
    e = engine(P)
    load_room16(e)
    ang = synthetic.beam_angles(NB)
    poses = np.zeros((P, 3))
    ranges = np.full((P, NB), -7.0)
    status = np.full((P, NB), 9, np.uint8)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(particle=0, ps=poses, n=P, a=ang, nb=NB, mr=30.0, flags=0, r=ranges, s=status):
        return e._lib.rbpf_cast_scans(e._h, particle, dp(ps), n, dp(a), nb, mr, flags, None if r is None else C.c_void_p(r.ctypes.data),
                                      None if s is None else C.c_void_p(s.ctypes.data))
    bad_pose, bad_ang = poses.copy(), ang.copy()
    bad_pose[2, 1] = np.nan
    bad_ang[5] = np.inf
    inf_pose = poses.copy()
    inf_pose[0, 2] = -np.inf
    cases = dict(particle_high=dict(particle=P), particle_low=dict(particle=-2), count=dict(particle=-1, n=P - 1),
                 count_more=dict(particle=-1, ps=np.zeros((P + 1, 3)), n=P + 1), no_ranges=dict(r=None), no_poses=dict(ps=None),
                 no_angles=dict(a=None), range_zero=dict(mr=0.0), range_neg=dict(mr=-1.0), range_inf=dict(mr=np.inf),
                 range_nan=dict(mr=np.nan), nan_pose=dict(ps=bad_pose), inf_theta=dict(ps=inf_pose), inf_angle=dict(a=bad_ang),
                 no_beams=dict(nb=0), neg_poses=dict(n=-1), flags=dict(flags=2))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert np.all(ranges == -7.0) and np.all(status == 9), name
    assert call() == 0 and np.all(status == 1) and np.all(ranges > 0)     # the engine is still usable
    ranges[:] = -7.0
    assert call(s=None) == 0 and np.all(ranges > 0)                       # status may be NULL
    assert call(particle=-1) == 0
    with pytest.raises(ValueError):
        e.cast_scans(np.zeros((2, 4)), ang)
    with pytest.raises(ValueError):
        e.cast_scans(poses, ang, particle="worst")
    # more beams than max_beams, and no scan set: neither matters
    f = engine(2, max_beams=8)
    load_room16(f)
    assert f.cast_scans(np.zeros(3), synthetic.beam_angles(100), particle=0).shape == (1, 100)
    e.close(); f.close()


# ---- 11. logs simulated in a map -----------------------------------------------------------------------------------------------
def test_mapsim_log_in_the_exact_room_equals_the_synthetic_log():
    from thesis_amd.datasets import mapsim, synthetic
    n = 12
    ang, _, odo, truth = synthetic.make_log(n, B)
    e = engine(2)
    load_room16(e, particle=0)
    a, r, o, t = mapsim.make_log(e, 0, synthetic.circle_trajectory(n), ang, noise_sigma=0.0, max_range=synthetic.MAX_RANGE)
    clean = np.stack([synthetic.cast_scan(p, ang, None) for p in truth])
    assert r.shape == clean.shape and np.all(np.abs(r - clean) <= 1e-9)
    assert np.array_equal(o, odo) and np.array_equal(t, truth) and np.array_equal(a, ang)      # equal seeds (the defaults)
    e.close()


# tests/test_gpu_load_map.py, test_localize_in_a_saved_map: its bounds on the best particle's distance from the truth
# (copied, not loosened).  Measured on an MI355X (seeded): 0.074 m / 0.0006 rad here, where the scans come from the built map's
# thick walls; 0.015 m / 0.0003 rad there with the analytic scans.
LOC_TOL_M, LOC_TOL_RAD = 0.1, 0.02


def test_localize_with_a_log_cast_from_a_built_map():
    from thesis_amd.datasets import mapsim, synthetic
    P, N = 256, 40
    ang = synthetic.beam_angles(B)
    truth = synthetic.circle_trajectory(N + 1)
    # the room16 map at the true poses of a whole circle, as test_localize_in_a_saved_map builds it
    full_ang, full_ranges, _, full_truth = synthetic.make_log(380, B, seed=77)
    src = engine(1)
    for k in range(0, 380, 10):
        src.set_scan(full_ranges[k], full_ang)
        src.map_update(full_truth[k:k + 1])
    m = src.render_map(0)
    src.close()
    e = engine(P, seed=5)
    e.load_map(m)
    e.map_updates = False
    _, ranges, odo, _ = mapsim.make_log(e, 0, truth, ang)                 # 41 scans cast from that map, default noise
    clean, st = e.cast_scans(truth, ang, particle=0, return_status=True)
    ref = np.stack([synthetic.cast_scan(p, ang, None) for p in truth])
    d = np.abs(clean - ref)[st == 1]
    print(f"cast in the built map vs the analytic room: {100 * np.mean(st == 1):.2f} % of {st.size} beams hit; of those "
          f"|difference| median {np.median(d):.4f} m, 95 % {np.quantile(d, 0.95):.4f} m, 99.9 % {np.quantile(d, 0.999):.4f} m, max {d.max():.4f} m; "
          f"mean signed {np.mean((clean - ref)[st == 1]):+.4f} m")
    rng = np.random.Generator(np.random.PCG64(17))
    e.set_state(poses=truth[0] + rng.normal(0, [0.2, 0.2, 0.05], size=(P, 3)), weights=1.0)
    for k in range(N):
        e.imu_update("velocity", odo[k], 1000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update(adj=False)
        e.resample()
    best = e.poses()[int(np.argmax(e.weights()))]
    dxy = float(np.hypot(*(best[:2] - truth[N][:2])))
    dth = float(abs((best[2] - truth[N][2] + np.pi) % (2 * np.pi) - np.pi))
    print(f"localization in the cast log: best particle {dxy:.4f} m / {dth:.4f} rad from the truth")
    assert dxy < LOC_TOL_M and dth < LOC_TOL_RAD, (dxy, dth)
    assert np.array_equal(e.render_map(7, box=(m.x0, m.x0 + m.cells.shape[0], m.y0, m.y0 + m.cells.shape[1])).cells, m.cells)
    e.close()
