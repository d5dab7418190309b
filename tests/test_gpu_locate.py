"""Global localization on the GPU (rbpf_locate_scan, kernels_locate.hip) against the NumPy oracle of tests/locate_oracle.py
run on the rendered maps: both rasters bit for bit.  Then what the call leaves alone, its device outputs, its argument checks,
handle lifetimes, and a filter that starts anywhere in a loaded map (ParticleEngine.relocalize).

End to end, measured on an MI355X (seeded; weighted mean pose after 40 scans against the truth): started at the true pose
0.0358 m / 0.00069 rad; relocalized from the first scan 0.0354 m / 0.00074 rad (bounds: the former plus one cell, 0.05 m, and
one rotation step, 0.0087 rad)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.locate_oracle import asym_room, locate

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


def load_room(e, particle=None):
    cells, x0, y0 = asym_room(float(e.cfg.cell_size))
    e.load_map(raster(e, (x0, x0 + cells.shape[0], y0, y0 + cells.shape[1]), cells), particle=particle)
    return (x0, x0 + cells.shape[0], y0, y0 + cells.shape[1])


def oracle(e, p, box, ranges, angles, n_rot):
    """The oracle on render_map(p): (best, rot)."""
    m = e.render_map(p)
    c = e.cfg
    return locate(m.cells, m.x0, m.y0, box, ranges, angles, n_rot, e.dim / float(c.tile_len_m), float(c.quantum),
                  float(c.occupied_threshold), float(c.match_min_range), float(c.match_max_range))[:2]


def assert_same(got, want, what=""):
    for name, g, w in zip(("best", "rot"), got, want):
        assert g.shape == w.shape and g.dtype == np.int32, (what, name, g.shape, w.shape, g.dtype)
        bad = g != w
        if bad.any():
            k = tuple(int(q) for q in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {name} differs in {int(bad.sum())} of {bad.size} cells; first {k}: got {g[k]}, oracle {w[k]}")


def scan_at(e, p, pose, angles):
    return e.cast_scans(np.asarray(pose, dtype=np.float64), angles, particle=p, max_range=30.0)[0]


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_loaded_room_equals_the_oracle(cs):
    from thesis_amd.datasets import synthetic
    e = engine(2, cs=cs)
    full = load_room(e, particle=1)
    assert e.dim == int(round(40 / cs)) and e.map_extent(1) == full
    n = full[1] - full[0]
    ang = synthetic.beam_angles(181)
    r = scan_at(e, 1, (2.17, -3.36, 2.0), ang)
    assert (r >= 11.0).any() and ((r > 0) & (r < 11.0)).any()            # beams beyond match_max_range are in the scan
    r[[0, 50]] = 0.0                                                      # and beams at 0
    r[60] = float(e.cfg.match_max_range)                                  # exactly the bound: unused
    inner = (full[0] + n // 4, full[0] + n // 4 + 70, full[2] + n // 3, full[2] + n // 3 + 45)       # end points leave the box
    beyond = (full[1] - n // 4, full[1] + 40, -37, 30)                                                 # partly where nothing was loaded
    for box, n_rot in ((inner, 360), (inner, 1), (beyond, 7), (full if cs == 0.1 else inner, 720 if cs == 0.05 else 360)):
        got = e.locate_scan(r, ang, particle=1, box=box, n_rot=n_rot)
        assert got[2] == tuple(box)
        assert_same(got[:2], oracle(e, 1, box, r, ang, n_rot), f"cs {cs}, box {box}, n_rot {n_rot}")
        assert (got[0] >= 0).any() and got[0].max() <= 2 * int(np.sum((r > 1e-3) & (r < 11.0)))
        assert np.array_equal(got[0] < 0, got[1] < 0)
    got = e.locate_scan(r, ang, particle=1, box=beyond, n_rot=7)
    assert np.all(got[0][n // 4:] == -1) and np.all(got[1][n // 4:] == -1) and (got[0][:n // 4] >= 0).any()     # beyond the raster: unknown
    # box=None is the map's extent; particle 0 has no map: no candidate anywhere
    assert e.locate_scan(r, ang, particle=1, n_rot=1)[2] == full
    b0, r0, _ = e.locate_scan(r, ang, particle=0, box=inner, n_rot=3)
    assert np.all(b0 == -1) and np.all(r0 == -1)
    # one beam; no used beam
    for rr, aa in ((np.array([3.0]), np.array([0.7])), (np.array([0.0, 30.0, 11.0, 1e-3]), np.zeros(4))):
        got = e.locate_scan(rr, aa, particle=1, box=inner, n_rot=7)
        assert_same(got[:2], oracle(e, 1, inner, rr, aa, 7), f"cs {cs}, {len(rr)} beams")
    assert set(np.unique(got[0]).tolist()) <= {-1, 0} and set(np.unique(got[1]).tolist()) <= {-1, 0} and (got[0] == 0).any()
    e.close()


def test_full_room_1081_beams_720_rotations():
    from thesis_amd.datasets import synthetic
    e = engine(1)
    full = load_room(e)
    ang = synthetic.beam_angles(B)
    r = scan_at(e, 0, (-3.05, 5.52, -1.2), ang)
    best, rot, box = e.locate_scan(r, ang, particle=0, n_rot=720)
    assert box == full
    for x, y in ((-200 + 37, -200 + 51), (-32, -32), (40, 75)):           # a corner with wall and unknown space, the centre, block A
        sub = (x, x + 64, y, y + 64)
        cut = (best[x - full[0]:x - full[0] + 64, y - full[2]:y - full[2] + 64], rot[x - full[0]:x - full[0] + 64, y - full[2]:y - full[2] + 64])
        assert_same(cut, oracle(e, 0, sub, r, ang, 720), f"sub-box {sub} of the full box")
        assert_same(e.locate_scan(r, ang, particle=0, box=sub, n_rot=720)[:2], cut, f"sub-box {sub} alone")
    from thesis_amd.locate import hypotheses
    h = hypotheses(best, rot, box, 720, 0.05, k=1)
    assert abs(h.poses[0, 0] + 3.05) <= 0.075 and abs(h.poses[0, 1] - 5.52) <= 0.075
    e.close()


def built_engine(P=3, steps=30, seed=11):
    """Maps built by `steps` scan updates of the synthetic log: threshold cells, ragged written boxes, unknown space inside."""
    from thesis_amd.datasets import synthetic
    ang, ranges, odo, truth = synthetic.make_log(steps + 1, B)
    e = engine(P, seed=seed)
    e.set_scan(ranges[0], ang)
    e.map_update(np.zeros((P, 3)))
    for k in range(steps):
        e.imu_update("velocity", odo[k], 1000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update(adj=False)
    return e, ang, ranges, truth


def test_built_maps_equal_the_oracle():
    from thesis_amd.datasets import synthetic
    e, ang, ranges, truth = built_engine()
    maps = [e.render_map(p, box=e.map_extent(None)).cells for p in range(e.P)]
    assert any(not np.array_equal(maps[0], m) for m in maps[1:])          # the particles hold different maps
    assert all((m > 10).any() and (m < 0).any() and ((m > 0) & (m <= 10)).any() and (m == 0).any() for m in maps)
    a181 = synthetic.beam_angles(181)
    r = synthetic.cast_scan(truth[17], a181)
    ext = e.map_extent(2)
    box = (-70, 40, -55, 66)
    got = e.locate_scan(r, a181, particle=2, box=box, n_rot=360)
    assert_same(got[:2], oracle(e, 2, box, r, a181, 360), "built map, particle 2")
    assert not np.array_equal(got[0], e.locate_scan(r, a181, particle=0, box=box, n_rot=360)[0])     # particle 0's map gives another answer
    edge = (ext[0] - 20, ext[0] + 50, ext[2] - 20, ext[2] + 60)           # over the ragged rim of the written box
    assert_same(e.locate_scan(ranges[5], ang, particle=1, box=edge, n_rot=7)[:2], oracle(e, 1, edge, ranges[5], ang, 7), "built map, rim")
    e.close()


def seam_maps(e, rng):
    """Random rasters across the seams of tile (0, 0) and at negative coordinates: free, occupied and threshold cells."""
    h = e.dim // 2
    boxes = [(h - 60, h + 50, h - 45, h + 40), (-h - 80, -h + 30, -h - 70, -h + 45), (-37, 55, -13, 71)]
    for b in boxes:
        c = rng.integers(-30, 11, size=(b[1] - b[0], b[3] - b[2])).astype(np.int8)
        hit = rng.random(c.shape) < 0.04
        c[hit] = rng.integers(11, 31, size=int(hit.sum())).astype(np.int8)
        e.load_map(raster(e, b, c), particle=1)
    return boxes


@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_seams_and_negative_coordinates(cs):
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs)) + 1))
    e = engine(2, cs=cs, pool_tiles=24, lattice_radius=1)
    boxes = seam_maps(e, rng)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)     # another map, which must not be seen
    h = e.dim // 2
    inv = e.dim / float(e.cfg.tile_len_m)
    ang = rng.uniform(-np.pi, np.pi, 181)
    r = rng.uniform(0.0, 140.0 / inv, 181)               # end points up to 140 cells away: over the seams into the other rasters
    r[:8] = rng.uniform(10.5, 12.0, 8)                   # around match_max_range
    for box, n_rot in (((-h - 50, -h + 45, -h - 40, -h + 50), 7), (boxes[0], 360), ((h - 20, h + 13, h - 33, h + 31), 720)):
        got = e.locate_scan(r, ang, particle=1, box=box, n_rot=n_rot)
        assert_same(got[:2], oracle(e, 1, box, r, ang, n_rot), f"cs {cs}, box {box}, n_rot {n_rot}")
        assert (got[0] > 0).any() and (got[0] == -1).any()
    # the lattice's last cells
    lo = -e.dim - h
    corner = (lo, lo + 40, lo, lo + 33)
    assert_same(e.locate_scan(r, ang, particle=1, box=corner, n_rot=7)[:2], oracle(e, 1, corner, r, ang, 7), "lattice corner")
    e.close()


# ---- 2. 0.025 m -------------------------------------------------------------------------------------------------------------------
def test_cell_size_0025():
    rng = np.random.Generator(np.random.PCG64(25))
    e = engine(2, cs=0.025, pool_tiles=24, lattice_radius=1)
    seam_maps(e, rng)
    h = e.dim // 2
    ang = rng.uniform(-np.pi, np.pi, 181)
    r = rng.uniform(0.0, 3.0, 181)
    r[:40] = rng.uniform(9.0, 11.5, 40)                  # offsets up to 440 cells
    box = (h - 40, h + 24, h - 30, h + 37)
    got = e.locate_scan(r, ang, particle=1, box=box, n_rot=360)
    assert_same(got[:2], oracle(e, 1, box, r, ang, 360), "0.025 m")
    assert (got[0] > 0).any()
    e.close()


# ---- 3. read-only -------------------------------------------------------------------------------------------------------------------
def rng_state(e):
    a, b = C.c_uint64(), C.c_uint64()
    e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(a), C.byref(b)))
    return a.value, b.value


def test_a_search_changes_nothing():
    from thesis_amd.datasets import synthetic
    e, ang, ranges, truth = built_engine(P=3, steps=8)

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.map_extent()) + tuple(e.render_map(p, box=e.map_extent()).cells for p in range(3))

    def same(a, b):
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    s0 = state()
    a = e.locate_scan(ranges[3], ang, particle=2, n_rot=90)
    b = e.locate_scan(ranges[3], ang, particle=2, n_rot=90)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    e.locate_scan(ranges[4], ang, particle="best", box=(-30, 30, -30, 30), n_rot=12)
    same(state(), s0)
    e.close()


def test_searches_interleaved_in_a_run_change_nothing():
    from thesis_amd.datasets import synthetic
    P, N = 16, 6
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
                e.locate_scan(ranges[k], ang, particle=k % P, n_rot=16)
            e.scan_update(adj=False)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)                             # an explicit u: the duplicate groups after it are used by the next match
            if e is mixed:
                e.locate_scan(ranges[k + 1], ang, particle="best", box=(-40, 40, -40, 40), n_rot=8)
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    assert np.array_equal(mixed.render_map(3, box=box).cells, plain.render_map(3, box=box).cells)
    assert mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    assert rng_state(mixed) == rng_state(plain)
    plain.close(); mixed.close()


# ---- 4. device outputs --------------------------------------------------------------------------------------------------------------
def test_device_output_equals_host_output():
    torch = pytest.importorskip("torch")
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    e = engine(2)
    load_room(e)
    ang = synthetic.beam_angles(361)
    r = scan_at(e, 1, (5.71, 1.13, 3.0), ang)
    box = (-150, -63, 20, 121)
    hb, hr, _ = e.locate_scan(r, ang, particle=1, box=box, n_rot=45)
    db, dr, dbox = e.locate_scan(r, ang, particle=1, box=box, n_rot=45, device=True)
    assert isinstance(db, torch.Tensor) and db.device.type == "cuda" and db.dtype == torch.int32 and dr.dtype == torch.int32 and dbox == box
    assert np.array_equal(db.cpu().numpy(), hb) and np.array_equal(dr.cpu().numpy(), hr)
    # a poisoned buffer: nothing outside [x1-x0][y1-y0] is written
    n, pad = hb.size, 96
    bufs = [torch.full((n + 2 * pad,), -77, dtype=torch.int32, device=db.device) for _ in range(2)]
    torch.cuda.synchronize()
    b4 = np.array(box, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = e._lib.rbpf_locate_scan(e._h, 1, b4.ctypes.data_as(C.POINTER(C.c_int32)), dp(r), dp(ang), len(r), 45, _lib.RBPF_LOCATE_DEVICE_OUT,
                                 C.c_void_p(bufs[0].data_ptr() + 4 * pad), C.c_void_p(bufs[1].data_ptr() + 4 * pad))
    assert rc == 0
    e.synchronize()
    for t, want in zip(bufs, (hb, hr)):
        t = t.cpu().numpy()
        assert np.all(t[:pad] == -77) and np.all(t[-pad:] == -77) and np.array_equal(t[pad:-pad].reshape(want.shape), want)
    # on a borrowed stream that is torch's current one, no extra synchronisation is needed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = e.locate_scan(r, ang, particle=1, box=box, n_rot=45, device=True)
        total = d2[0].sum() + d2[1].sum()                # consumed by torch in stream order
        same = torch.equal(d2[0], db) and torch.equal(d2[1], dr) and int(total) == int(hb.sum() + hr.sum())
        e.release_stream()
    assert same
    e.close()


# ---- 5. arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P, NB = 3, 16
    e = engine(P, lattice_radius=1)
    load_room(e)
    ang = synthetic.beam_angles(NB)
    rng_r = np.linspace(1.0, 6.0, NB)
    box = np.array([-20, 10, -8, 12], dtype=np.int32)
    best = np.full((30, 20), -7, np.int32)
    rot = np.full((30, 20), -9, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(particle=0, b=box, r=rng_r, a=ang, nb=NB, n_rot=8, flags=0, o=best, q=rot):
        return e._lib.rbpf_locate_scan(e._h, particle, None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)), dp(r), dp(a), nb, n_rot,
                                       flags, vp(o), vp(q))
    def with_(arr, k, val):
        out = arr.copy()
        out[k] = val
        return out
    edge = e.dim + e.dim // 2                            # lattice_radius 1: mosaic cells [-edge, edge)
    i32 = lambda *b: np.array(b, dtype=np.int32)
    cases = dict(particle_high=dict(particle=P), particle_all=dict(particle=-1), particle_low=dict(particle=-2), no_box=dict(b=None),
                 no_ranges=dict(r=None), no_angles=dict(a=None), no_best=dict(o=None), nan_range=dict(r=with_(rng_r, 3, np.nan)),
                 inf_range=dict(r=with_(rng_r, 0, np.inf)), nan_angle=dict(a=with_(ang, 15, np.nan)), inf_angle=dict(a=with_(ang, 5, -np.inf)),
                 no_beams=dict(nb=0), neg_beams=dict(nb=-1), many_beams=dict(nb=16385), no_rot=dict(n_rot=0), neg_rot=dict(n_rot=-3),
                 many_rot=dict(n_rot=4097), flags=dict(flags=2), flags_high=dict(flags=1 << 31), box_x=dict(b=i32(10, -20, -8, 12)),
                 box_y=dict(b=i32(-20, 10, 12, -8)), box_left=dict(b=i32(-edge - 1, -edge + 29, -8, 12)),
                 box_right=dict(b=i32(edge - 29, edge + 1, -8, 12)), box_top=dict(b=i32(-20, 10, edge - 19, edge + 1)),
                 box_huge=dict(b=i32(-2 ** 30, 2 ** 30, -2 ** 30, 2 ** 30)))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert np.all(best == -7) and np.all(rot == -9), name
    # between the two halves of a scan update
    e.set_scan(np.full(NB, 3.0), ang)
    e.scan_update_begin(adj=False)
    assert call() == _lib.RBPF_ESTATE and np.all(best == -7) and np.all(rot == -9)
    e.scan_update_end()
    assert call() == 0 and (best >= 0).any() and np.array_equal(best < 0, rot < 0)                 # the engine is still usable
    want = best.copy()
    best[:] = -7
    rot[:] = -9
    assert call(q=None) == 0 and np.array_equal(best, want) and np.all(rot == -9)                  # rot may be NULL
    assert call(b=i32(-edge, -edge + 30, edge - 20, edge)) == 0 and np.all(best == -1)             # the lattice's corner: allowed, unexplored
    assert call(b=i32(4, 4, -8, 12)) == 0                                                          # an empty box is no error
    with pytest.raises(ValueError):
        e.locate_scan(rng_r, ang[:5], particle=0)
    with pytest.raises(ValueError):
        e.locate_scan(rng_r, ang, particle="worst")
    e.close()


# ---- 6. handles come and go ---------------------------------------------------------------------------------------------------------
def test_handles_come_and_go():
    torch = pytest.importorskip("torch")
    from thesis_amd.datasets import synthetic
    ang = synthetic.beam_angles(91)
    first = None
    for k in range(6):
        e = engine(2, pool_tiles=16)
        load_room(e)
        s = torch.cuda.Stream() if k % 2 else None
        if s is not None:
            e.set_stream(s.cuda_stream)
        r = scan_at(e, 0, (0.33, 0.41, 0.3), ang)
        got = e.locate_scan(r, ang, particle=k % 2, box=(-60 - 40 * (k % 3), 30, -50, 45 + 30 * (k % 2)), n_rot=30 + 7 * k)     # the scratch grows
        got = e.locate_scan(r, ang, particle=k % 2, box=(-60, 30, -50, 45), n_rot=30)
        if first is None:
            first = got
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
        if k % 3 == 0:
            e.locate_scan(r, ang, particle=0, box=(-60, 30, -50, 45), n_rot=30, device=True)       # still queued when the handle goes
        if s is not None and k != 3:
            e.release_stream()
        e.close()


# ---- 7. start anywhere ----------------------------------------------------------------------------------------------------------------
def mean_pose_error(e, truth):
    p, w = e.poses(), e.weights()
    w = w / w.sum()
    x, y = float(w @ p[:, 0]), float(w @ p[:, 1])
    th = math.atan2(float(w @ np.sin(p[:, 2])), float(w @ np.cos(p[:, 2])))
    return math.hypot(x - truth[0], y - truth[1]), abs((th - truth[2] + math.pi) % (2 * math.pi) - math.pi)


def test_start_anywhere_in_a_loaded_map():
    from thesis_amd.datasets import mapsim, synthetic
    from tests.test_locate_oracle import POSES, AMBIGUOUS, pose_error
    P, N, n_rot, cell = 256, 40, 720, 0.05
    ang = synthetic.beam_angles(B)
    truth = synthetic.circle_trajectory(N) + np.array([0.33, 0.41, 0.0])      # block A lies ahead to the left, 5.7 m away
    errs = {}
    for how in ("known", "relocalized"):
        e = engine(P, seed=5)
        full = load_room(e)
        e.map_updates = False
        before = e.render_map(7, box=full).cells
        _, ranges, odo, _ = mapsim.make_log(e, 0, truth, ang)             # 41 scans cast from the map, default noise
        if how == "known":
            e.set_state(poses=truth[0], covs=0.0, weights=1.0)
        else:
            assert np.all(e.poses() == 0.0)                               # the filter knows nothing of truth[0]
            h = e.relocalize(ranges[0], ang, particle=0, k=8, n_rot=n_rot, seed=0)
            d = [pose_error(c, truth[0], cell, n_rot) for c in h.cells]
            print(f"hypotheses: scores {h.scores.tolist()} of at most {2 * h.n_used}; the first is {d[0][0]:.2f} cells / {d[0][1]:.2f} steps from the truth")
            assert d[0][0] <= 1.5 and d[0][1] <= 1.5 and h.scores[0] > h.scores[1]
            assert e.counters()["scan_updates"] == 0
        for k in range(N):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            e.scan_update(adj=False)
            e.resample()
        errs[how] = mean_pose_error(e, truth[N])
        assert np.array_equal(e.render_map(7, box=full).cells, before)    # localization: the maps stay as they are
        # from a corner only the two walls are in view: the truth is one of several equally good hypotheses
        if how == "relocalized":
            pose = POSES[AMBIGUOUS]
            r = scan_at(e, 0, pose, ang)
            h = e.relocalize(r, ang, particle=0, k=8, n_rot=n_rot, seed=1)
            d = [pose_error(c, pose, cell, n_rot) for c in h.cells]
            print(f"corner pose: scores {h.scores.tolist()}, distances {[round(q[0], 1) for q in d]} cells")
            assert any(q[0] <= 1.5 and q[1] <= 1.5 for q in d)
            assert np.array_equal(e.render_map(3, box=full).cells, before)
        e.close()
    (d0, t0), (d1, t1) = errs["known"], errs["relocalized"]
    print(f"weighted mean pose after {N} scans: known start {d0:.4f} m / {t0:.5f} rad, relocalized {d1:.4f} m / {t1:.5f} rad")
    assert d1 <= d0 + cell and t1 <= t0 + 2 * math.pi / n_rot, (errs)
