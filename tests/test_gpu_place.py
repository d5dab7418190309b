"""Map placement on the GPU (rbpf_place_map, kernels_place.hip) against the NumPy oracle of
tests/place_oracle.py: the warped and covered rasters bit for bit, every cell; the three merge modes on particles that hold
different maps; the state derived from the cells; argument checks that write nothing; the dry run that changes nothing; device
inputs and outputs; and a room written as another tool's map (0.03 m cells, rotated, off both grids) that a filter then
relocalizes in.

End to end (seeded; top hypothesis of relocalize against the true pose (2.17, -3.36, 2.0)): the errors in the directly loaded
room and in the placed foreign map are printed by the test; no MI355X run has recorded them yet (bound: the former plus one
destination cell diagonal and one source cell diagonal, 0.1131 m, and one rotation step, 0.0087 rad)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import place_oracle as po
from tests.locate_oracle import asym_room

pytestmark = pytest.mark.gpu

B = 1081
MODES = {"replace": po.REPLACE, "known": po.KNOWN, "add": po.ADD}


def engine(P, cs=0.05, **kw):
    from thesis_amd.engine import ParticleEngine
    kw.setdefault("pool_tiles", 8 * P + 16)
    kw.setdefault("max_beams", B)
    return ParticleEngine(P, cell_size=cs, **kw)


def raster(e, box, cells):
    from thesis_amd.mapio import MapRaster
    return MapRaster(x0=int(box[0]), y0=int(box[2]), cell_size=float(e.cfg.cell_size), quantum=float(e.cfg.quantum),
                     dim=e.dim, tile_len=float(e.cfg.tile_len_m), cells=cells)


def source(cells, cell, origin):
    from thesis_amd.mapio import SourceMap
    return SourceMap(cells=cells, cell_size=cell, origin=tuple(float(v) for v in origin), quantum=0.1)


def cell_of(e):
    return float(e.cfg.tile_len_m) / e.dim


def oracle(e, src, box, S):
    return po.warp(src.cells, src.cell_size, src.origin, box, cell_of(e), S)


def render(e, p, box):
    return e.render_map(p, box=box).cells


def grow(box, m):
    return (box[0] - m, box[1] + m, box[2] - m, box[3] + m)


def assert_same(got, want, what):
    for name, g, w in zip(("warped", "covered"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype)
        bad = g != w
        if bad.any():
            k = tuple(int(q) for q in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {name} differs in {int(bad.sum())} of {bad.size} cells; first {k}: got {g[k]}, oracle {w[k]}")


def rand_source(rng, shape, zeros=0.0):
    c = rng.integers(-30, 31, size=shape).astype(np.int8)
    if zeros:
        c[rng.random(shape) < zeros] = 0
    return c


def rng_state(e):
    a, b = C.c_uint64(), C.c_uint64()
    e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(a), C.byref(b)))
    return a.value, b.value


# ---- 1. the oracle sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_warp_equals_the_oracle(cs):
    from thesis_amd.mapio import placed_box
    e = engine(1, cs=cs, pool_tiles=4)
    assert e.dim == int(round(40 / cs)) and (e.dim % 32 == 0) == (cs == 0.05)      # 0.1 m: dim 400, a tile row ends in half an occupancy word
    cell, seam = cell_of(e), e.dim // 2                                              # tile (0, 0) ends at mosaic cell dim / 2
    n = 0
    for iy, yaw in enumerate((0.0, 0.3, math.pi / 2, -2.5)):
        for ir, ratio in enumerate((0.5, 1.0, 1.37, 2.0, 4.0)):
            rng = np.random.Generator(np.random.PCG64(100 * iy + ir))
            shape = (int(round(60 / ratio)) + 7, int(round(80 / ratio)) + 3)       # a footprint of about 60 x 80 cells
            # off both grids, the centre of the footprint on the corner of tile (0, 0): it lies across both seams whatever the yaw
            hx, hy = shape[0] * ratio * cell / 2, shape[1] * ratio * cell / 2
            origin = (seam * cell + 0.0123 - (math.cos(yaw) * hx - math.sin(yaw) * hy),
                      seam * cell - 0.0071 - (math.sin(yaw) * hx + math.cos(yaw) * hy), yaw)
            src = source(rand_source(rng, shape), ratio * cell, origin)
            foot = placed_box(src, cell, e.dim, 3)
            assert foot[0] < seam < foot[1] and foot[2] < seam < foot[3]
            mid = ((foot[0] + foot[1]) // 2, (foot[2] + foot[3]) // 2)
            boxes = [grow(foot, 5),                                                  # sticks out of the footprint on every side
                     (mid[0] - 3, mid[0] + 14, mid[1] - 17, mid[1] + 2),              # inside it (for small yaw), odd offsets
                     (foot[0] - 40, foot[0] + 1, foot[3] - 2, foot[3] + 33),          # touches a corner of it at most
                     (-100, -61, -300, -283),                                         # misses it entirely
                     (mid[0], mid[0] + 1, mid[1], mid[1] + 1)]                        # 1 x 1
            for S in (1, 2, 3, 8):
                for box in boxes:
                    w, c, b = e.warp_map(src, box=box, samples=S)
                    assert b == tuple(box)
                    assert_same((w, c), oracle(e, src, box, S), f"cs {cs}, yaw {yaw:.2f}, ratio {ratio}, S {S}, box {box}")
                    n += 1
                w, c, _ = e.warp_map(src, box=boxes[3], samples=S)
                assert not c.any() and not w.any()
            w, c, b = e.warp_map(src)                                                # the defaults: placed_box and S from the ratio
            S = min(8, max(2, math.ceil(2 * cell / src.cell_size)))
            assert b == foot
            assert_same((w, c), oracle(e, src, foot, S), f"cs {cs}, yaw {yaw:.2f}, ratio {ratio}, defaults")
            assert c.any() and (yaw in (0.0, math.pi / 2) or not c.all())
    assert n == 4 * 5 * 4 * 5
    assert e.counters()["tiles_in_use"] == 1 and e.map_extent() is None             # nothing was written
    e.close()


def test_warp_of_a_large_rotated_map():
    rng = np.random.Generator(np.random.PCG64(77))
    e = engine(1, pool_tiles=4)
    src = source(rand_source(rng, (700, 650)), 0.03, (-9.224998, -11.224998, 0.3))
    box = (-330, 310, -250, 420)                                                   # across four tiles, wider than two 256-column blocks
    got = e.warp_map(src, box=box, samples=2)
    assert_same(got[:2], oracle(e, src, box, 2), "large map")
    assert got[1].any() and not got[1].all()
    e.close()


# ---- 2. against existing code --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_on_grid_replace_equals_load(cs):
    from thesis_amd.mapio import source_from_raster
    rng = np.random.Generator(np.random.PCG64(31))
    P = 3
    A, Bq = engine(P, cs=cs), engine(P, cs=cs)
    h = A.dim // 2
    big = (-h - 60, h + 90, -3 * h - 30, h + 320)
    for b, S in (((h - 20, h + 30, h - 45, h + 19), None), ((-h - 37, -h + 5, -3 * h - 11, -h + 300), 1), ((5, 6, 7, 8), 3),
                 ((-61, -41, -h + 17, -h + 62), 8)):
        r = raster(A, b, rand_source(rng, (b[1] - b[0], b[3] - b[2])))
        A.load_map(r)
        assert Bq.place_map(source_from_raster(r), box=b, samples=S) == b
        # the default box holds the raster; where floor() of an origin such as -0.7000000000000001 / 0.1 adds a row, it is not covered
        d = Bq.place_map(source_from_raster(r), samples=S)
        assert d[0] <= b[0] and d[1] >= b[1] and d[2] <= b[2] and d[3] >= b[3] and d[1] - d[0] <= b[1] - b[0] + 2
    for p in range(P):
        assert np.array_equal(render(A, p, big), render(Bq, p, big)), p
    assert A.counters()["tiles_in_use"] == Bq.counters()["tiles_in_use"]
    A.close(); Bq.close()


def test_round_trips_between_cell_sizes():
    from thesis_amd.mapio import source_from_raster
    rng = np.random.Generator(np.random.PCG64(32))
    coarse, fine = engine(2, cs=0.1), engine(2, cs=0.05)
    # 0.1 m -> 0.05 m: every cell twice on both axes
    b = (150, 260, -231, -160)                                                     # across the seam of the coarse lattice at 200
    c = rand_source(rng, (b[1] - b[0], b[3] - b[2]))
    coarse.load_map(raster(coarse, b, c), particle=1)
    m = coarse.render_map(1)
    assert (m.x0, m.y0) == (b[0], b[2]) and np.array_equal(m.cells, c)
    fine.place_map(source_from_raster(m), particle=0)
    b2 = tuple(2 * v for v in b)
    assert np.array_equal(render(fine, 0, b2), np.repeat(np.repeat(c, 2, axis=0), 2, axis=1))
    out = render(fine, 0, grow(b2, 8))
    out[8:-8, 8:-8] = 0
    assert not out.any() and not render(fine, 1, grow(b2, 8)).any()
    # 0.05 m -> 0.1 m: the maximum of every 2 x 2 block
    b = (340, 460, -90, 38)                                                        # across the seam of the fine lattice at 400; even corners
    c = rand_source(rng, (b[1] - b[0], b[3] - b[2]))
    fine.load_map(raster(fine, b, c), particle=1)
    m = fine.render_map(1)
    coarse.place_map(source_from_raster(m), particle=0)
    b2 = tuple(v // 2 for v in b)
    assert np.array_equal(render(coarse, 0, b2), c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).max(axis=(1, 3)))
    coarse.close(); fine.close()


# ---- 3. modes, 4. derived state -------------------------------------------------------------------------------------------------------
def built_engine(P=4, steps=6, seed=11, cs=0.05):
    """Maps built by scan updates of the synthetic log: the particles hold different maps with saturated cells of both signs."""
    from thesis_amd.datasets import synthetic
    ang, ranges, odo, truth = synthetic.make_log(steps + 1, B)
    e = engine(P, cs=cs, seed=seed)
    e.set_scan(ranges[0], ang)
    for _ in range(12):                                   # twelve updates at the origin: walls reach +30, the floor -30
        e.map_update(np.zeros((P, 3)))
    for k in range(steps):
        e.imu_update("velocity", odo[k], 1000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update(adj=False)
    return e, ang, ranges, truth


@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_modes_merge_with_each_particles_own_map(cs):
    from thesis_amd.datasets import synthetic
    e, ang, ranges, truth = built_engine(cs=cs)
    P = e.P
    ext = e.map_extent(None)
    view = grow(ext, 60)
    maps = [render(e, p, view) for p in range(P)]
    assert any(not np.array_equal(maps[0], m) for m in maps[1:])
    assert all((m == 30).any() and (m == -30).any() for m in maps)
    rng = np.random.Generator(np.random.PCG64(41))
    cell = cell_of(e)
    vmin, vmax = -30, 30
    for k, (mode, yaw, sc) in enumerate((("replace", 0.3, 0.03), ("known", -2.5, 1.37 * cell), ("add", 0.7, 0.08), ("add", 0.0, cell))):
        n = int(14.0 / sc)
        src = source(rand_source(rng, (n, n + 9), zeros=0.3), sc, (-7.013 * math.cos(yaw) + 7.2 * math.sin(yaw) + 1.0, -7.013 * math.sin(yaw) - 7.2 * math.cos(yaw), yaw))
        box = (view[0] + 20 + k, view[1] - 31, view[2] + 17, view[3] - 25 - k)    # part of the old map lies outside the box
        S = 2 + k % 2
        before = [render(e, p, view) for p in range(P)]
        tiles0 = e.counters()["tiles_in_use"]
        wrp, cov = oracle(e, src, box, S)
        assert cov.any() and not cov.all() and ((wrp == 0) & (cov == 1)).any()
        assert e.place_map(src, box=box, samples=S, mode=mode) == box
        sl = (slice(box[0] - view[0], box[1] - view[0]), slice(box[2] - view[2], box[3] - view[2]))
        sat_hi = sat_lo = False
        for p in range(P):
            want = before[p].copy()
            want[sl] = po.merge(before[p][sl], wrp, cov, MODES[mode], vmin, vmax)
            got = render(e, p, view)
            bad = got != want
            assert not bad.any(), (mode, p, int(bad.sum()), [int(q) for q in np.argwhere(bad)[0]])
            s = before[p][sl].astype(np.int16) + wrp
            sat_hi |= bool(((s > vmax) & (cov == 1)).any())
            sat_lo |= bool(((s < vmin) & (cov == 1)).any())
        if mode == "add":
            assert sat_hi and sat_lo                      # the sum left the range at both ends and was clamped
        assert e.counters()["tiles_in_use"] >= tiles0
        ext = (min(ext[0], box[0]), max(ext[1], box[1]), min(ext[2], box[2]), max(ext[3], box[3]))
        assert e.map_extent(None) == ext                  # written boxes: the old ones and the box
    # one particle alone: the others keep their maps
    before = [render(e, p, view) for p in range(P)]
    src = source(rand_source(rng, (90, 120)), 0.04, (-2.0, -3.0, 1.1))
    box = e.place_map(src, particle=2, mode="add")
    wrp, cov = oracle(e, src, box, min(8, max(2, math.ceil(2 * cell / 0.04))))
    sl = (slice(box[0] - view[0], box[1] - view[0]), slice(box[2] - view[2], box[3] - view[2]))
    for p in range(P):
        want = before[p].copy()
        if p == 2:
            want[sl] = po.merge(before[p][sl], wrp, cov, po.ADD, vmin, vmax)
        assert np.array_equal(render(e, p, view), want), p

    # ---- 4. the state derived from the cells: a twin that loads the rendered result ----
    twin = engine(P, cs=cs, seed=11)
    for p in range(P):
        pe = e.map_extent(p)
        twin.load_map(raster(twin, pe, render(e, p, pe)), particle=p)
        assert twin.map_extent(p) == pe
    assert twin.map_extent(None) == e.map_extent(None)
    poses = truth[3] + np.random.Generator(np.random.PCG64(42)).normal(0, [0.5, 0.5, 0.3], size=(P, 3))
    a181 = synthetic.beam_angles(181)
    ra, sa = e.cast_scans(poses, a181, return_status=True)
    rb, sb = twin.cast_scans(poses, a181, return_status=True)
    assert np.array_equal(ra, rb) and np.array_equal(sa, sb) and (sa == 1).any()
    pts = np.random.Generator(np.random.PCG64(43)).uniform(-12, 12, size=(4000, 2))
    for x in (e, twin):
        x.set_scan(ranges[4], ang)
    for p in range(P):
        va, na = e.get_odds_at(p, pts)
        vb, nb = twin.get_odds_at(p, pts)
        assert np.array_equal(na, nb) and np.array_equal(va[~na], vb[~nb])
        ca, fa = e.match_inputs(p, poses[p])
        cb, fb = twin.match_inputs(p, poses[p])
        assert np.array_equal(ca, cb) and np.array_equal(fa, fb) and len(fa) > 0
    e.close(); twin.close()


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    import torch
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    rng = np.random.Generator(np.random.PCG64(8))
    P = 4
    e = engine(P, pool_tiles=7, lattice_radius=1)                       # every particle starts with its centre tile: 3 free
    b0 = (-30, 40, -20, 25)
    e.load_map(raster(e, b0, rand_source(rng, (70, 45))), particle=0)
    edge = e.dim + e.dim // 2                                           # lattice_radius 1: mosaic cells [-edge, edge)
    full = (-edge, edge, -edge, edge)

    def state():
        return e.counters()["tiles_in_use"], e.map_extent(None), [render(e, p, full) for p in range(P)]

    def same(a, b):
        assert a[0] == b[0] and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))

    s0 = state()
    assert s0[0] == P
    good = rand_source(rng, (40, 50))
    pose = np.array([-0.613, 0.277, 0.3])
    box = np.array([-20, 10, -8, 12], dtype=np.int32)
    wrp = np.full((30, 20), -7, np.int8)
    cov = np.full((30, 20), 9, np.uint8)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    i32 = lambda *b: np.array(b, dtype=np.int32)

    def call(particle=1, b=box, src=good, nsx=40, nsy=50, sc=0.03, ps=pose, S=2, mode=0, flags=0, w=wrp, c=cov):
        return e._lib.rbpf_place_map(e._h, particle, None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)), vp(src), nsx, nsy, sc,
                                     None if ps is None else ps.ctypes.data_as(C.POINTER(C.c_double)), S, mode, flags, vp(w), vp(c))

    def with_(arr, k, val):
        out = arr.copy()
        out[k] = val
        return out
    DRY = _lib.RBPF_PLACE_DRY
    cases = dict(no_box=dict(b=None), no_src=dict(src=None), no_pose=dict(ps=None), nsx_0=dict(nsx=0), nsy_neg=dict(nsy=-1),
                 src_huge=dict(nsx=65536, nsy=32768), box_huge=dict(b=i32(-2 ** 30, 2 ** 30, -2 ** 30, 2 ** 30)),
                 box_left=dict(b=i32(-edge - 1, -edge + 29, -8, 12)), box_right=dict(b=i32(edge - 29, edge + 1, -8, 12)),
                 box_top=dict(b=i32(-20, 10, edge - 19, edge + 1)), box_x=dict(b=i32(10, -20, -8, 12)), box_y=dict(b=i32(-20, 10, 12, -8)),
                 nan_x=dict(ps=with_(pose, 0, np.nan)), inf_y=dict(ps=with_(pose, 1, np.inf)), nan_yaw=dict(ps=with_(pose, 2, np.nan)),
                 cell_0=dict(sc=0.0), cell_neg=dict(sc=-0.03), cell_nan=dict(sc=float("nan")), cell_inf=dict(sc=float("inf")),
                 samples_0=dict(S=0), samples_9=dict(S=9), samples_neg=dict(S=-2), mode_3=dict(mode=3), mode_neg=dict(mode=-1),
                 flags_8=dict(flags=8), flags_high=dict(flags=1 << 31), particle_high=dict(particle=P), particle_low=dict(particle=-2),
                 value_high=dict(src=with_(good, (3, 4), 31)), value_low=dict(src=with_(good, (39, 49), -31)),
                 dry_without_outputs=dict(flags=DRY, w=None, c=None))
    for name, kw in cases.items():
        for extra in (0, DRY):
            if extra and name in ("particle_high", "particle_low"):
                continue                                                # a dry run ignores the particle
            k2 = dict(kw)
            k2["flags"] = k2.get("flags", 0) | extra
            assert call(**k2) == _lib.RBPF_EINVAL, (name, extra)
            assert np.all(wrp == -7) and np.all(cov == 9), name
    same(state(), s0)
    # a device source with one bad value: found on the device, nothing written; one particle, every particle, a dry run
    bad = torch.from_numpy(with_(good, (17, 3), -31)).to("cuda:0")
    torch.cuda.synchronize()
    for kw in (dict(particle=1), dict(particle=-1), dict(flags=DRY)):
        rc = e._lib.rbpf_place_map(e._h, kw.get("particle", 0), box.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(bad.data_ptr()), 40, 50, 0.03,
                                   pose.ctypes.data_as(C.POINTER(C.c_double)), 2, 0, _lib.RBPF_PLACE_DEVICE_IN | kw.get("flags", 0), vp(wrp), vp(cov))
        assert rc == _lib.RBPF_EINVAL, kw
        assert np.all(wrp == -7) and np.all(cov == 9), kw
    same(state(), s0)
    from thesis_amd.engine import RbpfError
    with pytest.raises(RbpfError) as ei:
        e.place_map(source(bad, 0.03, pose))
    assert ei.value.code == _lib.RBPF_EINVAL
    same(state(), s0)
    # too few free tiles: one lattice position per particle is missing, 4 in all, 3 are free
    big = i32(-30, 40, e.dim // 2 - 20, e.dim // 2 + 30)
    assert call(particle=-1, b=big, w=None, c=None) == _lib.RBPF_ENOMEM
    msg = e._lib.rbpf_last_error(e._h).decode()
    assert "needs 4 free tiles, the pool has 3" in msg, msg
    same(state(), s0)
    assert call(particle=-1, b=big, flags=DRY, w=None, c=np.zeros((70, 50), np.uint8)) == 0          # a dry run needs no tile
    # between the two halves of a scan update
    ang = synthetic.beam_angles(B)
    e.set_scan(synthetic.cast_scan((0, 0, 0), ang), ang)
    e.scan_update_begin()
    assert call() == _lib.RBPF_ESTATE and call(flags=DRY) == _lib.RBPF_ESTATE
    assert np.all(wrp == -7) and np.all(cov == 9)
    e.scan_update_end()
    # the engine is still usable; warped / covered may each be NULL; an empty box is no error
    s1 = state()
    assert call(flags=DRY, c=None) == 0 and np.all(cov == 9) and not np.all(wrp == -7)
    want = po.warp(good, 0.03, pose, tuple(box), cell_of(e), 2)
    assert np.array_equal(wrp, want[0])
    assert call(flags=DRY, w=None) == 0 and np.array_equal(cov, want[1])
    assert call(b=i32(4, 4, -8, 12)) == 0 and call(b=i32(4, 4, -8, 12), flags=DRY) == 0
    same(state(), s1)
    wrp[:] = -7
    assert call(particle=3) == 0 and np.array_equal(wrp, want[0]) and np.array_equal(cov, want[1])   # a real placement returns them too
    got = render(e, 3, tuple(box))
    assert np.array_equal(got, po.merge(s1[2][3][box[0] + edge:box[1] + edge, box[2] + edge:box[3] + edge], want[0], want[1], po.REPLACE, -30, 30))
    # Python-side refusals
    with pytest.raises(ValueError, match="mode"):
        e.place_map(source(good, 0.03, pose), mode="max")
    with pytest.raises(ValueError, match="quantum"):
        from thesis_amd.mapio import SourceMap
        e.place_map(SourceMap(cells=good, cell_size=0.03, origin=(0.0, 0.0, 0.0), quantum=0.05))
    with pytest.raises(ValueError):
        e.warp_map(source(good[0], 0.03, pose))
    e.close()


def test_the_lattice_corner_is_allowed():
    e = engine(2, pool_tiles=8, lattice_radius=1)
    edge = e.dim + e.dim // 2
    rng = np.random.Generator(np.random.PCG64(9))
    src = source(rand_source(rng, (80, 80)), 0.03, ((edge - 30) * 0.05 + 0.011, (-edge) * 0.05 - 0.7, 0.2))
    box = (edge - 33, edge, -edge, -edge + 41)
    assert e.place_map(src, particle=1, box=box, samples=3) == box
    w, c = oracle(e, src, box, 3)
    assert c.any() and np.array_equal(render(e, 1, box), po.merge(np.zeros_like(w), w, c, po.REPLACE, -30, 30))
    assert e.counters()["tiles_in_use"] == 3
    e.close()


# ---- 6. the dry run changes nothing; a placement dissolves duplicate groups ------------------------------------------------------------
def test_a_dry_run_changes_nothing():
    e, ang, ranges, truth = built_engine(P=3, steps=4)
    rng = np.random.Generator(np.random.PCG64(61))

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.map_extent()) + tuple(e.render_map(p, box=grow(e.map_extent(), 30)).cells for p in range(3))

    def same(a, b):
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    s0 = state()
    src = source(rand_source(rng, (300, 280)), 0.03, (-4.0, -5.0, 0.3))
    a = e.warp_map(src)
    b = e.warp_map(src)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[1].any()
    e.warp_map(src, box=(-900, -700, 850, 1000), samples=8)                # where no particle has a tile
    same(state(), s0)
    e.close()


def test_dry_runs_keep_duplicate_groups_and_a_placement_dissolves_them():
    from thesis_amd.datasets import synthetic
    P = 32
    ang, ranges, odo, truth = synthetic.make_log(5, B)
    rng = np.random.Generator(np.random.PCG64(62))
    src = source(rand_source(rng, (200, 200)), 0.03, (-3.0, -3.0, 0.4))
    plain, mixed = engine(P, seed=3), engine(P, seed=3)
    for e in (plain, mixed):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))

    def step(e, k):
        e.imu_update("velocity", odo[k], 1000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update(adj=False)
        w = e.weights()
        w[5] += 250.0
        e.set_state(weights=w)
        did, idx = e.resample(0.3)
        assert did and len(set(idx.tolist())) < P        # duplicates exist
    shared = []
    for k in range(3):
        for e in (plain, mixed):
            step(e, k)
            if e is mixed:
                e.warp_map(src)                          # between the resample and the next match
                e.warp_map(src, box=(-50, 60, -40, 30), samples=1)
        shared.append(plain.counters()["match_shared"])
        assert mixed.counters()["match_shared"] == shared[-1]
    assert shared[2] > shared[1] > shared[0]             # the duplicates shared their match, with dry runs in between or not
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    assert rng_state(mixed) == rng_state(plain)
    # a real placement into one particle: the next matcher runs once per particle
    mixed.place_map(src, particle=int(np.argmax(mixed.weights())), mode="known")
    s1 = mixed.counters()["match_shared"]
    mixed.imu_update("velocity", odo[3], 1000.0)
    mixed.set_scan(ranges[4], ang)
    mixed.scan_update(adj=False)
    assert mixed.counters()["match_shared"] == s1
    plain.close(); mixed.close()


# ---- 7. device inputs and outputs ------------------------------------------------------------------------------------------------------
def test_device_input_and_output_equal_host():
    import torch
    from thesis_amd import _lib
    rng = np.random.Generator(np.random.PCG64(71))
    e = engine(4)
    cells = rand_source(rng, (260, 310), zeros=0.2)
    pose = (-3.224998, 14.775002, -0.9)
    hs, ds = source(cells, 0.03, pose), source(torch.from_numpy(cells).to("cuda:0"), 0.03, pose)
    box = (-80, 120, 330, 470)                                          # across the seam at 400
    hw, hc, _ = e.warp_map(hs, box=box, samples=3)
    assert hc.any() and not hc.all()
    for s_in in (hs, ds):
        for dev in (False, True):
            w, c, b = e.warp_map(s_in, box=box, samples=3, device=dev)
            if dev:
                assert isinstance(w, torch.Tensor) and w.device.type == "cuda" and w.dtype == torch.int8 and c.dtype == torch.uint8
                w, c = w.cpu().numpy(), c.cpu().numpy()
            assert b == box and np.array_equal(w, hw) and np.array_equal(c, hc)
    # a poisoned buffer: nothing outside [x1-x0][y1-y0] is written
    n, pad = hw.size, 96
    bufs = [torch.full((n + 2 * pad,), 55, dtype=dt, device="cuda:0") for dt in (torch.int8, torch.uint8)]
    torch.cuda.synchronize()
    b4, p3 = np.array(box, dtype=np.int32), np.array(pose)
    rc = e._lib.rbpf_place_map(e._h, 0, b4.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(ds.cells.data_ptr()), 260, 310, 0.03,
                               p3.ctypes.data_as(C.POINTER(C.c_double)), 3, 0,
                               _lib.RBPF_PLACE_DEVICE_IN | _lib.RBPF_PLACE_DEVICE_OUT | _lib.RBPF_PLACE_DRY,
                               C.c_void_p(bufs[0].data_ptr() + pad), C.c_void_p(bufs[1].data_ptr() + pad))
    assert rc == 0
    e.synchronize()
    for t, want in zip(bufs, (hw, hc)):
        t = t.cpu().numpy()
        assert np.all(t[:pad] == 55) and np.all(t[-pad:] == 55) and np.array_equal(t[pad:-pad].reshape(want.shape), want)
    # placement: a device source leaves what a host source leaves
    e.place_map(hs, particle=0, box=box, samples=3, mode="known")
    e.place_map(ds, particle=2, box=box, samples=3, mode="known")
    view = grow(box, 20)
    r0 = render(e, 0, view)
    assert r0.any() and np.array_equal(render(e, 2, view), r0) and not render(e, 1, view).any()
    f = engine(4)
    f.place_map(ds, box=box, samples=3, mode="known")
    for p in range(4):
        assert np.array_equal(render(f, p, view), r0)
    # on a borrowed stream that is torch's current one, no extra synchronisation is needed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        f.set_stream(s.cuda_stream)
        t = torch.from_numpy(cells).to("cuda:0", non_blocking=False) + 0          # produced on the stream
        w, c, _ = f.warp_map(source(t, 0.03, pose), box=box, samples=3, device=True)
        total = int(w.to(torch.int64).sum() + c.to(torch.int64).sum())            # consumed by torch in stream order
        f.release_stream()
    assert total == int(hw.astype(np.int64).sum() + hc.astype(np.int64).sum())
    e.close(); f.close()


# ---- 8. end to end: a room written as another tool's map ---------------------------------------------------------------------------------
def write_foreign_map(stem, cells, cell, origin):
    """Trinary PGM + YAML of int8 cells [i][j] (+30 occupied, -30 free, 0 unknown), as map tools write them."""
    pix = np.full(cells.shape, 205, np.uint8)
    pix[cells > 0] = 0
    pix[cells < 0] = 254
    img = np.ascontiguousarray(pix.T[::-1, :])
    with open(stem + ".pgm", "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())
    with open(stem + ".yaml", "w") as f:
        f.write(f"image: {stem.split('/')[-1]}.pgm\nresolution: {cell!r}\norigin: [{origin[0]!r}, {origin[1]!r}, {origin[2]!r}]\n"
                "negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n")
    return stem + ".yaml"


def top_error(h, truth):
    p = h.poses[0]
    return math.hypot(p[0] - truth[0], p[1] - truth[1]), abs((p[2] - truth[2] + math.pi) % (2 * math.pi) - math.pi)


def test_relocalize_in_a_foreign_map(tmp_path):
    from thesis_amd.datasets import synthetic
    from thesis_amd.engine import ParticleEngine
    from thesis_amd.mapio import read_map_image
    P, n_rot, cell, sc, yaw = 4, 720, 0.05, 0.03, 0.4
    room, x0, y0 = asym_room(cell)
    # the foreign frame: 880 x 880 cells of 0.03 m, rotated by 0.4 about a centre that is off both grids
    n = 880
    half = n * sc / 2
    origin = (0.0137 - (math.cos(yaw) * half - math.sin(yaw) * half), -0.0071 - (math.sin(yaw) * half + math.cos(yaw) * half), yaw)
    foreign, fcov = po.resample(room, cell, (x0 * cell, y0 * cell, 0.0), (n, n), sc, origin, 2)
    assert set(np.unique(foreign).tolist()) == {-30, 0, 30}
    assert int(np.count_nonzero(foreign == -30)) > 0.9 * np.count_nonzero(room == -30) * (cell / sc) ** 2     # the whole floor is in it
    yml = write_foreign_map(str(tmp_path / "foreign"), foreign, sc, origin)
    src = read_map_image(yml, 0.1, -3.0, 3.0)
    assert np.array_equal(src.cells, foreign) and src.cell_size == sc and src.origin == origin

    direct, placed = engine(P, seed=5), engine(P, seed=5)
    full = (x0, x0 + room.shape[0], y0, y0 + room.shape[1])
    direct.load_map(raster(direct, full, room))
    box = placed.place_map(src)
    want = po.merge(np.zeros((box[1] - box[0], box[3] - box[2]), np.int8), *oracle(placed, src, box, 4), po.REPLACE, -30, 30)
    for p in range(P):
        assert np.array_equal(render(placed, p, box), want), p
    truth = (2.17, -3.36, 2.0)
    ang = synthetic.beam_angles(B)
    r = direct.cast_scans(np.asarray(truth), ang, particle=0, max_range=30.0)[0]
    errs = {}
    for name, e in (("direct", direct), ("placed", placed)):
        e.map_updates = False
        h = e.relocalize(r, ang, particle=0, k=8, n_rot=n_rot, seed=0)
        errs[name] = top_error(h, truth)
        print(f"{name}: top hypothesis {h.poses[0].tolist()}, score {h.scores[0]} of at most {2 * h.n_used}; "
              f"{errs[name][0]:.4f} m / {errs[name][1]:.5f} rad from the truth")
    (d0, t0), (d1, t1) = errs["direct"], errs["placed"]
    assert d1 <= d0 + math.sqrt(2) * (cell + sc) and t1 <= t0 + 2 * math.pi / n_rot, errs
    # a checkpoint saved after the placement restores the same map
    placed.save_checkpoint(str(tmp_path / "placed.npz"))
    g = ParticleEngine.from_checkpoint(str(tmp_path / "placed.npz"))
    for p in (0, P - 1):
        assert np.array_equal(render(g, p, box), want)
    direct.close(); placed.close(); g.close()
