"""Map loading and localization on the GPU (rbpf_load_map / rbpf_set_map_updates, kernels_load.hip): rasters written into
the particles' tiles come back bit for bit through render_map, agree with the host path (set_tile) through every kernel
that reads the maps, and a filter with map updates off localizes in a loaded map without changing it."""
import numpy as np
import pytest

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


def rand_cells(rng, box, lo=-30, hi=30):
    return rng.integers(lo, hi + 1, size=(box[1] - box[0], box[3] - box[2])).astype(np.int8)


def lattice_box(e):
    """The whole lattice in mosaic cells."""
    off = int(e.cfg.lattice_radius) * e.dim + e.dim // 2
    edge = (2 * int(e.cfg.lattice_radius) + 1) * e.dim - off
    return (-off, edge, -off, edge)


def render(e, p, box):
    return e.render_map(p, box=box).cells


def err_code(fn):
    from thesis_amd.engine import RbpfError
    with pytest.raises(RbpfError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_set_map_updates_round_trips():
    e = engine(2)
    assert e.map_updates is True
    e.map_updates = False
    assert e.map_updates is False
    e.map_updates = True
    assert e.map_updates is True
    e.close()


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------
def boxes(e):
    """Boxes that cross seams, sit at negative coordinates, start at awkward column offsets, are 1 x 1, touch the edge."""
    h = e.dim // 2
    lo, hi = lattice_box(e)[0], lattice_box(e)[1]
    out = [(h - 20, h + 30, h - 45, h + 19),            # crosses a seam in x and in y
           (-h - 37, -h + 5, -3 * h - 11, -h + 300),    # negative, two seams in y, wider than one 256-column block
           (5, 6, 7, 8),                                # 1 x 1
           (lo, lo + 17, hi - 33, hi),                  # lattice corner
           (hi - 5, hi, -40, 41)]                       # lattice edge in x
    out += [(-60 + 3 * o, -40 + 3 * o, -h + o, -h + o + 45) for o in (0, 1, 15, 16, 17, 31)]   # column offsets of a tile
    out += [(100 + o, 117 + o, 3 * h + o - 2, 3 * h + o + 29) for o in (0, 1, 15, 16, 17, 31)]   # and of the next one
    return out


@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_round_trip_through_render(cs):
    rng = np.random.Generator(np.random.PCG64(5))
    e = engine(3, cs=cs, pool_tiles=64)
    assert e.dim == int(round(40 / cs))
    full = lattice_box(e)
    # the other particles hold maps of their own, which must not move
    for p in (0, 2):
        b = (-e.dim // 2 - 50, e.dim // 2 + 70, -90 + p, 333)
        e.load_map(raster(e, b, rand_cells(rng, b)), particle=p)
    before = {p: render(e, p, full) for p in (0, 2)}
    model = np.zeros((full[1] - full[0], full[3] - full[2]), dtype=np.int8)
    ext = None
    for b in boxes(e):
        c = rand_cells(rng, b)
        e.load_map(raster(e, b, c), particle=1)
        got = render(e, 1, b)
        assert np.array_equal(got, c), (b, int(np.count_nonzero(got != c)))
        model[b[0] - full[0]:b[1] - full[0], b[2] - full[2]:b[3] - full[2]] = c
        ext = b if ext is None else (min(ext[0], b[0]), max(ext[1], b[1]), min(ext[2], b[2]), max(ext[3], b[3]))
    assert np.array_equal(render(e, 1, full), model)     # cells outside each box kept their values
    assert e.map_extent(1) == ext                        # written boxes: exactly the union of the loaded boxes
    for p in (0, 2):
        assert np.array_equal(render(e, p, full), before[p])
    e.close()


# ---- 2. overwrite a built map ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_overwrite_keeps_cells_outside_the_box(cs):
    from thesis_amd.datasets import synthetic
    ang, ranges, _, truth = synthetic.make_log(2, B)
    e = engine(2, cs=cs)
    e.set_scan(ranges[0], ang)
    e.map_update(np.zeros((2, 3)))
    ext = e.map_extent(0)
    rng = np.random.Generator(np.random.PCG64(9))
    for b in [(-37, 55, -13, 71), (-e.dim // 2 - 9, -e.dim // 2 + 23, 17, 18), (ext[0] + 3, ext[0] + 40, ext[2] + 1, ext[3] - 1)]:
        big = (b[0] - 40, b[1] + 40, b[2] - 40, b[3] + 40)
        old = render(e, 0, big)
        other = render(e, 1, big)
        c = rand_cells(rng, b)
        e.load_map(raster(e, b, c), particle=0)
        new = render(e, 0, big)
        inside = np.zeros(new.shape, dtype=bool)
        inside[40:-40, 40:-40] = True
        assert np.array_equal(new[inside].reshape(c.shape), c)
        assert np.array_equal(new[~inside], old[~inside])
        assert np.array_equal(render(e, 1, big), other)
    e.close()


# ---- 3. against the host path ----------------------------------------------------------------------------------------------
def _tiles_of(e, box, cells):
    """(centre, dim x dim cells) of every tile the box touches: the raster's cells, 0 elsewhere."""
    dim, tl, R = e.dim, float(e.cfg.tile_len_m), int(e.cfg.lattice_radius)
    off = R * dim + dim // 2
    out = []
    for a in range((box[0] + off) // dim, (box[1] - 1 + off) // dim + 1):
        for b in range((box[2] + off) // dim, (box[3] - 1 + off) // dim + 1):
            t = np.zeros((dim, dim), dtype=np.int8)
            X0, Y0 = a * dim - off, b * dim - off
            ax, bx = max(box[0], X0), min(box[1], X0 + dim)
            ay, by = max(box[2], Y0), min(box[3], Y0 + dim)
            t[ax - X0:bx - X0, ay - Y0:by - Y0] = cells[ax - box[0]:bx - box[0], ay - box[2]:by - box[2]]
            out.append((((a - R) * tl, (b - R) * tl), t))
    return out


def test_load_equals_set_tile_through_a_run():
    from thesis_amd.datasets import synthetic
    P, K = 16, 30
    ang, ranges, odo, truth = synthetic.make_log(6, B)
    # a map built at the true poses, shifted by a few cells so that its box crosses tile seams and starts mid-word
    src = engine(1)
    src.set_scan(ranges[0], ang)
    src.map_update(truth[:1])
    m = src.render_map(0)
    src.close()
    box = (m.x0 - 3, m.x0 - 3 + m.cells.shape[0], m.y0 + 5, m.y0 + 5 + m.cells.shape[1])
    A, Bq = engine(P), engine(P)
    A.load_map(raster(A, box, m.cells))
    for p in range(P):
        for c, t in _tiles_of(Bq, box, m.cells):
            Bq.set_tile(p, c, t)
    assert A.counters()["tiles_in_use"] == Bq.counters()["tiles_in_use"]
    rng = np.random.Generator(np.random.PCG64(3))
    start = truth[0] + rng.normal(0, [0.05, 0.05, 0.01], size=(P, 3))
    for e in (A, Bq):
        e.set_state(poses=start, weights=1.0)
    for k in range(5):
        guesses = truth[k + 1] + rng.normal(0, [0.03, 0.03, 0.01], size=(P, K, 3))
        mo = np.zeros((P, 13))
        mo[:, :3] = truth[k + 1] + rng.normal(0, 0.01, size=(P, 3))
        mo[:, 3:12] = np.diag([4e-4, 4e-4, 1e-4]).ravel()
        mo[:, 12] = 1.0
        for e in (A, Bq):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            if k in (1, 3):                              # the built-in matcher: it reads the occupancy words
                e.scan_update(adj=False, guesses=guesses)
            else:
                e.scan_update(adj=False, match_override=mo, guesses=guesses)
        if k in (1, 3):
            np.testing.assert_array_equal(A.match_results(), Bq.match_results())
        if k == 2:                                       # past the resample trigger: tiles are copied
            w = A.weights()
            w[3] += 250.0
            for e in (A, Bq):
                e.set_state(weights=w)
        da, ia = A.resample(0.41)
        db, ib = Bq.resample(0.41)
        assert da == db and np.array_equal(ia, ib)
        np.testing.assert_array_equal(A.poses(), Bq.poses())
        np.testing.assert_array_equal(A.weights(), Bq.weights())
    full = lattice_box(A)
    for p in range(P):
        assert np.array_equal(render(A, p, full), render(Bq, p, full)), p
    A.close(); Bq.close()


# ---- 4. device input -------------------------------------------------------------------------------------------------------
def test_device_input_equals_host_input():
    import torch
    rng = np.random.Generator(np.random.PCG64(21))
    e = engine(4)
    b = (-431, -17, 390, 811)
    c = rand_cells(rng, b)
    e.load_map(raster(e, b, c), particle=0)
    e.load_map(raster(e, b, torch.from_numpy(c).to("cuda:0")), particle=2)
    full = lattice_box(e)
    r0 = render(e, 0, full)
    assert np.array_equal(render(e, 2, full), r0)
    assert np.array_equal(render(e, 1, full), np.zeros_like(r0))
    f = engine(4)
    f.load_map(raster(f, b, torch.from_numpy(c).to("cuda:0")))
    for p in range(4):
        assert np.array_equal(render(f, p, full), r0)
    e.close(); f.close()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    import torch
    from thesis_amd import _lib
    rng = np.random.Generator(np.random.PCG64(8))
    e = engine(4, pool_tiles=7)                                       # every particle starts with its centre tile
    b0 = (-30, 40, -20, 25)
    e.load_map(raster(e, b0, rand_cells(rng, b0)), particle=0)       # inside the centre tile
    full = lattice_box(e)

    def state():
        return e.counters()["tiles_in_use"], e.map_extent(None), [render(e, p, full) for p in range(4)]

    def same(a, b):
        assert a[0] == b[0] and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))

    s0 = state()
    assert s0[0] == 4
    big = (-30, 40, 380, 430)                                          # two tiles per particle: 4 missing, 3 free
    code, msg = err_code(lambda: e.load_map(raster(e, big, rand_cells(rng, big))))
    assert code == _lib.RBPF_ENOMEM and "needs 4 free tiles, the pool has 3" in msg, msg
    same(state(), s0)
    c = rand_cells(rng, b0)
    c[3, 4] = 31                                                       # vmax is 30
    assert err_code(lambda: e.load_map(raster(e, b0, c), particle=1))[0] == _lib.RBPF_EINVAL
    c[3, 4] = -31
    assert err_code(lambda: e.load_map(raster(e, b0, torch.from_numpy(c).to("cuda:0")), particle=1))[0] == _lib.RBPF_EINVAL
    assert err_code(lambda: e.load_map(raster(e, b0, torch.from_numpy(c).to("cuda:0"))))[0] == _lib.RBPF_EINVAL
    same(state(), s0)
    off = (full[1] - 3, full[1] + 2, 0, 4)
    assert err_code(lambda: e.load_map(raster(e, off, rand_cells(rng, off)), particle=1))[0] == _lib.RBPF_EINVAL
    same(state(), s0)
    from thesis_amd.datasets import synthetic
    ang = synthetic.beam_angles(B)
    e.set_scan(synthetic.cast_scan((0, 0, 0), ang), ang)
    e.scan_update_begin()
    assert err_code(lambda: e.load_map(raster(e, b0, rand_cells(rng, b0)), particle=1))[0] == _lib.RBPF_ESTATE
    e.scan_update_end()
    # a raster that does not fit the engine, or has no cells
    from thesis_amd.mapio import MapRaster
    with pytest.raises(ValueError, match="cell_size"):
        e.load_map(MapRaster(x0=0, y0=0, cell_size=0.1, quantum=0.1, dim=400, tile_len=40.0, cells=c))
    with pytest.raises(ValueError, match="cells_from_probability"):
        e.load_map(MapRaster(x0=0, y0=0, cell_size=0.05, quantum=0.1, dim=800, tile_len=40.0, prob=np.zeros((2, 2), np.float32)))
    e.close()


# ---- 6. duplicate groups ---------------------------------------------------------------------------------------------------
def test_load_dissolves_duplicate_groups():
    from thesis_amd.datasets import synthetic
    P = 32
    ang, ranges, odo, truth = synthetic.make_log(4, B)
    e = engine(P)
    e.set_scan(ranges[0], ang)
    e.map_update(np.zeros((P, 3)))

    def step(k, force):
        e.imu_update("velocity", odo[k], 1000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update(adj=False)
        if force:
            w = e.weights()
            w[5] += 250.0
            e.set_state(weights=w)
        did, idx = e.resample(0.3)
        assert did and len(set(idx.tolist())) < P        # duplicates exist
    step(0, True)
    s0 = e.counters()["match_shared"]
    step(1, True)
    assert e.counters()["match_shared"] > s0             # without a load the duplicates share their match
    b = (-20, 30, -10, 15)
    e.load_map(raster(e, b, np.full((50, 25), 7, np.int8)), particle=int(np.argmax(e.weights())))
    s1 = e.counters()["match_shared"]
    e.imu_update("velocity", odo[2], 1000.0)
    e.set_scan(ranges[3], ang)
    e.scan_update(adj=False)
    assert e.counters()["match_shared"] == s1
    e.close()


# ---- 7. map updates off ----------------------------------------------------------------------------------------------------
def test_map_updates_off():
    from thesis_amd.datasets import synthetic
    P, N = 32, 6
    ang, ranges, odo, truth = synthetic.make_log(N + 1, B)
    on, off = engine(P, seed=11), engine(P, seed=11)
    for e in (on, off):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))
    off.map_updates = False
    full = lattice_box(off)
    maps = [render(off, p, full) for p in range(P)]
    for k in range(N):
        for e in (on, off):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            e.scan_update(adj=False)
        if k == 0:
            assert np.all(np.isfinite(on.match_results()[:, 3:12]))   # no particle on the NaN branch
            np.testing.assert_array_equal(off.poses(), on.poses())
            np.testing.assert_array_equal(off.weights(), on.weights())
        if k == 2:
            for e in (on, off):
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
        for e in (on, off):
            e.resample()
    assert off.counters()["resample_copies"] > 0
    for p in range(P):
        assert np.array_equal(render(off, p, full), maps[p]), p
    assert on.counters()["cells_written"] > off.counters()["cells_written"]
    import ctypes as C
    st = []
    for e in (on, off):
        a, b = C.c_uint64(), C.c_uint64()
        e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(a), C.byref(b)))
        st.append((a.value, b.value))
    assert st[0] == st[1] and st[0][0] == N + 1, st      # the proposal's stream advanced once per step in both
    on.close(); off.close()


def test_nan_branch_weight_on_the_unchanged_map():
    from thesis_amd.datasets import synthetic
    P, K = 8, 30
    ang, ranges, odo, truth = synthetic.make_log(2, B)
    e = engine(P)
    e.set_scan(ranges[0], ang)
    e.map_update(np.zeros((P, 3)))
    e.map_updates = False
    full = lattice_box(e)
    maps = [render(e, p, full) for p in range(P)]
    pose = np.array([0.04, -0.03, 0.02])
    e.set_state(poses=pose, weights=2.5)
    e.set_scan(ranges[1], ang)
    mo = np.zeros((P, 13))
    mo[:, :3] = pose
    mo[:, 3:12] = np.diag([4e-4, 4e-4, 1e-4]).ravel()
    mo[0, 3:12] = np.nan                                   # particle 0: the robot.py:73-78 branch
    rng = np.random.Generator(np.random.PCG64(2))
    e.scan_update(adj=False, match_override=mo, guesses=pose + rng.normal(0, 0.02, size=(P, K, 3)))
    np.testing.assert_array_equal(e.poses()[0], pose)
    # robot.py:75-77: 1 + sum of get_odds_at over the weighted beams (0.01 < range < 25 m), at the kept pose
    r = ranges[1]
    x, y = r * np.cos(ang), r * np.sin(ang)
    d = np.sqrt(x * x + y * y)
    sel = (d < e.cfg.weight_max_range) & (d > e.cfg.weight_min_range)
    c, s = np.cos(pose[2]), np.sin(pose[2])
    pts = np.stack([(c * x + (-s) * y) + pose[0], (s * x + c * y) + pose[1]], axis=1)[sel]
    vals, none = e.get_odds_at(0, pts)
    want = 2.5 + (1.0 + vals[~none].sum())
    np.testing.assert_allclose(e.weights()[0], want, rtol=1e-12, atol=1e-12)
    for p in range(P):
        assert np.array_equal(render(e, p, full), maps[p]), p
    e.close()


# ---- 8. localization end to end ----------------------------------------------------------------------------------------------
# Measured on an MI355X (seeded, so the same on every run): the best particle ends 0.015 m / 0.0003 rad from the truth.
# The bounds leave a wide margin and still fail when the filter loses the robot (the starts are 0.2 m / 0.05 rad off).
LOC_TOL_M, LOC_TOL_RAD = 0.1, 0.02


def test_localize_in_a_saved_map(tmp_path):
    from thesis_amd.datasets import synthetic
    from thesis_amd.mapio import read_occupancy_map, write_occupancy_map
    P, N = 256, 40
    ang, ranges, odo, truth = synthetic.make_log(N + 1, B)
    # the room16 map at the true poses of a whole circle
    full_ang, full_ranges, _, full_truth = synthetic.make_log(380, B, seed=77)
    src = engine(1)
    for k in range(0, 380, 10):
        src.set_scan(full_ranges[k], full_ang)
        src.map_update(full_truth[k:k + 1])
    m = src.render_map(0)
    src.close()
    _, yml = write_occupancy_map(str(tmp_path / "room16"), m)
    r = read_occupancy_map(yml, 0.1, -3.0, 3.0, cell_size=0.05, tile_len=40.0)
    assert np.array_equal(r.cells, m.cells) and (r.x0, r.y0) == (m.x0, m.y0)
    e = engine(P, seed=5)
    e.load_map(r)
    e.map_updates = False
    box = (r.x0, r.x0 + r.cells.shape[0], r.y0, r.y0 + r.cells.shape[1])
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
    c = e.counters()
    print(f"localization: best particle {dxy:.4f} m / {dth:.4f} rad from the truth; resample_copies {c['resample_copies']}, "
          f"bytes_copied {c['bytes_copied']}")
    assert dxy < LOC_TOL_M and dth < LOC_TOL_RAD, (dxy, dth)
    for p in range(P):
        assert np.array_equal(render(e, p, box), r.cells), p
    assert e.map_extent(None) == box
    e.close()


# ---- checkpoints and the ParticleFilter front ---------------------------------------------------------------------------------
def test_checkpoint_keeps_the_mode(tmp_path):
    from thesis_amd.engine import ParticleEngine
    e = engine(2, max_beams=64)
    b = (-5, 9, 3, 20)
    e.load_map(raster(e, b, np.full((14, 17), -4, np.int8)))
    e.map_updates = False
    e.save_checkpoint(str(tmp_path / "off.npz"))
    f = ParticleEngine.from_checkpoint(str(tmp_path / "off.npz"))
    assert f.map_updates is False
    assert np.array_equal(render(f, 1, b), render(e, 1, b))
    with np.load(str(tmp_path / "off.npz")) as d:                   # a checkpoint written before the key existed
        np.savez_compressed(str(tmp_path / "old.npz"), **{k: d[k] for k in d.files if k != "map_updates"})
    g = ParticleEngine.from_checkpoint(str(tmp_path / "old.npz"))
    assert g.map_updates is True
    e.close(); f.close(); g.close()


def test_particle_filter_passes_through():
    from thesis_amd.datasets import synthetic
    from thesis_amd.slam import ParticleFilter
    ang = synthetic.beam_angles(B)
    pf = ParticleFilter(4, ang, map_updates=False, keep_history=False)
    assert pf.map_updates is False and pf.engine.map_updates is False
    b = (-30, 30, -30, 30)
    c = np.full((60, 60), 12, np.int8)
    pf.load_map(raster(pf.engine, b, c), particle=2)
    assert np.array_equal(pf.render_map(2, box=b).cells, c)
    pf.map_update(synthetic.cast_scan((0.0, 0.0, 0.0), ang))
    assert np.array_equal(pf.render_map(2, box=b).cells, c)      # updates off: the scan left the map alone
    pf.map_updates = True
    assert pf.engine.map_updates is True
    pf.close()
