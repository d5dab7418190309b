"""Map read-out on the GPU (rbpf_map_extent / rbpf_render_map, kernels_render.hip): one particle's map and the whole
filter's map as dense rasters, checked against mosaics built on the host from ParticleEngine.tiles()."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def mosaic(e, p, box):
    """int8 [x1-x0][y1-y0] of particle p from its tiles: tile centre (A tile_len, B tile_len) holds mosaic cells
    X = A dim + i - dim // 2, Y = B dim + j - dim // 2; every other cell is 0."""
    x0, x1, y0, y1 = box
    out = np.zeros((x1 - x0, y1 - y0), dtype=np.int8)
    dim, tl = e.dim, float(e.cfg.tile_len_m)
    for (cx, cy), cells in e.tiles(p):
        X0, Y0 = int(round(cx / tl)) * dim - dim // 2, int(round(cy / tl)) * dim - dim // 2
        ax, bx = max(x0, X0), min(x1, X0 + dim)
        ay, by = max(y0, Y0), min(y1, Y0 + dim)
        if ax < bx and ay < by:
            out[ax - x0:bx - x0, ay - y0:by - y0] = cells[ax - X0:bx - X0, ay - Y0:by - Y0]
    return out


def filter_oracle(e, box, w):
    """float64 prob and occ_frac, one particle after the other."""
    q, thr = e.cfg.quantum, int(round(e.cfg.occupied_threshold / e.cfg.quantum))
    sp = np.zeros((box[1] - box[0], box[3] - box[2]))
    so = np.zeros_like(sp)
    count = np.zeros(sp.shape, dtype=np.int64)
    for p in range(e.P):
        m = mosaic(e, p, box)
        ex = np.exp(m.astype(np.float64) * q)
        sp += w[p] * (ex / (1.0 + ex))
        so += w[p] * (m > thr)
        count += m > thr
    return sp / w.sum(), so / w.sum(), count


def run_filter(P, steps, seed=7, force_resample_at=1):
    from thesis_amd import engine
    from thesis_amd.datasets import synthetic
    B = 1081
    ang, ranges, odo, _ = synthetic.make_log(steps, B, period=0.7)
    e = engine.ParticleEngine(P, max_beams=B, pool_tiles=4 * P, seed=seed)
    e.set_scan(ranges[0], ang)
    e.map_update(np.zeros((P, 3)))
    resampled = 0
    for k in range(steps - 1):
        e.imu_update("velocity", odo[k], 7000.0)
        e.set_scan(ranges[k + 1], ang)
        e.scan_update(adj=False)
        if k == force_resample_at:                      # past the main.py:50 trigger, so the maps get copied
            w = e.weights()
            w[0] += 250.0
            e.set_state(weights=w)
        did, _ = e.resample(float("nan"))
        resampled += did
    assert resampled >= 1
    return e


@pytest.fixture(scope="module")
def run64():
    e = run_filter(64, 6)
    yield e
    e.close()


def test_single_particle_raster_is_exact():
    from thesis_amd import engine
    e = engine.ParticleEngine(3, max_beams=64, pool_tiles=16, seed=3)
    rng = np.random.Generator(np.random.PCG64(11))
    tl = float(e.cfg.tile_len_m)
    for p, centres in ((0, [(-1, 0), (0, 0), (1, -1), (-3, 3)]), (1, [(0, 0), (0, 1), (3, -3)])):
        for (a, b) in centres:
            cells = np.zeros((e.dim, e.dim), dtype=np.int8)
            i0, j0 = rng.integers(0, 300, size=2)
            if abs(a) == 3:                           # lattice corner tiles: written up to the lattice edge
                cells[:] = rng.integers(-30, 31, size=cells.shape)
            else:
                cells[i0:i0 + 470, j0:j0 + 455] = rng.integers(-30, 31, size=(470, 455))
            e.set_tile(p, (a * tl, b * tl), cells)
    boxes = [(-420, -380, -7, 9),                     # across the seam X = -400
             (-1300, 500, -500, 900),                 # several tiles, seams in both directions
             (395, 1203, -1213, -389),                # seams, edges not 16-aligned
             (2790, 2813, -2810, -2780),              # partly outside the lattice (|X|, |Y| < 2800)
             (-2850, -2795, 2795, 2850),
             (5000, 5003, 0, 17),                     # wholly outside
             (-3, 13, 5, 5)]                          # empty
    for p in range(3):
        for box in boxes:
            r = e.render_map(p, box=box)
            assert r.prob is None and r.occ_frac is None and r.cells.dtype == np.int8
            assert (r.x0, r.y0) == (box[0], box[2])
            assert np.array_equal(r.cells, mosaic(e, p, box)), (p, box)
    for box in boxes[:3]:
        assert not e.render_map(2, box=box).cells.any()   # no tiles written
    e.close()


def test_filter_render_after_a_run(run64):
    from thesis_amd.mapio import resample_weights
    e = run64
    box = e.map_extent()
    assert box is not None
    P = e.P
    r = e.render_map(box=box)
    assert r.cells is None and r.prob.dtype == np.float32 and r.occ_frac.dtype == np.float32
    prob, occ, count = filter_oracle(e, box, np.ones(P))
    assert np.array_equal(r.occ_frac, (count / P).astype(np.float32))
    assert np.abs(r.prob.astype(np.float64) - prob).max() < 1e-6
    assert count.max() > 0 and (r.prob > 0.5).any() and (r.prob < 0.5).any()
    rng = np.random.Generator(np.random.PCG64(5))
    w_rand = rng.uniform(0.0, 3.0, P)
    w_zero = w_rand.copy()
    w_zero[::3] = 0.0
    cases = [(w_rand, w_rand), (w_zero, w_zero)]
    if resample_weights(e.weights()).sum() > 0:
        cases.append(("resample", resample_weights(e.weights())))
    for w, ww in cases:
        r = e.render_map(box=box, weights=w)
        prob, occ, _ = filter_oracle(e, box, ww)
        assert np.abs(r.prob.astype(np.float64) - prob).max() < 1e-6
        assert np.abs(r.occ_frac.astype(np.float64) - occ).max() < 1e-6
    only = e.render_map(box=box, fields=("occ_frac",))
    assert only.prob is None and np.array_equal(only.occ_frac, e.render_map(box=box).occ_frac)
    # a box wider than the extent: the cells around it hold no particle's tile data, or are outside the lattice
    big = (box[0] - 37, box[1] + 21, box[2] - 5, box[3] + 40)
    rb = e.render_map(box=big)
    assert np.array_equal(rb.prob[37:37 + box[1] - box[0], 5:5 + box[3] - box[2]], e.render_map(box=box).prob)


def test_filter_render_at_1024_particles():
    e = run_filter(1024, 4)
    box = e.map_extent()
    r = e.render_map(box=box)
    prob, occ, count = filter_oracle(e, box, np.ones(e.P))
    assert np.array_equal(r.occ_frac, (count / e.P).astype(np.float32))
    assert np.abs(r.prob.astype(np.float64) - prob).max() < 1e-6
    e.close()


def test_particle_split_does_not_change_the_result(run64, monkeypatch):
    e = run64
    ext = e.map_extent()
    cx, cy = (ext[0] + ext[1]) // 2, (ext[2] + ext[3]) // 2
    tiny = (cx - 23, cx + 18, cy - 9, cy + 30)            # few jobs: the particles are split into chunks
    large = (cx - 600, cx + 600, cy - 1000, cy + 1000)    # enough jobs: one chunk
    monkeypatch.delenv("RBPF_RENDER_SPLIT", raising=False)
    a = e.render_map(box=tiny)
    b = e.render_map(box=large)
    sub = (slice(tiny[0] - large[0], tiny[1] - large[0]), slice(tiny[2] - large[2], tiny[3] - large[2]))
    assert a.prob.tobytes() == np.ascontiguousarray(b.prob[sub]).tobytes()
    assert a.occ_frac.tobytes() == np.ascontiguousarray(b.occ_frac[sub]).tobytes()
    prob, occ, count = filter_oracle(e, tiny, np.ones(e.P))
    assert np.array_equal(a.occ_frac, (count / e.P).astype(np.float32))
    assert np.abs(a.prob.astype(np.float64) - prob).max() < 1e-6
    w = np.random.Generator(np.random.PCG64(9)).uniform(0.0, 2.0, e.P)
    ref = e.render_map(box=tiny, weights=w)
    for g in ("1", "2", "3", "8", "64"):                  # forced chunk counts (clamped to the number of groups)
        monkeypatch.setenv("RBPF_RENDER_SPLIT", g)
        for wt, want in ((None, a), (w, ref)):
            r = e.render_map(box=tiny, weights=wt)
            assert r.prob.tobytes() == want.prob.tobytes() and r.occ_frac.tobytes() == want.occ_frac.tobytes(), g
    monkeypatch.setenv("RBPF_RENDER_SPLIT", "1")
    one = e.render_map(box=large, weights=w)
    monkeypatch.delenv("RBPF_RENDER_SPLIT")
    for _ in range(3):                                    # bit-identical from call to call
        r = e.render_map(box=large, weights=w)
        assert r.prob.tobytes() == one.prob.tobytes() and r.occ_frac.tobytes() == one.occ_frac.tobytes()


def test_extent(run64):
    from thesis_amd import engine
    fresh = engine.ParticleEngine(4, max_beams=64, pool_tiles=8)
    assert fresh.map_extent() is None and fresh.map_extent(2) is None
    fresh.close()
    e = run64
    ext = e.map_extent()
    pad = 900
    outer = (ext[0] - pad, ext[1] + pad, ext[2] - pad, ext[3] + pad)
    boxes = []
    for p in list(range(0, e.P, 7)) + [e.P - 1]:
        bp = e.map_extent(p)
        boxes.append(bp)
        assert ext[0] <= bp[0] < bp[1] <= ext[1] and ext[2] <= bp[2] < bp[3] <= ext[3]
        m = mosaic(e, p, outer)
        xs, ys = np.nonzero(m)
        assert len(xs) > 0
        assert xs.min() + outer[0] >= bp[0] and xs.max() + outer[0] < bp[1]
        assert ys.min() + outer[2] >= bp[2] and ys.max() + outer[2] < bp[3]
        # inside that particle's tiles
        dim, tl = e.dim, float(e.cfg.tile_len_m)
        tiles = [(int(round(c[0] / tl)) * dim - dim // 2, int(round(c[1] / tl)) * dim - dim // 2) for c, _ in e.tiles(p)]
        for X, Y in ((bp[0], bp[2]), (bp[1] - 1, bp[2]), (bp[0], bp[3] - 1), (bp[1] - 1, bp[3] - 1)):
            assert any(X0 <= X < X0 + dim and Y0 <= Y < Y0 + dim for X0, Y0 in tiles)
    allnz = np.zeros((outer[1] - outer[0], outer[3] - outer[2]), dtype=bool)
    for p in range(e.P):
        allnz |= mosaic(e, p, outer) != 0
    xs, ys = np.nonzero(allnz)
    assert xs.min() + outer[0] >= ext[0] and xs.max() + outer[0] < ext[1]
    assert ys.min() + outer[2] >= ext[2] and ys.max() + outer[2] < ext[3]


def test_rendering_has_no_side_effects():
    from thesis_amd import engine
    from thesis_amd.mapio import resample_weights
    from thesis_amd.datasets import synthetic
    torch = pytest.importorskip("torch")
    P, B = 24, 1081
    ang, ranges, odo, _ = synthetic.make_log(7, B, period=0.7)
    a = engine.ParticleEngine(P, max_beams=B, pool_tiles=4 * P, seed=7)
    b = engine.ParticleEngine(P, max_beams=B, pool_tiles=4 * P, seed=7)
    for e in (a, b):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))

    def render_all(e):
        e.map_extent()
        e.map_extent(3)
        e.render_map(0)
        e.render_map("best")
        e.render_map(P - 1, box=(-50, 70, -20, 33))
        e.render_map()
        if resample_weights(e.weights()).sum() > 0:
            e.render_map(weights="resample")
        e.render_map(weights=np.arange(P, dtype=np.float64) + 1.0, box=(-30, 10, -12, 40))
        e.render_map(device=True)
        e.render_map(7, device=True)
        torch.cuda.synchronize()

    for k in range(6):
        render_all(a)
        for e in (a, b):
            e.imu_update("velocity", odo[k], 7000.0)
            e.set_scan(ranges[k + 1], ang)
            e.scan_update(adj=False)
        render_all(a)
        if k == 2:
            for e in (a, b):
                w = e.weights()
                w[0] += 250.0
                e.set_state(weights=w)
        da, ia = a.resample(float("nan"))
        db, ib = b.resample(float("nan"))
        assert da == db and np.array_equal(ia, ib)
    assert np.array_equal(a.poses(), b.poses()) and np.array_equal(a.covs(), b.covs()) and np.array_equal(a.weights(), b.weights())
    ra, rb = (C.c_uint64(), C.c_uint64()), (C.c_uint64(), C.c_uint64())
    for e, r in ((a, ra), (b, rb)):
        e._check(e._lib.rbpf_get_rng_state(e._h, C.byref(r[0]), C.byref(r[1])))
    assert (ra[0].value, ra[1].value) == (rb[0].value, rb[1].value)
    assert a.counters()["tiles_in_use"] == b.counters()["tiles_in_use"]
    for p in range(P):
        ta, tb = a.tiles(p), b.tiles(p)
        assert [c for c, _ in ta] == [c for c, _ in tb]
        for (_, ca), (_, cb) in zip(ta, tb):
            assert np.array_equal(ca, cb)
    a.close(); b.close()


def test_device_output_equals_host_output(run64):
    torch = pytest.importorskip("torch")
    e = run64
    box = e.map_extent()
    w = np.random.Generator(np.random.PCG64(2)).uniform(0.0, 1.0, e.P)
    h, d = e.render_map(box=box, weights=w), e.render_map(box=box, weights=w, device=True)
    assert isinstance(d.prob, torch.Tensor) and d.prob.device.type == "cuda" and d.cells is None
    assert np.array_equal(d.prob.cpu().numpy(), h.prob) and np.array_equal(d.occ_frac.cpu().numpy(), h.occ_frac)
    hc, dc = e.render_map(5), e.render_map(5, device=True)
    assert dc.cells.dtype == torch.int8 and np.array_equal(dc.cells.cpu().numpy(), hc.cells)
    # on a borrowed stream that is torch's current one, no extra synchronisation is needed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = e.render_map(box=box, weights=w, device=True)
        same = torch.equal(d2.prob, d.prob) and torch.equal(d2.occ_frac, d.occ_frac)
        e.release_stream()
    assert same


def test_errors_leave_outputs_untouched(run64):
    from thesis_amd import _lib
    from thesis_amd.engine import RbpfError
    e = run64
    P = e.P
    EINVAL, ESTATE = _lib.RBPF_EINVAL, _lib.RBPF_ESTATE
    n = 8 * 8
    cells = np.full(n, 77, dtype=np.int8)
    prob = np.full(n, 7.0, dtype=np.float32)
    occ = np.full(n, 9.0, dtype=np.float32)
    good = np.array([0, 8, -3, 5], dtype=np.int32)
    ones = np.ones(P)

    def call(particle, box=good, w=None, flags=0, c=None, pr=None, oc=None):
        b = np.asarray(box, dtype=np.int32)
        wp = None if w is None else np.ascontiguousarray(w, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        return e._lib.rbpf_render_map(e._h, particle, b.ctypes.data_as(C.POINTER(C.c_int32)), wp, flags,
                                      ptr(c), ptr(pr), ptr(oc))

    bad = [
        dict(particle=P, c=cells), dict(particle=-2, pr=prob),                     # particle index
        dict(particle=0, box=(8, 0, -3, 5), c=cells), dict(particle=-1, box=(0, 8, 5, -3), pr=prob),   # x1 < x0, y1 < y0
        dict(particle=0, box=(0, 65536, 0, 32769), c=cells),                      # more than 2^31 cells
        dict(particle=0), dict(particle=0, c=cells, pr=prob), dict(particle=0, c=cells, w=ones),   # NULL patterns
        dict(particle=-1, c=cells, pr=prob), dict(particle=-1),
        dict(particle=-1, pr=prob, w=-ones), dict(particle=-1, pr=prob, w=np.zeros(P)),             # weights
        dict(particle=-1, oc=occ, w=np.where(np.arange(P) == 3, np.nan, 1.0)),
        dict(particle=-1, oc=occ, w=np.where(np.arange(P) == 3, np.inf, 1.0)),
        dict(particle=-1, pr=prob, flags=6),                                       # unknown flag
    ]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert (cells == 77).all() and (prob == 7.0).all() and (occ == 9.0).all(), kw
    box4 = np.full(4, 5, dtype=np.int32)
    assert e._lib.rbpf_map_extent(e._h, P, box4.ctypes.data_as(C.POINTER(C.c_int32))) == EINVAL and (box4 == 5).all()
    with pytest.raises(RbpfError) as ei:
        e.render_map(0, box=(3, 1, 0, 4))
    assert ei.value.code == EINVAL
    with pytest.raises(RbpfError) as ei:
        e.render_map(box=good, weights=-ones)
    assert ei.value.code == EINVAL
    assert call(0, c=cells) == 0 and call(-1, pr=prob, oc=occ) == 0       # the same buffers, a good call
    # between scan_update_begin and _end
    from thesis_amd.datasets import synthetic
    ang = synthetic.beam_angles(e.cfg.max_beams, 1.5 * np.pi)
    e.set_scan(synthetic.cast_scan(e.poses()[0], ang, np.random.Generator(np.random.PCG64(4))), ang)
    cells[:] = 77
    e.scan_update_begin()
    try:
        assert call(0, c=cells) == ESTATE and (cells == 77).all()
        with pytest.raises(RbpfError) as ei:
            e.render_map()
        assert ei.value.code == ESTATE
    finally:
        e.scan_update_end()
    assert call(0, c=cells) == 0
