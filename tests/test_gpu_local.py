"""The local map on the GPU (rbpf_local_map, kernels_local.hip; ParticleEngine.local_map) against the NumPy oracle of
tests/local_oracle.py run on the rendered maps: every crop and all four fused sums by equality.  Then what the call leaves alone,
its device outputs, its argument checks and its limits."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import local_oracle as LO
from tests.cast_oracle import lattice_bounds
from tests.test_gpu_cast import engine, load_room16, raster, rng_state, seam_scene

pytestmark = pytest.mark.gpu

FILL = 0x55
GROUP = 64                                              # LOCAL_GROUP of rbpf_localbatch.h: poses of one group of the fusion


def inv_of(e):
    return e.dim / float(e.cfg.tile_len_m)


def thr_of(e):
    return float(e.cfg.occupied_threshold) / float(e.cfg.quantum)


def cell_of(e):
    return float(e.cfg.cell_size)


def pose_at(e, cell, frac, th):
    """The pose that stands at the fraction `frac` of mosaic cell `cell`."""
    return [(cell[0] + frac[0]) / inv_of(e), (cell[1] + frac[1]) / inv_of(e), th]


def rendered(e, p):
    """(cells, x0, y0) of particle p's map; a particle without a map gives one unknown cell."""
    m = e.render_map(p, box=e.map_extent(p) or (0, 1, 0, 1))
    return m.cells, m.x0, m.y0


def oracle_crops(e, maps, poses, particle, n, S, cell, offset):
    out = []
    for k, q in enumerate(np.asarray(poses, dtype=np.float64).reshape(-1, 3)):
        c, x0, y0 = maps[k if particle is None else particle]
        out.append(LO.crop(c, x0, y0, q, n, S, cell, offset, inv_of(e)))
    return np.stack(out)


def fields(lm):
    return np.stack([np.asarray(a) for a in (lm.occ_w, lm.free_w, lm.unknown_w, lm.sum_wv)], axis=-1)


def compare(e, maps, poses, particle, n, S, cell=None, offset=(0.0, 0.0), weights=None, what=""):
    """local_map with and without crops against the oracle; returns (LocalMap, oracle crops)."""
    from thesis_amd.local import quantise_weights
    cv = cell_of(e) if cell is None else cell
    kw = dict(particle=particle, size_m=n * cv, cell=cell, samples=S, weights=weights, offset=offset)
    got = e.local_map(poses, crops=True, **kw)
    want = oracle_crops(e, maps, poses, particle, n, S, cv, offset)
    assert got.crops.shape == want.shape and got.crops.dtype == np.int8, (what, got.crops.shape, want.shape)
    bad = got.crops != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} crop cells differ, first {tuple(np.argwhere(bad)[0])}"
    wq = None if weights is None else quantise_weights(weights)
    fw = LO.fuse(want, wq, thr_of(e))
    assert got.total == (len(want) if wq is None else int(wq.sum(dtype=np.uint64)))
    assert fields(got).dtype == np.int64 and np.array_equal(fields(got), fw), f"{what}: fused"
    lean = e.local_map(poses, crops=False, **kw)          # the crops stay in scratch, padded to 16-byte strips
    assert lean.crops is None and np.array_equal(fields(lean), fw), f"{what}: fused without crops"
    return got, want


def raw(e, particle, poses, n, S, cell=None, wq=None, offset=None, flags=0, null=(), n_poses=None, want_crops=True):
    """The C entry point with outputs prefilled with FILL: (rc, fused [n][n][4] int64, crops [N][n][n] int8)."""
    ps = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    N = len(ps) if n_poses is None else n_poses
    m = max(n, 1)
    fused = np.full((m, m, 4), FILL, np.int64)
    crops = np.full((max(len(ps), 1), m, m), FILL, np.int8)
    w = None if wq is None else np.ascontiguousarray(wq, dtype=np.uint32)
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = e._lib.rbpf_local_map(e._h, particle, None if "poses" in null else dp(ps), N,
                               None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint32)), n, cell_of(e) if cell is None else cell, S,
                               dp(off), flags, None if "fused" in null else C.c_void_p(fused.ctypes.data),
                               None if "crops" in null or not want_crops else C.c_void_p(crops.ctypes.data))
    return rc, fused, crops


def scene_engine(P=2, **kw):
    """Particle P - 1 holds the scenes of seam_scene (values -30 .. 30 with a few walls, across the seams of the home tile),
    particle 0 another map that must not be seen."""
    rng = np.random.Generator(np.random.PCG64(77))
    e = engine(P, pool_tiles=24, **kw)
    scenes = seam_scene(e.dim, rng)
    for b, c in scenes:
        e.load_map(raster(e, b, c), particle=P - 1)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)
    return e, scenes, rng


# ---- 1. shapes at which lanes and strips go wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [None, 0.025, 0.13])
def test_shapes_fractions_headings_and_cell_sizes(cell):
    e, scenes, rng = scene_engine()
    maps = [rendered(e, p) for p in range(2)]
    h = e.dim // 2
    poses = [pose_at(e, c, f, th) for c, f in (((3, 20), (0.5, 0.5)), ((h - 8, h + 3), (0.3, 0.7)), ((-h - 20, -h - 250), (0.9, 0.1)))
             for th in (0.0, math.pi / 2, 2.3, -0.4)]
    seen = set()
    for n in (1, 5, 16, 17, 33):
        for S in (1, 2, 3, 8):
            off = (0.0, 0.0) if (n + S) % 2 else (0.37, -0.21)
            got, want = compare(e, maps, poses, 1, n, S, cell, off, what=f"cell {cell} n {n} S {S} offset {off}")
            seen |= set(np.unique(want).tolist())
    assert min(seen) < 0 and 0 in seen and max(seen) > 10          # free, unknown and occupied cells were all cut out
    e.close()


# ---- 2. seams, missing tiles, written-box edges, the lattice edge ------------------------------------------------------------------
def test_seams_missing_tiles_and_the_lattice_edge():
    e, scenes, rng = scene_engine(lattice_radius=1)
    lo, hi = lattice_bounds(e.dim, 1)
    k = rng.integers(-30, 31, size=(30, 30)).astype(np.int8)
    e.load_map(raster(e, (hi - 30, hi, lo, lo + 30), k), particle=1)         # the lattice's corner
    maps = [rendered(e, p) for p in range(2)]
    h = e.dim // 2
    cells = [(int(rng.integers(b[0] - 10, b[1] + 10)), int(rng.integers(b[2] - 10, b[3] + 10))) for b, _ in scenes for _ in range(2)]
    cells += [(h, h), (h - 1, h - 1), (-h, -h - 1), (0, 0)]                  # tile corners; the other particle's block
    cells += [(hi - 4, lo + 6), (hi - 1, lo), (lo, hi - 1)]                  # the window hangs over the lattice's edge
    cells += [(hi + 3, lo - 2), (hi + 500, 0)]                               # the pose itself stands outside: legal, reads 0
    cells += [(-h - 100, h + 100)]                                           # a tile that was never allocated
    poses = [pose_at(e, c, rng.uniform(0.05, 0.95, 2), rng.uniform(-np.pi, np.pi)) for c in cells]
    for n, S, cell in ((17, 2, None), (33, 3, None), (40, 1, 0.13), (64, 2, 0.025)):
        got, want = compare(e, maps, poses, 1, n, S, cell, what=f"seams n {n} S {S} cell {cell}")
        assert not want[-1].any() and not want[-2].any() and want[:8].any()
    far = compare(e, maps, poses[-2:], 1, 16, 2, what="outside the lattice")[0]
    assert np.all(far.unknown_w == 2) and not far.sum_wv.any()
    other = compare(e, maps, [pose_at(e, (0, 0), (0.5, 0.5), 0.3)], 0, 33, 2, what="the other particle's map")[0]
    assert int((other.occ_w > 0).sum()) >= 90 and not (other.free_w > 0).any()     # its 10 x 10 block of walls and nothing else
    e.close()


# ---- 3. own maps and the slot table ---------------------------------------------------------------------------------------------------
def test_each_pose_in_its_own_particles_map_before_and_after_a_resample():
    P = 8
    rng = np.random.Generator(np.random.PCG64(5))
    e = engine(P)
    for p in range(P):
        c = rng.integers(-30, 11, size=(90, 70)).astype(np.int8)
        c[rng.random(c.shape) < 0.03] = 25
        e.load_map(raster(e, (-40 + 3 * p, 50 + 3 * p, -30 - 2 * p, 40 - 2 * p), c), particle=p)
    poses = np.array([pose_at(e, (int(rng.integers(-20, 30)), int(rng.integers(-20, 20))), rng.uniform(0.05, 0.95, 2), rng.uniform(-np.pi, np.pi))
                      for _ in range(P)])
    e.set_state(poses=poses)
    w = rng.uniform(0.5, 2.0, P)
    for stage in ("before", "after"):
        maps = [rendered(e, p) for p in range(P)]
        assert stage == "after" or all(not np.array_equal(maps[0][0], m[0]) for m in maps[1:])
        got, want = compare(e, maps, e.poses(), None, 33, 2, weights=w, what=f"own maps {stage} the resample")
        assert len({c.tobytes() for c in want}) >= 2
        assert np.array_equal(fields(e.local_map(particle=None, size_m=33 * cell_of(e), weights=w)), fields(got))     # poses=None: poses()
        one = compare(e, maps, e.poses(), 5, 17, 3, what=f"one map {stage} the resample")[0]
        assert one.total == P
        if stage == "before":
            lw = np.zeros(P)
            lw[[2, 5]] = 250.0
            e.set_state(weights=lw)
            did, idx = e.resample()
            assert did and len(set(idx.tolist())) < P                        # particles were duplicated: maps are shared or copied
    e.close()


# ---- 4. grouping and batching ---------------------------------------------------------------------------------------------------------
def weight_cases(N, rng):
    some = rng.integers(0, 1000, N).astype(np.uint32)
    some[rng.random(N) < 0.3] = 0
    some[0] = 17
    single = np.zeros(N, np.uint32)
    single[N // 2] = 5
    full = rng.integers(0, 3, N).astype(np.uint32)
    full[N - 1] = 0
    full[N - 1] = (1 << 31) - 1 - int(full.sum(dtype=np.uint64))             # the sum is exactly 2^31 - 1
    return {"zeros among them": some, "a single non-zero": single, "sum 2^31 - 1": full, "all one": None}


@pytest.mark.parametrize("N", [GROUP - 1, GROUP, GROUP + 1, 130])
def test_pose_groups_weights_and_batches(N, monkeypatch):
    from thesis_amd import _lib
    rng = np.random.Generator(np.random.PCG64(N))
    e = engine(2, max_odds_occ=12.7)                                         # lattice values up to 127
    assert e._lib is not None and round(float(e.cfg.max_odds_occ) / float(e.cfg.quantum)) == 127
    c = rng.integers(-30, 11, size=(60, 60)).astype(np.int8)
    c[rng.random(c.shape) < 0.05] = 127
    e.load_map(raster(e, (-30, 30, -30, 30), c), particle=1)
    maps = [rendered(e, p) for p in range(2)]
    poses = np.array([pose_at(e, (int(rng.integers(-12, 12)), int(rng.integers(-12, 12))), rng.uniform(0.05, 0.95, 2), rng.uniform(-np.pi, np.pi))
                      for _ in range(N)])
    n, S = 17, 2
    want = oracle_crops(e, maps, poses, 1, n, S, cell_of(e), (0.0, 0.0))
    assert (want == 127).any()
    for name, wq in weight_cases(N, rng).items():
        fw = LO.fuse(want, wq, thr_of(e))
        if name == "sum 2^31 - 1":
            assert int(wq.sum(dtype=np.uint64)) == (1 << 31) - 1 and fw[..., 3].max() > (1 << 32) and fw[..., 0].max() >= (1 << 31) - 3 * N
        for batch in (None, "1", "7"):
            if batch is None:
                monkeypatch.delenv("RBPF_LOCAL_BATCH", raising=False)
            else:
                monkeypatch.setenv("RBPF_LOCAL_BATCH", batch)
            for want_crops in (True, False):
                rc, fused, crops = raw(e, 1, poses, n, S, wq=wq, want_crops=want_crops)
                assert rc == 0, (name, batch, e._lib.rbpf_last_error(e._h))
                assert np.array_equal(fused, fw), f"N {N}, {name}, batch {batch}, crops {want_crops}"
                assert np.array_equal(crops, want) if want_crops else np.all(crops == FILL)
    monkeypatch.delenv("RBPF_LOCAL_BATCH", raising=False)
    rc, fused, crops = raw(e, 1, poses, n, S, null=("fused",))               # crops alone
    assert rc == 0 and np.array_equal(crops, want) and np.all(fused == FILL)
    e.close()


# ---- 5. the reason for the feature -------------------------------------------------------------------------------------------------------
def test_two_drifted_particles_agree_in_the_robots_frame():
    from tests.cast_oracle import room16_cells
    e = engine(2)
    cells, x0, y0 = room16_cells()
    n0 = cells.shape[0]
    e.load_map(raster(e, (x0, x0 + n0, y0, y0 + n0), cells), particle=0)
    # particle 1: the same room turned by pi / 2 about the centre of cell (0, 0), (X, Y) -> (-Y, X), and shifted by (7, -4) cells
    turned = np.ascontiguousarray(np.rot90(cells, 1))
    bx, by = -(y0 + n0 - 1) + 7, x0 - 4
    e.load_map(raster(e, (bx, bx + n0, by, by + n0), turned), particle=1)
    cs = cell_of(e)
    c0 = (37, -52)                                                            # the robot at a cell centre, near a pillar and a wall
    th = 0.0
    c1 = (-c0[1] + 7, c0[0] - 4)
    poses = [pose_at(e, c0, (0.5, 0.5), th), pose_at(e, c1, (0.5, 0.5), th + math.pi / 2)]
    maps = [rendered(e, p) for p in range(2)]
    got, want = compare(e, maps, poses, None, 128, 2, what="two frames, one room")
    assert np.array_equal(got.crops[0], got.crops[1]) and (got.crops[0] > 10).any() and (got.crops[0] == 0).any()
    assert got.total == 2 and set(np.unique(got.occ_w).tolist()) == {0, 2}
    assert np.array_equal(got.blocked(), got.crops[0] > 10) and np.array_equal(got.p_occ(), (got.crops[0] > 10).astype(np.float64))
    world = e.render_map(None, box=e.map_extent(None), fields=("occ_frac",)).occ_frac
    assert ((world > 0) & (world < 1)).any()                                 # the world-frame sum doubles the walls
    src = got.as_source(poses[0], float(e.cfg.quantum))
    assert src.cells.shape == (128, 128) and src.cell_size == cs and np.array_equal(src.cells, got.crops[0])
    assert np.allclose(src.origin, (poses[0][0] - 64 * cs, poses[0][1] - 64 * cs, 0.0), atol=1e-12)
    e.close()


# ---- 6. localization mode ------------------------------------------------------------------------------------------------------------
def test_one_map_in_every_particle():
    P = 6
    rng = np.random.Generator(np.random.PCG64(8))
    e = engine(P)
    load_room16(e)                                                            # every particle holds the room
    e.set_state(poses=np.column_stack([rng.uniform(-7.5, 7.5, (P, 2)), rng.uniform(-np.pi, np.pi, P)]))
    a = e.local_map(particle=None, weights="uniform", crops=True)
    b = e.local_map(e.poses(), particle=0, weights=None, crops=True)
    assert a.crops.shape == (P, 128, 128) and a.total == b.total == P
    assert np.array_equal(a.crops, b.crops) and np.array_equal(fields(a), fields(b)) and (a.occ_w > 0).any()
    compare(e, [rendered(e, 3)] * P, e.poses(), None, 64, 2, what="localization mode")
    e.close()


# ---- 7. limits and errors ------------------------------------------------------------------------------------------------------------
def test_the_largest_window_and_tables_that_do_not_fit_beside_it():
    from thesis_amd.engine import RbpfError
    e, scenes, rng = scene_engine()
    maps = [rendered(e, p) for p in range(2)]
    h = e.dim // 2
    pose = [pose_at(e, (h - 20, h + 10), (0.3, 0.6), 0.7)]
    assert LO.reach(267, cell_of(e), (0.0, 0.0), inv_of(e)) == 191           # side 383, the largest at 0.05 m
    compare(e, maps, pose, 1, 267, 1, what="side 383")
    with pytest.raises(RbpfError, match="384"):
        e.local_map(pose, particle=1, size_m=269 * cell_of(e), samples=1, weights=None)
    with pytest.raises(RbpfError, match="384"):
        e.local_map(pose, particle=1, size_m=16 * cell_of(e), samples=1, weights=None, offset=(0.0, 9.6))
    compare(e, maps, pose, 1, 250, 8, what="side 359 and 2000 samples an axis: the tables stay in memory")
    compare(e, maps, pose, 1, 2, 1, offset=(-9.0, 0.0), what="a small window far behind")
    e.close()


def test_bad_arguments_and_call_order_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P = 3
    e = engine(P)
    load_room16(e)
    poses = [[0.0, 0.0, 0.0], [1.0, 0.5, 1.0]]
    three = poses + [[-1.0, 0.0, 2.0]]
    big = 2.0 ** 30 / inv_of(e)
    cases = dict(
        no_poses=dict(null=("poses",)), no_outputs=dict(null=("fused", "crops")), nan_pose=dict(poses=[poses[0], [np.nan, 0.5, 1.0]]),
        inf_heading=dict(poses=[poses[0], [1.0, 0.5, np.inf]]), nan_cell=dict(cell=np.nan), inf_cell=dict(cell=np.inf), zero_cell=dict(cell=0.0),
        negative_cell=dict(cell=-0.05), nan_offset=dict(offset=[0.0, np.nan]), inf_offset=dict(offset=[-np.inf, 0.0]), no_cells=dict(n=0),
        negative_cells=dict(n=-4), no_samples=dict(S=0), nine_samples=dict(S=9), no_pose=dict(n_poses=0), negative_poses=dict(n_poses=-1),
        particle_high=dict(particle=P), particle_low=dict(particle=-2), each_its_own_needs_P_poses=dict(particle=-1),
        pose_far=dict(poses=[poses[0], [big, 0.0, 0.0]]), pose_far_negative=dict(poses=[poses[0], [0.0, -big, 0.0]]),
        zero_weights=dict(wq=[0, 0]), heavy_weights=dict(wq=[1 << 31, 0]), heavy_sum=dict(wq=[(1 << 31) - 1, 1]), flag=dict(flags=2),
        high_flag=dict(flags=1 << 31), window=dict(n=269), window_by_offset=dict(offset=[9.6, 0.0]))
    for name, kw in cases.items():
        args = dict(particle=1, poses=poses, n=8, S=2)
        args.update(kw)
        rc, fused, crops = raw(e, **args)
        assert rc == _lib.RBPF_EINVAL, (name, rc)
        assert np.all(fused == FILL) and np.all(crops == FILL), name
    rc, fused, crops = raw(e, 1, [poses[0], [0.0, -big, 0.0]], 8, 2)
    assert rc == _lib.RBPF_EINVAL and b"pose 1" in e._lib.rbpf_last_error(e._h)
    rc, fused, crops = raw(e, 1, poses, 269, 1)
    assert rc == _lib.RBPF_EINVAL and b"387" in e._lib.rbpf_last_error(e._h) and b"384" in e._lib.rbpf_last_error(e._h)
    assert e._lib.rbpf_local_map(None, 1, None, 1, None, 1, 0.05, 1, None, 0, None, None) == _lib.RBPF_EINVAL
    # n_poses * n * n >= 2^31: the count alone decides, before a pose is read
    rc, fused, crops = raw(e, 1, poses, 8, 2, n_poses=1 << 25)
    assert rc == _lib.RBPF_EINVAL and b"2^31" in e._lib.rbpf_last_error(e._h) and np.all(fused == FILL) and np.all(crops == FILL)
    # between the halves of a scan update
    ang, ranges, odo, truth = synthetic.make_log(2, 181)
    e.set_scan(ranges[0], ang)
    e.scan_update_begin(adj=False)
    rc, fused, crops = raw(e, 1, poses, 8, 2)
    assert rc == _lib.RBPF_ESTATE and np.all(fused == FILL) and np.all(crops == FILL)
    e.scan_update_end()
    rc, fused, crops = raw(e, 1, poses, 8, 2, wq=[3, 4], offset=[0.1, 0.0])   # the engine is still usable
    want = oracle_crops(e, [None, rendered(e, 1)], poses, 1, 8, 2, cell_of(e), (0.1, 0.0))
    assert rc == 0 and np.array_equal(crops, want) and np.array_equal(fused, LO.fuse(want, [3, 4], thr_of(e)))
    rc, fused, crops = raw(e, -1, three, 8, 2)                               # three poses, three particles, each its own
    assert rc == 0 and not np.any(crops == FILL) and np.all(fused[..., :3].sum(-1) <= 3)
    for bad in (dict(particle="worst"), dict(poses=np.zeros((2, 2))), dict(poses=np.zeros((0, 3))), dict(weights="heaviest"), dict(weights=[1.0]),
                dict(weights=[1.0, -1.0]), dict(weights=[0.0, 0.0]), dict(offset=(0.0,)), dict(cell=0.0), dict(size_m=-1.0)):
        args = dict(poses=poses, particle=1, weights=None)
        args.update(bad)
        with pytest.raises(ValueError):
            e.local_map(**args)
    e.close()


# ---- 8. no state change, device outputs ---------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_repeats_itself_and_writes_device_outputs():
    torch = pytest.importorskip("torch")
    P = 5
    rng = np.random.Generator(np.random.PCG64(21))
    e = engine(P)
    for p in range(P):
        c = rng.integers(-30, 31, size=(80, 80)).astype(np.int8)
        e.load_map(raster(e, (-40 + p, 40 + p, -40, 40), c), particle=p)
    e.set_state(poses=np.column_stack([rng.uniform(-1.5, 1.5, (P, 2)), rng.uniform(-np.pi, np.pi, P)]), weights=rng.uniform(0.0, 3.0, P))

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.map_extent()) + tuple(e.render_map(p).cells for p in range(P))

    s0 = state()
    a = e.local_map(size_m=3.2, crops=True)                                  # weights="resample", the engine's cell, each its own map
    b = e.local_map(size_m=3.2, crops=True)
    e.local_map(e.poses()[:3], particle="best", size_m=1.0, cell=0.02, samples=3, weights=[1.0, 0.0, 2.5], offset=(0.5, 0.0))
    assert a.crops.shape == (P, 64, 64) and a.crops.tobytes() == b.crops.tobytes() and fields(a).tobytes() == fields(b).tobytes()
    for x, y in zip(state(), s0):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    from thesis_amd.local import quantise_weights
    from thesis_amd.mapio import resample_weights
    assert a.total == int(quantise_weights(resample_weights(e.weights())).sum(dtype=np.uint64)) and 0 < a.total <= 1 << 30
    for crops in (True, False):
        d = e.local_map(size_m=3.2, crops=crops, device=True)
        for t in (d.occ_w, d.free_w, d.unknown_w, d.sum_wv):
            assert isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.int64 and tuple(t.shape) == (64, 64)
        assert np.array_equal(np.stack([t.cpu().numpy() for t in (d.occ_w, d.free_w, d.unknown_w, d.sum_wv)], axis=-1), fields(a)) and d.total == a.total
        # the shares are one float64 division each; a device may form it as a reciprocal and a product: 1.5 ulp at the most
        assert d.p_occ().dtype == torch.float64 and np.allclose(d.p_occ().cpu().numpy(), a.p_occ(), rtol=4e-16, atol=0.0)
        assert d.blocked(0.3, 0.1).dtype == torch.bool and np.array_equal(d.blocked(0.3, 0.1).cpu().numpy(), a.blocked(0.3, 0.1))
        if crops:
            assert d.crops.dtype == torch.int8 and np.array_equal(d.crops.cpu().numpy(), a.crops)
        else:
            assert d.crops is None
    odd = e.local_map(size_m=33 * cell_of(e), crops=True, device=True)       # n * n no multiple of 16: crops read byte by byte
    assert np.array_equal(odd.crops.cpu().numpy(), e.local_map(size_m=33 * cell_of(e), crops=True).crops)
    assert np.array_equal(odd.sum_wv.cpu().numpy(), e.local_map(size_m=33 * cell_of(e)).sum_wv)
    e.close()
