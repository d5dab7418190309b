"""Map building on the GPU (rbpf_build_map, kernels_build.hip) against the scalar oracle of tests/build_oracle.py: hits and seen,
both rasters exactly, every cell.  Then accumulation, device outputs, the argument checks, what the call leaves alone, and a run
rebuilt end to end (thesis_amd/rebuild.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.build_oracle import build_map as oracle_build
from tests.test_gpu_cast import B, engine, rng_state, room_poses
from tests.test_gpu_view_gain import largest_max_range

pytestmark = pytest.mark.gpu


def box_of(m):
    return (m.x0, m.x0 + m.hits.shape[0], m.y0, m.y0 + m.hits.shape[1])


def assert_same(got, want, what=""):
    assert got.hits.dtype == np.int32 and got.seen.dtype == np.int32
    for name, g, w in zip(("hits", "seen"), (got.hits, got.seen), want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = g != w
        if bad.any():
            k = tuple(int(q) for q in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {name} differs in {int(bad.sum())} of {bad.size} cells; first {k} (cell "
                                 f"{k[0] + got.x0}, {k[1] + got.y0}): got {g[k]}, oracle {w[k]}")


def check(e, poses, ranges, angles, what, cell_size=None, box=None, min_range=0.0, max_range=None):
    """build_map against the oracle over the same box; returns (BuiltMap, oracle steps)."""
    got = e.build_map(poses, ranges, angles, cell_size=cell_size, box=box, min_range=min_range, max_range=max_range)
    mr = float(e.cfg.max_ray_m) if max_range is None else max_range
    h, s, steps = oracle_build(poses, ranges, angles, got.cells_per_m, box_of(got), min_range, mr)
    assert_same(got, (h, s), what)
    assert np.all(got.hits >= 0) and np.all(got.hits <= got.seen) and got.seen.max() <= len(np.atleast_2d(ranges))
    return got, steps


def odd_ranges(ranges, min_range, max_range):
    """A handful of the ranges replaced by what is data and not an error: NaN, +inf, 0, one below min_range, one above max_range."""
    r = np.array(ranges, dtype=np.float64)
    flat = r.reshape(-1)
    for k, v in zip(range(3, flat.size, max(flat.size // 11, 1)), [np.nan, np.inf, 0.0, 0.5 * min_range, 1.5 * max_range, -np.inf, -1.0] * 2):
        flat[k] = v
    return r


# ---- 1. one scan, a box that cuts its window ------------------------------------------------------------------------------------
def test_one_scan_in_a_box_that_cuts_its_window():
    from thesis_amd.datasets import synthetic
    e = engine(2)
    ang = synthetic.beam_angles(61, 2 * np.pi)           # not a multiple of 64
    rng = np.random.Generator(np.random.PCG64(1))
    pose = np.array([[0.31, -0.17, 0.2]])                # cell (6, -4) at 0.05 m; 3 m is a window of 125 cells
    ranges = odd_ranges(rng.uniform(0.3, 3.6, (1, 61)), 0.2, 3.0)
    box = (6 - 40, 6 + 35, -4 - 30, -4 + 41)             # cut on all four sides; 71 columns
    got, steps = check(e, pose, ranges, ang, "one scan", box=box, min_range=0.2, max_range=3.0)
    assert got.hits.shape == (75, 71) and got.cell_size == 0.05 and got.cells_per_m == e.dim / float(e.cfg.tile_len_m)
    assert got.seen[40, 30] == 1 and got.seen.max() == 1 and 0 < got.hits.sum() < 61
    full, _ = check(e, pose, ranges, ang, "one scan, default box", min_range=0.2, max_range=3.0)
    assert box_of(full) == (6 - 62, 6 + 63, -4 - 62, -4 + 63)                       # floor(x inv) -+ (ceil(3 * 20) + 2)
    assert np.array_equal(full.seen[62 - 40:62 + 35, 62 - 30:62 + 41], got.seen) and full.seen.sum() > got.seen.sum()
    one = e.build_map(pose[0], ranges[0], ang, box=box, min_range=0.2, max_range=3.0)      # a single [3] pose and [B] scan
    assert_same(one, (got.hits, got.seen), "1-D arguments")
    print(f"one scan: {steps} oracle steps, {int(got.seen.sum())} of {int(full.seen.sum())} seen cells in the box")
    e.close()


# ---- 2. overlapping scans: the adds across workgroups -----------------------------------------------------------------------------
def room_scans(n_beams=181, min_range=0.3, max_range=9.0):
    from thesis_amd.datasets import synthetic
    ang, poses = synthetic.beam_angles(n_beams), np.concatenate([room_poses(), room_poses()])[:12]   # 12 poses, some of them twice
    ranges = np.stack([synthetic.cast_scan(p, ang, None) for p in poses])
    return poses, odd_ranges(ranges, min_range, max_range), ang


def test_overlapping_scans_equal_the_oracle_in_every_cell():
    e = engine(2)
    poses, ranges, ang = room_scans()
    assert poses.shape == (12, 3) and np.isnan(ranges).sum() >= 2 and np.isinf(ranges).sum() >= 2 and (ranges == 0).sum() >= 2
    got, steps = check(e, poses, ranges, ang, "room16", min_range=0.3, max_range=9.0)
    print(f"room16: {steps} oracle steps; hits up to {got.hits.max()}, seen up to {got.seen.max()} of 12 scans, "
          f"{int((got.seen > 0).sum())} cells seen")
    assert got.seen.max() >= 2 and got.hits.max() >= 2          # at the least where a pose comes twice
    assert got.hits.sum() < ranges.size                  # sets per scan: neighbouring beams end in the same wall cell
    e.close()


# ---- 3. other cell sizes, negative coordinates, a pose outside the box, a pose on a cell corner -----------------------------------------
@pytest.mark.parametrize("cs", [0.1, 0.025, 0.07])
def test_any_cell_size(cs):
    e = engine(2)                                        # the engine's own cells are 0.05 m
    inv = 1.0 / cs
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs))))
    ang = np.concatenate([np.arange(8) * (np.pi / 4), rng.uniform(-np.pi, np.pi, 53)])         # 61 beams, eight at multiples of 45 degrees
    poses = np.array([[0.0, 0.0, 0.0],                   # exactly on the corner of cell (0, 0)
                      [-1.37, -0.52, 2.0], [-0.013, 0.4, -1.0],                                # negative coordinates
                      [3.9, 0.3, 3.0]])                  # outside the box below, looking into it
    ranges = odd_ranges(rng.uniform(0.0, 5.0, (4, 61)), 0.1, 4.0)
    ranges[0, :8] = [1.0, 2.0, 3.0, 3.5, np.inf, 0.7, 2.2, 1.1]
    ranges[3, 0] = 3.8                                   # straight ahead, from outside into the box
    m = math.ceil(4.0 * inv) + 2
    box = (math.floor(-1.37 * inv) - m + 9, math.floor(2.0 * inv), math.floor(-0.52 * inv) - m + 5, math.floor(0.4 * inv) + m - 3)
    assert math.floor(3.9 * inv) >= box[1]
    got, steps = check(e, poses, ranges, ang, f"cs {cs}", cell_size=cs, box=box, min_range=0.1, max_range=4.0)
    assert got.cell_size == cs and got.cells_per_m == inv and got.seen.max() >= 2   # two 4-connected walks that cross share a cell
    alone, _ = check(e, poses[3:], ranges[3:], ang, f"cs {cs}, the pose outside", cell_size=cs, box=box, min_range=0.1, max_range=4.0)
    assert alone.seen.any() and alone.hits.any()
    away = e.build_map(poses[3:] + [40.0, 0.0, 0.0], ranges[3:], ang, cell_size=cs, box=box, max_range=4.0)   # a window that misses the box
    assert not away.hits.any() and not away.seen.any()
    check(e, poses, ranges, ang, f"cs {cs}, default box", cell_size=cs, min_range=0.1, max_range=4.0)
    print(f"cs {cs}: {steps} oracle steps in a box of {got.hits.shape}")
    e.close()


# ---- 4. the widest window --------------------------------------------------------------------------------------------------------
def test_the_widest_window_and_one_cell_more():
    from thesis_amd import _lib
    e = engine(2)
    inv = e.dim / float(e.cfg.tile_len_m)
    mr_max, mr_over = largest_max_range(inv)
    assert math.ceil(mr_max * inv) == 509 and math.ceil(mr_over * inv) == 510
    rng = np.random.Generator(np.random.PCG64(4))
    ang = np.linspace(-np.pi, np.pi, 64, endpoint=False)
    poses = np.array([[0.31, -0.17, 0.1], [-7.77, 3.21, -2.0]])
    ranges = rng.uniform(0.0, 1.2 * mr_max, (2, 64))
    ranges[:, ::4] = np.inf                              # free beams run the whole 509 cells
    got, steps = check(e, poses, ranges, ang, "widest window", max_range=mr_max)   # the full oracle: a second on the CPU
    assert got.hits.shape[0] >= 1023 and got.hits.shape[1] >= 1023
    print(f"widest window: {steps} oracle steps, box {got.hits.shape}, largest max_range {mr_max!r} m")
    # one float64 further the window is 1025 cells wide
    hits, seen = np.full((8, 8), -7, np.int32), np.full((8, 8), -7, np.int32)
    b4 = np.array([0, 8, -8, 0], np.int32)            # holds the pose's cell (6, -4)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p1, r1, a1 = np.ascontiguousarray(poses[:1]), np.ones(1), np.zeros(1)
    call = lambda mr: e._lib.rbpf_build_map(e._h, dp(p1), 1, dp(r1), dp(a1), 1, inv, b4.ctypes.data_as(C.POINTER(C.c_int32)), 0.0, mr, 0,
                                            C.c_void_p(hits.ctypes.data), C.c_void_p(seen.ctypes.data))
    assert call(mr_over) == _lib.RBPF_EINVAL and np.all(hits == -7) and np.all(seen == -7)
    msg = e._lib.rbpf_last_error(e._h).decode()
    assert "largest admissible" in msg and f"{509.0 / inv:.6f}" in msg, msg
    assert call(mr_max) == 0 and seen[6, 4] == 1 and seen.min() == 0 and not hits.any()   # the beam ends 20 cells away
    with pytest.raises(Exception, match="largest admissible"):
        e.build_map(poses, ranges, ang, cell_size=0.025, max_range=15.0)           # 600 cells
    e.close()


# ---- 5. accumulation, device outputs, repeatability ---------------------------------------------------------------------------------
def test_accumulate_device_outputs_and_repeatability():
    torch = pytest.importorskip("torch")
    e = engine(2)
    poses, ranges, ang = room_scans()
    kw = dict(min_range=0.3, max_range=9.0)
    whole = e.build_map(poses, ranges, ang, **kw)
    again = e.build_map(poses, ranges, ang, **kw)
    assert_same(again, (whole.hits, whole.seen), "the same call again")
    box = box_of(whole)
    first = e.build_map(poses[:7], ranges[:7], ang, box=box, **kw)
    both = e.build_map(poses[7:], ranges[7:], ang, into=first, **kw)
    assert both.hits is first.hits and both.seen is first.seen
    assert_same(both, (whole.hits, whole.seen), "two halves, accumulated")
    assert not np.array_equal(e.build_map(poses[:7], ranges[:7], ang, box=box, **kw).seen, whole.seen)
    dev = e.build_map(poses, ranges, ang, device=True, **kw)
    assert all(isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.int32 for t in (dev.hits, dev.seen))
    assert box_of(dev) == box
    assert_same(type(dev)(dev.hits.cpu().numpy(), dev.seen.cpu().numpy(), *dev[2:]), (whole.hits, whole.seen), "device outputs")
    d1 = e.build_map(poses[:7], ranges[:7], ang, box=box, device=True, **kw)
    d2 = e.build_map(poses[7:], ranges[7:], ang, into=d1, **kw)                   # `into` decides where the outputs live
    assert d2.hits is d1.hits and torch.equal(d2.hits, dev.hits) and torch.equal(d2.seen, dev.seen)
    # on a borrowed stream that is torch's current one, no extra synchronisation is needed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d3 = e.build_map(poses, ranges, ang, device=True, **kw)
        total = int(d3.hits.sum() + d3.seen.sum())       # consumed by torch in stream order
        e.release_stream()
    assert total == int(whole.hits.sum()) + int(whole.seen.sum())
    with pytest.raises(ValueError):
        e.build_map(poses, ranges, ang, into=first, cell_size=0.1, **kw)          # another cell size
    with pytest.raises(ValueError):
        e.build_map(poses, ranges, ang, into=first, box=(0, 4, 0, 4), **kw)       # another box
    with pytest.raises(ValueError):
        e.build_map(poses, ranges[:, :5], ang, **kw)                               # ranges are [N, B]
    e.close()


# ---- 6. arguments; nothing else changes ---------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    N, NB = 3, 16
    e = engine(2)
    inv0 = e.dim / float(e.cfg.tile_len_m)
    ang = synthetic.beam_angles(NB)
    poses = np.zeros((N, 3))
    ranges = np.full((N, NB), 2.0)
    box = np.array([-50, 50, -40, 40], np.int32)
    hits, seen = np.full((100, 80), -7, np.int32), np.full((100, 80), -7, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(ps=poses, n=N, rg=ranges, a=ang, nb=NB, inv=inv0, b=box, lo=0.0, hi=5.0, flags=0, h=hits, s=seen):
        return e._lib.rbpf_build_map(e._h, dp(ps), n, dp(rg), dp(a), nb, inv, None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)),
                                     lo, hi, flags, vp(h), vp(s))

    def untouched():
        return np.all(hits == -7) and np.all(seen == -7)
    bad_pose, inf_pose, bad_ang = poses.copy(), poses.copy(), ang.copy()
    bad_pose[2, 1] = np.nan
    inf_pose[0, 2] = -np.inf
    bad_ang[5] = np.inf
    i32 = lambda *v: np.array(v, np.int32)
    cases = dict(no_poses=dict(ps=None), no_ranges=dict(rg=None), no_angles=dict(a=None), no_box=dict(b=None), no_outputs=dict(h=None, s=None),
                 no_scans=dict(n=0), neg_scans=dict(n=-1), no_beams=dict(nb=0), too_many_rays=dict(n=1 << 16, nb=1 << 15),
                 empty_box_x=dict(b=i32(5, 5, 0, 8)), empty_box_y=dict(b=i32(0, 8, 3, 2)),
                 huge_box=dict(b=i32(-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1)), big_box=dict(b=i32(0, 1 << 16, 0, (1 << 15) + 1)),
                 nan_pose=dict(ps=bad_pose), inf_theta=dict(ps=inf_pose), inf_angle=dict(a=bad_ang),
                 inv_nan=dict(inv=np.nan), inv_inf=dict(inv=np.inf), inv_zero=dict(inv=0.0), inv_neg=dict(inv=-20.0),
                 min_nan=dict(lo=np.nan), min_inf=dict(lo=np.inf), min_neg=dict(lo=-0.1),
                 max_nan=dict(hi=np.nan), max_inf=dict(hi=np.inf), max_zero=dict(hi=0.0), max_neg=dict(hi=-1.0),
                 flags=dict(flags=4), window=dict(hi=26.0))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert untouched(), name
    # a NaN or an infinite range is data
    odd = ranges.copy()
    odd[0, :4] = [np.nan, np.inf, -np.inf, 0.0]
    assert call(rg=odd) == 0 and seen.max() == N and hits.max() == N and seen.min() == 0
    hits[:], seen[:] = -7, -7
    # between the two halves of a scan update the handle's stream and scratch are spoken for
    full = synthetic.beam_angles(B)
    e.set_scan(synthetic.cast_scan((0.0, 0.0, 0.0), full, None), full)
    e.scan_update_begin(adj=False)
    assert call() == _lib.RBPF_ESTATE and untouched()
    e.scan_update_end()
    assert call(s=None) == 0 and hits.max() == N and np.all(seen == -7)              # either output may be NULL
    hits[:] = -7
    assert call(h=None) == 0 and seen.max() == N and np.all(hits == -7)
    assert call(flags=_lib.RBPF_BUILD_ACCUMULATE) == 0 and seen.max() == 2 * N and seen.min() == 0 and hits.max() == N - 7 and hits.min() == -7
    e.close()


def test_builds_interleaved_in_a_run_change_nothing():
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
                e.build_map(truth[:3], ranges[:3, ::6], ang[::6], max_range=6.0)
            e.scan_update(adj=False)
            if e is mixed:
                e.build_map(truth[k:k + 2], ranges[k:k + 2], ang, cell_size=0.1)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)                             # an explicit u: the duplicate groups after it are used by the next match
            if e is mixed:
                e.build_map(e.poses()[:4], ranges[:4, ::6], ang[::6], max_range=6.0, device=True)
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    assert rng_state(mixed) == rng_state(plain) and mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    for p in (0, 3, P - 1):
        assert np.array_equal(mixed.render_map(p, box=box).cells, plain.render_map(p, box=box).cells)
    plain.close(); mixed.close()


# ---- 7. a run, rebuilt ------------------------------------------------------------------------------------------------------------
def test_a_run_rebuilt_at_half_the_cell_size():
    from thesis_amd import rebuild
    from thesis_amd.datasets import synthetic
    from thesis_amd.slam import ParticleFilter
    steps, nb = 20, 121
    ang, ranges, odo, truth = synthetic.make_log(steps, nb)
    pf = ParticleFilter(64, ang, seed=5, history="device", keep_scans=True)
    pf.map_update(ranges[0])
    for k in range(steps):
        pf.imu_update(odo[k], 1000.0)
        pf.map_update(ranges[k + 1])
        pf.resample()
    e = pf.engine
    assert pf.scans.records == list(range(1, 2 * steps + 2, 2)) and e.track_info()["n_records"] == 2 * steps + 2
    got = rebuild.rebuild(e, pf.scans, ang, particle="best", cell_size=0.025, max_range=8.0)
    path = e.trajectory("best")[pf.scans.records]
    rec, kept = pf.scans.ranges_for()
    assert np.array_equal(kept, ranges) and got.cell_size == 0.025 and got.cells_per_m == 40.0
    h, s, n_steps = oracle_build(path, ranges, ang, 40.0, box_of(got), 0.0, 8.0)
    assert_same(got, (h, s), "rebuilt run")
    ci, cj = np.floor(path[:, 0] * 40.0).astype(int) - got.x0, np.floor(path[:, 1] * 40.0).astype(int) - got.y0
    assert ci.min() >= 0 and cj.min() >= 0 and ci.max() < got.hits.shape[0] and cj.max() < got.hits.shape[1]    # the box holds the trajectory
    assert np.all(got.hits <= got.seen) and got.seen.max() <= steps + 1 and np.all(got.seen[ci, cj] >= 1)
    mean = rebuild.rebuild(e, pf.scans, ang, particle="mean", cell_size=0.025, max_range=8.0)
    assert mean.seen.max() <= steps + 1 and mean.hits.sum() > 0
    src = rebuild.as_source(got, engine=e)
    assert src.cell_size == 0.025 and src.cells.dtype == np.int8 and (src.cells > 0).any() and (src.cells < 0).any()
    fresh = engine(2)
    placed = fresh.place_map(src, particle=0)
    cells = fresh.render_map(0, box=placed).cells
    assert (cells > 0).any() and (cells < 0).any()
    print(f"rebuilt run: {n_steps} oracle steps, raster {got.hits.shape}, {int((got.hits > 0).sum())} cells hit, placed in {placed}")
    fresh.close()
    pf.close()


def test_a_full_trajectory_log_keeps_no_scan_without_a_record():
    from thesis_amd import rebuild
    from thesis_amd.datasets import synthetic
    from thesis_amd.slam import ParticleFilter
    ang, ranges, odo, _ = synthetic.make_log(3, 61)
    pf = ParticleFilter(4, ang, history="device", history_capacity=4, keep_scans=True)     # record 0 is the start
    pf.map_update(ranges[0])                             # record 1
    pf.imu_update(odo[0], 1000.0)                        # record 2
    pf.map_update(ranges[1])                             # record 3: the log is full
    pf.imu_update(odo[1], 1000.0)
    pf.map_update(ranges[2])                             # dropped: no record, no scan kept
    info = pf.engine.track_info()
    assert info["n_records"] == 4 and info["dropped"] == 2 and pf.scans.records == [1, 3]
    got = rebuild.rebuild(pf.engine, pf.scans, ang, particle=0, max_range=6.0)
    path = pf.engine.lineage([0])[1][:, 0, :]
    h, s, _ = oracle_build(path[[1, 3]], ranges[:2], ang, got.cells_per_m, box_of(got), 0.0, 6.0)
    assert_same(got, (h, s), "two kept scans")
    with pytest.raises(ValueError):
        ParticleFilter(4, ang, keep_scans=True)          # scans are kept under the records of the device log
    assert ParticleFilter.__init__.__kwdefaults__["keep_scans"] is False
    pf.close()
