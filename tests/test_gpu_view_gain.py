"""View gain on the GPU (rbpf_view_gain, kernels_gain.hip) against the scalar oracle of tests/gain_oracle.py run on the rendered
maps: gain, seen and unknown, all three exactly.  Then what the call leaves alone, its device outputs, its argument checks, and
thesis_amd/explore.py's ranking."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.gain_oracle import classify, lattice_bounds, room16_cells, visited
from tests.test_gpu_cast import B, built_engine, engine, load_room16, raster, rng_state, room_poses, seam_scene

pytestmark = pytest.mark.gpu


def vmin_of(e):
    return int(round(float(e.cfg.min_odds_emp) / float(e.cfg.quantum)))


def oracle(e, p, poses, angles, max_range, tables):
    """The oracle on render_map(p): ([(gain [N], seen [N], unknown [N]) per table], steps)."""
    m = e.render_map(p)
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    inv = e.dim / float(e.cfg.tile_len_m)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = [(np.zeros(len(poses), np.int64), np.zeros(len(poses), np.int32), np.zeros(len(poses), np.int32)) for _ in tables]
    steps = 0
    for n, q in enumerate(poses):
        V, st = visited(m.cells, m.x0, m.y0, lo, hi, inv, float(e.cfg.quantum), float(e.cfg.occupied_threshold), q, angles, max_range)
        steps += st
        for o, t in zip(out, tables):
            o[0][n], o[1][n], o[2][n] = classify(V, m.cells, m.x0, m.y0, vmin_of(e), t)
    return out, steps


def assert_same(got, want, what=""):
    assert got.gain.dtype == np.int64 and got.seen.dtype == np.int32 and got.unknown.dtype == np.int32
    for name, g, w in zip(("gain", "seen", "unknown"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), f"{what}: {name} differs: got {g.tolist()}, oracle {w.tolist()}"


def random_table(seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, (1 << 20) + 1, size=61).astype(np.int32)


# ---- the exact room --------------------------------------------------------------------------------------------------------
def test_room16_equals_the_oracle():
    from thesis_amd import explore
    from thesis_amd.datasets import synthetic
    e = engine(4)
    load_room16(e)
    ang, poses = synthetic.beam_angles(B), room_poses()[:6]
    tabs = [explore.entropy_table(e.cfg), random_table(3)]
    tabs[1][[0, 30, 60]] = [1 << 20, 0, 1 << 20]                          # both ends of the admitted range
    want, steps = oracle(e, 2, poses, ang, 15.0, tabs)
    print(f"room16: {steps} oracle steps, seen {want[0][1].tolist()}, unknown {want[0][2].tolist()}")
    assert_same(e.view_gain(poses, ang, particle=2, max_range=15.0), want[0], "default table")
    assert_same(e.view_gain(poses, ang, particle=2, max_range=15.0, table=tabs[1]), want[1], "random table")
    one = e.view_gain(poses[3], ang, particle=0, max_range=15.0)          # a single [3] pose
    assert one.gain.shape == (1,) and one.gain[0] == want[0][0][3] and one.seen[0] == want[0][1][3]
    e.close()


# ---- maps the engine built ---------------------------------------------------------------------------------------------------
def test_built_maps_equal_the_oracle_for_every_particle():
    from thesis_amd import explore
    from thesis_amd.datasets import synthetic
    e = built_engine()
    P = e.P
    ang = synthetic.beam_angles(B)[::4]
    k = int(np.argmax(e.weights()))
    poses = e.poses()[k] + np.array([[0.0, 0.0, 0.0], [1.3, -0.9, 1.0], [-2.1, 1.7, -2.0]])
    got = e.view_gain(poses, ang, particle=None)                          # max_range: cfg.max_ray_m
    assert got.gain.shape == got.seen.shape == got.unknown.shape == (P, 3)
    tab = explore.entropy_table(e.cfg)
    steps = 0
    for p in range(P):
        want, st = oracle(e, p, poses, ang, float(e.cfg.max_ray_m), [tab])
        steps += st
        assert_same(type(got)(got.gain[p], got.seen[p], got.unknown[p]), want[0], f"particle {p} of particle=None")
    print(f"built maps: {steps} oracle steps; seen {got.seen[k].tolist()}, unknown {got.unknown[k].tolist()}")
    assert len({tuple(r) for r in got.gain.tolist()}) > 1                 # the particles hold different maps
    assert np.all(got.unknown > 0) and np.all(got.unknown < got.seen)
    for p in (k, (k + 5) % P):
        one = e.view_gain(poses, ang, particle=p)
        assert_same(one, (got.gain[p], got.seen[p], got.unknown[p]), f"particle={p}")
    assert_same(e.view_gain(poses, ang), (got.gain[k], got.seen[k], got.unknown[k]), "particle='best'")
    e.close()


# ---- seams, missing tiles, the lattice edge, the largest window ----------------------------------------------------------------
def largest_max_range(inv):
    """The largest float64 max_range with ceil(max_range * inv) <= 509 (a window of 1023 cells), and the next one up."""
    m = 509.0 / inv
    while math.ceil(m * inv) > 509:
        m = math.nextafter(m, 0.0)
    while math.ceil(math.nextafter(m, math.inf) * inv) <= 509:
        m = math.nextafter(m, math.inf)
    return m, math.nextafter(m, math.inf)


@pytest.mark.parametrize("cs", [0.05, 0.1, 0.025])
def test_seams_missing_tiles_and_the_lattice_edge(cs):
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs)) + 1))
    e = engine(2, cs=cs, pool_tiles=24, lattice_radius=1)
    dim, h = e.dim, e.dim // 2
    for b, c in seam_scene(dim, rng):
        e.load_map(raster(e, b, c), particle=1)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)     # another map, which must not be seen
    inv = dim / float(e.cfg.tile_len_m)
    lo, hi = lattice_bounds(dim, 1)
    col = lambda Y: (Y + dim + h) % dim                                   # tile-local column of mosaic Y (R = 1)
    cell = lambda X, Y, th: [(X + 0.3) / inv, (Y + 0.6) / inv, th]
    y31 = hi - 1 - (dim - 32) % 32                                        # the last column = 31 (mod 32) before the lattice's edge
    assert col(h) == 0 and col(31 - h) == 31 and col(h + 64) == 64 and col(y31) % 32 == 31 and hi - 32 <= y31 < hi
    mr_max, mr_over = largest_max_range(inv)
    assert math.ceil(mr_max * inv) == 509 and math.ceil(mr_over * inv) == 510
    corner = np.array([cell(h - 3, h, 0.4), cell(h + 2, 31 - h, -2.0)])              # the four-tile corner; columns 0 and 31
    edge = np.array([cell(hi - 9, h + 64, 0.1), cell(lo + 4, y31, 1.5),   # windows that leave the lattice
                     cell(hi + 3, 0, 0.0)])                               # an origin outside it: nothing
    inside = np.array([cell(-20, 11, 3.0), cell(-h - 25, -h - 245, 0.7), cell(3, -h - 60, -1.57)])
    cases = [(corner, synthetic.beam_angles(257, 2 * np.pi), 240 * cs), (edge, synthetic.beam_angles(65, 2 * np.pi), 150 * cs),
             (inside, np.array([0.3]), 300 * cs), (inside, synthetic.beam_angles(63), 90 * cs),
             (corner[:1], synthetic.beam_angles(65, 2 * np.pi), mr_max)]                # the widest window: 1023 cells
    tab = random_table(int(round(1000 * cs)))
    steps = 0
    for poses, ang, mr in cases:
        want, st = oracle(e, 1, poses, ang, mr, [tab])
        steps += st
        assert_same(e.view_gain(poses, ang, particle=1, max_range=mr, table=tab), want[0], f"cs {cs}, {len(ang)} beams, {mr} m")
    assert e.view_gain(edge, synthetic.beam_angles(65, 2 * np.pi), particle=1, max_range=150 * cs).seen[2] == 0
    print(f"cs {cs}: {steps} oracle steps; largest max_range {mr_max!r} m")
    # one float64 further the window is 1025 cells wide
    out = [np.full(1, -7, np.int64), np.full(1, -7, np.int32), np.full(1, -7, np.int32)]
    pose, ang = np.ascontiguousarray(corner[:1]), np.zeros(1)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    call = lambda mr: e._lib.rbpf_view_gain(e._h, 1, dp(pose), 1, dp(ang), 1, mr, tab.ctypes.data_as(C.POINTER(C.c_int32)), 0,
                                            *[C.c_void_p(o.ctypes.data) for o in out])
    assert call(mr_over) == _lib.RBPF_EINVAL and all(int(o[0]) == -7 for o in out)
    msg = e._lib.rbpf_last_error(e._h).decode()
    assert "largest admissible" in msg and f"{509.0 / inv:.6f}" in msg, msg
    assert call(mr_max) == 0 and out[1][0] > 0
    e.close()


# ---- a set, not a sum over rays --------------------------------------------------------------------------------------------------
def test_cells_are_counted_once():
    from thesis_amd import explore
    from thesis_amd.datasets import synthetic
    e = engine(2)
    load_room16(e, particle=0)
    pose = room_poses()[1:3]
    tab = explore.entropy_table(e.cfg)
    one = e.view_gain(pose, [0.7], particle=0, max_range=9.0)
    for n in (2, 64, 300):
        assert_same(e.view_gain(pose, [0.7] * n, particle=0, max_range=9.0), one, f"{n} identical beams")
    assert_same(one, oracle(e, 0, pose, [0.7], 9.0, [tab])[0][0], "one beam")
    # a dense fan in a fresh (all-unknown) map: near the sensor hundreds of beams cross the same cells
    fan = synthetic.beam_angles(720, 2 * np.pi)
    fresh = e.view_gain([0.31, -0.17, 0.2], fan, particle=1, max_range=4.0)
    want, steps = oracle(e, 1, [0.31, -0.17, 0.2], fan, 4.0, [tab])
    assert_same(fresh, want[0], "fresh map")
    assert fresh.seen[0] == fresh.unknown[0] and fresh.gain[0] == int(fresh.seen[0]) * int(tab[0 - vmin_of(e)])
    print(f"fresh map: {fresh.seen[0]} distinct cells from {steps} cell tests of 720 beams")
    assert steps > 2 * fresh.seen[0]
    e.close()


# ---- thresholds, the hit cell ----------------------------------------------------------------------------------------------------
def test_threshold_is_strict_and_the_hit_cell_is_seen():
    e = engine(2)
    assert float(e.cfg.occupied_threshold) / float(e.cfg.quantum) == 10.0
    c = np.zeros((12, 3), np.int8)
    c[5] = 10                                            # exactly the threshold: free, seen through
    c[7] = -30
    c[9] = 11                                            # the hit: seen
    c[10] = 11                                           # behind the hit: not seen
    c[11] = -30
    e.load_map(raster(e, (0, 12, -1, 2), c))
    inv = e.dim / float(e.cfg.tile_len_m)
    pose = np.array([[0.5 / inv, 0.5 / inv, 0.0]])
    hot = lambda v: (np.arange(-30, 31) == v).astype(np.int32)
    tabs = [np.ones(61, np.int32), hot(10), hot(11), hot(-30), hot(0)]
    want = oracle(e, 1, pose, [0.0], 5.0, tabs)[0]
    for t, w in zip(tabs, want):
        assert_same(e.view_gain(pose, [0.0], particle=1, max_range=5.0, table=t), w, "threshold")
    assert [int(w[0][0]) for w in want] == [10, 1, 1, 1, 7] and want[0][1][0] == 10 and want[0][2][0] == 7
    e.close()


# ---- read-only ---------------------------------------------------------------------------------------------------------------------
def test_a_view_gain_changes_nothing():
    from thesis_amd.datasets import synthetic
    e = built_engine(P=8, steps=6)
    ang = synthetic.beam_angles(181)

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.render_map(0).cells, e.render_map(5).cells, e.map_extent())

    def same(a, b):
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    s0 = state()
    first = e.view_gain(e.poses(), ang, particle=None)
    e.view_gain(e.poses() + 0.3, ang, particle=5, max_range=25.0, table=random_table(1))
    same(state(), s0)
    assert_same(e.view_gain(e.poses(), ang, particle=None), first, "the same call again")
    e.close()


def test_view_gains_interleaved_in_a_run_change_nothing():
    from thesis_amd.datasets import synthetic
    P, N = 16, 6
    ang, ranges, odo, truth = synthetic.make_log(N + 1, B)
    gang = synthetic.beam_angles(91)
    plain, mixed = engine(P, seed=11), engine(P, seed=11)
    for e in (plain, mixed):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))
    for k in range(N):
        for e in (plain, mixed):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            if e is mixed:
                e.view_gain(truth[:3], gang, particle=None)
            e.scan_update(adj=False)
            if e is mixed:
                e.view_gain(truth[:3], gang, particle=k % P)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)                             # an explicit u: the duplicate groups after it are used by the next match
            if e is mixed:
                e.view_gain(e.poses(), gang)
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    assert np.array_equal(mixed.render_map(3, box=box).cells, plain.render_map(3, box=box).cells)
    assert mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    plain.close(); mixed.close()


# ---- device outputs ----------------------------------------------------------------------------------------------------------------
def test_device_output_equals_host_output():
    torch = pytest.importorskip("torch")
    from thesis_amd.datasets import synthetic
    e = engine(4)
    load_room16(e)
    ang, poses = synthetic.beam_angles(361), room_poses()
    for particle in (1, None):
        hst = e.view_gain(poses, ang, particle=particle, max_range=9.0)
        dev = e.view_gain(poses, ang, particle=particle, max_range=9.0, device=True)
        assert all(isinstance(t, torch.Tensor) and t.device.type == "cuda" for t in dev)
        assert (dev.gain.dtype, dev.seen.dtype, dev.unknown.dtype) == (torch.int64, torch.int32, torch.int32)
        assert_same(type(hst)(*[t.cpu().numpy() for t in dev]), hst, f"device outputs, particle={particle}")
    assert hst.gain.shape == (4, len(poses)) and np.all(hst.gain == hst.gain[0])      # load_room16 wrote every particle
    # on a borrowed stream that is torch's current one, no extra synchronisation is needed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = e.view_gain(poses, ang, particle=None, max_range=9.0, device=True)
        total = d2.gain.sum() + d2.seen.sum() + d2.unknown.sum()          # consumed by torch in stream order
        same = all(torch.equal(a, b) for a, b in zip(d2, dev)) and int(total) == int(hst.gain.sum() + hst.seen.sum() + hst.unknown.sum())
        e.release_stream()
    assert same
    e.close()


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib, explore
    from thesis_amd.datasets import synthetic
    P, N, NB = 4, 3, 16
    e = engine(P)
    load_room16(e)
    ang = synthetic.beam_angles(NB)
    poses = np.zeros((N, 3))
    tab = explore.entropy_table(e.cfg)
    gain, seen, unk = np.full((P, N), -7, np.int64), np.full((P, N), -7, np.int32), np.full((P, N), -7, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(particle=0, ps=poses, n=N, a=ang, nb=NB, mr=15.0, t=tab, flags=0, g=gain, s=seen, u=unk):
        return e._lib.rbpf_view_gain(e._h, particle, dp(ps), n, dp(a), nb, mr, None if t is None else t.ctypes.data_as(C.POINTER(C.c_int32)),
                                     flags, vp(g), vp(s), vp(u))

    def untouched():
        return np.all(gain == -7) and np.all(seen == -7) and np.all(unk == -7)
    bad_pose, bad_ang, inf_pose, neg_tab, big_tab = poses.copy(), ang.copy(), poses.copy(), tab.copy(), tab.copy()
    bad_pose[2, 1] = np.nan
    bad_ang[5] = np.inf
    inf_pose[0, 2] = -np.inf
    neg_tab[17] = -1
    big_tab[60] = (1 << 20) + 1
    cases = dict(particle_high=dict(particle=P), particle_low=dict(particle=-2), no_gain=dict(g=None), no_poses=dict(ps=None),
                 no_angles=dict(a=None), no_table=dict(t=None), range_zero=dict(mr=0.0), range_neg=dict(mr=-1.0),
                 range_inf=dict(mr=np.inf), range_nan=dict(mr=np.nan), range_wide=dict(mr=26.0), nan_pose=dict(ps=bad_pose),
                 inf_theta=dict(ps=inf_pose), inf_angle=dict(a=bad_ang), no_beams=dict(nb=0), no_poses_count=dict(n=0),
                 neg_poses=dict(n=-1), too_many_rays=dict(n=1 << 16, nb=1 << 15), table_neg=dict(t=neg_tab), table_big=dict(t=big_tab),
                 flags=dict(flags=2))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert untouched(), name
    # between the two halves of a scan update the maps are in flux
    ranges = synthetic.cast_scan((0.0, 0.0, 0.0), synthetic.beam_angles(B), None)
    e.set_scan(ranges, synthetic.beam_angles(B))
    e.scan_update_begin(adj=False)
    assert call() == _lib.RBPF_ESTATE and call(particle=-1) == _lib.RBPF_ESTATE and untouched()
    e.scan_update_end()
    assert call() == 0 and np.all(gain[0] > 0) and np.all(seen[0] > 0) and np.all(gain[1:] == -7)    # the engine is still usable
    gain[:] = -7
    assert call(s=None, u=None) == 0 and np.all(gain[0] > 0) and np.all(seen[1:] == -7)              # seen and unknown may be NULL
    assert call(particle=-1) == 0 and np.all(gain > 0) and np.all(unk >= 0)
    with pytest.raises(ValueError):
        e.view_gain(np.zeros((2, 4)), ang)
    with pytest.raises(ValueError):
        e.view_gain(poses, ang, particle="worst")
    with pytest.raises(ValueError):
        e.view_gain(poses, ang, table=np.ones(60, np.int32))
    e.close()


# ---- explore.next_view -------------------------------------------------------------------------------------------------------------
def test_next_view_looks_into_the_unknown_half():
    from thesis_amd import explore
    from thesis_amd.datasets import synthetic
    cells, x0, y0 = room16_cells()
    cells[cells == 0] = -30                              # the room observed ...
    cells[200:] = 0                                      # ... but for its right half (X >= 0)
    e = engine(2)
    e.load_map(raster(e, (x0, x0 + 400, y0, y0 + 400), cells))
    ang = synthetic.beam_angles(61, np.pi / 2)           # a 90 degree fan: a view into the known half sees nothing unknown
    kw = dict(k=8, spacing_m=2.0, n_headings=8, clearance_cells=4, max_range=8.0)
    nv = explore.next_view(e, ang, particle="best", **kw)
    cand = nv.candidates
    assert len(cand) >= 32 and len(cand) % 8 == 0 and np.all(np.abs(cand[:, 0] + 0.025) < 1e-12)     # on the frontier column X = -1
    want, steps = oracle(e, 0, cand, ang, 8.0, [explore.entropy_table(e.cfg)])
    print(f"next_view: {len(cand)} candidates, {steps} oracle steps; best {nv.poses[0].tolist()} with {nv.scores[0]:.1f} bits")
    assert np.array_equal(nv.gain, want[0][0])
    order, scores = explore.rank(want[0][0], k=8)
    assert np.array_equal(nv.order, order) and np.array_equal(nv.scores, scores[order]) and np.array_equal(nv.poses, cand[order])
    assert np.all(np.cos(nv.poses[:4, 2]) > 0.5)         # the best views face +x, the unknown half
    # an unknown cell is worth 3.6 observed ones (65536 : 18101 with the default table)
    assert nv.scores[0] > 2 * scores[np.argmin(scores)] and np.cos(cand[np.argmin(scores), 2]) < -0.5
    every = explore.next_view(e, ang, particle=None, weights=[3.0, 1.0], **kw)       # both particles hold this map
    assert every.gain.shape == (2, len(cand)) and np.array_equal(every.order, nv.order) and np.array_equal(every.scores, nv.scores)
    e.close()
