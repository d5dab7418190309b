"""Path checks on the GPU (rbpf_check_paths, kernels_paths.hip) against the scalar oracle of
tests/paths_oracle.py run on the rendered maps: all four results of every (particle, path) by equality.  Then every particle
at once and each its own, maps the engine built, the seeded fuzz, what the call leaves alone, its device outputs, its argument
checks, and a path planned, checked and cut short."""
import ctypes as C

import numpy as np
import pytest

from tests import paths_oracle as PO
from tests import travel_oracle as T
from tests.cast_oracle import lattice_bounds
from tests.test_gpu_cast import built_engine, engine, load_room16, raster, rng_state, seam_scene

pytestmark = pytest.mark.gpu

SETTINGS = ((0, 1), (7, 8), (20, 21), (20, 320))
FILL = -77


def inv_of(e):
    return e.dim / float(e.cfg.tile_len_m)


def metres(e, cells):
    """Cell centres in metres, [..., 2]."""
    return (np.asarray(cells, dtype=np.float64) + 0.5) / inv_of(e)


def radius(e, inflate):
    """A radius_m that check_paths turns into exactly `inflate`: floor(radius * inv * 5)."""
    return (inflate + 0.5) / (inv_of(e) * 5.0)


def box_of(e, paths):
    """The smallest box holding the cells of every waypoint, and so every walked cell and every side cell."""
    c = np.concatenate([T.cells_of(np.asarray(p, dtype=np.float64)[:, :2], inv_of(e)) for p in paths])
    return (int(c[:, 0].min()), int(c[:, 0].max()) + 1, int(c[:, 1].min()), int(c[:, 1].max()) + 1)


def oracle(e, p, paths, inflate, clear_max, through=False, exempt=False):
    """(int32 [K, 4], steps int32 [K]) of the oracle on render_map(p) over the paths' box grown by the margin."""
    box = box_of(e, paths)
    grown = e.render_map(p, box=T.grown_box(box, clear_max)).cells
    f = PO.Field(grown, box, float(e.cfg.quantum), float(e.cfg.occupied_threshold), inflate, clear_max, through)
    return f.check_xy(paths, inv_of(e), exempt)


def stacked(chk):
    return np.stack([np.asarray(a) for a in chk[:4]], axis=-1)


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape, got.dtype)
    bad = np.argwhere(got != want)
    if len(bad):
        k = tuple(int(q) for q in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at {k}: got {got[k[:-1]].tolist() if got.ndim > 1 else got[k]}, "
                             f"oracle {want[k[:-1]].tolist() if want.ndim > 1 else want[k]}")


def expect(e, p, paths, inflate, clear_max, through=False, exempt=False, what=""):
    """check_paths of one particle equals the oracle; returns the PathCheck."""
    chk = e.check_paths(paths, particle=p, radius_m=radius(e, inflate), clear_max=clear_max, through_unknown=through, start_exempt=exempt)
    assert (chk.inflate, chk.clear_max) == (inflate, clear_max)
    res, steps = oracle(e, p, paths, inflate, clear_max, through, exempt)
    label = f"{what} inflate {inflate} clear_max {clear_max} through {through} exempt {exempt}"
    same(stacked(chk), res, label)
    same(chk.steps, steps, label + " steps")
    return chk


def scene_engine(P=1, **kw):
    """The fuzz scene in particle 0's map at negative coordinates across the seam X = -dim / 2: (engine, (x0, y0), cells)."""
    e = engine(P, **kw)
    x0, y0 = -e.dim // 2 - 77, -31
    c = PO.fuzz_scene()
    e.load_map(raster(e, (x0, x0 + c.shape[0], y0, y0 + c.shape[1]), c), particle=0)
    return e, (x0, y0), c


def snake(rng, n_steps, shape):
    """Waypoint cells of a path of exactly n_steps steps inside a raster of `shape`: random legs, then one along x."""
    pts = [rng.integers(0, np.array(shape))]
    left = n_steps - 1
    while left > 90:
        q = rng.integers(0, np.array(shape))
        n = int(np.abs(q - pts[-1]).max())
        if 0 < n <= left - 1:
            pts.append(q)
            left -= n
    last = pts[-1].copy()
    last[0] += left if last[0] + left < shape[0] else -left
    return np.array(pts + [last])


# ---- 1. lengths, octants, repeats ---------------------------------------------------------------------------------------------------
def test_lengths_octants_and_repeats_equal_the_oracle():
    e, (x0, y0), c = scene_engine()
    rng = np.random.default_rng(3)
    origin = np.array([x0, y0])
    paths = [metres(e, snake(rng, n, c.shape) + origin) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1100)]
    a = np.array([x0 + 50, y0 + 70])
    for d in ((9, 0), (9, 4), (9, 9), (4, 9), (0, 9), (-4, 9), (-9, 9), (-9, 4), (-9, 0), (-9, -4), (-9, -9), (-4, -9), (0, -9), (4, -9), (9, -9), (9, -4)):
        paths.append(metres(e, [a, a + d]))                                 # the axes, the exact diagonals and both halves of every quadrant
    paths.append(metres(e, [a, a, a + (3, 1), a + (3, 1), a + (3, 1), a + (-2, 6), a + (-2, 6)]))      # repeated waypoints
    paths.append(metres(e, [a, a + (12, 5), a + (3, -7), a]))              # back to its first cell
    paths.append(metres(e, [a + (0, 1), a, a + (0, 1), a]))
    chk = None
    for inflate, clear_max in SETTINGS[:2]:
        for through, exempt in ((False, False), (True, False), (False, True), (True, True)):
            chk = expect(e, 0, paths, inflate, clear_max, through, exempt, "lengths")
    assert chk.steps[:9].tolist() == [1, 2, 63, 64, 65, 255, 256, 257, 1100] and chk.steps[9:25].tolist() == [10] * 16
    assert chk.steps[25:].tolist() == [9, 32, 4]
    chk = expect(e, 0, paths, 20, 320, False, False, "lengths")
    assert chk.clear.any() and not chk.clear.all() and chk.min_clearance.max() > 21
    assert np.allclose(chk.clearance_metres(), chk.min_clearance * (0.05 / 5))
    e.close()


# ---- 2. the least of two blocked steps, unknown steps across a wave ---------------------------------------------------------------
def test_the_least_blocked_step_wins_across_lanes_and_rounds():
    e = engine(1)
    for first, second in ((70, 200), (67, 130), (130, 195), (3, 64), (63, 64)):      # lanes 6 / 8, 3 / 2, 2 / 3, 3 / 0, 63 / 0
        c = np.full((5, 300), PO.FREE, np.int8)
        c[2, 10 + first] = c[2, 10 + second] = PO.WALL
        c[0, 40:141] = 0                                                    # 101 unknown cells beside the way
        e.load_map(raster(e, (100, 105, -150, 150), c))
        way = metres(e, [(102, -140), (102, 120)])
        chk = expect(e, 0, [way, way[::-1], metres(e, [(100, -140), (100, 120)])], 0, 1, what=f"walls at {first}, {second}")
        assert chk.first_blocked.tolist() == [first, 260 - second, 30] and chk.first_unknown.tolist() == [-1, -1, 30]
        assert chk.n_unknown.tolist() == [0, 0, 101] and chk.steps.tolist() == [261] * 3
        chk = expect(e, 0, [way], 7, 8, what=f"walls at {first}, {second}")
        assert chk.first_blocked[0] == first - 1
    e.close()


# ---- 3. seams, partial occupancy words, missing tiles, the lattice edge ----------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_seams_missing_tiles_and_the_lattice_edge(cs):
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs))))
    e = engine(2, cs=cs, pool_tiles=24, lattice_radius=1)
    assert e.dim == int(round(40 / cs))
    scenes = seam_scene(e.dim, rng)
    for b, c in scenes:
        e.load_map(raster(e, b, np.where(c > 10, c, np.where(rng.random(c.shape) < 0.1, 0, PO.FREE)).astype(np.int8)), particle=1)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)     # another map, which must not be seen
    lo, hi = lattice_bounds(e.dim, 1)
    k = np.where(rng.random((30, 30)) < 0.05, PO.WALL, PO.FREE).astype(np.int8)
    e.load_map(raster(e, (hi - 30, hi, lo, lo + 30), k), particle=1)        # the lattice's corner
    regions = [b for b, _ in scenes[:3]] + [(hi - 40, hi, lo, lo + 40)]
    for b in regions:
        # around the written box too: cells of a tile never written, and tiles that are not there
        g = (max(b[0] - 25, lo), min(b[1] + 25, hi), max(b[2] - 25, lo), min(b[3] + 25, hi))
        paths = PO.fuzz_paths(rng, 60, (g[1] - g[0], g[3] - g[2]), (g[0], g[2]), inv_of(e), leg=40)
        for inflate, clear_max in SETTINGS:
            expect(e, 1, list(paths), inflate, clear_max, what=f"cs {cs} region {b}")
        chk = expect(e, 1, list(paths), 0, 1, True, True, what=f"cs {cs} region {b}")
        assert chk.clear.any() and not chk.clear.all() and (chk.n_unknown > 0).any()
    edge = [metres(e, [(hi - 1, lo), (hi - 1, lo + 39), (hi - 12, lo)]), metres(e, [(hi - 3, lo + 2), (hi - 1, lo)])]
    expect(e, 1, edge, 20, 320, what="along the lattice edge")
    h = e.dim // 2
    corner = [metres(e, [(h - 9, h - 9), (h + 8, h + 8)]), metres(e, [(h + 5, h - 6), (h - 6, h + 5), (h - 1, h - 1), (h, h)])]
    expect(e, 1, corner, 7, 8, what="the corner shared by four tiles")
    chk = expect(e, 0, list(paths) + corner, 7, 8, what="a map without these tiles")
    assert np.all(chk.first_blocked == 0) and np.array_equal(chk.n_unknown, chk.steps) and np.all(chk.min_clearance == 8)
    assert np.all(e.check_paths(corner, particle=0, through_unknown=True).clear)
    e.close()


# ---- 4. every particle, each its own, device outputs ----------------------------------------------------------------------------------
def test_every_particle_and_each_its_own():
    torch = pytest.importorskip("torch")
    e, (x0, y0), c = scene_engine(3)
    e.load_map(raster(e, (x0, x0 + 150, y0, y0 + 150), c.T[:150, :150].copy()), particle=2)     # the walls along the other axis
    rng = np.random.default_rng(9)                                          # particle 1 holds no map at all
    paths = PO.fuzz_paths(rng, 3 * 50, (150, 150), (x0, y0), inv_of(e))
    for inflate, clear_max in ((0, 1), (7, 40)):
        allp = e.check_paths(paths, particle=None, radius_m=radius(e, inflate), clear_max=clear_max)
        assert allp.first_blocked.shape == (3, 150) and allp.steps.shape == (150,)
        want = [oracle(e, p, list(paths), inflate, clear_max) for p in range(3)]
        same(stacked(allp), np.stack([w[0] for w in want]), "every particle")
        same(allp.steps, want[0][1], "steps")
        assert np.all(allp.first_blocked[1] == 0) and len(np.unique(stacked(allp)[[0, 2]], axis=0)) == 2
        share = allp.p_clear()
        assert np.allclose(share, allp.clear.mean(axis=0), rtol=0, atol=1e-15) and share.max() <= 2 / 3 + 1e-12 and share.max() > 0.6
        assert np.array_equal(allp.p_clear([1.0, 0.0, 1.0]), allp.clear[[0, 2]].mean(axis=0))
        own = e.check_paths(paths.reshape(3, 50, 3, 2), particle=None, radius_m=radius(e, inflate), clear_max=clear_max, own=True)
        assert own.first_blocked.shape == (3, 50) and own.steps.shape == (3, 50)
        same(stacked(own), np.stack([stacked(allp)[p, 50 * p:50 * (p + 1)] for p in range(3)]), "own")
        same(own.steps, allp.steps.reshape(3, 50), "own steps")
        for kw in (dict(), dict(own=True)):
            q = paths.reshape(3, 50, 3, 2) if kw else paths
            d = e.check_paths(q, particle=None, radius_m=radius(e, inflate), clear_max=clear_max, device=True, **kw)
            assert isinstance(d.first_blocked, torch.Tensor) and d.first_blocked.device.type == "cuda" and d.n_unknown.dtype == torch.int32
            assert np.array_equal(stacked([a.cpu().numpy() for a in d[:4]]), stacked(own if kw else allp))
            assert isinstance(d.steps, np.ndarray) and np.array_equal(d.steps, (own if kw else allp).steps)
            assert np.array_equal(d.p_clear(), (own if kw else allp).p_clear())
    one = e.check_paths(paths, particle=2, device=True)
    assert np.array_equal(one.first_blocked.cpu().numpy(), e.check_paths(paths, particle=2).first_blocked)
    ragged = [paths[0], paths[1][:1], paths[2][:2]]                         # a list of paths of different lengths
    assert e.check_paths(ragged, particle=0).steps.tolist() == [allp.steps[0], 1, oracle(e, 0, [paths[2][:2]], 0, 1)[1][0]]
    e.close()


@pytest.fixture(scope="module")
def built():
    e = built_engine()
    yield e
    e.close()


def test_rollouts_in_the_maps_the_engine_built(built):
    from thesis_amd import plan
    e = built
    assert e.counters()["resample_copies"] > 0
    poses = e.poses()
    arcs = plan.rollouts(poses, [0.3, 0.6, 0.6, 2.0, 3.0], [0.0, 0.7, -0.7, 0.3, 0.0], 3.0, 0.1)       # the last two leave the room
    assert arcs.shape == (e.P, 5, 31, 2)
    own = e.check_paths(arcs, particle=None, radius_m=0.2, clear_max=60, own=True)
    allp = e.check_paths(arcs[3], particle=None, radius_m=0.2, clear_max=60)
    assert own.inflate == 20 and allp.first_blocked.shape == (e.P, 5)
    for p in (0, 3, 7, e.P - 1):
        res, steps = oracle(e, p, list(arcs[p]), 20, 60)
        same(stacked(own)[p], res, f"own rollouts, particle {p}")
        same(own.steps[p], steps, "steps")
        same(stacked(allp)[p], oracle(e, p, list(arcs[3]), 20, 60)[0], f"particle 3's rollouts in the map of {p}")
    clear = np.concatenate([own.clear.ravel(), allp.clear.ravel()])
    assert clear.any() and not clear.all() and len(np.unique(stacked(allp), axis=0)) > 1       # the particles hold different maps
    order = plan.rank_rollouts(allp, min_p_clear=0.5)
    assert np.all(allp.p_clear()[order] >= 0.5) and len(order) == int((allp.p_clear() >= 0.5).sum())
    k = int(np.argmax(e.weights()))
    assert np.array_equal(e.check_paths(arcs[3], radius_m=0.2).first_blocked, e.check_paths(arcs[3], particle=k, radius_m=0.2).first_blocked)


# ---- 5. the seeded fuzz ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate,clear_max", SETTINGS)
def test_fuzz(inflate, clear_max):
    e, (x0, y0), c = scene_engine()
    paths = PO.fuzz_paths(np.random.default_rng(100 + inflate + clear_max), 400, c.shape, (x0, y0), inv_of(e))
    chk = expect(e, 0, list(paths), inflate, clear_max, what="fuzz")         # all 400, none left out
    blocked = float((chk.first_blocked >= 0).mean())
    print(f"fuzz inflate {inflate} clear_max {clear_max}: blocked share {blocked:.2f}, unknown on {int((chk.first_unknown >= 0).sum())} paths")
    assert len(chk.first_blocked) == 400 and 0.1 <= blocked <= 0.9 and (chk.first_unknown >= 0).sum() >= 10
    for through, exempt in ((True, False), (False, True)):
        expect(e, 0, list(paths[:100]), inflate, clear_max, through, exempt, what="fuzz")
    e.close()


# ---- 6. arguments and state ---------------------------------------------------------------------------------------------------------------
def raw(e, particle, xy, start, n_paths=None, inflate=0, clear_max=1, flags=0, null=(), rows=None):
    """rbpf_check_paths itself: (return code, out, steps), both prefilled with FILL."""
    xy = None if xy is None else np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    start = None if start is None else np.ascontiguousarray(start, np.int32)
    n = (len(start) - 1 if start is not None else 1) if n_paths is None else n_paths
    out = np.full((rows if rows is not None else max(n, 1) * (e.P if particle == -1 and not flags & 8 else 1), 4), FILL, np.int32)
    steps = np.full(max(n, 1), FILL, np.int32)
    rc = e._lib.rbpf_check_paths(e._h, particle, None if xy is None or "xy" in null else xy.ctypes.data_as(C.POINTER(C.c_double)),
                                 None if start is None or "start" in null else start.ctypes.data_as(C.POINTER(C.c_int32)), n, inflate, clear_max,
                                 flags, None if "out" in null else C.c_void_p(out.ctypes.data), steps.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, steps


def test_bad_arguments_and_call_order_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P = 3
    e = engine(P)
    load_room16(e)
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    xy = [[0.0, 0.0], [1.0, 0.5], [2.0, -0.5], [0.3, 0.3], [0.1, 0.9], [-2.0, 1.0]]
    start = [0, 2, 3, 6]
    beyond = (hi + 0.5) / inv_of(e)
    long_way = [[(lo + 0.5) / inv_of(e), 0.0], [(hi - 0.5) / inv_of(e), 0.0]] * 500     # 999 legs of the lattice's width: more than 2^20 steps
    cases = dict(
        no_xy=dict(null=("xy",)), no_offsets=dict(null=("start",)), no_out=dict(null=("out",)), nan=dict(xy=xy[:4] + [[np.nan, 0.0]] + xy[5:]),
        inf=dict(xy=xy[:5] + [[0.0, -np.inf]]), offsets_from_one=dict(start=[1, 2, 3, 6]), empty_path=dict(start=[0, 2, 2, 6]),
        offsets_back=dict(start=[0, 3, 2, 6]), no_paths=dict(n_paths=0), negative_paths=dict(n_paths=-1), particle_high=dict(particle=P),
        particle_low=dict(particle=-2), inflate_negative=dict(inflate=-1), clear_max_equal=dict(inflate=4, clear_max=4),
        clear_max_large=dict(clear_max=321), flag=dict(flags=16), own_with_particle=dict(flags=8), own_with_best=dict(particle=0, flags=8, start=[0, 1, 2, 3]),
        own_remainder=dict(particle=-1, flags=8, start=[0, 2, 3, 4, 6]), outside=dict(xy=xy[:5] + [[beyond, 0.0]]),
        outside_low=dict(xy=[[0.0, (lo - 0.5) / inv_of(e)]] + xy[1:]), far_outside=dict(xy=xy[:2] + [[1e300, 0.0]] + xy[3:]),
        too_long=dict(xy=long_way, start=[0, 1000]))
    for name, kw in cases.items():
        args = dict(particle=1, xy=xy, start=start)
        args.update(kw)
        rc, out, steps = raw(e, **args)
        assert rc == _lib.RBPF_EINVAL, (name, rc)
        assert np.all(out == FILL) and np.all(steps == FILL), name
    rc, out, steps = raw(e, 1, xy[:5] + [[beyond, 0.0]], start)
    assert rc == _lib.RBPF_EINVAL and b"path 2, waypoint 2" in e._lib.rbpf_last_error(e._h)
    assert e._lib.rbpf_check_paths(None, 1, None, None, 1, 0, 1, 0, None, None) == _lib.RBPF_EINVAL
    # between the halves of a scan update
    ang, ranges, odo, truth = synthetic.make_log(2, 181)
    e.set_scan(ranges[0], ang)
    e.scan_update_begin(adj=False)
    rc, out, steps = raw(e, 1, xy, start)
    assert rc == _lib.RBPF_ESTATE and np.all(out == FILL) and np.all(steps == FILL)
    e.scan_update_end()
    rc, out, steps = raw(e, 1, xy, start, flags=2)                           # the engine is still usable
    want = oracle(e, 1, [np.array(xy[:2]), np.array(xy[2:3]), np.array(xy[3:])], 0, 1, True)
    assert rc == 0 and steps[0] == 21 and steps[1] == 1 and not np.any(out == FILL)
    same(out, want[0], "after the step")
    same(steps, want[1], "after the step, steps")
    rc, out, steps = raw(e, -1, xy, start, flags=8)                          # three paths, three particles, each its own
    assert rc == 0 and out.shape == (3, 4) and not np.any(out == FILL)
    st = np.array(start, np.int32)
    q = np.array(xy)
    o = np.full((3, 4), FILL, np.int32)
    assert e._lib.rbpf_check_paths(e._h, 1, q.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_int32)), 3, 0, 1, 0,
                                   C.c_void_p(o.ctypes.data), None) == 0 and not np.any(o == FILL)      # steps may be NULL
    for bad in (dict(particle="worst"), dict(own=True), dict(own=True, particle=None)):
        with pytest.raises(ValueError):
            e.check_paths(q.reshape(3, 2, 2), **bad)
    with pytest.raises(ValueError):
        e.check_paths([])
    with pytest.raises(ValueError):
        e.check_paths(np.zeros((2, 3, 1)))
    e.close()


def test_too_many_results_write_nothing():
    """P * n_paths >= 2^29 with every path in every map: 1024 particles, 2^19 one-waypoint paths, every table valid."""
    from thesis_amd import _lib
    P, n = 1024, 1 << 19
    e = engine(P, cs=0.1, pool_tiles=P)
    xy = np.zeros((n, 2))
    start = np.arange(n + 1, dtype=np.int32)
    rc, out, steps = raw(e, -1, xy, start, rows=1)
    assert rc == _lib.RBPF_EINVAL and b"2^29" in e._lib.rbpf_last_error(e._h)
    assert np.all(out == FILL) and np.all(steps == FILL)
    rc, out, steps = raw(e, -1, xy, start, flags=8)                          # each path in its own particle's map: 2^19 results, far below
    assert rc == 0 and np.all(steps == 1) and out.shape == (n, 4)
    assert np.all(out == [0, 0, 1, 1])                                       # no map anywhere: unknown, so blocked, at step 0
    e.close()


def test_a_call_changes_nothing_and_repeats_itself(built):
    from thesis_amd import plan
    e = built

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.render_map(0).cells, e.render_map(5).cells, e.map_extent())

    s0 = state()
    arcs = plan.rollouts(e.poses(), np.linspace(0.2, 1.0, 7), np.linspace(-0.8, 0.8, 7), 3.0, 0.1)
    a = e.check_paths(arcs, particle=None, radius_m=0.15, clear_max=60, own=True)
    b = e.check_paths(arcs, particle=None, radius_m=0.15, clear_max=60, own=True)
    e.check_paths(arcs[2], particle=None, through_unknown=True, start_exempt=True)
    e.check_paths(arcs[2], particle=4)
    for x, y in zip(a[:5], b[:5]):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(state(), s0):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)


# ---- 7. planned, checked, cut short ---------------------------------------------------------------------------------------------------
def test_a_planned_path_checks_clear_and_is_cut_short():
    from thesis_amd import plan
    e = engine(2)
    c = np.full((90, 90), PO.WALL, np.int8)
    c[5:85, 5:85] = PO.FREE
    c[35:55, 30:60] = PO.WALL                                               # a pillar between start and goal
    box = (-e.dim // 2 - 40, -e.dim // 2 + 50, -20, 70)                      # across the seam X = -dim / 2
    e.load_map(raster(e, box, c), particle=1)
    start, goal = metres(e, (box[0] + 10, box[2] + 44)), metres(e, (box[0] + 80, box[2] + 46))
    for radius_m in (0.0, 0.2):
        tr = e.travel_cost(start, [goal], particle=1, radius_m=radius_m)
        assert tr.goal_cost[0] > 0
        path = plan.path_to(tr, goal)
        chk = e.check_paths([path], particle=1, radius_m=radius_m, start_exempt=True)
        assert chk.clear[0] and chk.steps[0] == len(path) and chk.inflate == tr.inflate and chk.first_unknown[0] == -1
        assert np.array_equal(plan.path_cells(path, tr.inv), np.floor(path * tr.inv).astype(np.int64))
        assert not e.check_paths([path[[0, -1]]], particle=1, radius_m=radius_m, start_exempt=True).clear[0]      # the pillar is in the way
        blocked = e.check_paths([path[[0, -1]]], particle=1, radius_m=radius_m)
        cell = plan.path_cells(path[[0, -1]], tr.inv)[blocked.first_blocked[0]] - [box[0], box[2]]
        assert 35 - 5 <= cell[0] < 55 + 5 and 30 - 5 <= cell[1] < 60 + 5       # first_blocked maps back to a place at the pillar
        short = plan.shortcut_in(e, path, particle=1, radius_m=radius_m)
        assert 3 <= len(short) < len(path) / 4 and short[0].tolist() == path[0].tolist() and short[-1].tolist() == path[-1].tolist()
        assert np.hypot(*np.diff(short, axis=0).T).sum() < np.hypot(*np.diff(path, axis=0).T).sum()
        assert e.check_paths([short], particle=1, radius_m=radius_m, start_exempt=True).clear[0]
        both = plan.shortcut_in(e, path, particle=None, radius_m=radius_m, min_share=0.5)      # particle 0 holds no map: half the share
        assert np.array_equal(both, short)
        with pytest.raises(ValueError):
            plan.shortcut_in(e, path, particle=None, radius_m=radius_m, min_share=1.0)
    e.close()
