"""Rollout checks on the GPU (rbpf_check_rollouts, check_rollouts_kernel in kernels_paths.hip): templates in the
robot's frame placed at poses on the device.  Every comparison is twofold and by equality, `steps` included: with the scalar
oracle of tests/paths_oracle.py on the rendered map, walking plan.place_templates of the same poses and templates, and with
check_paths of those placed paths - the entry point that has the host form the cells."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.cast_oracle import lattice_bounds
from tests.test_gpu_cast import built_engine, engine, load_room16, raster, rng_state, seam_scene
from tests.test_gpu_paths import FILL, SETTINGS, inv_of, metres, oracle, radius, same, scene_engine, stacked
from tests.test_rollouts_oracle import fuzz_inputs
from tests import paths_oracle as PO
from thesis_amd import plan

pytestmark = pytest.mark.gpu


def placed(poses, templates):
    """[N][K] paths in metres: template k at pose n by plan.place_templates; the templates may differ in length."""
    cols = [plan.place_templates(np.asarray(poses, dtype=np.float64).reshape(-1, 3), np.asarray(t, dtype=np.float64)[None])[:, 0] for t in templates]
    return [[col[n] for col in cols] for n in range(len(cols[0]))]


def reach_of(e, templates):
    return int(math.ceil(max(float(np.abs(np.asarray(t, dtype=np.float64)[:, :2]).sum(axis=1).max()) for t in templates) * inv_of(e))) + 2


def compare(e, p, poses, templates, inflate, clear_max, through=False, exempt=False, what=""):
    """check_rollouts of every pose in particle p's map equals check_paths of the placed templates and the oracle; returns it."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    kw = dict(particle=p, radius_m=radius(e, inflate), clear_max=clear_max, through_unknown=through, start_exempt=exempt)
    chk = e.check_rollouts(poses, templates, **kw)
    assert (chk.inflate, chk.clear_max) == (inflate, clear_max)
    N, K = len(poses), len(templates)
    paths = [q for row in placed(poses, templates) for q in row]
    label = f"{what} inflate {inflate} clear_max {clear_max} through {through} exempt {exempt}"
    ref = e.check_paths(paths, **kw)
    same(stacked(chk), stacked(ref).reshape(N, K, 4), label + ", against check_paths")
    same(chk.steps, ref.steps.reshape(N, K), label + ", steps against check_paths")
    res, steps = oracle(e, p, paths, inflate, clear_max, through, exempt)
    same(stacked(chk), res.reshape(N, K, 4), label + ", against the oracle")
    same(chk.steps, steps.reshape(N, K), label + ", steps against the oracle")
    return chk


def pose_in(e, cell, frac, theta):
    return [(cell[0] + frac[0]) / inv_of(e), (cell[1] + frac[1]) / inv_of(e), theta]


# ---- 1. the prefix sum and the lanes' edges ---------------------------------------------------------------------------------------
def zigzag(sizes, span):
    """Template cells whose segments along x have the lengths `sizes`, turning round inside 0 .. span; y wanders by less."""
    pts, x, d = [(0, 0)], 0, 1
    for j, n in enumerate(sizes):
        if not 0 <= x + d * n <= span:
            d = -d
        x += d * n
        pts.append((x, (j + 1) % 3 - 1))
    return pts


def test_prefix_and_lane_edges_equal_the_oracle():
    e, (x0, y0), c = scene_engine()
    inv = inv_of(e)
    held = [0] * 10 + list(range(1, 52)) + [51] * 10 + list(range(52, 109))      # repeated waypoints at the start and across waypoint 64
    cells = [[(0, 0)], [(0, 0), (62, 0)], [(i, i % 2) for i in range(64)], [(i, 0) for i in range(65)],
             [(i // 2, -(i // 4 % 2)) for i in range(127)],                       # every waypoint twice, in both rounds of 64
             zigzag([2] * 125 + [3, 3], 150), [(0, 0), (63, 5)], [(0, 0), (64, -64)], [(x, 0) for x in held]]
    templates = [np.asarray(t, dtype=np.float64) / inv for t in cells]
    assert [len(t) for t in templates] == [1, 2, 64, 65, 127, 128, 2, 2, 128]
    poses = [pose_in(e, (x0 + 10, y0 + 75), (0.5, 0.5), 0.0), pose_in(e, (x0 + 120, y0 + 70), (0.3, 0.7), 2.3),
             pose_in(e, (x0 + 70, y0 + 100), (0.9, 0.1), -0.4)]                  # the last walks across the seam X = -dim / 2
    assert poses[2][0] * inv < -e.dim // 2 < (poses[2][0] + 2.0) * inv
    chk = None
    for inflate, clear_max in SETTINGS[:2]:
        for through, exempt in ((False, False), (True, False), (False, True), (True, True)):
            chk = compare(e, 0, poses, templates, inflate, clear_max, through, exempt, "lane edges")
    assert chk.steps[0].tolist() == [1, 63, 64, 65, 64, 257, 64, 65, 109]
    chk = compare(e, 0, poses, templates, 20, 21, what="lane edges")
    assert chk.clear.any() and not chk.clear.all() and chk.first_blocked.shape == (3, 9) and chk.steps.dtype == np.int32
    one = e.check_rollouts(poses[1], np.stack([templates[1], templates[6]]), particle=0)      # a [3] pose, templates as one array
    assert one.first_blocked.shape == (1, 2)
    e.close()


# ---- 2. the least of two blocked steps, whichever lane and round finds them ---------------------------------------------------------
def test_the_least_blocked_step_wins_across_lanes_and_rounds():
    e = engine(1)
    inv = inv_of(e)
    templates = [np.array([[0.0, 0.0], [260.0, 0.0]]) / inv, np.stack([np.arange(128) * (260.0 / 127.0), np.zeros(128)], axis=1) / inv]
    up, down = math.pi / 2, -math.pi / 2
    poses = [pose_in(e, (102, -140), (0.5, 0.5), up), pose_in(e, (102, 120), (0.5, 0.5), down), pose_in(e, (100, -140), (0.5, 0.5), up)]
    for first, second in ((70, 200), (67, 130), (130, 195), (3, 64), (63, 64)):      # lanes 6 / 8, 3 / 2, 2 / 3, 3 / 0, 63 / 0
        c = np.full((5, 300), PO.FREE, np.int8)
        c[2, 10 + first] = c[2, 10 + second] = PO.WALL
        c[0, 40:141] = 0                                                    # 101 unknown cells beside the way
        e.load_map(raster(e, (100, 105, -150, 150), c))
        chk = compare(e, 0, poses, templates, 0, 1, what=f"walls at {first}, {second}")
        for k in range(2):
            assert chk.first_blocked[:, k].tolist() == [first, 260 - second, 30] and chk.first_unknown[:, k].tolist() == [-1, -1, 30]
            assert chk.n_unknown[:, k].tolist() == [0, 0, 101] and chk.steps[:, k].tolist() == [261] * 3
        chk = compare(e, 0, poses[:1], templates, 7, 8, what=f"walls at {first}, {second}")
        assert chk.first_blocked[0].tolist() == [first - 1] * 2
    e.close()


# ---- 3. seams, partial occupancy words, missing tiles, the lattice edge ----------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_seams_missing_tiles_and_the_lattice_edge(cs):
    from thesis_amd.engine import RbpfError
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs)) + 1))
    e = engine(2, cs=cs, pool_tiles=24, lattice_radius=1)
    scenes = seam_scene(e.dim, rng)
    for b, c in scenes:
        e.load_map(raster(e, b, np.where(c > 10, c, np.where(rng.random(c.shape) < 0.1, 0, PO.FREE)).astype(np.int8)), particle=1)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)     # another map, which must not be seen
    lo, hi = lattice_bounds(e.dim, 1)
    k = np.where(rng.random((30, 30)) < 0.05, PO.WALL, PO.FREE).astype(np.int8)
    e.load_map(raster(e, (hi - 30, hi, lo, lo + 30), k), particle=1)        # the lattice's corner
    tm = plan.arc_templates([0.3, 0.3, 0.5, 0.0], [0.0, 1.2, -0.9, 0.0], 2.0, 0.25)      # the last stands still: nine waypoints in one cell
    reach = reach_of(e, tm)                                                  # |lx| + |ly| of an arc's end exceeds its chord of 1 m
    assert 1.0 * inv_of(e) + 2 <= reach <= math.sqrt(2.0) * inv_of(e) + 3
    h, first, last = e.dim // 2, lo + reach, hi - 1 - reach

    def poses_at(cells):
        return [pose_in(e, q, rng.uniform(0.05, 0.95, 2), rng.uniform(-np.pi, np.pi)) for q in cells]

    regions = {}
    for n, (b, _) in enumerate(scenes):                                     # beside and inside every written box
        regions[f"box {b}"] = poses_at([(int(np.clip(rng.integers(b[0] - 10, b[1] + 10), first, last)), int(np.clip(rng.integers(b[2] - 10, b[3] + 10), first, last)))
                                        for _ in range(3)])
    regions["the corner shared by four tiles"] = poses_at([(h, h), (h - 1, h - 1), (h - 1, h + 3)])
    regions["a tile that is not there"] = poses_at([(-h - 100, h + 100), (-h - 90, h + 120)])
    regions["a tile never written there"] = poses_at([(h + 200 * e.dim // 800, -h - 200 * e.dim // 800)])
    # the pose's cell exactly `reach` cells from the lattice's edges, heading out of the lattice and along it
    regions["reach cells from the low corner"] = [pose_in(e, (first, first), (0.05, 0.05), th) for th in (-2.4, math.pi, -math.pi / 2)]
    regions["reach cells from the written corner"] = [pose_in(e, (last, first), (0.95, 0.05), th) for th in (-0.8, 0.0, -math.pi / 2)]
    regions["reach cells from the high corner"] = [pose_in(e, (last, last), (0.95, 0.95), th) for th in (0.8, math.pi / 2)]
    seen = []
    for name, poses in regions.items():
        for inflate, clear_max in SETTINGS:
            chk = compare(e, 1, poses, tm, inflate, clear_max, what=f"cs {cs} {name}")
        assert np.all(chk.steps[:, 3] == 1)
        seen.append(stacked(compare(e, 1, poses, tm, 0, 1, True, True, what=f"cs {cs} {name}")).reshape(-1, 4))
    seen = np.concatenate(seen)
    assert (seen[:, 0] < 0).any() and (seen[:, 0] >= 0).any() and (seen[:, 3] > 0).any()
    chk = compare(e, 0, regions["the corner shared by four tiles"], tm, 7, 8, what="a map without these tiles")
    assert np.all(chk.first_blocked == 0) and np.array_equal(chk.n_unknown, chk.steps) and np.all(chk.min_clearance == 8)
    for cell in ((first - 1, 0), (0, first - 1), (last + 1, 0), (0, last + 1)):      # one cell farther out: refused, and said which
        with pytest.raises(RbpfError, match="pose 1"):
            e.check_rollouts([pose_in(e, (0, 0), (0.5, 0.5), 0.0), pose_in(e, cell, (0.5, 0.5), 1.0)], tm, particle=1)
    e.close()


# ---- 4. each pose in its own particle's map, device outputs, maps the engine built -----------------------------------------------
def test_each_pose_in_its_own_particles_map():
    torch = pytest.importorskip("torch")
    e, (x0, y0), c = scene_engine(3)
    e.load_map(raster(e, (x0, x0 + 150, y0, y0 + 150), c.T[:150, :150].copy()), particle=2)     # the walls along the other axis
    poses, tm = fuzz_inputs(inv_of(e), (x0, y0))                             # particle 1 holds no map at all
    poses = poses[[3, 11, 12]]
    poses[2, :2] = (np.array([x0 + 75, y0 + 64]) + 0.4) / inv_of(e)
    arcs = plan.place_templates(poses, tm)
    for inflate, clear_max in ((0, 1), (7, 40)):
        kw = dict(particle=None, radius_m=radius(e, inflate), clear_max=clear_max)
        own = e.check_rollouts(poses, tm, **kw)
        assert own.first_blocked.shape == (3, 16) and own.steps.shape == (3, 16)
        ref = e.check_paths(arcs, own=True, **kw)
        same(stacked(own), stacked(ref), "against check_paths, each its own")
        same(own.steps, ref.steps, "steps against check_paths")
        for p in range(3):
            res, steps = oracle(e, p, list(arcs[p]), inflate, clear_max)
            same(stacked(own)[p], res, f"pose {p} in the map of particle {p}")
            same(own.steps[p], steps, "steps")
        assert np.all(own.first_blocked[1] == 0) and len(np.unique(stacked(own)[[0, 2]].reshape(-1, 4), axis=0)) > 3
        d = e.check_rollouts(poses, tm, device=True, **kw)
        for a in d[:5]:
            assert isinstance(a, torch.Tensor) and a.device.type == "cuda" and a.dtype == torch.int32
        assert np.array_equal(stacked([a.cpu().numpy() for a in d[:4]]), stacked(own)) and np.array_equal(d.steps.cpu().numpy(), own.steps)
        assert np.array_equal(d.p_clear(), own.p_clear()) and np.array_equal(d.clearance_metres(), own.clearance_metres())
    one = e.check_rollouts(poses, tm, particle=2, device=True)
    assert np.array_equal(one.first_blocked.cpu().numpy(), e.check_rollouts(poses, tm, particle=2).first_blocked)
    e.close()


@pytest.fixture(scope="module")
def built():
    e = built_engine()
    yield e
    e.close()


def fan():
    return plan.arc_templates([0.3, 0.6, 0.6, 2.0, 3.0], [0.0, 0.7, -0.7, 0.3, 0.0], 3.0, 0.1)       # the last two leave the room


def test_rollouts_from_the_poses_of_the_maps_the_engine_built(built):
    e = built
    assert e.counters()["resample_copies"] > 0
    poses, tm = e.poses(), fan()
    assert tm.shape == (5, 31, 2)
    arcs = plan.place_templates(poses, tm)
    own = e.check_rollouts(poses, tm, particle=None, radius_m=0.2, clear_max=60)
    assert own.inflate == 20 and own.first_blocked.shape == (e.P, 5)
    ref = e.check_paths(arcs, particle=None, radius_m=0.2, clear_max=60, own=True)
    same(stacked(own), stacked(ref), "against check_paths, each its own")
    same(own.steps, ref.steps, "steps against check_paths")
    for p in (0, 3, 7, e.P - 1):
        res, steps = oracle(e, p, list(arcs[p]), 20, 60)
        same(stacked(own)[p], res, f"own rollouts, particle {p}")
        same(own.steps[p], steps, "steps")
    assert own.clear.any() and not own.clear.all()
    k = int(np.argmax(e.weights()))
    assert np.array_equal(stacked(e.check_rollouts(poses, tm, particle="best", radius_m=0.2)), stacked(e.check_rollouts(poses, tm, particle=k, radius_m=0.2)))


# ---- 5. the seeded fuzz ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate,clear_max", SETTINGS)
def test_fuzz(inflate, clear_max):
    e, (x0, y0), c = scene_engine()
    poses, tm = fuzz_inputs(inv_of(e), (x0, y0))
    assert poses.shape == (64, 3) and tm.shape == (16, 5, 2)
    chk = compare(e, 0, poses, tm, inflate, clear_max, what="fuzz")          # all 64 * 16, none left out
    blocked = float((chk.first_blocked >= 0).mean())
    print(f"fuzz inflate {inflate} clear_max {clear_max}: blocked share {blocked:.2f}, unknown on {float((chk.first_unknown >= 0).mean()):.2f} of the paths")
    assert chk.first_blocked.shape == (64, 16) and 0.1 <= blocked <= 0.9
    for through, exempt in ((True, False), (False, True)):
        sub = compare(e, 0, poses[:16], tm, inflate, clear_max, through, exempt, what="fuzz")
        if exempt:
            share = float((sub.first_blocked >= 0).mean())
            assert 0.1 <= share <= 0.9
    e.close()


# ---- 6. arguments and call order ------------------------------------------------------------------------------------------------------
def raw(e, particle, poses, xy, start, n_poses=None, n_tmpl=None, inflate=0, clear_max=1, flags=0, null=(), rows=None):
    """rbpf_check_rollouts itself: (return code, out, steps), both prefilled with FILL."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    start = np.ascontiguousarray(start, np.int32)
    N = len(poses) if n_poses is None else n_poses
    K = len(start) - 1 if n_tmpl is None else n_tmpl
    n = rows if rows is not None else max(N, 1) * max(K, 1)
    out, steps = np.full((n, 4), FILL, np.int32), np.full(n, FILL, np.int32)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = e._lib.rbpf_check_rollouts(e._h, particle, None if "poses" in null else poses.ctypes.data_as(D), N, None if "xy" in null else xy.ctypes.data_as(D),
                                    None if "start" in null else start.ctypes.data_as(I), K, inflate, clear_max, flags,
                                    None if "out" in null else C.c_void_p(out.ctypes.data), None if "steps" in null else C.c_void_p(steps.ctypes.data))
    return rc, out, steps


def test_bad_arguments_and_call_order_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P = 3
    e = engine(P)
    load_room16(e)
    inv = inv_of(e)
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    poses = [[0.0, 0.0, 0.0], [1.0, 0.5, 1.0]]
    xy = [[0.0, 0.0], [0.5, 0.1], [0.0, 0.0], [0.3, 0.3], [0.1, 0.9], [-0.5, 0.2]]       # rmax 1.0 m: reach 22 cells
    start = [0, 2, 3, 6]
    three = poses + [[-1.0, 0.0, 2.0]]
    edge = lambda cell: [(cell + 0.5) / inv, 0.0, 0.3]
    line = np.stack([np.arange(128) * (206.4 / 127.0), np.zeros(128)], axis=1)           # 127 * 2 * (4128 + 2) >= 2^20
    cases = dict(
        no_poses=dict(null=("poses",)), no_xy=dict(null=("xy",)), no_offsets=dict(null=("start",)), no_out=dict(null=("out",)),
        nan_pose=dict(poses=[poses[0], [np.nan, 0.5, 1.0]]), inf_heading=dict(poses=[poses[0], [1.0, 0.5, np.inf]]),
        nan_template=dict(xy=xy[:4] + [[np.nan, 0.0]] + xy[5:]), inf_template=dict(xy=xy[:5] + [[0.0, -np.inf]]),
        template_beyond_float64=dict(xy=xy[:5] + [[1.7e308, 0.0]]), offsets_from_one=dict(start=[1, 2, 3, 6]), empty_template=dict(start=[0, 2, 2, 6]),
        offsets_back=dict(start=[0, 3, 2, 6]), long_template=dict(xy=np.zeros((129, 2)), start=[0, 129]), no_pose=dict(n_poses=0),
        negative_poses=dict(n_poses=-1), no_template=dict(n_tmpl=0), negative_templates=dict(n_tmpl=-1), particle_high=dict(particle=P),
        particle_low=dict(particle=-2), each_its_own_needs_P_poses=dict(particle=-1), inflate_negative=dict(inflate=-1),
        clear_max_equal=dict(inflate=4, clear_max=4), clear_max_large=dict(clear_max=321), flag=dict(flags=16), own=dict(flags=8),
        own_each=dict(particle=-1, poses=three, flags=8), pose_outside=dict(poses=[poses[0], edge(hi)]), pose_far_outside=dict(poses=[poses[0], [1e300, 0.0, 0.0]]),
        reach_leaves_high=dict(poses=[poses[0], edge(hi - 22)]), reach_leaves_low=dict(poses=[poses[0], edge(lo + 21)]),
        too_many_steps=dict(xy=line, start=[0, 128]))
    for name, kw in cases.items():
        args = dict(particle=1, poses=poses, xy=xy, start=start)
        args.update(kw)
        rc, out, steps = raw(e, **args)
        assert rc == _lib.RBPF_EINVAL, (name, rc)
        assert np.all(out == FILL) and np.all(steps == FILL), name
    rc, out, steps = raw(e, 1, [poses[0], edge(hi - 22)], xy, start)
    assert rc == _lib.RBPF_EINVAL and b"pose 1" in e._lib.rbpf_last_error(e._h)
    for cell in (hi - 23, lo + 22):                                          # exactly reach cells from the edge: taken
        rc, out, steps = raw(e, 1, [poses[0], edge(cell)], xy, start)
        assert rc == 0 and not np.any(out == FILL) and not np.any(steps == FILL), cell
    assert e._lib.rbpf_check_rollouts(None, 1, None, 1, None, None, 1, 0, 1, 0, None, None) == _lib.RBPF_EINVAL
    # between the halves of a scan update
    ang, ranges, odo, truth = synthetic.make_log(2, 181)
    e.set_scan(ranges[0], ang)
    e.scan_update_begin(adj=False)
    rc, out, steps = raw(e, 1, poses, xy, start)
    assert rc == _lib.RBPF_ESTATE and np.all(out == FILL) and np.all(steps == FILL)
    e.scan_update_end()
    rc, out, steps = raw(e, 1, poses, xy, start, flags=2)                    # the engine is still usable
    templates = [np.array(xy[:2]), np.array(xy[2:3]), np.array(xy[3:])]
    want = compare(e, 1, poses, templates, 0, 1, True, what="after the step")
    assert rc == 0 and steps.tolist()[:2] == [11, 1]
    same(out, stacked(want).reshape(-1, 4), "after the step")
    same(steps, want.steps.reshape(-1), "after the step, steps")
    rc, out, steps = raw(e, -1, three, xy, start)                            # three poses, three particles, each its own
    assert rc == 0 and not np.any(out == FILL) and not np.any(steps == FILL)
    rc, out, steps = raw(e, 1, poses, xy, start, null=("steps",))            # steps may be NULL
    assert rc == 0 and not np.any(out == FILL) and np.all(steps == FILL)
    for bad in (dict(particle="worst"), dict(poses=np.zeros((2, 2))), dict(poses=np.zeros((0, 3))), dict(templates=[]), dict(templates=np.zeros((2, 3, 1)))):
        args = dict(poses=poses, templates=templates, particle=1)
        args.update(bad)
        with pytest.raises(ValueError):
            e.check_rollouts(**args)
    e.close()


def test_too_many_results_write_nothing():
    """n_poses * n_tmpl >= 2^29: 1024 particles, each pose in its own map, and 2^19 one-waypoint templates, every table valid."""
    from thesis_amd import _lib
    P, n = 1024, 1 << 19
    e = engine(P, cs=0.1, pool_tiles=P)
    poses, xy, start = np.zeros((P, 3)), np.zeros((n, 2)), np.arange(n + 1, dtype=np.int32)
    rc, out, steps = raw(e, -1, poses, xy, start, rows=1)
    assert rc == _lib.RBPF_EINVAL and b"2^29" in e._lib.rbpf_last_error(e._h)
    assert np.all(out == FILL) and np.all(steps == FILL)
    rc, out, steps = raw(e, -1, poses, xy[:512], start[:513])                # 2^19 results, far below
    assert rc == 0 and np.all(steps == 1) and out.shape == (n, 4)
    assert np.all(out == [0, 0, 1, 1])                                       # no map anywhere: unknown, so blocked, at step 0
    e.close()


# ---- 7. state and repeatability -------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_and_repeats_itself(built):
    e = built

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.render_map(0).cells, e.render_map(5).cells, e.map_extent())

    s0 = state()
    tm = plan.arc_templates(np.linspace(0.2, 1.0, 7), np.linspace(-0.8, 0.8, 7), 3.0, 0.1)
    a = e.check_rollouts(e.poses(), tm, particle=None, radius_m=0.15, clear_max=60)
    b = e.check_rollouts(e.poses(), tm, particle=None, radius_m=0.15, clear_max=60)
    e.check_rollouts(e.poses()[:5], tm, particle=4, through_unknown=True, start_exempt=True)
    for x, y in zip(a[:5], b[:5]):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(state(), s0):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)


# ---- 8. ranked as the paths would be --------------------------------------------------------------------------------------------------
def test_ranking_equals_that_of_the_placed_paths(built):
    e = built
    tm = plan.arc_templates(np.repeat([0.3, 0.6, 0.9], 5), np.tile(np.linspace(-1.0, 1.0, 5), 3), 3.0, 0.25)
    kw = dict(particle=None, radius_m=0.2, clear_max=60, start_exempt=True)
    chk = e.check_rollouts(e.poses(), tm, **kw)
    ref = e.check_paths(plan.place_templates(e.poses(), tm), own=True, **kw)
    dev = e.check_rollouts(e.poses(), tm, device=True, **kw)
    for share in (0.95, 0.5, 0.0):
        want = plan.rank_rollouts(ref, weights=e.weights(), min_p_clear=share)
        assert np.array_equal(plan.rank_rollouts(chk, weights=e.weights(), min_p_clear=share), want)
        assert np.array_equal(plan.rank_rollouts(dev, weights=e.weights(), min_p_clear=share), want)
    assert len(plan.rank_rollouts(chk, min_p_clear=0.0)) == 15
