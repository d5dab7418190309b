"""Footprint checks on the GPU (rbpf_check_footprints, kernels_footprint.hip): rollouts driven by a robot that is
no disc.  Every comparison is by equality, `steps` included, with the scalar oracle of tests/footprint_oracle.py on the rendered
map; min_clearance and steps are also those of check_rollouts of the same poses, templates and clear_max, bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import footprint_oracle as FO
from tests import paths_oracle as PO
from tests.cast_oracle import lattice_bounds
from tests.test_footprint_oracle import FUZZ_SETTINGS, fuzz_inputs, fuzz_table, rectangle
from tests.test_gpu_cast import built_engine, engine, load_room16, raster, rng_state, seam_scene
from tests.test_gpu_paths import FILL, SETTINGS, inv_of, radius, same, scene_engine, stacked
from thesis_amd import plan

pytestmark = pytest.mark.gpu

FLAG_COMBOS = ((False, -1), (True, -1), (False, 2), (True, 0))


def cell_of(e):
    return float(e.cfg.tile_len_m) / e.dim


def pose_in(e, cell, frac, theta):
    return [(cell[0] + frac[0]) / inv_of(e), (cell[1] + frac[1]) / inv_of(e), theta]


def table_of(e, spans_per_bin):
    """A Footprint from a list of span lists, one per bin, for this engine's cell size."""
    offs = np.zeros(len(spans_per_bin) + 1, np.int32)
    np.cumsum([len(b) for b in spans_per_bin], out=offs[1:])
    return plan.Footprint(np.array([s for b in spans_per_bin for s in b], np.int32).reshape(-1, 3), offs, len(spans_per_bin), cell_of(e))


def bar(e, H, cells=6):
    """An outline that is not symmetric: a bar of `cells` cells ahead of the robot's centre, so that every bin covers other cells."""
    c = cell_of(e)
    return plan.footprint_table(np.array([[cells * c, 0.4 * c], [-0.4 * c, 0.4 * c], [-0.4 * c, -0.4 * c], [cells * c, -0.4 * c]]), c, H, pad_m=0.0)


def oracle(e, p, poses, templates, headings, fp, inflate, clear_max, through=False, exempt=-1):
    rolls = FO.rollout_cells(poses, templates, headings, fp.H, inv_of(e))
    box = FO.box_of(rolls)
    wide = e.render_map(p, box=FO.grown_box(box, clear_max, FO.table_reach(fp))).cells
    f = FO.Field(wide, box, float(e.cfg.quantum), float(e.cfg.occupied_threshold), inflate, clear_max, fp, through)
    return FO.check_all(f, rolls, exempt)


def compare(e, p, poses, templates, headings, fp, inflate, clear_max, through=False, exempt=-1, what=""):
    """check_footprints of every pose in particle p's map equals the oracle, and check_rollouts where the two must agree; returns it."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    kw = dict(particle=p, radius_m=radius(e, inflate), clear_max=clear_max, through_unknown=through)
    chk = e.check_footprints(poses, templates, headings, fp, exempt_cells=None if exempt < 0 else exempt, **kw)
    assert (chk.inflate, chk.clear_max) == (inflate, clear_max)
    label = f"{what} inflate {inflate} clear_max {clear_max} through {through} exempt {exempt}"
    res, steps = oracle(e, p, poses, templates, headings, fp, inflate, clear_max, through, exempt)
    same(stacked(chk), res, label + ", against the oracle")
    same(chk.steps, steps, label + ", steps against the oracle")
    ref = e.check_rollouts(poses, templates, **kw)
    assert chk.min_clearance.tobytes() == ref.min_clearance.tobytes() and chk.steps.tobytes() == ref.steps.tobytes(), label + ": check_rollouts"
    return chk


# ---- 1. waypoint counts, step counts, repeated waypoints --------------------------------------------------------------------------
def zigzag(sizes, span):
    pts, x, d = [(0, 0)], 0, 1
    for j, n in enumerate(sizes):
        if not 0 <= x + d * n <= span:
            d = -d
        x += d * n
        pts.append((x, (j + 1) % 3 - 1))
    return pts


def test_waypoint_counts_step_counts_and_repeats_equal_the_oracle():
    e, (x0, y0), c = scene_engine()
    inv = inv_of(e)
    rng = np.random.default_rng(2)
    held = [0] * 10 + list(range(1, 52)) + [51] * 10 + list(range(52, 109))      # repeated waypoints at the start and across waypoint 64
    cells = [[(0, 0)], [(0, 0), (62, 0)], [(i, i % 2) for i in range(64)], [(i, 0) for i in range(65)],
             [(i // 2, -(i // 4 % 2)) for i in range(127)],                       # every waypoint twice, in both rounds of 64
             zigzag([2] * 125 + [3, 3], 150), [(0, 0), (63, 5)], [(0, 0), (64, -64)], [(x, 0) for x in held]]
    templates = [np.asarray(t, dtype=np.float64) / inv for t in cells]
    headings = [rng.uniform(-4.0, 4.0, size=len(t)) for t in templates]           # a heading of its own for every waypoint, the repeated ones too
    assert [len(t) for t in templates] == [1, 2, 64, 65, 127, 128, 2, 2, 128]
    poses = [pose_in(e, (x0 + 10, y0 + 75), (0.5, 0.5), 0.0), pose_in(e, (x0 + 120, y0 + 70), (0.3, 0.7), 2.3),
             pose_in(e, (x0 + 70, y0 + 100), (0.9, 0.1), -0.4)]                  # the last walks across the seam X = -dim / 2
    fp = fuzz_table()
    chk = None
    for inflate, clear_max in SETTINGS[:2]:
        for through, exempt in FLAG_COMBOS:
            chk = compare(e, 0, poses, templates, headings, fp, inflate, clear_max, through, exempt, "lane edges")
    assert chk.steps[0].tolist() == [1, 63, 64, 65, 64, 257, 64, 65, 109]
    chk = compare(e, 0, poses, templates, headings, bar(e, 32), 0, 40, True, what="a bar")
    assert chk.clear.any() and not chk.clear.all() and chk.first_blocked.shape == (3, 9) and chk.steps.dtype == np.int32
    one = e.check_footprints(poses[1], np.stack([templates[1], templates[6]]), np.zeros((2, 2)), fp, particle=0)      # a [3] pose, arrays
    assert one.first_blocked.shape == (1, 2)
    e.close()


# ---- 2. a turn on the spot -------------------------------------------------------------------------------------------------------------
def test_a_turn_on_the_spot_sweeps_every_heading():
    e = engine(1)
    c = np.full((40, 40), PO.FREE, np.int8)
    c[25, 20] = PO.WALL                                                     # five cells ahead of (20, 20) along +x: only heading 0 reaches it
    e.load_map(raster(e, (100, 140, -20, 20), c))
    fp = bar(e, 8)
    pose = pose_in(e, (120, 0), (0.5, 0.5), 0.0)
    spot = np.zeros((8, 2))
    turn = np.arange(8) * (math.pi / 4)
    all8 = compare(e, 0, [pose], [spot], [turn], fp, 0, 1, what="a full turn")
    assert stacked(all8)[0, 0].tolist() == [0, -1, 1, 0] and all8.steps.tolist() == [[1]]
    for k in range(8):
        rest = compare(e, 0, [pose], [spot[:7]], [np.delete(turn, k)], fp, 0, 1, what=f"a turn without heading {k}")
        assert bool(rest.clear[0, 0]) == (k == 0)
    away = compare(e, 0, [pose_in(e, (120, 0), (0.5, 0.5), math.pi)], [spot[:1]], [[0.0]], fp, 0, 1, what="looking away")
    assert away.clear.all() and compare(e, 0, [pose], [spot[:1]], [[0.0]], fp, 0, 1).first_blocked.tolist() == [[0]]
    e.close()


# ---- 3. the least of two blocked steps, whichever lane and round finds them ---------------------------------------------------------
def test_the_least_blocked_step_wins_across_lanes_and_rounds():
    e = engine(1)
    inv = inv_of(e)
    templates = [np.array([[0.0, 0.0], [260.0, 0.0]]) / inv, np.stack([np.arange(128) * (260.0 / 127.0), np.zeros(128)], axis=1) / inv]
    headings = [np.zeros(2), np.zeros(128)]
    up, down = math.pi / 2, -math.pi / 2
    poses = [pose_in(e, (102, -140), (0.5, 0.5), up), pose_in(e, (102, 120), (0.5, 0.5), down)]
    dot = table_of(e, [[(0, 0, 0)]])
    for first, second in ((70, 200), (63, 64), (3, 64)):
        c = np.full((5, 300), PO.FREE, np.int8)
        c[2, 10 + first] = c[2, 10 + second] = PO.WALL
        e.load_map(raster(e, (100, 105, -150, 150), c))
        chk = compare(e, 0, poses, templates, headings, dot, 0, 1, what=f"walls at {first}, {second}")
        for k in range(2):
            assert chk.first_blocked[:, k].tolist() == [first, 260 - second] and chk.steps[:, k].tolist() == [261] * 2
        chk = compare(e, 0, poses, templates, headings, fuzz_table(), 0, 1, True, what=f"walls at {first}, {second}, 9 x 5")
        assert chk.first_blocked[0].tolist() == [max(first - 4, 0)] * 2      # the rectangle looks along the way: four cells ahead
    e.close()


# ---- 4. span widths across occupancy-word boundaries ------------------------------------------------------------------------------------
def test_span_widths_across_word_boundaries():
    rng = np.random.default_rng(9)
    e = engine(1)
    # bin 0 covers 292 cells: at 0.3 % walls and 0.3 % unknown cells about four poses in ten see none of either
    c = np.where(rng.random((60, 220)) < 0.003, PO.WALL, np.where(rng.random((60, 220)) < 0.003, 0, PO.FREE)).astype(np.int8)
    e.load_map(raster(e, (40, 100, -110, 110), c))                          # columns on both sides of Y = 0: words of every offset
    fp = table_of(e, [[(0, 0, 0), (1, -16, 15), (2, -16, 16), (3, -32, 31), (-1, 31, 31), (-2, -63, 0), (-3, 0, 63), (4, 1, 33)],
                      [(0, -32, 31)], [(0, 0, 0)], [(2, -1, 62), (0, 0, 0)]])
    assert sorted(set(int(s[2] - s[1] + 1) for s in fp.spans)) == [1, 32, 33, 64]
    poses = [pose_in(e, (55 + k % 30, -36 + k), (0.5, 0.5), 0.0) for k in range(72)]      # every alignment of a span against the 32-cell words
    templates, headings = [np.zeros((1, 2)), np.array([[0.0, 0.0], [0.16, 0.1]])], [[0.0], [math.pi / 2, math.pi]]
    seen = []
    for through, exempt in FLAG_COMBOS:
        seen.append(stacked(compare(e, 0, poses, templates, headings, fp, 0, 1, through, exempt, what="span widths")))
    seen = np.concatenate(seen).reshape(-1, 4)
    assert (seen[:, 0] < 0).any() and (seen[:, 0] >= 0).any() and (seen[:, 1] >= 0).any() and (seen[:, 1] < 0).any()
    e.close()


# ---- 5. seams, partial occupancy words, missing tiles, the lattice edge -------------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_seams_missing_tiles_and_the_lattice_edge(cs):
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs)) + 1))
    e = engine(2, cs=cs, pool_tiles=24, lattice_radius=1)
    scenes = seam_scene(e.dim, rng)
    for b, c in scenes:
        e.load_map(raster(e, b, np.where(c > 10, c, np.where(rng.random(c.shape) < 0.1, 0, PO.FREE)).astype(np.int8)), particle=1)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)     # another map, which must not be seen
    lo, hi = lattice_bounds(e.dim, 1)
    k = np.where(rng.random((30, 30)) < 0.02, PO.WALL, PO.FREE).astype(np.int8)
    e.load_map(raster(e, (hi - 30, hi, lo, lo + 30), k), particle=1)        # the lattice's corner
    c = cell_of(e)
    fp = plan.footprint_table(rectangle(9 * c, 5 * c), c, 32, pad_m=0.0)
    turns = [0.0, 1.2, -0.9, 0.0]
    tm, hd = plan.arc_templates([0.3, 0.3, 0.5, 0.0], turns, 2.0, 0.25), plan.arc_headings(turns, 2.0, 0.25)
    h = e.dim // 2

    def poses_at(cells):
        return [pose_in(e, q, rng.uniform(0.05, 0.95, 2), rng.uniform(-np.pi, np.pi)) for q in cells]

    regions = {}
    for b, _ in scenes:                                                     # beside and inside every written box
        regions[f"box {b}"] = poses_at([(int(rng.integers(b[0] - 8, b[1] + 8)), int(rng.integers(b[2] - 8, b[3] + 8))) for _ in range(3)])
    regions["the corner shared by four tiles"] = poses_at([(h, h), (h - 1, h - 1), (h - 1, h + 3)])
    regions["a tile that is not there"] = poses_at([(-h - 100, h + 100), (-h - 90, h + 120)])
    seen = []
    for name, poses in regions.items():
        for inflate, clear_max in ((0, 1), (7, 40)):
            compare(e, 1, poses, tm, hd, fp, inflate, clear_max, what=f"cs {cs} {name}")
        seen.append(stacked(compare(e, 1, poses, tm, hd, fp, 0, 1, True, 1, what=f"cs {cs} {name}")).reshape(-1, 4))
    seen = np.concatenate(seen)
    assert (seen[:, 0] < 0).any() and (seen[:, 0] >= 0).any() and (seen[:, 3] > 0).any()
    # two cells from the lattice's edges (the reach of a template that stands still): the rectangle covers cells outside the
    # lattice, which are unknown
    still, ahead = [np.zeros((1, 2))], [[0.0]]
    edge = [pose_in(e, (hi - 3, lo + 2), (0.5, 0.5), 0.0), pose_in(e, (hi - 3, lo + 2), (0.5, 0.5), math.pi / 2), pose_in(e, (lo + 2, lo + 2), (0.5, 0.5), 0.3),
            pose_in(e, (hi - 3, hi - 3), (0.9, 0.9), -2.0), pose_in(e, (hi - 8, lo + 6), (0.5, 0.5), math.pi / 2)]
    for through in (False, True):
        chk = compare(e, 1, edge, still, ahead, fp, 0, 1, through, what=f"cs {cs} the lattice's edge")
        assert chk.n_unknown[:4, 0].tolist() == [1] * 4 and (through or chk.first_blocked[:4, 0].tolist() == [0] * 4)
    assert compare(e, 1, edge[4:], still, ahead, fp, 0, 1, what="inside the corner's box").n_unknown.tolist() == [[0]]
    e.close()


# ---- 6. bins that wrap ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 7, 256])
def test_bins_wrap(H):
    e, (x0, y0), c = scene_engine()
    fp = bar(e, H)
    rng = np.random.default_rng(H)
    poses = [pose_in(e, (x0 + int(rng.integers(20, 180)), y0 + int(rng.integers(20, 130))), rng.uniform(0.05, 0.95, 2), th)
             for th in (-0.1, -3.0, -2 * math.pi, -7.5, 6.2, 2 * math.pi * (H - 0.6) / H, 13.0, -math.pi)]
    turns = np.array([1.5, -1.5, 3.0, 0.4])
    tm, hd = plan.arc_templates([0.3, 0.3, 0.1, 0.5], turns, 2.0, 0.25), plan.arc_headings(turns, 2.0, 0.25) + np.array([[0.0], [0.0], [2.0], [-9.0]])
    pb, tb = plan.heading_bins(np.array(poses)[:, 2], H), plan.heading_bins(hd, H)
    assert H == 1 or ((pb[:, None, None] + tb[None]).max() >= H and pb.max() == H - 1)
    for through, exempt in FLAG_COMBOS[:2]:
        chk = compare(e, 0, poses, tm, hd, fp, 0, 1, through, exempt, what=f"H {H}")
    assert chk.clear.any() and not chk.clear.all()
    e.close()


# ---- 7. the exemption ------------------------------------------------------------------------------------------------------------------------
def test_exempt_radii():
    e = engine(1)
    fp = table_of(e, [[(dx, -2, 2) for dx in range(-4, 5)]])               # 9 x 5 cells, one bin
    still, ahead = [np.zeros((1, 2))], [[0.0]]
    pose = [pose_in(e, (20, 20), (0.5, 0.5), 1.0)]
    for wall, clear_from in ((2, 2), (3, 3), (4, 99)):                      # a wall `wall` cells ahead: exempt within that Chebyshev distance
        c = np.full((40, 40), PO.FREE, np.int8)
        c[20 + wall, 21] = PO.WALL
        c[21, 20] = 0                                                       # an unknown cell next to the robot, inside every radius but 0
        e.load_map(raster(e, (0, 40, 0, 40), c))
        for exempt in (-1, 0, 1, 3):
            for through in (False, True):
                chk = compare(e, 0, pose, still, ahead, fp, 0, 1, through, exempt, what=f"wall {wall}")
                blocked = not (exempt >= clear_from and (through or exempt >= 1))      # not through: the unknown cell blocks too unless exempt
                assert stacked(chk)[0, 0].tolist() == [0 if blocked else -1, 0, 1 if wall > 1 else 0, 1], (wall, exempt, through)
    # the centre's own tests are exempt too: the robot stands on an occupied cell
    c = np.full((40, 40), PO.FREE, np.int8)
    c[20, 20] = PO.WALL
    e.load_map(raster(e, (0, 40, 0, 40), c))
    move = [np.array([[0.0, 0.0], [0.3, 0.0]])]
    assert compare(e, 0, [pose_in(e, (20, 20), (0.5, 0.5), 0.0)], move, [[0.0, 0.0]], fp, 7, 8, False, 0).first_blocked.tolist() == [[1]]      # the next centre is too near
    assert compare(e, 0, [pose_in(e, (20, 20), (0.5, 0.5), 0.0)], move, [[0.0, 0.0]], fp, 0, 1, False, 0).first_blocked.tolist() == [[-1]]
    assert compare(e, 0, [pose_in(e, (20, 20), (0.5, 0.5), 0.0)], move, [[0.0, 0.0]], fp, 0, 1, False, -1).first_blocked.tolist() == [[0]]
    e.close()


# ---- 8. three particles, three maps, three pairings, device outputs ------------------------------------------------------------------
def test_three_pairings_and_device_outputs():
    torch = pytest.importorskip("torch")
    e, (x0, y0), c = scene_engine(3)
    e.load_map(raster(e, (x0, x0 + 150, y0, y0 + 150), c.T[:150, :150].copy()), particle=2)     # the walls along the other axis
    poses, tm, hd = fuzz_inputs(inv_of(e), (x0, y0))                         # particle 1 holds no map at all
    poses = poses[[3, 11, 12]]
    poses[2, :2] = (np.array([x0 + 75, y0 + 64]) + 0.4) / inv_of(e)
    fp = fuzz_table()
    for inflate, clear_max, through, exempt in ((0, 1, False, -1), (7, 40, True, 1)):
        kw = dict(radius_m=radius(e, inflate), clear_max=clear_max, through_unknown=through, exempt_cells=None if exempt < 0 else exempt)
        own = e.check_footprints(poses, tm, hd, fp, particle=None, **kw)
        every = e.check_footprints(poses[0], tm, hd, fp, particle=None, **kw)
        assert own.first_blocked.shape == every.first_blocked.shape == own.steps.shape == every.steps.shape == (3, 16)
        for p in range(3):
            res, steps = oracle(e, p, poses[p:p + 1], tm, hd, fp, inflate, clear_max, through, exempt)
            same(stacked(own)[p], res[0], f"pose {p} in the map of particle {p}")
            same(own.steps[p], steps[0], "steps")
            res, steps = oracle(e, p, poses[:1], tm, hd, fp, inflate, clear_max, through, exempt)
            same(stacked(every)[p], res[0], f"pose 0 in the map of particle {p}")
            same(every.steps[p], steps[0], "steps")
            one = e.check_footprints(poses, tm, hd, fp, particle=p, **kw)
            res, steps = oracle(e, p, poses, tm, hd, fp, inflate, clear_max, through, exempt)
            same(stacked(one), res, f"every pose in the map of particle {p}")
        assert np.all(own.n_unknown[1] == own.steps[1]) and len(np.unique(stacked(own)[[0, 2]].reshape(-1, 4), axis=0)) > 3
        for host, args in ((own, dict(poses=poses, particle=None)), (every, dict(poses=poses[0], particle=None)), (one, dict(poses=poses, particle=2))):
            d = e.check_footprints(templates=tm, headings=hd, footprint=fp, device=True, **args, **kw)
            for a in d[:5]:
                assert isinstance(a, torch.Tensor) and a.device.type == "cuda" and a.dtype == torch.int32
            assert np.array_equal(stacked([a.cpu().numpy() for a in d[:4]]), stacked(host)) and np.array_equal(d.steps.cpu().numpy(), host.steps)
            assert np.array_equal(d.p_clear(), host.p_clear()) and np.array_equal(d.clearance_metres(), host.clearance_metres())
    # a world path across the posterior: a template at the pose (0, 0, 0), where the placement is the identity
    path = np.array([[x0 + 30.5, y0 + 30.5], [x0 + 30.5, y0 + 50.5], [x0 + 45.5, y0 + 50.5]]) / inv_of(e)
    world = e.check_footprints(np.zeros(3), [path], [plan.path_headings(path)], fp, particle=None)
    for p in range(3):
        res, steps = oracle(e, p, np.zeros((1, 3)), [path], [plan.path_headings(path)], fp, 0, 1)
        same(stacked(world)[p], res[0], "a world path")
    assert world.p_clear().shape == (1,) and world.steps.tolist() == [[36]] * 3
    e.close()


@pytest.fixture(scope="module")
def built():
    e = built_engine()
    yield e
    e.close()


def test_rollouts_from_the_poses_of_the_maps_the_engine_built(built):
    e = built
    assert e.counters()["resample_copies"] > 0
    turns = [0.0, 0.7, -0.7, 0.3, 0.0]
    poses, tm, hd = e.poses(), plan.arc_templates([0.3, 0.6, 0.6, 2.0, 3.0], turns, 3.0, 0.1), plan.arc_headings(turns, 3.0, 0.1)
    fp = plan.footprint_table(rectangle(0.8, 0.5), cell_of(e), 64)
    own = e.check_footprints(poses, tm, hd, fp, particle=None, radius_m=0.2, clear_max=60, exempt_cells=2)
    ref = e.check_rollouts(poses, tm, particle=None, radius_m=0.2, clear_max=60)
    assert own.inflate == 20 and own.first_blocked.shape == (e.P, 5)
    assert own.min_clearance.tobytes() == ref.min_clearance.tobytes() and own.steps.tobytes() == ref.steps.tobytes()
    for p in (0, 3, 7, e.P - 1):
        res, steps = oracle(e, p, poses[p:p + 1], tm, hd, fp, 20, 60, False, 2)
        same(stacked(own)[p], res[0], f"own rollouts, particle {p}")
        same(own.steps[p], steps[0], "steps")
    assert own.clear.any() and not own.clear.all()
    assert len(plan.rank_rollouts(own, weights=e.weights(), min_p_clear=0.0)) == 5


# ---- 9. the seeded fuzz ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate,clear_max,through,exempt", FUZZ_SETTINGS)
def test_fuzz(inflate, clear_max, through, exempt):
    e, (x0, y0), c = scene_engine()
    poses, tm, hd = fuzz_inputs(inv_of(e), (x0, y0))
    chk = compare(e, 0, poses, tm, hd, fuzz_table(), inflate, clear_max, through, exempt, what="fuzz")      # all 25 * 16, none left out
    blocked = float((chk.first_blocked >= 0).mean())
    print(f"fuzz {inflate} {clear_max} {through} {exempt}: blocked share {blocked:.2f}, unknown on {float((chk.first_unknown >= 0).mean()):.2f} of the rollouts")
    assert chk.first_blocked.shape == (25, 16) and 0.1 <= blocked <= 0.9
    e.close()


# ---- 10. arguments and call order ----------------------------------------------------------------------------------------------------------
def raw(e, particle, poses, xy, tbin, start, spans, fstart, n_poses=None, n_tmpl=None, n_bins=None, inflate=0, clear_max=1, exempt=-1, flags=0,
        null=(), rows=None):
    """rbpf_check_footprints itself: (return code, out, steps), both prefilled with FILL."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    tbin, start = np.ascontiguousarray(tbin, np.int32), np.ascontiguousarray(start, np.int32)
    spans, fstart = np.ascontiguousarray(spans, np.int32).reshape(-1, 3), np.ascontiguousarray(fstart, np.int32)
    N = len(poses) if n_poses is None else n_poses
    K = len(start) - 1 if n_tmpl is None else n_tmpl
    H = len(fstart) - 1 if n_bins is None else n_bins
    n = rows if rows is not None else max(N, e.P, 1) * max(K, 1)
    out, steps = np.full((n, 4), FILL, np.int32), np.full(n, FILL, np.int32)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ptr = lambda name, a, T: None if name in null else a.ctypes.data_as(T)
    rc = e._lib.rbpf_check_footprints(e._h, particle, ptr("poses", poses, D), N, ptr("xy", xy, D), ptr("tbin", tbin, I), ptr("start", start, I), K,
                                      ptr("spans", spans, I), ptr("fstart", fstart, I), H, inflate, clear_max, exempt, flags,
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
    poses = [[0.0, 0.0, 0.0], [1.0, 0.5, -1.0]]
    xy = [[0.0, 0.0], [0.5, 0.1], [0.0, 0.0], [0.3, 0.3], [0.1, 0.9], [-0.5, 0.2]]       # rmax 1.0 m: reach 22 cells
    tbin, start = [0, 1, 3, 0, 2, 3], [0, 2, 3, 6]
    spans, fstart = [[0, -2, 2], [1, -2, 2], [0, 0, 0], [-1, 0, 0], [0, -1, 1], [0, 0, 3]], [0, 2, 3, 4, 6]      # four bins
    three = poses + [[-1.0, 0.0, 2.0]]
    edge = lambda cell: [(cell + 0.5) / inv, 0.0, 0.3]
    line = np.stack([np.arange(128) * (206.4 / 127.0), np.zeros(128)], axis=1)
    span = lambda s: spans[:5] + [s]
    cases = dict(
        no_poses=dict(null=("poses",)), no_xy=dict(null=("xy",)), no_offsets=dict(null=("start",)), no_out=dict(null=("out",)),
        no_bins=dict(null=("tbin",)), no_spans=dict(null=("spans",)), no_span_offsets=dict(null=("fstart",)),
        nan_pose=dict(poses=[poses[0], [np.nan, 0.5, 1.0]]), inf_heading=dict(poses=[poses[0], [1.0, 0.5, np.inf]]),
        huge_heading=dict(poses=[poses[0], [1.0, 0.5, 4e9]]), nan_template=dict(xy=xy[:4] + [[np.nan, 0.0]] + xy[5:]),
        template_beyond_float64=dict(xy=xy[:5] + [[1.7e308, 0.0]]), offsets_from_one=dict(start=[1, 2, 3, 6]), empty_template=dict(start=[0, 2, 2, 6]),
        long_template=dict(xy=np.zeros((129, 2)), tbin=np.zeros(129), start=[0, 129]), no_pose=dict(n_poses=0), no_template=dict(n_tmpl=0),
        negative_templates=dict(n_tmpl=-1), particle_high=dict(particle=P), particle_low=dict(particle=-2),
        two_poses_three_particles=dict(particle=-1), inflate_negative=dict(inflate=-1), clear_max_equal=dict(inflate=4, clear_max=4),
        clear_max_large=dict(clear_max=321), flag=dict(flags=16), start_exempt_flag=dict(flags=4), own=dict(flags=8),
        pose_outside=dict(poses=[poses[0], edge(hi)]), reach_leaves_high=dict(poses=[poses[0], edge(hi - 22)]), reach_leaves_low=dict(poses=[poses[0], edge(lo + 21)]),
        too_many_steps=dict(xy=line, tbin=np.zeros(128), start=[0, 128]),
        bin_high=dict(tbin=[0, 1, 4, 0, 2, 3]), bin_low=dict(tbin=[0, 1, 3, 0, -1, 3]), no_bin=dict(n_bins=0), bins_negative=dict(n_bins=-1),
        bins_many=dict(n_bins=257, fstart=np.arange(258), spans=np.zeros((257, 3))), span_offsets_from_one=dict(fstart=[1, 2, 3, 4, 6]),
        empty_bin=dict(fstart=[0, 2, 2, 4, 6]), span_offsets_back=dict(fstart=[0, 3, 2, 4, 6]),
        bin_of_257_spans=dict(fstart=[0, 1, 2, 3, 260], spans=np.zeros((260, 3))), dx_high=dict(spans=span([128, 0, 0])), dx_low=dict(spans=span([-128, 0, 0])),
        y0_low=dict(spans=span([0, -128, -100])), y1_high=dict(spans=span([0, 100, 128])), y_backwards=dict(spans=span([0, 3, 2])), wide=dict(spans=span([0, 0, 64])),
        exempt_low=dict(exempt=-2), exempt_high=dict(exempt=256))
    for name, kw in cases.items():
        args = dict(particle=1, poses=poses, xy=xy, tbin=tbin, start=start, spans=spans, fstart=fstart)
        args.update(kw)
        rc, out, steps = raw(e, **args)
        assert rc == _lib.RBPF_EINVAL, (name, rc)
        assert np.all(out == FILL) and np.all(steps == FILL), name
    base = (xy, tbin, start, spans, fstart)
    rc, out, steps = raw(e, 1, poses, xy, tbin, start, span([0, 0, 64]), fstart)
    assert rc == _lib.RBPF_EINVAL and b"bin 3, span 1" in e._lib.rbpf_last_error(e._h)
    rc, out, steps = raw(e, 1, poses, xy, [0, 1, 3, 0, 2, 4], start, spans, fstart)
    assert rc == _lib.RBPF_EINVAL and b"template 2, waypoint 2" in e._lib.rbpf_last_error(e._h)
    rc, out, steps = raw(e, 1, [poses[0], edge(hi - 22)], *base)
    assert rc == _lib.RBPF_EINVAL and b"pose 1" in e._lib.rbpf_last_error(e._h)
    big = np.zeros((256, 3), np.int32)
    rc, out, steps = raw(e, 1, poses, xy, tbin, start, np.concatenate([spans[:4], big]), [0, 2, 3, 4, 260], exempt=255)      # 256 spans, exempt 255: taken
    assert rc == 0 and not np.any(out[:6] == FILL)
    rc, out, steps = raw(e, 1, poses, xy, tbin, start, span([127, -127, -64]), fstart)      # the bounds' edges
    assert rc == 0
    assert e._lib.rbpf_check_footprints(None, 1, None, 1, None, None, None, 1, None, None, 1, 0, 1, -1, 0, None, None) == _lib.RBPF_EINVAL
    # between the halves of a scan update
    ang, ranges, odo, truth = synthetic.make_log(2, 181)
    e.set_scan(ranges[0], ang)
    e.scan_update_begin(adj=False)
    rc, out, steps = raw(e, 1, poses, *base)
    assert rc == _lib.RBPF_ESTATE and np.all(out == FILL) and np.all(steps == FILL)
    e.scan_update_end()
    rc, out, steps = raw(e, 1, poses, *base, flags=2, exempt=1)              # the engine is still usable
    fp = table_of(e, [spans[:2], spans[2:3], spans[3:4], spans[4:]])
    templates = [np.array(xy[:2]), np.array(xy[2:3]), np.array(xy[3:])]
    step = 2 * math.pi / 4
    want = compare(e, 1, poses, templates, [[0.0, step], [3 * step], [0.0, 2 * step, -step]], fp, 0, 1, True, 1, what="after the step")
    assert rc == 0 and steps.tolist()[:2] == [11, 1]
    same(out[:6], stacked(want).reshape(-1, 4), "after the step")
    same(steps[:6], want.steps.reshape(-1), "after the step, steps")
    for ps in (three, poses[:1]):                                           # each pose its own particle; one pose in every particle's map
        rc, out, steps = raw(e, -1, ps, *base)
        assert rc == 0 and not np.any(out == FILL) and not np.any(steps == FILL)
    rc, out, steps = raw(e, 1, poses, *base, null=("steps",))                # steps may be NULL
    assert rc == 0 and not np.any(out[:6] == FILL) and np.all(steps == FILL)
    for bad in (dict(particle="worst"), dict(poses=np.zeros((2, 2))), dict(templates=[]), dict(headings=[[0.0, 0.0]]), dict(headings=[[0.0], [0.0], [0.0] * 3]),
                dict(footprint=plan.Footprint(fp.spans, fp.offsets, fp.H, 2 * fp.cell))):
        args = dict(poses=poses, templates=templates, headings=[[0.0, 0.0], [0.0], [0.0] * 3], footprint=fp, particle=1)
        args.update(bad)
        with pytest.raises(ValueError):
            e.check_footprints(**args)
    e.close()


def test_too_many_results_write_nothing():
    """rows * n_tmpl >= 2^29: 1024 particles, one pose in every map, and 2^19 one-waypoint templates, every table valid."""
    from thesis_amd import _lib
    P, n = 1024, 1 << 19
    e = engine(P, cs=0.1, pool_tiles=P)
    xy, start = np.zeros((n, 2)), np.arange(n + 1, dtype=np.int32)
    rc, out, steps = raw(e, -1, np.zeros((1, 3)), xy, np.zeros(n), start, [[0, 0, 0]], [0, 1], rows=1)
    assert rc == _lib.RBPF_EINVAL and b"2^29" in e._lib.rbpf_last_error(e._h)
    assert np.all(out == FILL) and np.all(steps == FILL)
    rc, out, steps = raw(e, -1, np.zeros((1, 3)), xy[:512], np.zeros(512), start[:513], [[0, 0, 0]], [0, 1])      # 2^19 results, far below
    assert rc == 0 and np.all(steps == 1) and out.shape == (n, 4)
    assert np.all(out == [0, 0, 1, 1])                                       # no map anywhere: unknown, so blocked, at step 0
    e.close()


# ---- 11. state and repeatability -------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_and_repeats_itself(built):
    e = built

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.render_map(0).cells, e.render_map(5).cells, e.map_extent())

    s0 = state()
    turns = np.linspace(-0.8, 0.8, 7)
    tm, hd = plan.arc_templates(np.linspace(0.2, 1.0, 7), turns, 3.0, 0.1), plan.arc_headings(turns, 3.0, 0.1)
    fp = plan.footprint_table(rectangle(0.8, 0.5), cell_of(e), 64)
    a = e.check_footprints(e.poses(), tm, hd, fp, particle=None, radius_m=0.15, clear_max=60)
    b = e.check_footprints(e.poses(), tm, hd, fp, particle=None, radius_m=0.15, clear_max=60)
    e.check_footprints(e.poses()[:5], tm, hd, fp, particle=4, through_unknown=True, exempt_cells=3)
    e.check_footprints(e.poses()[0], tm, hd, fp, particle=None)
    for x, y in zip(a[:5], b[:5]):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(state(), s0):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)


# ---- 12. the door, end to end ------------------------------------------------------------------------------------------------------------------
def test_the_door_end_to_end():
    """A 0.9 m door in a wall and a 0.8 m x 0.5 m robot: lengthwise it fits, at its circumscribed radius it does not, sideways it
    does not."""
    e = engine(1)
    c = np.full((120, 120), PO.FREE, np.int8)
    c[60:62] = PO.WALL
    c[60:62, 51:69] = PO.FREE                                              # 18 cells of 0.05 m
    e.load_map(raster(e, (0, 120, 0, 120), c))
    fp = plan.footprint_table(rectangle(0.8, 0.5), cell_of(e), 64)
    pose = pose_in(e, (30, 59), (0.5, 0.99), 0.0)                           # on the door's axis
    straight = np.stack([np.linspace(0.0, 3.0, 13), np.zeros(13)], axis=1)[None]
    through = compare(e, 0, [pose], straight, np.zeros((1, 13)), fp, 25, 60, what="the door, lengthwise")      # inscribed radius 0.25 m
    assert through.clear.all() and through.steps.tolist() == [[61]] and through.min_clearance.tolist() == [[45]]
    disc = e.check_rollouts([pose], straight, particle=0, radius_m=0.5 * math.hypot(0.8, 0.5), clear_max=60)
    assert disc.inflate == 47 and 20 <= int(disc.first_blocked[0, 0]) <= 30
    sideways = compare(e, 0, [pose], straight, np.full((1, 13), math.pi / 2), fp, 25, 60, what="the door, sideways")
    assert 15 <= int(sideways.first_blocked[0, 0]) <= 25
    ranked = plan.rank_rollouts(e.check_footprints([pose], np.concatenate([straight, straight]), [np.zeros(13), np.full(13, math.pi / 2)], fp, particle=0,
                                                   radius_m=0.25, clear_max=60))
    assert ranked.tolist() == [0]
    e.close()
