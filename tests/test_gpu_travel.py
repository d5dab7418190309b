"""Travel cost on the GPU (rbpf_travel_cost, kernels_travel.hip) against the scalar oracle of
tests/travel_oracle.py run on the rendered maps: cost, clearance and goal costs by equality.  Then the margin, unknown cells,
the sources, every particle at once, what the call leaves alone, its device outputs and its argument checks, and a path to a
reachable view."""
import ctypes as C

import numpy as np
import pytest

from tests import travel_oracle as T
from tests.cast_oracle import lattice_bounds
from tests.test_gpu_cast import built_engine, engine, load_room16, raster, rng_state, seam_scene

pytestmark = pytest.mark.gpu

FREE, WALL = -30, 30


def inv_of(e):
    return e.dim / float(e.cfg.tile_len_m)


def centre(e, X, Y):
    return [(X + 0.5) / inv_of(e), (Y + 0.5) / inv_of(e)]


def oracle(e, p, box, starts, goals, inflate, clear_max, through_unknown=False):
    """(cost, clearance, goal_cost) of the oracle on render_map(p) over the box grown by the margin."""
    grown = e.render_map(p, box=T.grown_box(box, clear_max)).cells
    return T.travel(grown, box, inv_of(e), float(e.cfg.quantum), float(e.cfg.occupied_threshold), starts, goals, inflate,
                    clear_max, through_unknown)


def same(tr, want, what=""):
    """A Travel of one particle equals the oracle's (cost, clearance, goal_cost)."""
    for name, got, ref in zip(("cost", "clearance", "goal_cost"), tr[:3], want):
        if got is None:
            continue
        got = np.asarray(got)
        assert got.shape == ref.shape and got.dtype == ref.dtype, (what, name, got.shape, got.dtype)
        bad = got != ref
        if bad.any():
            k = tuple(int(q) for q in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {name} differs in {int(bad.sum())} of {bad.size} places; first {k}: got {got[k]}, oracle {ref[k]}")


def raw(e, particle, box, starts, goals, inflate, clear_max, flags=0, want=("cost", "clearance", "goal"), n_start=None,
        n_goals=None, fill=-77):
    """rbpf_travel_cost itself: (return code, cost, clearance, goal_cost, rounds); outputs not in `want` are passed as NULL, the
    others are prefilled with `fill`."""
    nx, ny = (4, 4) if box is None else (max(int(box[1]) - int(box[0]), 0), max(int(box[3]) - int(box[2]), 0))
    s = None if starts is None else np.ascontiguousarray(starts, np.float64).reshape(-1, 2)
    g = None if goals is None else np.ascontiguousarray(goals, np.float64).reshape(-1, 2)
    ns = (0 if s is None else len(s)) if n_start is None else n_start
    ng = (0 if g is None else len(g)) if n_goals is None else n_goals
    np_ = e.P if particle < 0 else 1
    cost = np.full((nx, ny), fill, np.int32) if "cost" in want else None
    clear = np.full((nx, ny), fill & 0xffff, np.uint16) if "clearance" in want else None
    goal = np.full((np_, max(ng, 1)) if particle < 0 else (max(ng, 1),), fill, np.int32) if "goal" in want else None
    rounds = C.c_int32(fill)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    b = None if box is None else np.array(box, np.int32)
    rc = e._lib.rbpf_travel_cost(e._h, particle, None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)), dp(s), ns, dp(g), ng,
                                 inflate, clear_max, flags, vp(cost), vp(clear), vp(goal), C.byref(rounds))
    return rc, cost, clear, goal, rounds.value


# ---- 1. the exact room ---------------------------------------------------------------------------------------------------------
def test_room16_equals_the_oracle_with_every_null_pattern():
    e = engine(2)
    load_room16(e)                                       # walls 30 round an interior of 0: unknown, so crossed only with the flag
    box = e.map_extent(1)
    assert box == (-200, 200, -200, 200)
    starts = [[0.0, 0.0], [6.5, -7.0]]
    goals = [[7.9, 7.9], [-7.99, 0.0], [4.0, 4.0], [0.0, 0.0], [30.0, 0.0], [-3.1, 5.2]]     # a corner, beside a wall, in a pillar, a start, outside
    for radius in (0.0, 0.2):
        tr = e.travel_cost(starts, goals, particle=1, radius_m=radius, through_unknown=True)
        assert tr.box == box and tr.inflate == (0 if radius == 0.0 else 20) and tr.clear_max == tr.inflate + 1 and tr.rounds > 0
        want = oracle(e, 1, box, starts, goals, tr.inflate, tr.clear_max, True)
        same(tr, want, f"room16 radius {radius}")
        assert tr.goal_cost[2] == -1 and tr.goal_cost[3] == 0 and tr.goal_cost[4] == -1 and tr.goal_cost[5] > 0
        assert (tr.goal_cost[0] >= 0) == (radius == 0.0)                   # the corner cell touches two walls
        print(f"room16 radius {radius}: {tr.rounds} rounds, {(tr.cost >= 0).sum()} cells reached, largest cost {tr.cost.max()}")
        if radius:
            for pattern in (("cost",), ("clearance",), ("goal",), ("cost", "goal"), ("clearance", "goal")):
                rc, c, cl, g, rounds = raw(e, 1, box, starts, goals, tr.inflate, tr.clear_max, 2, pattern)
                assert rc == 0 and rounds == tr.rounds, pattern
                same((c, cl, g), want, f"room16 {pattern}")
    # without the flag nothing but the start cells carries the robot: the interior is unknown
    tr = e.travel_cost(starts, goals, particle=1, radius_m=0.0)
    same(tr, oracle(e, 1, box, starts, goals, 0, 1), "room16 known-free only")
    assert (tr.cost == 0).sum() == 2 and (tr.cost == -1).sum() == tr.cost.size - 2
    e.close()


# ---- 2. a maze that needs many rounds ----------------------------------------------------------------------------------------
def maze_cells():
    """200 x 150 free cells, walls at x = 10 k with a 3-cell gap at alternating ends, 3 % clutter."""
    c = np.full((200, 150), FREE, np.int8)
    clutter = np.random.default_rng(1).random(c.shape) < 0.03
    for k in range(1, 20):
        c[10 * k] = WALL
    c[clutter] = WALL
    for k in range(1, 20):
        c[10 * k, (slice(2, 5) if k % 2 else slice(145, 148))] = FREE
    return c


def test_a_serpentine_maze_across_a_tile_seam():
    e = engine(1)
    h = e.dim // 2
    x0, y0 = -h - 77, -31                                 # negative, no multiple of 64, across the seam X = -h
    cells = maze_cells()
    box = (x0, x0 + 200, y0, y0 + 150)
    e.load_map(raster(e, box, cells))
    start = centre(e, x0 + 3, y0 + 3)
    goals = [centre(e, x0 + 195, y0 + 75), centre(e, x0 + 10, y0 + 50)]
    tr = e.travel_cost([start], goals, particle=0)
    want = oracle(e, 0, box, [start], goals, 0, 1)
    same(tr, want, "maze")
    reached = int((want[0] >= 0).sum())
    print(f"maze: {tr.rounds} rounds for 12 blocks, largest cost {want[0].max()}, {reached} cells reached")
    assert reached > 26000 and want[0].max() > 13000 and tr.goal_cost[0] > 13000       # the far end is reached, the long way
    assert tr.rounds > 12                                 # more rounds than blocks: no single pass over the box does this
    cut = (x0, x0 + 193, y0, y0 + 150)                    # the last blocks along x are one cell wide
    tr = e.travel_cost([start], goals, particle=0, box=cut)
    same(tr, oracle(e, 0, cut, [start], goals, 0, 1), "maze, cut box")
    assert tr.goal_cost[0] == -1 and tr.cost[192].max() > 13000 and tr.rounds > 12
    cut = (x0, x0 + 193, y0, y0 + 129)                    # and those along y: the gaps at y = 145 .. 147 are outside, the maze ends at x = 20
    tr = e.travel_cost([start], goals, particle=0, box=cut)
    same(tr, oracle(e, 0, cut, [start], goals, 0, 1), "maze, box cut twice")
    assert tr.cost[:20].max() > 0 and np.all(tr.cost[21:] == -1)
    inside = centre(e, x0 + 10, y0 + 50)                  # a start inside the first wall
    tr = e.travel_cost([inside], goals, particle=0)
    want = oracle(e, 0, box, [inside], goals, 0, 1)
    same(tr, want, "maze, start in a wall")
    assert cells[10, 50] == WALL and tr.cost[10, 50] == 0 and tr.goal_cost[1] == 0 and tr.cost[9, 50] == 5 and tr.cost[11, 50] == 5
    for radius in (0.05, 0.09):                           # an inflated robot: the clutter narrows the corridors, then shuts them
        tr = e.travel_cost([start], goals, particle=0, radius_m=radius)
        want = oracle(e, 0, box, [start], goals, tr.inflate, tr.clear_max)
        same(tr, want, f"maze radius {radius}")
        print(f"maze radius {radius}: inflate {tr.inflate}, {tr.rounds} rounds, {(want[0] >= 0).sum()} cells reached")
    e.close()


# ---- 3. the margin -------------------------------------------------------------------------------------------------------------
def test_occupied_cells_outside_the_box_count():
    e = engine(2, pool_tiles=40, lattice_radius=1)
    c = np.full((24, 24), FREE, np.int8)                  # raster cell (i, j) = mosaic (i - 2, j - 2): the box is its inner 20 x 20
    c[2 + 2:, 2 + 10] = WALL                              # a wall Y = 10 from X = 2 on: the passage is X = 0, 1
    for p in (0, 1):
        e.load_map(raster(e, (-2, 22, -2, 22), c), particle=p)
    e.load_map(raster(e, (-1, 0, 10, 11), np.full((1, 1), WALL, np.int8)), particle=1)     # one cell outside the box, beside the passage
    box = (0, 20, 0, 20)
    start, goal = centre(e, 5, 3), centre(e, 5, 16)
    for p in (0, 1):
        for inflate, clear_max in ((0, 1), (5, 6), (5, 320), (9, 10)):
            rc, cost, clear, g, _ = raw(e, p, box, [start], [goal], inflate, clear_max)
            assert rc == 0
            same((cost, clear, g), oracle(e, p, box, [start], [goal], inflate, clear_max), f"margin p {p} inflate {inflate} clear_max {clear_max}")
            if inflate == 5:
                assert (g[0] >= 0) == (p == 0)            # the outside cell closes the passage
                assert clear[0, 10] == min(10 if p == 0 else 5, clear_max)
            if clear_max == 320:
                assert clear[0, 0] == (54 if p == 0 else 52)               # (2, 10) is the nearest occupied cell, or (-1, 10)
    # a box in the lattice's corner: the grown box leaves the lattice, where v = 0
    lo, hi = lattice_bounds(e.dim, 1)
    rng = np.random.default_rng(5)
    k = np.where(rng.random((30, 30)) < 0.05, WALL, FREE).astype(np.int8)
    k[15, 15] = FREE
    corner = (hi - 30, hi, lo, lo + 30)
    e.load_map(raster(e, corner, k), particle=0)
    s = centre(e, hi - 15, lo + 15)
    for inflate, clear_max in ((0, 1), (6, 320)):
        rc, cost, clear, g, _ = raw(e, 0, corner, [s], [centre(e, hi - 1, lo)], inflate, clear_max)
        assert rc == 0
        same((cost, clear, g), oracle(e, 0, corner, [s], [centre(e, hi - 1, lo)], inflate, clear_max), f"lattice corner {clear_max}")
    assert raw(e, 0, (hi - 30, hi + 1, lo, lo + 30), [s], None, 0, 1, want=("cost",))[0] == -1
    e.close()


# ---- 4. unknown and weakly occupied cells ------------------------------------------------------------------------------------
def test_unknown_cells_block_unless_crossing_is_allowed():
    e = engine(1)
    c = np.full((12, 20), FREE, np.int8)
    c[:, 8:] = 0                                          # unknown from Y = 8 on: Y = 7 is the frontier
    c[:, 14] = 7                                          # 0 < v quantum <= threshold
    c[:, 17] = 11                                         # occupied
    box = (40, 52, -10, 10)
    e.load_map(raster(e, box, c))
    start = centre(e, 45, -8)
    for through in (False, True):
        tr = e.travel_cost([start], None, particle=0, through_unknown=through)
        same(tr, oracle(e, 0, box, [start], None, 0, 1, through), f"unknown, through {through}")
        assert tr.goal_cost is None
        assert np.all(tr.cost[:, 7] >= 0)                 # the frontier cells are reached
        assert np.all((tr.cost[:, 8:17] >= 0) == through) # the unknown and the weakly occupied cells behind them
        assert np.all(tr.cost[:, 17:] == -1)              # never an occupied cell, nor what lies behind the wall
    e.close()


# ---- 5. sources ------------------------------------------------------------------------------------------------------------------
def test_sources():
    e = engine(2)
    rng = np.random.Generator(np.random.PCG64(8))
    (box, c) = seam_scene(e.dim, rng)[0]                  # sparse occupied cells round the corner shared by four tiles
    c = np.where(c > 10, c, FREE).astype(np.int8)
    e.load_map(raster(e, box, c), particle=1)
    free = np.argwhere(c < 0)
    a, b = (centre(e, box[0] + i, box[2] + j) for i, j in (free[7], free[-9]))
    outside = [[(box[1] + 0.5) / inv_of(e), a[1]], [a[0], (box[2] - 0.5) / inv_of(e)]]
    tr = e.travel_cost(outside, [a, outside[0]], particle=1)
    assert np.all(tr.cost == -1) and tr.goal_cost.tolist() == [-1, -1] and np.all(tr.clearance <= 1)
    fa, fb = (e.travel_cost([s], [outside[1], b], particle=1) for s in (a, b))
    both = e.travel_cost([a, outside[0], b], [outside[1], b], particle=1)
    same(fa, oracle(e, 1, box, [a], [outside[1], b], 0, 1), "one source")
    assert np.array_equal(both.cost, np.where(fa.cost < 0, fb.cost, np.where(fb.cost < 0, fa.cost, np.minimum(fa.cost, fb.cost))))
    assert both.goal_cost.tolist() == [-1, 0] and fa.goal_cost[0] == -1 and fa.goal_cost[1] == fb.cost[tuple(free[7])] > 0
    empty = e.travel_cost([a], particle=0, box=box)       # a particle without a tile here: all unknown
    assert (empty.cost == 0).sum() == 1 and (empty.cost == -1).sum() == empty.cost.size - 1
    e.close()


# ---- 5b. the rounds: what the host queues, reads and counts ---------------------------------------------
def free_square(e):
    """40 x 40 known-free cells in one block, a start inside: (box, start, the cost of every cell)."""
    box = (10, 50, -20, 20)
    e.load_map(raster(e, box, np.full((40, 40), FREE, np.int8)))
    di, dj = np.abs(np.mgrid[0:40, 0:40] - np.array([7, 30]).reshape(2, 1, 1))
    return box, centre(e, box[0] + 7, box[2] + 30), (5 * np.maximum(di, dj) + 2 * np.minimum(di, dj)).astype(np.int32)


def test_rounds_of_one_block_with_work():
    e = engine(1)
    box, start, cost = free_square(e)
    tr = e.travel_cost([start], particle=0, box=box)
    same(tr, oracle(e, 0, box, [start], None, 0, 1), "free square")
    assert np.array_equal(tr.cost, cost)
    # round 0 changes the block, round 1 runs it and changes nothing, rounds 2 .. 7 of the first read find no dirty block
    assert e.travel_stats() == {"rounds": 8, "block_runs": 2, "blocks": 1} and tr.rounds == 8
    e.close()


def test_rounds_of_one_block_with_one_round_per_read(monkeypatch):
    e = engine(1)
    box, start, cost = free_square(e)
    monkeypatch.setenv("RBPF_TRAVEL_ROUNDS_PER_READ", "1")
    tr = e.travel_cost([start], particle=0, box=box)
    assert np.array_equal(tr.cost, cost)
    assert e.travel_stats() == {"rounds": 2, "block_runs": 2, "blocks": 1} and tr.rounds == 2
    e.close()


def test_rounds_with_nothing_to_do():
    e = engine(1)
    box = (0, 100, 0, 100)                                # 2 x 2 blocks
    e.load_map(raster(e, box, np.full((100, 100), FREE, np.int8)))
    tr = e.travel_cost([centre(e, -3, 50)], particle=0, box=box)          # the only start lies outside the box
    assert np.all(tr.cost == -1) and tr.cost.shape == (100, 100)
    assert e.travel_stats() == {"rounds": 8, "block_runs": 0, "blocks": 4} and tr.rounds == 8
    e.close()


# ---- 6. maps the engine built: every particle, state, device outputs, a path ---------------------------------------------------
@pytest.fixture(scope="module")
def built():
    e = built_engine()
    yield e
    e.close()


GOALS = [[1.0, 0.5], [-2.0, 1.5], [3.0, -3.0], [0.2, 6.0], [40.0, 0.0]]


def test_every_particle(built, monkeypatch):
    e = built
    P, box = e.P, e.map_extent(None)
    poses = e.poses()
    # three goals where the particles' maps disagree (known free in some, not in others) beside a cell free in all of them
    free = np.stack([e.render_map(p, box=box).cells < 0 for p in range(P)])
    core = np.pad(free.all(axis=0), 1)
    beside = core[:-2, 1:-1] | core[2:, 1:-1] | core[1:-1, :-2] | core[1:-1, 2:]
    mixed = np.argwhere(free.any(axis=0) & ~free.all(axis=0) & beside)
    assert len(mixed) >= 3
    goals = [centre(e, box[0] + i, box[2] + j) for i, j in mixed[[0, len(mixed) // 2, -1]]] + GOALS[:1] + GOALS[4:]
    for starts in (poses[:, :2], poses[3, :2]):           # n_start == P: each particle's own pose; n_start == 1
        allp = e.travel_cost(starts, goals, particle=None)
        assert allp.cost is None and allp.clearance is None and allp.goal_cost.shape == (P, 5) and allp.box == box
        own = lambda p: starts[p] if np.ndim(starts) == 2 else starts
        fields = [e.travel_cost(own(p), goals, particle=p, box=box) for p in range(P)]
        assert np.array_equal(allp.goal_cost, np.stack([f.goal_cost for f in fields]))
        assert np.all(allp.goal_cost[:, 4] == -1) and np.all(allp.goal_cost[:, 3] > 0)
        assert len(np.unique(allp.goal_cost, axis=0)) > 1                  # the particles hold different maps
        for p in (0, 7, P - 1):
            same(fields[p], oracle(e, p, box, [own(p)], goals, allp.inflate, allp.clear_max), f"built map, particle {p}")
        monkeypatch.setenv("RBPF_TRAVEL_BATCH", "3")                       # 16 particles in six batches
        batched = e.travel_cost(starts, goals, particle=None)
        monkeypatch.delenv("RBPF_TRAVEL_BATCH")
        assert np.array_equal(batched.goal_cost, allp.goal_cost) and batched.rounds > allp.rounds
    inflated = e.travel_cost(poses[:, :2], GOALS, particle=None, radius_m=0.1)
    assert np.array_equal(inflated.goal_cost, np.stack([e.travel_cost(poses[p, :2], GOALS, particle=p, box=box, radius_m=0.1).goal_cost for p in range(P)]))
    best = e.travel_cost(poses[0, :2], GOALS, radius_m=0.1)
    k = int(np.argmax(e.weights()))
    assert np.array_equal(best.goal_cost, e.travel_cost(poses[0, :2], GOALS, particle=k, radius_m=0.1).goal_cost)


def test_a_call_changes_nothing_and_repeats_itself(built):
    torch = pytest.importorskip("torch")
    e = built

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.render_map(0).cells, e.render_map(5).cells, e.map_extent())

    s0 = state()
    start = e.poses()[2, :2]
    a = e.travel_cost(start, GOALS, particle=2, radius_m=0.15, clear_max=60)
    b = e.travel_cost(start, GOALS, particle=2, radius_m=0.15, clear_max=60)
    e.travel_cost(e.poses()[:, :2], GOALS, particle=None, through_unknown=True)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a.clearance.max() == 60 and a.clearance.min() == 0 and (a.cost > 0).any()
    for x, y in zip(state(), s0):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    d = e.travel_cost(start, GOALS, particle=2, radius_m=0.15, clear_max=60, device=True)
    assert isinstance(d.cost, torch.Tensor) and d.cost.device.type == "cuda" and d.cost.dtype == torch.int32
    assert d.clearance.dtype == torch.int16 and d.goal_cost.dtype == torch.int32 and d.rounds == a.rounds
    assert np.array_equal(d.cost.cpu().numpy(), a.cost) and np.array_equal(d.clearance.cpu().numpy().view(np.uint16), a.clearance)
    assert np.array_equal(d.goal_cost.cpu().numpy(), a.goal_cost)
    dall = e.travel_cost(e.poses()[:, :2], GOALS, particle=None, radius_m=0.15, device=True)
    assert np.array_equal(dall.goal_cost.cpu().numpy(), e.travel_cost(e.poses()[:, :2], GOALS, particle=None, radius_m=0.15).goal_cost)
    s = torch.cuda.Stream()                               # on a borrowed stream that is torch's current one
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = e.travel_cost(start, GOALS, particle=2, radius_m=0.15, clear_max=60, device=True)
        ok = torch.equal(d2.cost, d.cost) and torch.equal(d2.clearance, d.clearance) and int(d2.cost.sum()) == int(a.cost.sum())
        e.release_stream()
    assert ok


def test_a_path_to_a_reachable_view(built):
    from thesis_amd import explore, plan
    from thesis_amd.datasets import synthetic
    e = built
    k = int(np.argmax(e.weights()))
    pose = e.poses()[k]
    ang = synthetic.beam_angles(91)
    nv = explore.next_reachable_view(e, ang, e.poses(), particle=None, k=6, radius_m=0.2, travel_weight=0.5, min_reach=0.6)
    assert len(nv.poses) > 0 and np.all(nv.reach[nv.order] >= 0.6) and nv.goal_cost.shape == nv.gain.shape == (e.P, len(nv.candidates))
    assert np.all(np.diff(nv.scores) <= 0)
    one = explore.next_reachable_view(e, ang, pose, particle=k, k=6, radius_m=0.2)
    assert len(one.poses) > 0 and np.all(one.goal_cost[one.order] >= 0)
    goal = one.poses[0]
    tr = e.travel_cost(pose, [goal[:2]], particle=k, radius_m=0.2)
    path = plan.path_to(tr, goal[:2])
    cells = np.floor(path * tr.inv).astype(int)
    assert cells[0].tolist() == np.floor(pose[:2] * tr.inv).astype(int).tolist()
    assert cells[-1].tolist() == np.floor(goal[:2] * tr.inv).astype(int).tolist()
    ij = cells - [tr.box[0], tr.box[2]]
    assert tr.cost[tuple(ij[0])] == 0 and tr.cost[tuple(ij[-1])] == tr.goal_cost[0] == one.goal_cost[one.order[0]]
    assert np.all(tr.clearance[tuple(ij[1:].T)] > tr.inflate) and np.abs(np.diff(ij, axis=0)).max() == 1
    assert plan.cost_metres(tr.goal_cost[0], tr.cell) >= 0.98 * np.hypot(*(path[-1] - path[0]))     # 7 / 5 is a little less than sqrt(2)


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_call_order_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P = 3
    e = engine(P)
    load_room16(e)
    box = (-40, 30, -20, 50)
    s, g = [[0.0, 0.0]], [[0.5, 0.5], [1.0, -0.5]]
    sP = [[0.0, 0.0]] * P
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))

    def untouched(out, fill=-77):
        return all(a is None or np.all(a == (fill & 0xffff if a.dtype == np.uint16 else fill)) for a in out[1:4]) and out[4] == fill

    cases = dict(
        no_box=dict(box=None), no_starts=dict(starts=None, n_start=1), no_outputs=dict(want=()),
        goal_cost_without_goals=dict(goals=None, want=("goal",)), goal_cost_zero_goals=dict(n_goals=0, want=("cost", "goal")),
        negative_goals=dict(n_goals=-1, want=("cost",)), all_with_cost=dict(particle=-1, starts=sP, want=("cost", "goal")),
        all_with_clearance=dict(particle=-1, starts=sP, want=("clearance", "goal")), all_without_goal_cost=dict(particle=-1, starts=sP, want=()),
        all_two_starts=dict(particle=-1, starts=sP[:2], want=("goal",)), no_start=dict(n_start=0), negative_starts=dict(n_start=-1),
        nan_start=dict(starts=[[np.nan, 0.0]]), inf_start=dict(starts=[[0.0, 0.0], [0.0, -np.inf]]), nan_goal=dict(goals=[[0.0, 0.0], [0.0, np.nan]]),
        particle_high=dict(particle=P), particle_low=dict(particle=-2), box_reversed=dict(box=(30, -40, -20, 50)), box_empty=dict(box=(0, 0, 0, 10)),
        box_outside=dict(box=(hi - 5, hi + 1, 0, 10)), box_outside_low=dict(box=(0, 10, lo - 1, lo + 5)), box_large=dict(box=(lo, lo + 16385, lo, lo + 8192), want=("goal",)),
        inflate_negative=dict(inflate=-1), clear_max_equal=dict(inflate=4, clear_max=4), clear_max_large=dict(clear_max=321), flags=dict(flags=4))
    for name, kw in cases.items():
        args = dict(particle=1, box=box, starts=s, goals=g, inflate=0, clear_max=1)
        args.update(kw)
        out = raw(e, args.pop("particle"), args.pop("box"), **args)
        assert out[0] == _lib.RBPF_EINVAL, (name, out[0])
        assert untouched(out), name
    assert e._lib.rbpf_travel_cost(None, 1, None, None, 1, None, 0, 0, 1, 0, None, None, None, None) == _lib.RBPF_EINVAL
    # between the halves of a scan update
    ang, ranges, odo, truth = synthetic.make_log(2, 181)
    e.set_scan(ranges[0], ang)
    e.scan_update_begin(adj=False)
    out = raw(e, 1, box, s, g, 0, 1)
    assert out[0] == _lib.RBPF_ESTATE and untouched(out)
    e.scan_update_end()
    out = raw(e, 1, box, s, g, 0, 1, 2)                   # the engine is still usable; rounds may be NULL
    assert out[0] == 0 and not untouched(out) and out[4] > 0
    b = np.array(box, np.int32)
    st = np.zeros((1, 2))
    cl = np.zeros((70, 70), np.uint16)
    assert e._lib.rbpf_travel_cost(e._h, 1, b.ctypes.data_as(C.POINTER(C.c_int32)), st.ctypes.data_as(C.POINTER(C.c_double)), 1, None, 0, 0, 7, 0,
                                   None, C.c_void_p(cl.ctypes.data), None, None) == 0 and cl.max() == 7
    with pytest.raises(ValueError):
        e.travel_cost(s, particle="worst")
    with pytest.raises(ValueError):
        e.travel_cost(s, particle=None)                   # no goals: nothing to compute
    with pytest.raises(ValueError):
        e.travel_cost([0.0], g)
    e.close()
