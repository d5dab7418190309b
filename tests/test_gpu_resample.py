"""What a resample moves (kernels_resample.hip) against the NumPy model of tests/resample_oracle.py, everything by equality.

1. Every launch path - state permutation fused (P <= 1024) or at the head of the copy kernel, planning fused (P <= 4096) or one
   launch per stage, jobs within the grid or through the queue, no job at all, no trigger - on both entry points: rbpf_resample
   from weights and rbpf_apply_resample_local from a source list.  The maps come from map updates (tight, different written
   boxes) and differ in their tile sets, so copies allocate and release tiles.
2. Directed geometry at P = 16 with loaded rasters, whose written boxes are known exactly: the union of the two boxes, the
   16-byte cell groups and the 32-column occupancy words at every border, and the bytes moved.
3. What tiles() cannot see: the occupancy words through travel_cost's clearance, the written boxes through map_extent and
   render_map, the free stack by allocating every free tile, and pool exhaustion as an error code."""
import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests import resample_oracle as R
from tests import travel_oracle as T
from tests.resample_scenes import (ANC, CLEAR_MAX, DEAD, HOME, NEAR, TILE, Loaded, Scene, apply_sources, bits, check_hidden, extras,
                                   fill_the_pool, free_positions, geometry_cases, load_one_cell, make_engine, queue_sources,
                                   same_tiles, scene_poses, steady, tile_count)

pytestmark = pytest.mark.gpu


# ---- 1. maps built by map updates, every launch path -------------------------------------------------------------------------
def pattern(P, n2, n3, seed):
    """Copies per old particle: n2 particles twice, n3 three times, n2 + 2 n3 not at all, every other one once.  An extra tile
    goes where it was not (its owner copied) and leaves where it was (its owner dead)."""
    rng = np.random.default_rng(seed)
    x = extras(P)
    rest = [int(p) for p in rng.permutation(P) if p not in x]
    two, rest = [x[0]] + rest[:n2 - 1], rest[n2 - 1:]
    three, rest = [x[2]] + rest[:n3 - 1], rest[n3 - 1:]
    dead = [x[1]] + rest[:n2 + 2 * n3 - 1]
    cnt = np.ones(P, dtype=np.int64)
    cnt[two], cnt[three], cnt[dead] = 2, 3, 0
    assert cnt.sum() == P
    return cnt


def weights_of(cnt):
    """Log-weights for which systematic resampling gives exactly cnt copies: -inf counts 0 (main.py:53), the rest is linear."""
    return np.where(cnt == 0, -np.inf, 1000.0 * cnt)


def compared_particles(P, idx, old_maps, new_maps):
    """All of them up to 1100 particles; beyond, every copy destination, every particle whose tile positions changed and every
    16th of the others."""
    if P <= 1100:
        return list(range(P))
    must = set(R.copy_destinations(idx)) | {j for j in range(P) if set(old_maps[j]) != set(new_maps[j])}
    rest = [j for j in range(P) if j not in must]
    return sorted(must | set(rest[::16]))


def resample_and_compare(sc, idx_want, entry, what, did_want=True, u=0.37, hidden=()):
    """One resample of the scene's engine through `entry`, everything compared with the model; returns the model's state."""
    e, P = sc.e, sc.e.P
    idx_want = np.asarray(idx_want, dtype=np.int64)
    c0 = e.counters()
    if entry == "weights":
        did, idx = e.resample(u)
        assert did == did_want, what
        assert np.array_equal(idx, idx_want), (what, np.nonzero(idx != idx_want)[0][:8])
    else:
        apply_sources(e, idx_want)
    c1 = e.counters()
    m = R.move(sc.poses, sc.covs, sc.weights, sc.maps, idx_want, did_want)
    assert np.array_equal(bits(e.poses()), bits(m.poses)), what
    assert np.array_equal(bits(e.covs()), bits(m.covs)), what
    assert np.array_equal(bits(e.weights()), bits(m.weights)), what
    assert c1["tiles_in_use"] == m.tiles_in_use, (what, c1["tiles_in_use"], m.tiles_in_use)
    assert c1["resample_copies"] - c0["resample_copies"] == m.copies, (what, c1["resample_copies"] - c0["resample_copies"], m.copies)
    if not did_want:
        assert steady(c1) == steady(c0), what
    for j in range(P):
        assert tile_count(e, j) == len(m.maps[j]), (what, j)
        assert e.map_extent(j) == sc.extent[idx_want[j]], (what, j, e.map_extent(j), sc.extent[idx_want[j]])
    dests = R.copy_destinations(idx_want)
    compared = compared_particles(P, idx_want, sc.maps, m.maps)
    assert set(dests) <= set(compared)
    for j in compared:
        same_tiles(e, j, m.maps[j], what)
    for j in hidden:
        near = NEAR if j in dests else None              # a destination's slot was some dead particle's: look where those wrote
        check_hidden(e, j, m.maps[j], sc.extent[idx_want[j]], what, also=near)
    print(f"{what}: {len(dests)} jobs, {m.copies} tile copies, {len(compared)} particles read back, {len(hidden)} looked through")
    return m


def moved_scene(sc, m, idx):
    """The scene after a resample, as the model has it: the state before the next one."""
    sc.poses, sc.covs, sc.weights, sc.maps = m.poses, m.covs, m.weights, m.maps
    sc.extent = [sc.extent[i] for i in idx]
    return sc


def some_hidden(idx, n_dest=6, n_other=3):
    dests = R.copy_destinations(idx)
    others = [j for j in range(len(idx)) if j not in set(dests)]
    return dests[:n_dest] + others[::max(1, len(others) // n_other)][:n_other]


@pytest.mark.parametrize("entry", ["weights", "sources"])
@pytest.mark.parametrize("P", [1024, 1025, 4096, 4097])
def test_every_launch_shape_moves_what_the_model_moves(P, entry):
    cnt = pattern(P, 40, 12, seed=P + (entry == "sources"))
    idx = np.repeat(np.arange(P), cnt)
    if entry == "weights":
        did, ref = orc.resample_indices(weights_of(cnt), 0.37)
        assert did and np.array_equal(ref, idx)
    sc = Scene(P, weights=weights_of(cnt) if entry == "weights" else None)
    sc.check_is_varied()
    dests = R.copy_destinations(idx)
    x = extras(P)
    assert len(dests) == 64
    assert (idx == x[0]).sum() == 2 and (idx == x[1]).sum() == 0 and (idx == x[2]).sum() == 3 and (idx == x[3]).sum() == 1
    hidden = dests if (P, entry) == (1025, "weights") else some_hidden(idx)            # every destination of one run
    far_gain = [j for j in dests if idx[j] in x]         # destinations that gain the far tile (allocation)
    hidden = sorted(set(hidden) | set(far_gain[:1]))
    resample_and_compare(sc, idx, entry, f"P {P} from {entry}", hidden=hidden)
    sc.e.close()


@pytest.mark.parametrize("entry", ["weights", "sources"])
def test_more_jobs_than_workgroups_go_through_the_queue(entry):
    P = 1100
    cnt = pattern(P, 100, 250, seed=7 + (entry == "sources"))
    if entry == "weights":
        did, idx = orc.resample_indices(weights_of(cnt), 0.37)
        assert did
        idx = np.asarray(idx)
    else:
        idx = np.repeat(np.arange(P), cnt)
    mult = np.bincount(idx, minlength=P)
    assert len(R.copy_destinations(idx)) >= 513 and mult.max() >= 3 and (mult == 1).any() and np.all(np.diff(idx) >= 0)
    sc = Scene(P, weights=weights_of(cnt) if entry == "weights" else None)
    resample_and_compare(sc, idx, entry, f"queue from {entry}", hidden=some_hidden(idx)[:4] + R.copy_destinations(idx)[-2:])
    sc.e.close()


@pytest.mark.parametrize("n_jobs", [0, 1])
def test_no_job_and_one_job_still_permute_the_state(n_jobs):
    P = 1025                                             # the state permutation rides at the head of the copy kernel
    sc = Scene(P)
    idx = np.arange(P)
    if n_jobs:
        idx[500] = 499
    assert len(R.copy_destinations(idx)) == n_jobs and not np.any(sc.weights == 1.0)
    m = resample_and_compare(sc, idx, "sources", f"{n_jobs} jobs", hidden=[499, 500, 501])
    assert np.all(m.weights == 1.0)
    sc.e.close()


@pytest.mark.parametrize("P", [1025, 4097])
def test_without_the_trigger_nothing_changes(P):
    w = np.random.default_rng(P).uniform(0.0, 200.0, size=P)
    w[3], w[P - 2] = 0.0, 200.0                          # spread exactly 200: main.py:50 asks for more
    did, idx = orc.resample_indices(w, 0.37)
    assert not did and idx == list(range(P))
    sc = Scene(P, weights=w)
    m = resample_and_compare(sc, idx, "weights", f"no trigger at {P}", did_want=False, hidden=[0, 5, P - 1])
    assert np.array_equal(bits(m.weights), bits(w)) and np.array_equal(bits(m.poses), bits(sc.poses))
    sc.e.close()


def test_two_resamples_in_a_row_then_a_map_update():
    P = 1025
    cnt1, cnt2 = pattern(P, 40, 12, seed=21), pattern(P, 30, 20, seed=22)
    did, idx1 = orc.resample_indices(weights_of(cnt1), 0.61)
    assert did
    idx1, idx2 = np.asarray(idx1), np.repeat(np.arange(P), cnt2)
    sc = Scene(P, weights=weights_of(cnt1))
    m1 = resample_and_compare(sc, idx1, "weights", "first of two", u=0.61)
    sc = moved_scene(sc, m1, idx1)
    m2 = resample_and_compare(sc, idx2, "sources", "second of two", hidden=some_hidden(idx2))
    # a map update lands in the map the model says each particle has: 64 of them against a fresh engine that was given the
    # modelled maps (a particle's update depends on its pose and its map alone)
    e = sc.e
    dests = R.copy_destinations(idx2)
    chosen = sorted(dests[:32] + [j for j in range(0, P, 16) if j not in dests[:32]][:32])
    assert len(chosen) == 64
    rng = np.random.default_rng(3)
    poses = scene_poses(P, rng)
    ranges, angles = np.array([3.0, 2.2, 3.7, 1.9, 2.8, 3.4, 2.0, 3.1]), np.arange(8) * (np.pi / 4) - 0.3
    fresh = make_engine(64, pool=64 * 10)
    for k, j in enumerate(chosen):
        for c, cells in m2.maps[j].items():
            fresh.set_tile(k, c, cells)
    for eng, ps in ((e, poses), (fresh, poses[chosen])):
        eng.set_scan(ranges, angles)
        eng.map_update(ps)
    changed = 0
    for k, j in enumerate(chosen):
        want = dict(fresh.tiles(k))
        same_tiles(e, j, want, f"map update after two resamples, new particle {j}")
        changed += any(c not in m2.maps[j] or not np.array_equal(want[c], m2.maps[j][c]) for c in want)
    assert changed == 64
    fresh.close()
    e.close()


# ---- 2. directed box and occupancy-word geometry -----------------------------------------------------------------------------
GEOMETRY = [(cs, name) for cs in (0.1, 0.05) for name in geometry_cases(400)] + [(0.025, "corner_of_the_tile")]


@pytest.mark.parametrize("cs,name", GEOMETRY)
def test_union_of_the_written_boxes_cell_groups_and_occupancy_words(cs, name):
    dim = int(round(TILE / cs))
    src, dst = geometry_cases(dim)[name]
    ld = Loaded(cs, {ANC: src, DEAD: dst}, pool=48)
    assert ld.dim == dim and ld.e.counters()["tiles_in_use"] == 16 + len(set(src) - {HOME}) + len(set(dst) - {HOME})
    m, nbytes = ld.copy_anc_over_dead(f"{name} at {cs}")
    print(f"{name} at {cs}: {m.copies} tile copies, {nbytes} bytes")
    if name == "two_allocated_two_released":
        assert set(m.maps[ANC + 1]) == {HOME, (40.0, -40.0), (40.0, 0.0)} and m.tiles_in_use == 16 + 2 + 2
    ld.e.close()


def test_an_ancestor_that_holds_the_whole_lattice():
    centres = [(40.0 * a, 40.0 * b) for a in range(-3, 4) for b in range(-3, 4)]
    src = {c: (7 * k, 7 * k + 2 + k % 3, 390 - 8 * k, 399 - 8 * k + k % 5) for k, c in enumerate(centres)}
    dst = {HOME: (300, 320, 0, 50), (80.0, 80.0): (0, 10, 0, 10)}
    ld = Loaded(0.1, {ANC: src, DEAD: dst}, pool=16 + 48 + 1 + 47 + 2)
    assert len(ld.maps[ANC]) == 49 and ld.e.counters()["tiles_in_use"] == 16 + 48 + 1
    m, nbytes = ld.copy_anc_over_dead("whole lattice")
    assert m.copies == 49 and m.tiles_in_use == 16 + 2 * 48
    ld.e.close()


# ---- 3. the free stack and its exhaustion ------------------------------------------------------------------------------------
def test_the_free_stack_after_tiles_were_allocated_and_released():
    from thesis_amd.engine import RbpfError
    from thesis_amd._lib import RBPF_ENOMEM
    pool = 40
    src = {(40.0, -40.0): (3, 9, 380, 399), (40.0, 0.0): (390, 399, 0, 17)}
    dst = {(-40.0, 0.0): (0, 40, 31, 32), (-40.0, 40.0): (7, 7, 64, 95), (0.0, 40.0): (100, 140, 100, 140), HOME: (1, 2, 3, 4)}
    ld = Loaded(0.1, {ANC: src, DEAD: dst}, pool=pool)
    e = ld.e
    assert e.counters()["tiles_in_use"] == 21
    m, _ = ld.copy_anc_over_dead("before the pool is filled")                          # two tiles allocated, three released
    assert m.tiles_in_use == 20
    made = fill_the_pool(ld, pool - 20)
    assert e.counters()["tiles_in_use"] == pool
    with pytest.raises(RbpfError) as err:                                              # exactly the free tiles can be had, no more
        load_one_cell(ld, 0, free_positions(ld.maps[0])[-1], 1, 1)
    assert err.value.code == RBPF_ENOMEM                 # (refused before anything was written: the model did not change)
    # every tile handed out is zero but for its cell - the released ones (the first to be handed out again) were wiped in cells and
    # occupancy words - and no tile was handed out twice: every earlier map still reads as before
    inv = ld.dim / TILE
    for p in range(16):
        same_tiles(e, p, ld.maps[p], "after the pool was filled")
    for p, c, x, y in made:
        ox, oy = R.tile_origin(c, ld.dim, TILE)
        box = (ox, ox + ld.dim, oy, oy + ld.dim)
        clear = T.clearance(R.mosaic(ld.maps[p], T.grown_box(box, CLEAR_MAX), ld.dim, TILE), CLEAR_MAX,
                            float(e.cfg.quantum), float(e.cfg.occupied_threshold))
        assert (clear == 0).sum() == 1 and clear[x, y] == 0
        tr = e.travel_cost([[(box[1] + 2) / inv, (box[3] + 2) / inv]], particle=p, box=box, clear_max=CLEAR_MAX, through_unknown=True)
        assert np.array_equal(tr.clearance, clear), (p, c, np.argwhere(tr.clearance != clear)[:4])
    assert e.counters()["tiles_in_use"] == pool
    e.close()


def full_pool_scene(free, release):
    """A pool with `free` free tiles in which copying ANC over DEAD allocates one tile; with `release` DEAD also holds a tile
    that ANC does not, which the copy gives up."""
    src, dst = {(40.0, 0.0): (5, 9, 5, 9)}, ({(-40.0, 0.0): (7, 8, 7, 8)} if release else {})
    used = 16 + 1 + len(dst)
    ld = Loaded(0.1, {ANC: src, DEAD: dst}, pool=used + 3 + free)
    fill_the_pool(ld, 3)
    assert ld.e.counters()["tiles_in_use"] == used + 3 == int(ld.e.cfg.pool_tiles) - free
    return ld


@pytest.mark.parametrize("release", [False, True])
def test_a_resample_needs_as_many_free_tiles_as_it_allocates(release):
    """Exhaustion is an error code at the next checked call, never silent - also when the same job releases a tile: released
    tiles return to the stack only after the copies, so the net number of tiles does not count."""
    from thesis_amd.engine import RbpfError
    from thesis_amd._lib import RBPF_ENOMEM
    idx = np.array(sorted([p for p in range(16) if p != DEAD] + [ANC]))
    ld = full_pool_scene(0, release)
    queue_sources(ld.e, idx)
    with pytest.raises(RbpfError) as err:
        ld.e.synchronize()
    assert err.value.code == RBPF_ENOMEM
    ld.e.close()                                         # the maps are incomplete: nothing more is asked of this engine
    ld = full_pool_scene(1, release)                     # one free tile is enough, and then everything is as modelled
    m, _ = ld.copy_anc_over_dead(f"one free tile, release {release}")
    assert ld.e.counters()["tiles_in_use"] == int(ld.e.cfg.pool_tiles) - (1 if release else 0)
    ld.e.close()
