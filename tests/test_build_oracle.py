"""The map-building oracle (tests/build_oracle.py) on cases small enough to work out by hand, and round the scan
casting oracle: ranges cast in a walled raster, rebuilt at the same cell size from the same poses."""
import math

import numpy as np

from tests.build_oracle import build_map, scan_sets, walk, walk_dir
from tests.cast_oracle import cast

INF, NAN = math.inf, math.nan


def counts(poses, ranges, angles, box, inv=1.0, min_range=0.0, max_range=8.0):
    h, s, _ = build_map(poses, ranges, angles, inv, box, min_range, max_range)
    return h, s


def cells_of(raster, box):
    """{(X, Y): count} of the non-zero cells."""
    return {(int(i) + box[0], int(j) + box[2]): int(raster[i, j]) for i, j in np.argwhere(raster)}


# ---- one beam ---------------------------------------------------------------------------------------------------------------
def test_a_beam_that_ends_exactly_on_a_cell_edge_has_entered_the_next_cell():
    pose = (0.5, 0.5, 0.0)                               # a cell centre; the beam runs along +x: crossings at 0.5, 1.5, 2.5
    assert walk(pose, 0.0, 1.0, 2.5) == [(0, 0), (1, 0), (2, 0), (3, 0)]          # tk == tend counts as entered
    assert walk(pose, 0.0, 1.0, math.nextafter(2.5, 0.0)) == [(0, 0), (1, 0), (2, 0)]
    box = (-2, 6, -2, 3)
    h, s = counts([pose], [[2.5]], [0.0], box)
    assert cells_of(h, box) == {(3, 0): 1} and cells_of(s, box) == {(0, 0): 1, (1, 0): 1, (2, 0): 1, (3, 0): 1}


def test_range_zero_hits_the_origin_cell():
    box = (-1, 2, -1, 2)
    h, s = counts([(0.5, 0.5, 0.3)], [[0.0]], [1.1], box)
    assert cells_of(h, box) == {(0, 0): 1} and cells_of(s, box) == {(0, 0): 1}


def test_a_tie_steps_in_y():
    d = 0.7071067811865476                               # from a cell corner along the diagonal: both crossings at the same parameter
    assert walk_dir(1.0, 1.0, d, d, 3.0) == [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3)]
    assert walk_dir(1.0, 1.0, -d, -d, 1.5) == [(1, 1), (1, 0), (0, 0), (0, -1), (-1, -1)]   # 0 steps to the crossing: fx = fy = 0
    assert walk_dir(1.0, 1.0, d, -d, 1.5) == [(1, 1), (1, 0), (1, -1), (2, -1)]


def test_a_beam_along_an_axis_never_crosses_the_other_one():
    assert walk_dir(0.5, 0.5, 0.0, 1.0, 2.0) == [(0, 0), (0, 1), (0, 2)]           # dx == 0
    assert walk_dir(0.5, 0.5, 0.0, -1.0, 0.5) == [(0, 0), (0, -1)]
    assert walk((0.5, 0.5, 0.0), 0.0, 1.0, 1.5) == [(0, 0), (1, 0), (2, 0)]        # dy == 0 from host cos / sin


def test_negative_coordinates_floor():
    pose = (-0.25, -0.25, 0.0)                           # cell (-1, -1), not (0, 0)
    assert walk(pose, math.pi, 1.0, 1.0) == [(-1, -1), (-2, -1)]                     # along -x: crossings at 0.75, 1.75
    box = (-4, 1, -3, 1)
    h, s = counts([pose], [[1.0]], [math.pi], box)
    assert cells_of(h, box) == {(-2, -1): 1} and cells_of(s, box) == {(-1, -1): 1, (-2, -1): 1}
    h, s = counts([pose], [[1.0]], [math.pi], (0, 3, 0, 3))                        # a box the ray never enters
    assert not h.any() and not s.any()
    h, s = counts([pose], [[1.0]], [math.pi], (-2, 0, -1, 0))                      # the walk is not clipped: it starts outside this box
    assert cells_of(h, (-2, 0, -1, 0)) == {(-2, -1): 1} and cells_of(s, (-2, 0, -1, 0)) == {(-1, -1): 1, (-2, -1): 1}


def test_skipped_and_free_beams():
    pose, box = (0.5, 0.5, 0.0), (-1, 8, -1, 2)
    for r in (NAN, 0.4, -1.0, -INF):                     # NaN and r < min_range: nothing at all
        h, s = counts([pose], [[r]], [0.0], box, min_range=0.5, max_range=3.0)
        assert not h.any() and not s.any(), r
    for r in (INF, 3.0000001, 1e300):                    # beyond max_range: free to max_range = 3 (crossings 0.5, 1.5, 2.5), no hit
        h, s = counts([pose], [[r]], [0.0], box, min_range=0.5, max_range=3.0)
        assert not h.any() and cells_of(s, box) == {(0, 0): 1, (1, 0): 1, (2, 0): 1, (3, 0): 1}, r
    h, s = counts([pose], [[3.0]], [0.0], box, min_range=0.5, max_range=3.0)      # r == max_range returns
    assert cells_of(h, box) == {(3, 0): 1}
    h, s = counts([pose], [[0.5]], [0.0], box, min_range=0.5, max_range=3.0)      # r == min_range is kept
    assert cells_of(h, box) == {(1, 0): 1}


# ---- sets per scan ------------------------------------------------------------------------------------------------------------
def test_counts_are_per_scan():
    pose, box = (0.5, 0.5, 0.0), (-1, 6, -1, 3)
    one = counts([pose], [[2.0]], [0.0], box)
    two_beams = counts([pose], [[2.0, 2.0, 2.2]], [0.0, 0.0, 0.0], box)            # the same cells three times in ONE scan
    assert all(np.array_equal(a, b) for a, b in zip(one, two_beams)) and one[1].max() == 1
    two_scans = counts([pose, pose], [[2.0], [2.0]], [0.0], box)                   # the same cells in TWO scans
    assert np.array_equal(two_scans[0], 2 * one[0]) and np.array_equal(two_scans[1], 2 * one[1])


def test_a_cell_passed_by_one_beam_and_hit_by_another_counts_once_in_each():
    pose, box = (0.5, 0.5, 0.0), (-1, 6, -1, 3)
    h, s = counts([pose], [[1.0, 3.0]], [0.0, 0.0], box)                           # the first beam hits (1, 0), the second passes it
    assert cells_of(h, box) == {(1, 0): 1, (3, 0): 1}
    assert cells_of(s, box) == {(0, 0): 1, (1, 0): 1, (2, 0): 1, (3, 0): 1}
    H, V, steps = scan_sets(pose, [1.0, 3.0], [0.0, 0.0], 1.0, 0.0, 8.0)
    assert H <= V and steps == 2 + 4
    assert np.all(h <= s)


# ---- round the cast -------------------------------------------------------------------------------------------------------------
def test_ranges_cast_in_a_walled_room_rebuild_its_walls():
    """Ranges from the walk of DESIGN 3.7 in a walled raster, rebuilt at the same inv from the same poses.  The end cell of a
    return beam is the cast's hit cell or a 4-neighbour of it on the ray: the range is t / inv and (t / inv) * inv lies within two
    roundings of t, so the end can fall one step short of the hit cell, or one step past it at a tie.  Equality with the hit cell
    is NOT a property."""
    n, x0, inv, q, thr, mr = 120, -60, 20.0, 0.1, 1.0, 15.0
    cells = np.zeros((n, n), np.int8)
    cells[:6, :] = cells[-6:, :] = cells[:, :6] = cells[:, -6:] = 30                # the outer walls
    cells[70:73, 6:80] = 30                                                        # an inner wall
    occupied = lambda X, Y: 0 <= X - x0 < n and 0 <= Y - x0 < n and cells[X - x0, Y - x0] * q > thr
    rng = np.random.Generator(np.random.PCG64(5))
    angles = np.linspace(-0.75 * np.pi, 0.75 * np.pi, 1081)[::7]
    poses = np.stack([rng.uniform(-2.4, 0.4, 40), rng.uniform(-2.4, 2.4, 40), rng.uniform(-np.pi, np.pi, 40)], axis=1)
    tally = {"hit": 0, "before": 0, "after": 0}
    box = (x0, x0 + n, x0, x0 + n)
    all_ranges = []
    for pose in poses:
        assert not occupied(math.floor(pose[0] * inv), math.floor(pose[1] * inv))
        ranges, status, _ = cast(cells, x0, x0, -10000, 10000, inv, q, thr, pose, angles, mr)
        assert np.all(status == 1)                       # the room is closed
        all_ranges.append(ranges)
        for r, a in zip(ranges, angles):
            ray = walk(pose, a, inv, mr * inv)
            k = next(i for i, c in enumerate(ray) if occupied(*c))                 # the cast's hit cell
            end = walk(pose, a, inv, float(r) * inv)[-1]
            where = {ray[k]: "hit", ray[k - 1]: "before"}
            if k + 1 < len(ray):
                where[ray[k + 1]] = "after"
            assert end in where, (pose.tolist(), a, r, end, ray[k])
            assert abs(end[0] - ray[k][0]) + abs(end[1] - ray[k][1]) <= 1
            tally[where[end]] += 1
    print(f"round trip: {tally} of {len(poses) * len(angles)} beams")
    assert tally["hit"] > 10 * (tally["before"] + tally["after"])
    # the rebuilt map: every hit lies on a wall cell or next to one, and the free space inside was seen and never hit
    hits, seen, _ = build_map(poses, np.stack(all_ranges), angles, inv, box, 0.0, mr)
    wall = cells * q > thr
    near = wall.copy()
    near[1:, :] |= wall[:-1, :]; near[:-1, :] |= wall[1:, :]; near[:, 1:] |= wall[:, :-1]; near[:, :-1] |= wall[:, 1:]
    assert np.all(hits <= seen) and seen.max() <= len(poses)
    assert not hits[~near].any() and hits[wall].sum() > 0.8 * hits.sum()
