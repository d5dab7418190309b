"""tests/resample_oracle.py pinned on the CPU: the model of the move against oracle.rbpf_oracle.resample on deep copies of
OracleRobot (main.py:46-79, robot.py:141-149), and its geometry helpers against values worked out by hand."""
import copy

import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests import resample_oracle as R

CELL, TILE = 4.0, 40                                     # 10 x 10 cells per tile: the move does not depend on the size


def population(weights, seed):
    """OracleRobots with distinct poses, covariances and one to three tiles of random cells each."""
    rng = np.random.default_rng(seed)
    centres = [(0, 0), (40, 0), (0, -40), (-40, 40), (80, -80)]
    out = []
    for p, w in enumerate(weights):
        r = orc.OracleRobot(CELL, TILE)
        r.x, r.y, r.theta = [0.0, float(rng.normal())], [0.0, float(rng.normal())], [0.0, float(rng.normal())]
        r.cov = rng.normal(size=(3, 3)).astype(np.longdouble)
        r.weight = [1.0, w]
        r.map.tiles[0].map = rng.integers(-30, 31, size=(10, 10)).astype(np.float64)
        for k in rng.permutation(4)[:(p + seed) % 3]:
            t = orc.OracleTile(*centres[1 + k], TILE, CELL)
            t.map = rng.integers(-30, 31, size=(10, 10)).astype(np.float64)
            r.map.tiles.append(t)
        out.append(r)
    return out


def as_model_input(robots):
    poses = np.array([r.pose() for r in robots], dtype=np.float64)
    covs = np.array([np.asarray(r.cov, dtype=np.float64) for r in robots])
    weights = np.array([r.weight[-1] for r in robots], dtype=np.float64)
    maps = [{(float(t.cx), float(t.cy)): t.map.astype(np.int8) for t in r.map.tiles} for r in robots]
    return poses, covs, weights, maps


CASES = [
    ([10, -250, -100, 300, 5, -np.inf, 0, 42], 0.25),                      # the weights of test_resample_moves_maps_and_state
    ([0.0, 500.0, 1.0, 2.0, 900.0, 3.0, 4.0, 0.5], 0.6),
    ([1.0, 2.0, 3.0, 201.0], 0.0),                                         # spread exactly 200: no trigger
    ([1.0, 2.0, 3.0, 201.5], 0.999),
    ([7.0], 0.5),                                                          # one particle never resamples
    ([-np.inf, 5.0], 0.3),
    ([-np.inf, -np.inf, 1000.0, -np.inf, 1000.0], 0.37),                   # one ancestor three times, the other twice
    ([-300.0, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, -8.0, -9.0, -10.0, -11.0], 0.5),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_model_equals_the_reference_resample_on_deep_copies(case):
    weights, u = CASES[case]
    robots = population(weights, seed=case)
    poses, covs, w, maps = as_model_input(robots)
    did, idx = orc.resample_indices(weights, u)
    assert did == (max(weights) - min(weights) > 200)
    after = orc.resample(copy.deepcopy(robots), u)
    got = R.move(poses, covs, w, maps, idx, did)
    assert len(after) == len(robots) and len({id(r) for r in after}) == len(robots)      # copies are objects of their own
    assert len({id(t) for r in after for t in r.map.tiles}) == sum(len(r.map.tiles) for r in after) == got.tiles_in_use
    want_p, want_c, want_w, want_m = as_model_input(after)
    assert np.array_equal(got.poses, want_p) and np.array_equal(got.covs, want_c) and np.array_equal(got.weights, want_w)
    assert np.all(got.weights == 1.0) if did else np.array_equal(got.weights, w)
    for j in range(len(robots)):
        assert set(got.maps[j]) == set(want_m[j]), j
        for c in want_m[j]:
            assert np.array_equal(got.maps[j][c], want_m[j][c]), (j, c)
    # the reference copies a robot exactly when its ancestor is that of the particle before (main.py:70-74): count them on a
    # population of the very objects
    same = orc.resample(robots, u)
    made = [j for j, r in enumerate(same) if did and r is not robots[idx[j]]]
    assert made == (R.copy_destinations(idx) if did else [])
    assert got.copies == sum(len(same[j].map.tiles) for j in made)


def test_the_model_refuses_what_no_resample_gives():
    poses, covs, w, maps = as_model_input(population([1.0, 2.0, 3.0], 0))
    with pytest.raises(AssertionError):
        R.move(poses, covs, w, maps, [1, 0, 2], True)                      # ancestors are never out of order
    with pytest.raises(AssertionError):
        R.move(poses, covs, w, maps, [0, 1, 3], True)


def test_written_box_extent_and_mosaic():
    dim, tl = 10, 40.0
    a, b = np.zeros((dim, dim), np.int8), np.zeros((dim, dim), np.int8)
    assert R.written_box(a) is None and R.extent({(0.0, 0.0): a}, dim, tl) is None
    a[2, 9] = 5; a[4, 3] = -1
    b[0, 0] = 7
    assert R.written_box(a) == (2, 4, 3, 9)
    assert R.tile_origin((0.0, 0.0), dim, tl) == (-5, -5) and R.tile_origin((-40.0, 80.0), dim, tl) == (-15, 15)
    tiles = {(0.0, 0.0): a, (-40.0, 80.0): b}
    assert R.extent(tiles, dim, tl) == (-15, 0, -2, 16)
    assert R.extent(tiles, dim, tl, boxes={(0.0, 0.0): (0, 9, 0, 9), (-40.0, 80.0): None}) == (-5, 5, -5, 5)
    m = R.mosaic(tiles, (-16, 1, -3, 17), dim, tl)
    assert m.shape == (17, 20) and np.count_nonzero(m) == 3
    assert m[1, 18] == 7 and m[-5 + 2 + 16, -5 + 9 + 3] == 5 and m[-5 + 4 + 16, -5 + 3 + 3] == -1
    assert np.array_equal(R.mosaic(tiles, (-5, 5, -5, 5), dim, tl), a)


def test_copy_bytes_by_hand():
    c, far = (0.0, 0.0), (40.0, 0.0)
    assert R.copy_bytes({c: None}, {c: None}, 400) == 0
    assert R.copy_bytes({c: (5, 5, 0, 0)}, {}, 400) == 2 * 1 * 16
    assert R.copy_bytes({c: (5, 5, 399, 399)}, {c: None}, 400) == 2 * 1 * 16          # columns 384 .. 399: the last group is whole
    assert R.copy_bytes({c: (5, 5, 795, 795)}, {}, 800) == 2 * 1 * 16
    assert R.copy_bytes({c: (50, 52, 15, 16)}, {}, 400) == 2 * 3 * 32                  # across a group border
    assert R.copy_bytes({c: (50, 52, 15, 16)}, {c: (10, 10, 100, 100)}, 400) == 2 * 43 * 112
    assert R.copy_bytes({c: None}, {c: (10, 19, 100, 100)}, 400) == 2 * 10 * 16        # nothing to read, but the old cells are wiped
    assert R.copy_bytes({c: (0, 0, 0, 0)}, {far: (0, 399, 0, 399)}, 400) == 32         # a tile the source lacks is released, not copied
    assert R.copy_bytes({c: (0, 0, 0, 0), far: (1, 2, 16, 47)}, {}, 400) == 32 + 2 * 2 * 32
