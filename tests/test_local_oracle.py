"""The local map's oracle (tests/local_oracle.py) held to literals worked out by hand, and local.quantise_weights.  Cells of
0.5 m (inv = 2) and poses at quarter metres keep every number exact in binary, so the expected crops follow on paper."""
import math

import numpy as np
import pytest

from tests import local_oracle as lo

F, W = -5, 20                                           # a free cell, the wall


def six():
    """A 6 x 6 map of free cells, mosaic cells 0 .. 5 on both axes, with one wall cell at (4, 2)."""
    cells = np.full((6, 6), F, np.int8)
    cells[4, 2] = W
    return cells


POSE = (1.75, 1.75)                                     # the centre of cell (3, 3)


def both(cells, pose, n, S, offset=(0.0, 0.0)):
    a = lo.crop_scalar(cells, 0, 0, pose, n, S, 0.5, offset, 2.0)
    assert np.array_equal(a, lo.crop(cells, 0, 0, pose, n, S, 0.5, offset, 2.0))
    return a


def test_tables():
    gx, gy = lo.tables(4, 1, 0.5)
    assert gx.tolist() == [-0.75, -0.25, 0.25, 0.75] and gy.tolist() == gx.tolist()
    gx, gy = lo.tables(2, 2, 0.5, (1.0, -0.5))
    assert gx.tolist() == [0.625, 0.875, 1.125, 1.375] and gy.tolist() == [-0.875, -0.625, -0.375, -0.125]
    assert lo.reach(4, 0.5, (0.0, 0.0), 2.0) == math.ceil(math.sqrt(8.0)) + 2 == 5


def test_heading_zero_nearest_and_supersampled():
    # S = 1: the samples stand at x = 1.0, 1.5, 2.0, 2.5, exactly: cells 2 .. 5, so the crop is cells[2:6, 2:6]
    want = np.full((4, 4), F, np.int8)
    want[2, 0] = W
    assert np.array_equal(both(six(), POSE + (0.0,), 4, 1), want)
    # S = 2: samples a quarter cell from the boundaries; output cell i holds the map cells {1,2}, {2,3}, {3,4}, {4,5}.  The wall
    # (4, 2) lies in i = 2, 3 and j = 0, 1: the max keeps it in all four
    want = np.full((4, 4), F, np.int8)
    want[2:4, 0:2] = W
    assert np.array_equal(both(six(), POSE + (0.0,), 4, 2), want)


def test_quarter_turns_turn_the_crop():
    zero = both(six(), POSE + (0.0,), 4, 2)
    # theta = pi / 2: the robot's x is the world's y: crop[i][j] = crop0[3 - j][i]; the wall lands in rows 0, 1, columns 0, 1
    want = np.full((4, 4), F, np.int8)
    want[0:2, 0:2] = W
    got = both(six(), POSE + (math.pi / 2,), 4, 2)
    assert np.array_equal(got, want) and np.array_equal(got, np.rot90(zero, -1))
    # theta = pi: crop[i][j] = crop0[3 - i][3 - j]
    want = np.full((4, 4), F, np.int8)
    want[0:2, 2:4] = W
    got = both(six(), POSE + (math.pi,), 4, 2)
    assert np.array_equal(got, want) and np.array_equal(got, zero[::-1, ::-1])


def test_an_offset_of_one_cell_shifts_the_crop_by_one_row():
    zero = both(six(), POSE + (0.0,), 4, 1)
    got = both(six(), POSE + (0.0,), 4, 1, offset=(0.5, 0.0))
    assert np.array_equal(got[:3], zero[1:])
    assert got[3].tolist() == [0, 0, 0, 0]              # map cell X = 6: outside the raster, v = 0


def test_fuse_counts_integer_weights():
    a, b = both(six(), POSE + (0.0,), 4, 2), both(six(), POSE + (math.pi,), 4, 2)
    f = lo.fuse(np.stack([a, b]), [3, 5], 10.0)
    assert f.dtype == np.int64 and f.shape == (4, 4, 4)
    assert f[2, 0].tolist() == [3, 5, 0, 3 * W + 5 * F]          # the wall in the first crop only
    assert f[0, 2].tolist() == [5, 3, 0, 5 * W + 3 * F]
    assert f[0, 0].tolist() == [0, 8, 0, 8 * F]
    unknown = lo.fuse(np.zeros((2, 1, 1), np.int8), None, 10.0)
    assert unknown[0, 0].tolist() == [0, 0, 2, 0]
    assert lo.fuse(np.full((1, 1, 1), 10, np.int8), None, 10.0)[0, 0].tolist() == [0, 0, 0, 10]     # strict: 10 is not above 10


def test_quantise_weights():
    from thesis_amd.local import quantise_weights
    q = quantise_weights([1.0, 1.0, 1.0])
    assert q.dtype == np.uint32 and q.tolist() == [357913941] * 3
    assert quantise_weights([0.0, 2.0]).tolist() == [0, 1 << 30]
    assert quantise_weights([1.0, 3.0], bits=4).tolist() == [4, 12]
    for bad in ([1.0, -1.0], [1.0, math.nan], [1.0, math.inf], [0.0, 0.0], []):
        with pytest.raises(ValueError):
            quantise_weights(bad)
