"""tests/frontier_oracle.py against cases drawn by hand and against the host path it restates: explore.frontier_cells and the
cells explore.candidate_poses keeps before it thins them (no GPU)."""
import numpy as np

from tests import frontier_oracle as F
from tests.test_explore import half_known_room
from thesis_amd import explore
from thesis_amd.mapio import MapRaster

Q, THR = 0.1, 1.0
FREE, WALL = -30, 30


def run(cells, clear=0, min_size=1, max_regions=8, outside=0, box=None):
    """The oracle on an [8, 8] box at (x0, y0) = (10, -20) whose surroundings hold `outside`."""
    m = F.margin(clear)
    grown = np.pad(np.asarray(cells, np.int8), m, constant_values=outside)
    box = box or (10, 10 + len(cells), -20, -20 + len(cells[0]))
    return F.regions(grown, box, clear, min_size, max_regions, Q, THR)


def drawn(rows):
    """'.' unknown, 'o' free, '#' occupied, '+' known and weakly occupied (5)."""
    return np.array([[{".": 0, "o": FREE, "#": WALL, "+": 5}[ch] for ch in r] for r in rows], np.int8)


def test_a_square_a_diagonal_pair_and_two_single_cells():
    c = drawn(["........",
               ".o......",
               "..o.....",
               "........",
               "....oo..",
               ".o.ooo..",
               "........",
               ".......o"])
    label, table, counts = run(c)
    want = np.full((8, 8), -1, np.int32)
    want[1, 1] = want[2, 2] = 9                            # diagonal neighbours are one region
    want[4, 4] = want[4, 5] = want[5, 3] = want[5, 4] = want[5, 5] = 36
    want[5, 1] = 41                                        # two cells apart from (5, 3): its own region
    want[7, 7] = 63
    assert np.array_equal(label, want) and counts.tolist() == [9, 4, 4]
    # size 5: sums 23 / 21, centroid (5, 4) rounded half up from (4.6, 4.2): a member
    assert table[0].tolist() == [36, 5, 23, 21, 14, 15, -17, -15, 15, -16]
    # size 2: centroid (1.5, 1.5) -> (2, 2)
    assert table[1].tolist() == [9, 2, 3, 3, 11, 12, -19, -18, 12, -18]
    assert table[2].tolist() == [41, 1, 5, 1, 15, 15, -19, -19, 15, -19] and table[3, 0] == 63      # equal sizes: the smaller label first
    assert np.all(table[4:] == -1)
    label2, table2, counts2 = run(c, min_size=2, max_regions=1)
    assert np.array_equal(label2, want) and counts2.tolist() == [9, 4, 1] and np.array_equal(table2[0], table[0])
    assert run(c, min_size=6)[2].tolist() == [9, 4, 0] and np.all(run(c, min_size=6)[1] == -1)


def test_a_ring_whose_centroid_is_no_member():
    c = drawn(["........",
               "..ooo...",
               "..o.o...",
               "..ooo...",
               "........",
               "........",
               "........",
               "........"])
    label, table, counts = run(c)
    assert counts.tolist() == [8, 1, 1] and (label == 10).sum() == 8 and label[2, 3] == -1
    # centroid (2, 3) is the hole: four members at distance 1, the smallest L wins: (1, 3)
    assert table[0].tolist() == [10, 8, 16, 24, 11, 13, -18, -16, 11, -17]


def test_known_neighbours_the_box_edge_and_the_clearance():
    c = drawn(["oooooooo",
               "oooooooo",
               "oo+ooooo",
               "oooooooo",
               "oooooooo",
               "oooooooo",
               "oooooooo",
               "oooooooo"])
    assert run(c, outside=FREE)[2].tolist() == [0, 0, 0]                   # everything known: no frontier, "+" is known too
    label, _, counts = run(c, outside=0)                                  # unknown outside the box: the rim, one region
    assert counts.tolist() == [28, 1, 1] and np.all(label[1:7, 1:7] == -1) and np.all(label[0] == 0)
    c[4, 4] = 0                                                            # a hole of unknown: its four 4-neighbours
    label, _, counts = run(c, outside=FREE)
    assert counts.tolist() == [4, 1, 1] and sorted(np.argwhere(label >= 0).tolist()) == [[3, 4], [4, 3], [4, 5], [5, 4]]
    assert np.all(label[label >= 0] == 3 * 8 + 4)                          # joined through their diagonals
    for clear, d, gone in ((0, 1, False), (1, 1, True), (1, 2, False), (2, 2, True), (2, 3, False)):
        k = c.copy()
        k[3 - d, 4 + d] = 11                                               # just over the threshold, at Chebyshev distance d of (3, 4)
        label = run(k, clear=clear, outside=FREE)[0]
        assert (label[3, 4] == -1) == gone, (clear, d)
        k[3 - d, 4 + d] = 10                                               # exactly the threshold: not occupied
        assert run(k, clear=clear, outside=FREE)[0][3, 4] >= 0
    # an occupied cell outside the box counts
    grown = np.pad(c, 2, constant_values=FREE)
    assert F.regions(grown, (0, 8, 0, 8), 2, 1, 4, Q, THR)[2][0] == 4
    grown[0, 6] = WALL                                                     # (-2, 4): distance 5 of (3, 4)
    assert F.regions(grown, (0, 8, 0, 8), 2, 1, 4, Q, THR)[2][0] == 4
    box = (3, 8, 0, 8)                                                     # the box cut so that (3, 4) is its first row: (1, 4) is two rows outside
    g2 = np.pad(c, 2, constant_values=FREE)[3:]
    g2[0, 6] = WALL
    label = F.regions(g2, box, 2, 1, 4, Q, THR)[0]
    assert label[0, 4] == -1 and (label >= 0).sum() == 3


def kept_by_candidate_poses(raster, clear):
    """The cells candidate_poses keeps before it thins them: with one-cell squares nothing is thinned."""
    cell = float(raster.tile_len) / int(raster.dim)
    poses = explore.candidate_poses(raster, spacing_m=cell, n_headings=1, clearance_cells=clear, occupied_threshold=THR)
    return np.round(poses[:, :2] / cell - 0.5).astype(np.int64)


def check_against_explore(raster):
    c = np.asarray(raster.cells)
    box = (raster.x0, raster.x0 + c.shape[0], raster.y0, raster.y0 + c.shape[1])
    origin = np.array([box[0], box[2]])
    label, _, counts = F.regions(np.pad(c, 1), box, 0, 1, 4, float(raster.quantum), THR)
    free_occ = c.astype(np.float64) * float(raster.quantum) > THR         # with clear 0 an occupied cell is never v < 0
    assert not (free_occ & (c < 0)).any()
    assert np.array_equal(np.argwhere(label >= 0) + origin, explore.frontier_cells(raster)) and counts[0] == (label >= 0).sum()
    for clear in (1, 4):
        label = F.regions(np.pad(c, clear), box, clear, 1, 4, float(raster.quantum), THR)[0]
        assert np.array_equal(np.argwhere(label >= 0) + origin, kept_by_candidate_poses(raster, clear)), clear


def test_the_mask_is_that_of_the_host_path():
    check_against_explore(half_known_room())
    rng = np.random.default_rng(3)
    for shape, x0, y0 in (((37, 23), -11, 5), ((16, 70), 100, -300)):
        c = rng.choice(np.array([0, 0, FREE, FREE, FREE, -3, 7, 10, 11, WALL], np.int8), size=shape, p=[.15, .15, .2, .2, .15, .05, .03, .02, .02, .03])
        check_against_explore(MapRaster(x0=x0, y0=y0, cell_size=0.05, quantum=Q, dim=800, tile_len=40.0, cells=c))


def test_labels_are_region_minima_on_a_random_raster():
    rng = np.random.default_rng(7)
    c = np.where(rng.random((40, 33)) < 0.55, FREE, 0).astype(np.int8)
    label, table, counts = run(c, max_regions=1024, box=(0, 40, 0, 33))
    assert counts[1] == counts[2] == len(np.unique(label[label >= 0])) and counts[0] == (label >= 0).sum() == table[:counts[2], 1].sum()
    for row in table[:counts[2]]:
        ij = np.argwhere(label == row[0])
        assert len(ij) == row[1] and (ij[:, 0] * 33 + ij[:, 1]).min() == row[0] and label[row[8], row[9]] == row[0]
        assert [ij[:, 0].sum(), ij[:, 1].sum(), ij[:, 0].min(), ij[:, 0].max(), ij[:, 1].min(), ij[:, 1].max()] == row[2:8].tolist()
    assert np.all(np.diff(table[:counts[2], 1]) <= 0)
