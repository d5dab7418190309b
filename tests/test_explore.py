"""thesis_amd/explore.py on the host: the entropy table, frontier cells and candidate poses of a half-known room."""
from types import SimpleNamespace

import numpy as np

from thesis_amd import explore
from thesis_amd.mapio import MapRaster

CFG = SimpleNamespace(quantum=0.1, min_odds_emp=-3.0, max_odds_occ=3.0)


def half_known_room():
    """A 6 m x 4 m room at 0.05 m, walls 2 cells thick; the left half observed (free -30, walls 30), the right half 0."""
    c = np.full((120, 80), -30, np.int8)
    c[:2] = c[-2:] = 30
    c[:, :2] = c[:, -2:] = 30
    c[60:] = 0
    return MapRaster(x0=-60, y0=-40, cell_size=0.05, quantum=0.1, dim=800, tile_len=40.0, cells=c)


def test_entropy_table():
    t = explore.entropy_table(CFG)
    assert t.dtype == np.int32 and t.shape == (61,)
    assert t[30] == 65536 and np.array_equal(t, t[::-1])                 # 1 bit at v = 0; symmetric in v
    assert np.all(np.diff(t[30:]) < 0) and t.min() > 0                   # strictly falling with |v|
    p = 1.0 / (1.0 + np.exp(-3.0))
    assert abs(t[60] / 65536 - -(p * np.log2(p) + (1 - p) * np.log2(1 - p))) < 1e-5


def test_frontier_cells_of_a_half_known_room():
    m = half_known_room()
    f = explore.frontier_cells(m)
    want = np.array([[-1, Y] for Y in range(-38, 38)])                   # the free column next to the unknown half
    assert np.array_equal(f, want)
    # a raster's edge borders cells that are 0: free cells there are frontier too
    tiny = MapRaster(x0=3, y0=4, cell_size=0.05, quantum=0.1, dim=800, tile_len=40.0, cells=np.full((3, 3), -5, np.int8))
    assert len(explore.frontier_cells(tiny)) == 8 and [4, 5] not in explore.frontier_cells(tiny).tolist()


def test_candidate_poses_of_a_half_known_room():
    m = half_known_room()
    c = explore.candidate_poses(m, spacing_m=1.0, n_headings=4, clearance_cells=6)
    assert c.shape[1] == 3 and len(c) % 4 == 0
    xy = c[::4, :2]
    assert np.array_equal(c[:4, 2], 2 * np.pi * np.arange(4) / 4) and np.all(c[1::4, :2] == xy)
    cells = np.floor(xy / 0.05).astype(int)
    assert np.all(cells[:, 0] == -1)                                      # on the frontier column
    assert np.all(np.abs(cells[:, 1] + 0.5) <= 40 - 2 - 6 - 0.5)          # 6 cells clear of the walls
    sq = np.floor(xy / 1.0).astype(int)
    assert len(np.unique(sq, axis=0)) == len(sq) == 4                     # one per 1 m square: y in -2 .. 2 m
    assert len(explore.candidate_poses(m, spacing_m=1.0, n_headings=1, clearance_cells=40)) == 0


def test_rank_takes_the_weighted_mean_and_breaks_ties_low():
    g = np.array([[65536, 0, 65536 * 3], [65536, 65536 * 4, 65536]])
    order, scores = explore.rank(g, k=2)
    assert order.tolist() == [1, 2] and scores.tolist() == [1.0, 2.0, 2.0]
    order, _ = explore.rank(g, weights=[3.0, 1.0], k=3)
    assert order.tolist() == [2, 0, 1]
    assert explore.rank(g[0], k=3)[0].tolist() == [2, 0, 1]
