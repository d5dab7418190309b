"""explore.region_poses, posterior_regions and next_frontier_view over a stub engine whose frontier_regions is the scalar oracle
(no GPU)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import frontier_oracle as F
from thesis_amd import explore

CELL = 0.05                                                # 20 cells per metre: a 1 m square is 20 x 20 cells
FREE = -30


def frontiers(per_particle, K=3):
    """Frontiers of particle=None from [(rep_X, rep_Y, size), ...] per particle, largest first as the table is."""
    P = len(per_particle)
    t = np.full((P, K, 10), -1, np.int64)
    counts = np.zeros((P, 3), np.int32)
    for p, regs in enumerate(per_particle):
        for k, (X, Y, size) in enumerate(sorted(regs, key=lambda r: -r[2])):
            t[p, k] = [k, size, 0, 0, X, X, Y, Y, X, Y]
        counts[p] = [sum(r[2] for r in regs), len(regs), len(regs)]
    return explore.Frontiers(None, t.view(explore.REGION_DTYPE)[..., 0], counts, (-100, 100, -100, 100), CELL)


def test_region_poses():
    fr = frontiers([[(5, -7, 9), (40, 2, 4)]])
    one = explore.Frontiers(None, fr.regions[0], fr.counts[0], fr.box, CELL)
    poses = explore.region_poses(one, n_headings=4)
    assert poses.shape == (8, 3)
    assert np.array_equal(poses[::4, :2], (np.array([[5, -7], [40, 2]]) + 0.5) * CELL) and np.all(poses[1:4, :2] == poses[0, :2])
    assert np.array_equal(poses[:4, 2], 2 * np.pi * np.arange(4) / 4) and np.array_equal(poses[4:, 2], poses[:4, 2])
    assert np.array_equal(np.floor(poses[:, :2] / CELL).astype(int)[::4], [[5, -7], [40, 2]])
    empty = explore.Frontiers(None, fr.regions[0], np.array([0, 0, 0], np.int32), fr.box, CELL)
    assert explore.region_poses(empty).shape == (0, 3)
    with pytest.raises(ValueError):
        explore.region_poses(fr)
    assert explore.REGION_FIELDS == F.FIELDS


def test_posterior_regions_support_ties_minorities_and_the_cap():
    # square (0, 0): particles 0 and 1 (particle 0 twice: it counts once); square (2, 0): particles 2 and 3;
    # square (0, 2): particles 0, 1, 2; square (-1, -1): particle 3 alone
    fr = frontiers([[(5, 5, 7), (9, 9, 3), (5, 45, 2)],
                    [(6, 5, 8), (5, 45, 6)],
                    [(45, 5, 4), (6, 44, 5)],
                    [(45, 5, 9), (-3, -3, 30)]])
    pr = explore.posterior_regions(fr)
    assert pr.cells.tolist() == [[5, 45], [5, 5], [45, 5], [-3, -3]]      # by support; the tie at 0.5 row-major
    assert pr.support.tolist() == [0.75, 0.5, 0.5, 0.25] and pr.size.tolist() == [6, 8, 9, 30]
    # the cell of a square: the rep with the largest weight sum, ties to the smaller (X, Y)
    assert explore.posterior_regions(fr, weights=[1.0, 2.0, 1.0, 1.0]).cells.tolist()[:2] == [[5, 45], [6, 5]]
    heavy = explore.posterior_regions(fr, weights=[1.0, 1.0, 1.0, 5.0])
    assert heavy.cells.tolist() == [[45, 5], [-3, -3], [5, 45], [5, 5]] and heavy.support.tolist() == [0.75, 0.625, 0.375, 0.25]
    assert explore.posterior_regions(fr, min_support=0.3).cells.tolist() == [[5, 45], [5, 5], [45, 5]]      # the minority's square goes
    assert explore.posterior_regions(fr, min_support=0.5, max_candidates=2).cells.tolist() == [[5, 45], [5, 5]]
    assert explore.posterior_regions(fr, spacing_m=10.0).support.tolist() == [1.0, 0.25]                  # one square holds all but (-3, -3)
    assert explore.posterior_regions(fr, spacing_m=10.0).cells.tolist() == [[5, 45], [-3, -3]]           # (5, 45) and (45, 5) have two particles each
    none = explore.posterior_regions(frontiers([[], []]))
    assert none.cells.shape == (0, 2) and none.support.shape == (0,)
    with pytest.raises(ValueError):
        explore.posterior_regions(fr, weights=[1.0, 2.0])


class StubEngine:
    """weights / frontier_regions / view_gain of an engine that holds the given rasters, all over one box."""
    def __init__(self, maps, weights, gain_of):
        self.maps, self.w, self.gain_of = maps, np.asarray(weights, float), gain_of
        self.P = len(maps)
        self.box = (-30, 30, 0, 60)
        self.asked = []

    def weights(self):
        return self.w

    def frontier_regions(self, particle="best", box=None, clearance_cells=4, min_size=1, max_regions=64, labels=True):
        self.asked.append(particle)
        out = [F.regions(np.pad(m, F.margin(clearance_cells)), self.box, clearance_cells, min_size, max_regions, 0.1, 1.0)
               for m in (self.maps if particle is None else [self.maps[particle]])]
        t, c = np.stack([o[1] for o in out]), np.stack([o[2] for o in out])
        if particle is not None:
            t, c = t[0], c[0]
        return explore.Frontiers(out[0][0] if labels and particle is not None else None, t.view(explore.REGION_DTYPE)[..., 0], c, self.box, CELL)

    def view_gain(self, cand, angles, particle="best", max_range=None, table=None):
        g = np.array([[self.gain_of(p, c) for c in cand] for p in range(self.P)], np.int64)
        return SimpleNamespace(gain=g if particle is None else g[particle])


def test_next_frontier_view_proposes_what_the_best_map_lacks_only_over_the_posterior():
    near = np.zeros((60, 60), np.int8)
    near[10:20, 10:50] = FREE                             # a known strip in unknown surroundings: its rim is one region
    both = near.copy()
    both[40:50, 10:50] = FREE                             # a second strip that the best particle's map lacks
    crack = near.copy()
    crack[30, 30] = FREE                                  # one cell: below min_size
    gain_of = lambda p, c: int(65536 * (3 + (c[0] > 0.5) + (c[2] == 0.0)))   # the far strip shows more; heading 0 a little more
    e = StubEngine([near, both, both, crack], [5.0, 1.0, 1.0, 1.0], gain_of)
    best = explore.next_frontier_view(e, None, particle="best", k=4, n_headings=2)
    assert e.asked == [0] and best.gain.shape == (2,) and len(best.poses) == 2 and np.all(best.support == 1.0)
    assert np.all(best.poses[:, 0] < 0.0) and best.size.tolist() == [96, 96]            # the rim of a 10 x 40 strip
    assert best.scores.tolist() == [4.0, 3.0] and best.poses[0, 2] == 0.0
    assert explore.next_frontier_view(e, None, particle=1, k=8, n_headings=2).gain.shape == (4,)
    post = explore.next_frontier_view(e, None, particle=None, k=4, n_headings=2)      # uniform weights
    assert e.asked[-1] is None and post.gain.shape == (4, 4) and post.candidates.shape == (4, 3)
    far = post.poses[:, 0] > 0.5
    assert far.tolist() == [True, False, True, False] and post.scores.tolist() == [5.0, 4.0, 4.0, 3.0]    # the tie at 4: the lower index
    assert post.support.tolist() == [0.5, 1.0, 0.5, 1.0] and post.size.tolist() == [96, 96, 96, 96]
    cells = np.floor(post.poses[:, :2] / CELL).astype(int)
    assert np.all((cells[far, 0] >= 10) & (cells[far, 0] < 20)) and np.all((cells[~far, 0] >= -20) & (cells[~far, 0] < -10))
    assert not any((np.floor(c[:2] / CELL).astype(int) == [0, 30]).all() for c in post.candidates)        # the crack is no candidate
    weighted = explore.next_frontier_view(e, None, particle=None, weights=e.weights(), k=4, n_headings=2, min_support=0.3)
    assert np.all(weighted.poses[:, 0] < 0.5) and weighted.support.tolist() == [1.0, 1.0]   # 2 / 8 of the weight see the far strip
    small = explore.next_frontier_view(e, None, particle=3, k=8, n_headings=1, min_size=1)
    assert small.size.tolist() == [96, 1]
    with pytest.raises(ValueError):
        explore.next_frontier_view(e, None, particle=3, min_size=97)
    with pytest.raises(ValueError):
        explore.next_frontier_view(e, None, particle="worst")
