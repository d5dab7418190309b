"""thesis_amd/plan.py and explore.next_reachable_view on the host: paths walked down a field of tests/travel_oracle.py, and the
ranking of reachable views on a stub engine."""
from types import SimpleNamespace

import numpy as np

from tests import travel_oracle as T
from tests.test_explore import half_known_room
from thesis_amd import explore, plan

INV, Q, THR = 20.0, 0.1, 1.0


def field(seed=3, shape=(60, 45), inflate=0, clear_max=1):
    rng = np.random.default_rng(seed)
    c = np.full(shape, -30, np.int8)
    c[20, :35] = 30
    c[40, 10:] = 30
    c[rng.random(shape) < 0.06] = 30
    c[2, 2] = -30
    box = (-13, -13 + shape[0], 7, 7 + shape[1])
    m = T.margin(clear_max)
    start = [(-13 + 2.5) / INV, (7 + 2.5) / INV]
    cost, clear, _ = T.travel(np.pad(c, m), box, INV, Q, THR, [start], None, inflate, clear_max)
    return plan.Travel(cost, clear, None, 0, box, 1.0 / INV, INV, inflate, clear_max), c


def test_cost_metres():
    m = plan.cost_metres(np.array([[0, 5, 7], [-1, 12, 100]], np.int32), 0.05)
    assert np.allclose(m[0], [0.0, 0.05, 0.07]) and np.isnan(m[1, 0]) and np.allclose(m[1, 1:], [0.12, 1.0])


def test_paths_are_connected_cost_what_the_field_says_and_cut_no_corner():
    for inflate, clear_max in ((0, 1), (5, 6)):
        tr, cells = field(inflate=inflate, clear_max=clear_max)
        reached = np.argwhere(tr.cost > 0)
        assert len(reached) > 1000 and (tr.cost == -1).sum() > 100
        x0, y0 = tr.box[0], tr.box[2]
        diagonals = 0
        for i, j in reached[::37].tolist() + [reached[np.argmax(tr.cost[tuple(reached.T)])].tolist()]:
            goal = [(x0 + i + 0.25) / INV, (y0 + j + 0.75) / INV]
            p = plan.path_to(tr, goal)
            ij = np.floor(p * INV).astype(int) - [x0, y0]
            assert np.allclose(p * INV - np.floor(p * INV), 0.5)                 # cell centres
            assert ij[-1].tolist() == [i, j] and tr.cost[tuple(ij[0])] == 0 and ij[0].tolist() == [2, 2]
            step = np.abs(np.diff(ij, axis=0))
            assert step.max() == 1 and np.all(step.sum(axis=1) >= 1)            # connected, no pause
            assert int(np.where(step.sum(axis=1) == 2, 7, 5).sum()) == tr.cost[i, j]
            assert np.all(tr.cost[tuple(ij.T)] >= 0) and np.all(np.diff(tr.cost[tuple(ij.T)]) > 0)
            for (a, b), (c, d) in zip(ij[:-1], ij[1:]):
                if a != c and b != d:
                    diagonals += 1
                    assert tr.cost[c, b] >= 0 and tr.cost[a, d] >= 0 and cells[c, b] < 0 and cells[a, d] < 0
            if inflate:
                assert np.all(tr.clearance[tuple(ij[1:].T)] > inflate)
        assert diagonals > 20


def test_no_path_where_the_cost_is_minus_one_or_the_goal_is_outside():
    tr, _ = field()
    i, j = np.argwhere(tr.cost == -1)[5]
    assert plan.path_to(tr, [(tr.box[0] + i + 0.5) / INV, (tr.box[2] + j + 0.5) / INV]) is None
    assert plan.path_to(tr, [100.0, 100.0]) is None
    p = plan.path_to(tr, [(tr.box[0] + 2.5) / INV, (tr.box[2] + 2.5) / INV])     # the start itself
    assert p.shape == (1, 2)


class StubEngine:
    """render_map / weights / view_gain / travel_cost of an engine whose gains and costs are given per candidate xy."""
    def __init__(self, P, gain_of, cost_of):
        self.P, self.gain_of, self.cost_of = P, gain_of, cost_of
        self.cfg = SimpleNamespace(occupied_threshold=1.0)
        self.calls = []

    def weights(self):
        return np.ones(self.P)

    def render_map(self, p):
        return half_known_room()

    def view_gain(self, cand, angles, particle="best", max_range=None, table=None):
        g = np.array([[self.gain_of(p, c) for c in cand] for p in range(self.P)], np.int64)
        return SimpleNamespace(gain=g if particle is None else g[particle])

    def travel_cost(self, starts, goals=None, particle="best", radius_m=0.0, through_unknown=False):
        self.calls.append((np.asarray(starts), particle, radius_m))
        c = np.array([[self.cost_of(p, g) for g in goals] for p in range(self.P)], np.int32)
        return plan.Travel(None, None, c if particle is None else c[particle], 1, (0, 1, 0, 1), 0.05, 20.0, 0, 1)


def test_next_reachable_view_drops_the_unreachable_and_weighs_the_way():
    cand = explore.candidate_poses(half_known_room(), 1.0, 2, 4, 1.0)
    ys = np.unique(cand[:, 1])
    assert len(ys) >= 3
    gain_of = lambda p, c: int(65536 * (10 + 5 * (c[1] == ys[0]) + 3 * (c[1] == ys[1]) + (c[2] == 0.0)))
    # ys[0]: the best gain, but reached in no map; ys[1]: reached in particle 0's map only; the rest: 1 m per |y| away in both
    def cost_of(p, g):
        if g[1] == ys[0] or (g[1] == ys[1] and p == 1):
            return -1
        return int(round(100 * (1 + abs(g[1] - ys[-1]))))
    e = StubEngine(2, gain_of, cost_of)
    r = explore.next_reachable_view(e, None, [0.1, 0.2, 0.3], particle=None, k=4, n_headings=2, radius_m=0.25)
    assert np.array_equal(r.candidates, cand) and r.gain.shape == (2, len(cand)) and r.goal_cost.shape == (2, len(cand))
    assert np.array_equal(r.reach, np.where(cand[:, 1] == ys[0], 0.0, np.where(cand[:, 1] == ys[1], 0.5, 1.0)))
    assert np.all(cand[r.order][:, 1] != ys[0]) and np.all(r.reach[r.order] >= 0.5) and len(r.order) == 4
    assert r.poses[0, 1] == ys[1] and r.poses[0, 2] == 0.0 and r.scores[0] == 14.0      # travel_weight 0: the gain alone
    assert np.array_equal(r.poses, cand[r.order]) and np.all(np.diff(r.scores) <= 0)
    assert e.calls[0][1] is None and e.calls[0][2] == 0.25
    strict = explore.next_reachable_view(e, None, [0.1, 0.2], particle=None, k=4, n_headings=2, min_reach=0.75)
    assert np.all(cand[strict.order][:, 1] != ys[1]) and np.all(strict.reach[strict.order] == 1.0)
    # a weight on the way: 1 bit per metre moves the nearest candidate (ys[-1], 1 m) ahead of ys[1] (3 bits more, but farther)
    far = 0.05 / 5 * cost_of(0, [0, ys[1]])
    near = explore.next_reachable_view(e, None, [0.1, 0.2], particle=None, k=4, n_headings=2, travel_weight=3.5 / (far - 1.0))
    assert near.poses[0, 1] == ys[-1] and near.scores[0] == 11.0 - 3.5 / (far - 1.0) * 1.0
    one = explore.next_reachable_view(e, None, [0.1, 0.2], particle=1, k=50, n_headings=2)
    assert one.gain.shape == (len(cand),) and set(np.unique(one.reach)) == {0.0, 1.0}
    assert np.all(np.isin(cand[one.order][:, 1], ys[2:])) and len(one.order) == 2 * (len(ys) - 2)
