"""The host side of the path checks (thesis_amd/plan.py: path_cells, shortcut, rollouts, rank_rollouts, PathCheck) against
tests/paths_oracle.py, and the oracle against the travel oracle: what plan.path_to walks checks clear."""
import numpy as np
import pytest

from tests import paths_oracle as PO
from tests import travel_oracle as T
from thesis_amd import plan

INV, Q, THR = 20.0, 0.1, 1.0
SETTINGS = ((0, 1), (7, 8), (20, 21), (20, 320))


def centres(cells):
    return (np.asarray(cells, dtype=np.float64) + 0.5) / INV


# ---- the walk ----------------------------------------------------------------------------------------------------------------------
def test_closed_form_equals_the_incremental_walk_on_every_short_segment():
    for dx in range(-12, 13):
        for dy in range(-12, 13):
            cells = [(3, -4), (3 + dx, -4 + dy)]
            got = plan.walk_cells(cells)
            want = PO.bresenham(cells)
            assert got.tolist() == [list(c) for c in want], (dx, dy)
            assert len(got) == 1 + max(abs(dx), abs(dy)) and got[-1].tolist() == list(cells[1])
            if len(got) > 1:
                assert np.abs(np.diff(got, axis=0)).max() == 1


def test_closed_form_equals_the_incremental_walk_on_long_segments():
    rng = np.random.default_rng(12)
    edge = 21 * 1600                                       # a lattice of 21 tiles of 1600 cells
    for k in range(10000):
        span = edge if k % 250 == 0 else int(rng.integers(13, 200))     # forty as long as the lattice, the others anywhere in it
        a = rng.integers(-edge // 2, edge // 2 - span + 1, size=2)
        b = a + rng.integers(0, span, size=2) * rng.choice([-1, 1], size=2)
        b = np.clip(b, -edge // 2, edge // 2 - 1)
        if k % 10 == 0:
            b[int(rng.integers(2))] = a[int(rng.integers(2))]              # an axis, or a repeat of a coordinate
        got = plan.walk_cells([a, b])
        want = np.array(PO.bresenham([a, b]))
        assert got.shape == want.shape and np.array_equal(got, want), (a, b)


def test_path_cells_takes_metres_repeats_and_single_points():
    p = np.array([[0.26, -0.01, 9.0], [0.26, -0.01, 9.0], [0.41, 0.12, 9.0], [0.26, -0.01, 9.0]])
    cells = plan.path_cells(p, INV)
    assert cells[0].tolist() == [5, -1] and cells[-1].tolist() == [5, -1] and cells.tolist() == [list(c) for c in PO.bresenham([(5, -1), (5, -1), (8, 2), (5, -1)])]
    assert len(cells) == 7
    assert plan.path_cells(p[:1], INV).tolist() == [[5, -1]]
    with pytest.raises(ValueError):
        plan.path_cells(np.zeros((0, 2)), INV)


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def maze(inflate, clear_max):
    """(Travel over the fuzz scene from its corner, Field, the scene's cells)."""
    c = PO.fuzz_scene()
    box = (-13, -13 + c.shape[0], 7, 7 + c.shape[1])
    grown = np.pad(c, T.margin(clear_max))
    start = centres([(box[0] + 3, box[2] + 3)])[0]
    cost, clear, _ = T.travel(grown, box, INV, Q, THR, [start], None, inflate, clear_max)
    tr = plan.Travel(cost, clear, None, 0, box, 1.0 / INV, INV, inflate, clear_max)
    return tr, PO.Field(grown, box, Q, THR, inflate, clear_max), c


@pytest.mark.parametrize("inflate,clear_max", [(0, 1), (7, 8), (11, 12)])
def test_what_path_to_walks_checks_clear(inflate, clear_max):
    tr, f, _ = maze(inflate, clear_max)
    reached = np.argwhere(tr.cost > 0)
    assert len(reached) > 5000
    n = 0
    for i, j in reached[::211]:
        p = plan.path_to(tr, centres([(tr.box[0] + i, tr.box[2] + j)])[0])
        res, steps = f.check_xy([p], INV, start_exempt=True)
        assert res[0, 0] == -1 and steps[0] == len(p), (i, j, res)
        assert res[0, 2] == min(clear_max, int(tr.clearance[tuple((np.floor(p * INV).astype(int) - [tr.box[0], tr.box[2]]).T)].min()))
        n += 1
    assert n >= 40


def test_a_path_pushed_into_a_wall_reports_the_step():
    tr, f, c = maze(0, 1)
    x0, y0 = tr.box[0], tr.box[2]
    assert c[20, 40] == PO.WALL and np.all(c[15:20, 40] == PO.FREE)
    res, steps = f.check_xy([centres([(x0 + 15, y0 + 40), (x0 + 25, y0 + 40)])], INV)
    assert res[0].tolist()[:2] == [5, -1] and steps[0] == 11 and res[0, 2] == 0
    tr7, f7, _ = maze(7, 8)                               # d > 7 needs a free cell between the robot and the wall
    res, _ = f7.check_xy([centres([(x0 + 15, y0 + 40), (x0 + 25, y0 + 40)])], INV)
    assert res[0, 0] == 4
    # the unknown patch: rows 70 .. 109, columns 60 .. 109
    res, _ = f.check_xy([centres([(x0 + 65, y0 + 70), (x0 + 75, y0 + 70)])], INV)
    assert res[0].tolist() == [5, 5, 1, 6]
    through = PO.Field(np.pad(c, 1), tr.box, Q, THR, 0, 1, through_unknown=True)
    res, _ = through.check_xy([centres([(x0 + 65, y0 + 70), (x0 + 75, y0 + 70)])], INV)
    assert res[0].tolist() == [-1, 5, 1, 6]


def test_a_diagonal_gap_between_two_occupied_cells_blocks():
    c = np.full((8, 8), PO.FREE, np.int8)
    c[3, 4] = c[4, 3] = PO.WALL
    f = PO.Field(np.pad(c, 1), (0, 8, 0, 8), Q, THR, 0, 1)
    res, _ = f.check_xy([centres([(1, 1), (6, 6)])], INV)
    assert res[0, 0] == 3                                  # (3, 3) -> (4, 4) would cut both corners
    res, _ = f.check_xy([centres([(1, 1), (3, 3)]), centres([(4, 4), (6, 6)]), centres([(3, 3), (3, 3), (4, 4)])], INV)
    assert res[:, 0].tolist() == [-1, -1, 1]
    res, _ = f.check_xy([centres([(4, 3), (5, 4)])], INV, start_exempt=True)     # standing in a wall: the start is exempt, as a side cell too
    assert res[0, 0] == -1 and res[0, 2] == 0
    res, _ = f.check_xy([centres([(4, 3), (5, 4), (4, 3)])], INV, start_exempt=True)
    assert res[0, 0] == -1
    res, _ = f.check_xy([centres([(4, 3), (5, 4)])], INV)
    assert res[0, 0] == 0


def test_the_fuzz_scene_shows_both_outcomes():
    c = PO.fuzz_scene()
    box = (0, 200, 0, 150)
    for inflate, clear_max in SETTINGS:
        f = PO.Field(np.pad(c, T.margin(clear_max)), box, Q, THR, inflate, clear_max)
        paths = PO.fuzz_paths(np.random.default_rng(100 + inflate + clear_max), 400, c.shape, (0, 0), INV)
        res, steps = f.check_xy(list(paths), INV)
        share = float((res[:, 0] >= 0).mean())
        print(f"inflate {inflate}, clear_max {clear_max}: blocked share {share:.2f}, unknown on {int((res[:, 1] >= 0).sum())} paths, steps {steps.min()} .. {steps.max()}")
        assert 0.1 <= share <= 0.9 and (res[:, 1] >= 0).sum() >= 10 and steps.max() <= 17


# ---- shortcut ----------------------------------------------------------------------------------------------------------------------------
def oracle_clear(f, exempt_from=None):
    def clear(legs):
        out = []
        for leg in legs:
            ex = exempt_from is not None and np.array_equal(leg[0], exempt_from)
            out.append(f.check_xy([leg], INV, start_exempt=ex)[0][0, 0] < 0)
        return np.array(out)
    return clear


def length(p):
    return float(np.hypot(*np.diff(p, axis=0).T).sum())


def test_shortcut_returns_a_clear_chain_no_longer_than_the_path():
    tr, f, _ = maze(7, 8)
    far = np.argwhere(tr.cost > 0)
    i, j = far[np.argmax(tr.cost[tuple(far.T)] * (far[:, 0] < 45))]        # beyond two walls
    p = plan.path_to(tr, centres([(tr.box[0] + i, tr.box[2] + j)])[0])
    assert len(p) > 150
    calls = []
    clear = oracle_clear(f, p[0])
    s = plan.shortcut(p, lambda legs: (calls.append(len(legs)), clear(legs))[1], lookahead=24)
    assert len(calls) == 1 and calls[0] == sum(min(24, len(p) - 1 - k) for k in range(len(p) - 1))
    assert s[0].tolist() == p[0].tolist() and s[-1].tolist() == p[-1].tolist() and 2 <= len(s) < len(p) / 4
    assert length(s) < length(p)
    assert {tuple(q) for q in s.tolist()} <= {tuple(q) for q in p.tolist()}
    assert f.check_xy([s], INV, start_exempt=True)[0][0, 0] == -1           # the whole chain under the same rule
    assert np.array_equal(plan.shortcut(p, clear, lookahead=1), p)         # nothing but the path's own legs: the path itself
    with pytest.raises(ValueError):
        plan.shortcut(p, lambda legs: np.zeros(len(legs), bool))


def test_shortcut_in_an_empty_room_is_the_straight_line():
    c = np.full((40, 40), PO.FREE, np.int8)
    f = PO.Field(np.pad(c, 1), (0, 40, 0, 40), Q, THR, 0, 1)
    stairs = centres([(2 + (k + 1) // 2, 3 + k // 2) for k in range(41)])
    s = plan.shortcut(stairs, oracle_clear(f))
    assert s.tolist() == [stairs[0].tolist(), stairs[-1].tolist()]
    s = plan.shortcut(stairs, oracle_clear(f), lookahead=16)                # 40 legs in chains of 16: ties to fewer waypoints, then lower indices
    assert len(s) == 4 and np.isclose(length(s), length(stairs[[0, -1]]))
    assert plan.shortcut(stairs[:1], oracle_clear(f)).tolist() == stairs[:1].tolist()


# ---- rollouts --------------------------------------------------------------------------------------------------------------------------
def test_rollouts():
    r = plan.rollouts([1.0, 2.0, np.pi / 2], [0.5, 1.0, 1.0], [0.0, 2 * np.pi / 4.0, -2 * np.pi / 4.0], 4.0, 0.1)
    assert r.shape == (3, 41, 2)
    assert np.allclose(r[0, :, 0], 1.0) and np.allclose(r[0, :, 1], 2.0 + 0.5 * 0.1 * np.arange(41))     # straight along +y
    for k, side in ((1, -1.0), (2, 1.0)):                 # a full circle of radius v / w closes on itself; it turns left for w > 0
        assert np.allclose(r[k, 0], [1.0, 2.0]) and np.allclose(r[k, -1], [1.0, 2.0], atol=1e-12)
        centre = np.array([1.0 + side * 4.0 / (2 * np.pi), 2.0])
        assert np.allclose(np.hypot(*(r[k] - centre).T), 4.0 / (2 * np.pi))
        assert np.allclose(r[k, 10], centre + [0.0, 4.0 / (2 * np.pi)])
    poses = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, np.pi / 2]])
    many = plan.rollouts(poses, [0.5, 1.0], [0.0, 0.3], 2.0, 0.25)
    assert many.shape == (2, 2, 9, 2)
    assert np.allclose(many[1], plan.rollouts(poses[1], [0.5, 1.0], [0.0, 0.3], 2.0, 0.25)) and np.allclose(many[0, 0, -1], [1.0, 0.0])
    tiny = plan.rollouts([0.0, 0.0, 0.0], [1.0, 1.0], [0.0, 1e-12], 3.0, 0.5)
    assert np.allclose(tiny[0], tiny[1], atol=1e-11)
    with pytest.raises(ValueError):
        plan.rollouts([0.0, 0.0], [1.0], [0.0], 1.0, 0.1)


def check_of(first_blocked, min_clearance):
    fb = np.asarray(first_blocked, np.int32)
    z = np.zeros_like(fb)
    return plan.PathCheck(fb, z - 1, np.asarray(min_clearance, np.int32), z, np.full(fb.shape[-1:], 5, np.int32), 0.05, 0, 40)


def test_path_check_shares_and_rank_rollouts():
    one = check_of([-1, 3, -1, -1], [20, 0, 40, 20])
    assert one.clear.tolist() == [True, False, True, True] and one.p_clear().tolist() == [1.0, 0.0, 1.0, 1.0]
    assert np.allclose(one.clearance_metres(), [0.2, 0.0, 0.4, 0.2])
    assert plan.rank_rollouts(one).tolist() == [2, 0, 3]                     # the largest clearance; the tie to the lower index
    assert plan.rank_rollouts(one, end_cost=[50, 1, 50, -1]).tolist() == [0, 2, 3]
    assert plan.rank_rollouts(one, end_cost=[50, 1, 50, 40], clearance_weight=1.0).tolist() == [2, 3, 0]
    many = check_of([[-1, -1, 4, -1], [-1, 2, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, 0]], [[10, 30, 30, 8]] * 4)
    assert many.p_clear().tolist() == [1.0, 0.75, 0.75, 0.75]
    assert np.allclose(many.p_clear([0.0, 0.0, 2.0, 2.0]), [1.0, 1.0, 1.0, 0.5])
    assert plan.rank_rollouts(many).tolist() == [0] and plan.rank_rollouts(many, min_p_clear=0.75).tolist() == [1, 2, 0, 3]
    assert plan.rank_rollouts(many, weights=[0.0, 0.0, 2.0, 2.0]).tolist() == [1, 2, 0]
    cost = np.array([[10, 10, 10, 10], [30, 10, 10, 10], [10, 10, 10, 10], [10, 10, -1, 10]])
    assert plan.rank_rollouts(many, end_cost=cost, min_p_clear=0.75).tolist() == [1, 3, 0, 2]
    cost[0, 1] = -1                                        # no way in a particle of weight 0: it does not count
    assert plan.rank_rollouts(many, end_cost=cost, weights=[0.0, 0.0, 2.0, 2.0], min_p_clear=0.5).tolist() == [0, 1, 3, 2]
    with pytest.raises(ValueError):
        many.p_clear([1.0, 1.0])
