"""tests/travel_oracle.py on its own: the closed forms and the rules of DESIGN.md 3.12 on rasters small enough to check by hand."""
import numpy as np

from tests import travel_oracle as T

INV, Q, THR = 20.0, 0.1, 1.0
FREE, WALL = -30, 30


def centre(i, j):
    return [(i + 0.5) / INV, (j + 0.5) / INV]


def run(cells, starts, goals=None, inflate=0, clear_max=1, through_unknown=False, outside=0):
    """The oracle on `cells` as the box (0, nx, 0, ny), the margin filled with `outside`."""
    m = T.margin(clear_max)
    grown = np.pad(np.asarray(cells, np.int8), m, constant_values=outside)
    box = (0, cells.shape[0], 0, cells.shape[1])
    return T.travel(grown, box, INV, Q, THR, starts, goals, inflate, clear_max, through_unknown)


def test_an_open_field_is_the_chamfer_metric():
    cost, clear, goal = run(np.full((40, 40), FREE, np.int8), [centre(7, 9)], [centre(39, 0), [5.0, 5.0]])
    i, j = np.indices((40, 40))
    dx, dy = np.abs(i - 7), np.abs(j - 9)
    assert np.array_equal(cost, 5 * np.maximum(dx, dy) + 2 * np.minimum(dx, dy))
    assert cost.dtype == np.int32 and clear.dtype == np.uint16 and np.all(clear == 1)
    assert goal.tolist() == [5 * 32 + 2 * 9, -1]                           # the second goal lies outside the box


def test_clearance_is_the_closed_form_and_counts_cells_outside_the_box():
    c = np.full((30, 30), FREE, np.int8)
    c[10, 12] = 11                                                        # just above the threshold
    c[20, 5] = 10                                                         # exactly the threshold: not occupied
    _, clear, _ = run(c, [centre(0, 0)], clear_max=60)
    i, j = np.indices(c.shape)
    dx, dy = np.abs(i - 10), np.abs(j - 12)
    assert np.array_equal(clear, np.minimum(5 * np.maximum(dx, dy) + 2 * np.minimum(dx, dy), 60))
    # an occupied ring outside the box: the distance to the nearest margin cell
    _, clear, _ = run(np.full((9, 9), FREE, np.int8), [centre(4, 4)], clear_max=320, outside=WALL)
    edge = np.minimum(np.minimum(i[:9, :9], 8 - i[:9, :9]), np.minimum(j[:9, :9], 8 - j[:9, :9])) + 1
    assert np.array_equal(clear, 5 * edge)


def test_no_corner_is_cut_and_a_one_cell_gap_is_passed():
    c = np.full((9, 9), FREE, np.int8)
    c[4, :5] = WALL
    c[5, 5:] = WALL                                                       # (4, 4) and (5, 5) touch at a corner only
    cost, _, _ = run(c, [centre(0, 0)])
    assert cost[4, 5] > 0 and cost[3, 8] > 0 and np.all(cost[6:] == -1) and cost[5, 4] == -1
    c = np.full((9, 9), FREE, np.int8)
    c[4] = WALL
    c[4, 4] = FREE
    cost, _, _ = run(c, [centre(0, 4)])
    assert cost[4, 4] == 20 and cost[8, 4] == 40 and cost[5, 3] == 25 + 5 and cost[5, 5] == 30   # through the gap, then sideways: no diagonal out of it
    assert np.all(cost[c == WALL] == -1)


def test_a_corridor_is_passable_exactly_when_its_centre_line_clears_the_inflation():
    for w in range(1, 8):
        c = np.full((12, w + 2), FREE, np.int8)
        c[:, 0] = c[:, -1] = WALL
        centre_d = 5 * ((w + 1) // 2)                                     # chamfer distance of the centre line to the nearer wall
        for inflate in (0, 4, 5, 9, 10, 14, 15, 19, 20):
            cost, clear, _ = run(c, [centre(0, (w + 1) // 2)], inflate=inflate, clear_max=inflate + 1)
            assert int(clear[6].max()) == min(centre_d, inflate + 1)
            assert (cost[11].max() >= 0) == (centre_d > inflate), (w, inflate)
            assert cost[0, (w + 1) // 2] == 0                             # the robot is where it is, whatever the inflation


def test_a_start_inside_a_wall_costs_nothing_and_leaves_it():
    c = np.full((7, 7), FREE, np.int8)
    c[3, 2:5] = WALL
    cost, _, _ = run(c, [centre(3, 3)])
    assert cost[3, 3] == 0 and cost[2, 3] == 5 and cost[4, 3] == 5 and cost[3, 2] == -1 and cost[3, 4] == -1
    assert cost[2, 2] == 10 and cost[2, 4] == 10                          # round the corner of (3, 2): the diagonal from (3, 3) is barred


def test_unknown_and_weakly_occupied_cells_block_unless_crossing_is_allowed():
    c = np.full((5, 9), FREE, np.int8)
    c[:, 4] = 0                                                           # unknown column
    c[:, 6] = 5                                                           # 0 < v quantum <= threshold
    cost, _, _ = run(c, [centre(2, 0)])
    assert np.all(cost[:, :4] >= 0) and np.all(cost[:, 4:] == -1)
    cost, _, _ = run(c, [centre(2, 0)], through_unknown=True)
    assert np.all(cost >= 0) and cost[2, 8] == 40
    c[:, 6] = 11
    cost, _, _ = run(c, [centre(2, 0)], through_unknown=True)
    assert np.all(cost[:, :6] >= 0) and np.all(cost[:, 6:] == -1)


def test_sources_outside_the_box_and_several_sources():
    c = np.full((20, 20), FREE, np.int8)
    c[8, 3:17] = WALL
    cost, _, goal = run(c, [[-1.0, 0.2], [5.0, 5.0]], [centre(1, 1)])
    assert np.all(cost == -1) and goal.tolist() == [-1]
    a, _, _ = run(c, [centre(1, 1)])
    b, _, _ = run(c, [centre(18, 15)])
    both, _, _ = run(c, [centre(1, 1), centre(18, 15), [9.0, 9.0]])
    assert np.array_equal(both, np.minimum(a, b))


def test_cells_of_floors_towards_minus_infinity():
    assert T.cells_of([[-0.01, 0.0], [0.0499999, -0.05], [0.05, -0.0500001]], INV).tolist() == [[-1, 0], [0, -1], [1, -2]]
