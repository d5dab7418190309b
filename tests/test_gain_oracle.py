"""The view-gain oracle (tests/gain_oracle.py) on hand-made rasters: what the visited SET holds and what the three sums count."""
import numpy as np

from tests.gain_oracle import view_gain, visited

INV, Q, THR, VMIN = 20.0, 0.1, 1.0, -30
LO, HI = -1400, 1400
ONES = np.ones(61, np.int64)


def run(cells, x0, y0, pose, angles, max_range, table=ONES):
    g, s, u, _ = view_gain(cells, x0, y0, LO, HI, INV, Q, THR, VMIN, table, [pose], angles, max_range)
    return int(g[0]), int(s[0]), int(u[0])


def cell_pose(X, Y, th=0.0):
    return ((X + 0.5) / INV, (Y + 0.5) / INV, th)


def test_a_thick_wall_contributes_only_its_first_layer():
    c = np.full((40, 21), -30, np.int8)
    c[20:22, :] = 30                                     # a wall two cells thick across the fan
    ang = np.linspace(-0.4, 0.4, 33)
    V, _ = visited(c, 0, -10, LO, HI, INV, Q, THR, cell_pose(5, 0), ang, 5.0)
    assert {X for X, Y in V if c[X, Y + 10] > 10} == {20}                 # the hit layer is seen, the one behind it is not
    assert max(X for X, Y in V) == 20 and (5, 0) in V                    # nothing behind a hit; the origin cell is seen
    one = np.zeros(61, np.int64)
    one[30 - VMIN] = 1
    g, s, u = run(c, 0, -10, cell_pose(5, 0), ang, 5.0, one)
    assert g == len({Y for X, Y in V if X == 20}) and u == 0 and s == len(V)


def test_a_diagonal_gap_is_not_seen_through():
    c = np.full((30, 30), -30, np.int8)
    for k in range(30):
        c[k, 29 - k] = 30                                # an 8-connected diagonal wall: a Bresenham line would slip through
    ang = np.linspace(0.0, np.pi / 2, 91)
    V, _ = visited(c, 0, 0, LO, HI, INV, Q, THR, cell_pose(2, 2, 0.0), ang, 5.0)
    assert all(X + Y <= 29 for X, Y in V)
    assert any(X + Y == 29 for X, Y in V)


def test_identical_beams_give_the_result_of_one():
    rng = np.random.Generator(np.random.PCG64(5))
    c = rng.integers(-30, 11, size=(60, 60)).astype(np.int8)
    c[rng.random(c.shape) < 0.03] = 25
    pose = (1.234, 1.567, 0.3)
    tab = rng.integers(0, 1 << 20, size=61)
    assert run(c, 0, 0, pose, [0.7] * 64, 4.0, tab) == run(c, 0, 0, pose, [0.7], 4.0, tab)


def test_tables_of_ones_and_one_hot():
    rng = np.random.Generator(np.random.PCG64(6))
    c = rng.integers(-30, 11, size=(80, 80)).astype(np.int8)
    c[rng.random(c.shape) < 0.02] = 30
    pose, ang = (2.01, 1.99, -1.0), np.linspace(-np.pi, np.pi, 48, endpoint=False)
    g, s, u = run(c, 0, 0, pose, ang, 1.5)
    assert g == s and 0 < u < s                          # a table of ones counts the cells
    V, _ = visited(c, 0, 0, LO, HI, INV, Q, THR, pose, ang, 1.5)
    for v in (0, -7, 30):
        hot = np.zeros(61, np.int64)
        hot[v - VMIN] = 1
        assert run(c, 0, 0, pose, ang, 1.5, hot)[0] == sum(int(c[X, Y]) == v for X, Y in V)
    assert run(c, 0, 0, pose, ang, 1.5, (np.arange(61) == 30).astype(np.int64))[0] == u       # value 0 is `unknown`


def test_outside_the_raster_is_unknown_and_outside_the_lattice_is_nothing():
    c = np.full((4, 4), -30, np.int8)
    g, s, u = run(c, 0, 0, cell_pose(1, 1), [0.0], 1.0)                  # 21 cells along +x: 3 in the raster
    assert (s, u) == (21, 18)
    assert run(c, 0, 0, (HI / INV + 1.0, 0.0, 0.0), [0.0], 1.0) == (0, 0, 0)           # the origin outside the lattice
    g, s, u = run(c, 0, 0, cell_pose(HI - 3, 0), [0.0], 1.0)             # the ray leaves the lattice after 3 cells
    assert s == 3
