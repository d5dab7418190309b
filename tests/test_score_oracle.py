"""The oracle of rbpf_score_maps (tests/score_oracle.py) against cases counted by hand and against the identities of the
specification (include/rbpf_hip.h).  No GPU."""
import numpy as np

from tests import score_oracle as S

Q, THR = 0.1, 1.0                     # the default quantum and occupied threshold: occupied is v > 10
FREE, WALL = -30, 30


def grown(cells, tol, rim=0):
    """`cells` over the box with a rim of `tol` cells of value `rim` round it."""
    return np.pad(np.asarray(cells, np.int64), int(tol), constant_values=rim)


def run(cells, ref, tol=0, table=None, g=None):
    cells = np.asarray(cells)
    box = (0, cells.shape[0], 0, cells.shape[1])
    return S.scores(grown(cells, tol) if g is None else g, box, ref, tol, table, Q, THR)


def field(out, name):
    return int(out[S.FIELDS.index(name)])


def test_hand_counted_5x5():
    m = np.array([[-3, -3, -3, 0, 0],
                  [-3, 20, 20, 0, 0],
                  [-3, 20, -3, 0, 5],
                  [0, 0, 0, 0, 5],
                  [0, 0, 0, 11, 11]])
    r = np.array([[-1, -1, 0, 0, 30],
                  [-1, 30, 30, 0, 0],
                  [0, -2, -2, 0, 0],
                  [0, 0, 0, 0, 12],
                  [-5, 0, 0, 0, 12]])
    out = run(m, r, tol=0, table=np.arange(61))
    # the map: F at (0,0) (0,1) (0,2) (1,0) (2,0) (2,2); O at (1,1) (1,2) (2,1) (4,3) (4,4); U the other 14
    # the reference: F at (0,0) (0,1) (1,0) (2,1) (2,2) (4,0); O at (0,4) (1,1) (1,2) (3,4) (4,4); U the other 14
    want_n = [4, 2, 0,       # map F: (0,0) (0,1) (1,0) (2,2) | (0,2) (2,0) | -
              1, 11, 2,      # map U: (4,0) | the rest | (0,4) (3,4)
              1, 1, 3]       # map O: (2,1) | (4,3) | (1,1) (1,2) (4,4)
    assert out[:9].tolist() == want_n and sum(want_n) == 25
    assert field(out, "hit_m") == field(out, "hit_r") == 3               # tol 0: the cells occupied on both sides
    # |v - r|: row 0: 2 2 3 0 30; row 1: 2 10 10 0 0; row 2: 3 22 1 0 5; row 3: 0 0 0 0 7; row 4: 5 0 0 11 1
    assert field(out, "l1") == 37 + 22 + 31 + 7 + 17
    assert field(out, "tab") == int((m + 30).sum())                      # table[k] = k: the sum of v - vmin
    out1 = run(m, r, tol=1)
    # tol 1: map O (2,1) has reference O (1,1) next to it, (4,3) has (3,4) and (4,4): all five confirmed; reference O (0,4) has
    # no map O within one cell ((1,3) (1,4) (0,3) are not occupied), (3,4) has (4,3) (4,4): four of five found
    assert (field(out1, "hit_m"), field(out1, "hit_r")) == (5, 4)
    assert out1[:9].tolist() == want_n and field(out1, "l1") == field(out, "l1") and field(out1, "tab") == 0


def test_each_class_pair_alone():
    vals = {S.F: -7, S.U: 3, S.O: 25}
    for a in (S.F, S.U, S.O):
        for b in (S.F, S.U, S.O):
            out = run(np.full((5, 5), vals[a]), np.full((5, 5), vals[b]))
            want = [0] * 9
            want[3 * a + b] = 25
            assert out[:9].tolist() == want
            assert field(out, "l1") == 25 * abs(vals[a] - vals[b])
            assert field(out, "hit_m") == field(out, "hit_r") == (25 if a == b == S.O else 0)


def test_identities_on_random_rasters():
    rng = np.random.default_rng(5)
    vals = np.array([FREE, -4, 0, 0, 3, 10, 11, WALL])
    for nx, ny in ((7, 9), (33, 20), (64, 65)):
        box = (0, nx, 0, ny)
        big = rng.choice(vals, size=(nx + 32, ny + 32), p=[.3, .1, .2, .2, .05, .05, .05, .05])
        ref = rng.choice(vals, size=(nx, ny))
        tab = rng.integers(0, 1 << 20, 61)
        prev = None
        for tol in (0, 1, 2, 5, 16):
            g = big[16 - tol:16 + nx + tol, 16 - tol:16 + ny + tol]
            out = S.scores(g, box, ref, tol, tab, Q, THR)
            assert out[:9].sum() == nx * ny
            if tol == 0:
                assert field(out, "hit_m") == field(out, "hit_r") == field(out, "n_OO")
            if prev is not None:
                assert field(out, "hit_m") >= field(prev, "hit_m") and field(out, "hit_r") >= field(prev, "hit_r")
                assert np.array_equal(out[[0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12]], prev[[0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12]])
            prev = out
            own = S.scores(g, box, g[tol:tol + nx, tol:tol + ny], tol, tab, Q, THR)
            n = own[:9].reshape(3, 3)
            assert np.array_equal(n, np.diag(np.diag(n))) and field(own, "l1") == 0
            if tol == 0:
                assert field(own, "hit_m") == field(own, "hit_r") == field(own, "n_OO")
        # the reference is the particle's own render and nothing occupied lies outside the box: both hits are n[O][O] at any tol
        inner = big[16:16 + nx, 16:16 + ny]
        own = S.scores(grown(inner, 3), box, inner, 3, None, Q, THR)
        assert field(own, "hit_m") == field(own, "hit_r") == field(own, "n_OO") > 0 and field(own, "tab") == 0


def test_a_wall_shifted_by_one_cell():
    m, r = np.full((9, 9), FREE), np.full((9, 9), FREE)
    m[4, 1:8] = WALL
    r[5, 1:8] = WALL
    out0, out1 = run(m, r, tol=0), run(m, r, tol=1)
    assert (field(out0, "hit_m"), field(out0, "hit_r"), field(out0, "n_OO")) == (0, 0, 0)
    assert (field(out1, "hit_m"), field(out1, "hit_r")) == (7, 7)
    assert field(out0, "n_OF") == field(out0, "n_FO") == 7 and field(out0, "l1") == 14 * 60


def test_occupied_just_outside_the_box_counts_for_the_map_only():
    m, r = np.zeros((5, 5), int), np.zeros((5, 5), int)
    r[0, 2] = WALL                                        # a reference wall on the box edge
    g = grown(m, 1)
    g[0, 3] = WALL                                        # the map's wall one cell outside the box, next to it
    out = run(m, r, tol=1, g=g)
    assert field(out, "hit_r") == 1 and field(out, "hit_m") == 0 and field(out, "n_UO") == 1
    assert field(run(m, r, tol=1), "hit_r") == 0          # without it the reference's wall is not found
    # a map wall on the box edge: the reference has nothing outside the box that could confirm it
    m[4, 4] = WALL
    assert field(run(m, r, tol=1), "hit_m") == 0
    g = grown(m, 1)
    out = run(m, r, tol=1, g=g)
    assert field(out, "hit_m") == 0 and field(out, "n_OU") == 1


def test_the_threshold_is_strict():
    at = int(round(THR / Q))
    m = np.array([[at, at + 1, at - 1, 0, -1]])
    out = run(m, m)
    assert out[:9].reshape(3, 3).tolist() == [[1, 0, 0], [0, 3, 0], [0, 0, 1]]
    assert S.classes(m, Q, THR).tolist() == [[S.U, S.O, S.U, S.U, S.F]]
    assert field(out, "hit_m") == field(out, "hit_r") == 1
