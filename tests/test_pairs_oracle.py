"""Pair matching without a GPU: the NumPy oracle of tests/pairs_oracle.py against its scalar form, against the refinement oracle
on a raster that holds exactly the pair's hit cells, against hand cases, and the property the feature is for: in the asymmetric
room a displaced query comes back towards the truth when it is matched against five neighbouring scans (DESIGN.md 3.18 has the
numbers)."""
import math

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds
from tests.locate_oracle import asym_room
from tests.pairs_oracle import field_at, hit_cells, match_one, match_pairs, score_scalar
from tests.refine_oracle import refine_one, window_reach

QUANTUM, THRESHOLD = 0.1, 1.0
STEP = math.radians(0.5)
LO, HI = 0.3, 11.0


def room_scan(cells, x0, y0, cell, pose, angles, max_range=12.0):
    lo, hi = lattice_bounds(int(round(40 / cell)), 3)
    return cast(cells, x0, y0, lo, hi, 1.0 / cell, QUANTUM, THRESHOLD, pose, angles, max_range)[0]


@pytest.fixture(scope="module")
def room():
    """Eight seeded poses on free cells of the asymmetric room, each followed by five neighbours within 0.3 m and 0.2 rad:
    (poses [48, 3], scans [48, 91], angles [91]); scan 6 m is query m, scans 6 m + 1 .. 6 m + 5 its run."""
    cells, x0, y0 = asym_room(0.05)
    ang = np.linspace(-0.75 * math.pi, 0.75 * math.pi, 91)
    rng = np.random.Generator(np.random.PCG64(18))

    def free(x, y):
        return cells[int(math.floor(x * 20.0)) - x0, int(math.floor(y * 20.0)) - y0] < 0
    poses = []
    while len(poses) < 48:
        x, y = rng.uniform(-7.5, 7.5, 2)
        if not free(x, y):
            continue
        th = rng.uniform(-math.pi, math.pi)
        group = [(x, y, th)]
        while len(group) < 6:
            dx, dy, dth = rng.uniform(-1.0, 1.0, 3) * (0.3, 0.3, 0.2)
            if free(x + dx, y + dy):
                group.append((x + dx, y + dy, th + dth))
        poses += group
    poses = np.array(poses)
    scans = np.stack([room_scan(cells, x0, y0, 0.05, p, ang) for p in poses])
    return poses, scans, ang


def run(poses, ranges, angles, pairs, guesses=None, cell=0.05, lo=LO, hi=HI, S=1, W=16, R=20, step=STEP):
    return match_pairs(poses, ranges, angles, pairs, guesses, 1.0 / cell, lo, hi, S, W, R, step)


def test_a_scan_in_its_own_run_matches_itself_for_every_substep(room):
    poses, scans, ang = room
    for S in (1, 2, 4, 8, 16):
        for inv in (20.0, 10.0, 1.0 / 0.037):
            out, m8, scores = match_pairs(poses, scans, ang, [[3, 1, 6], [7, 7, 8]], None, inv, LO, HI, S, 5, 2, STEP)
            for m, q in enumerate((3, 7)):
                n_used = int(np.sum((scans[q] > LO) & (scans[q] < HI)))
                assert m8[m, :6].tolist() == [0, 0, 0, 2 * n_used, 2 * n_used, n_used] and n_used > 40, (S, inv)
                assert out[m].tobytes() == poses[q].tobytes()
                assert scores[m].max() == 2 * n_used
            assert m8[1, 6] == m8[1, 5] and m8[0, 6] > 4 * m8[0, 5] - 40    # n_ref counts beams: one scan, five scans


def test_equals_the_refinement_oracle_on_a_raster_of_the_hit_cells(room):
    poses, scans, ang = room
    guess = poses[6] + np.array([0.21, -0.13, 0.03])
    for S, W, R, inv in ((1, 6, 2, 20.0), (4, 9, 1, 20.0), (2, 3, 2, 10.0), (16, 32, 0, 1.0 / 0.037)):
        H, n_ref = hit_cells(poses, scans, ang, 7, 12, inv, LO, HI)
        xs, ys = [c[0] for c in H], [c[1] for c in H]
        x0, y0 = min(xs) - 3, min(ys) - 3
        cells = np.zeros((max(xs) - x0 + 4, max(ys) - y0 + 4), np.int8)
        for (X, Y) in H:
            cells[X - x0, Y - y0] = 30
        want = refine_one(cells, x0, y0, guess, scans[6], ang, inv, QUANTUM, THRESHOLD, LO, HI, S, W, R, STEP)
        got = match_one(poses, scans, ang, (6, 7, 12), guess, inv, LO, HI, S, W, R, STEP)
        assert got[0].tobytes() == want[0].tobytes() and got[1][:6].tolist() == want[1].tolist() and got[1][6:].tolist() == [n_ref, 0]
        assert np.array_equal(got[2], want[2]) and got[2].max() > 0


def test_vector_form_equals_scalar_form(room):
    poses, scans, ang = room
    guess = poses[12] + np.array([-0.11, 0.17, -0.02])
    for S in (1, 4):
        _, m8, scores = match_pairs(poses, scans, ang, [[12, 13, 16]], [guess], 20.0, LO, HI, S, 5, 2, STEP)
        for i, j, k in ((0, 0, 0), (-5, 5, -2), (5, -5, 2), (3, 1, 1), tuple(int(v) for v in m8[0, :3])):
            assert score_scalar(poses, scans, ang, (12, 13, 16), guess, 20.0, LO, HI, S, i, j, k, STEP) == scores[0, k + 2, i + 5, j + 5]
        assert m8[0, 3] == scores.max() > m8[0, 4] == scores[0, 2, 5, 5]


def wall_scans():
    """Scan 0 sees a wall along x at y = 1.0125 from (0, 0, pi / 2), 81 beams whose end points lie 0.05 m apart; scan 1 is its
    middle 21 beams, the rest NaN; scan 2 has no used beam."""
    xs = (np.arange(81) - 40) * 0.05 + 0.0125
    ang = np.arctan2(-xs, 1.0125)                        # sensor frame: the sensor looks along +y
    r = np.hypot(xs, 1.0125)
    short = np.full(81, np.nan)
    short[30:51] = r[30:51]
    none = np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, LO, HI] + [20.0] * 74)
    poses = np.array([[0.0, 0.0, math.pi / 2]] * 3)
    return poses, np.stack([r, short, none]), ang


def test_ties_go_to_the_smallest_rotation_and_the_shortest_shift():
    poses, scans, ang = wall_scans()
    guess = np.array([[0.0, -0.1, math.pi / 2]])         # two cells short of the wall
    out, m8, scores = run(poses, scans, ang, [[1, 0, 1]], guess, W=6, R=2, step=0.0)      # rot_step 0: every rotation ties
    assert m8[0].tolist() == [0, 2, 0, 42, int(scores[0, 2, 6, 6]), 21, 81, 0] and m8[0, 4] < 42
    assert np.all(scores[0, :, :, 8] == 42)             # every shift along the wall, every rotation: the maximum
    assert out[0].tolist() == [0.0, -0.1 + 2.0 / 20.0, math.pi / 2]
    again, m8b, _ = run(poses, scans, ang, [[1, 0, 1]], out, W=6, R=2, step=STEP)
    assert m8b[0, :5].tolist() == [0, 0, 0, 42, 42] and again.tobytes() == out.tobytes()


def test_an_empty_run_and_an_empty_query_return_the_guess():
    poses, scans, ang = wall_scans()
    guess = np.array([[0.123456789, -1.987654321, 0.777]] * 2)
    out, m8, scores = run(poses, scans, ang, [[0, 2, 3], [2, 0, 2]], guess, W=3, R=2)
    assert out.tobytes() == guess.tobytes() and not scores.any() and scores.shape == (2, 5, 7, 7)
    assert m8.tolist() == [[0, 0, 0, 0, 0, 81, 0, 0], [0, 0, 0, 0, 0, 0, 102, 0]]


def border_case():
    """S = 1, W = 4, max_range 2 m at 0.05 m: Mw = 46 round the query's cell (0, 0).  Two reference scans put a point on every
    cell from three inside the window's border to two outside it, 43 .. 48, along +x and along +y; the query's two beams end
    in cells 40 on either axis, 44 at the largest shift.  Returns (poses, scans, angles, pair, Mw)."""
    ang = np.array([0.0] * 6 + [math.pi / 2] * 6 + [0.0, math.pi / 2])
    reach = (np.arange(43, 49) + 0.5) / 20.0 - 2.0       # 0.175 .. 0.425 m from the reference poses
    scans = np.full((3, 14), np.nan)
    scans[0, :6], scans[1, 6:12], scans[2, 12:] = reach, reach, 1.9999
    poses = np.array([[2.0, 0.025, 0.0], [0.025, 2.0, 0.0], [0.0499, 0.0499, 0.0]])
    return poses, scans, ang, (2, 0, 2), window_reach(2.0, 20.0, 4, 1)


def test_reference_points_round_the_window_border():
    """The border cells' dil depends on the ring one cell outside the window.  The scalar form has no window, and the whole
    volume equals it.  (A beam's end cell stays within ceil(max_range inv) + W of the guess's cell, two short of Mw: the bound,
    and so the ring, has slack, and no scan can read the border cells themselves.)"""
    poses, scans, ang, pair, Mw = border_case()
    H, n_ref = hit_cells(poses, scans, ang, 0, 2, 20.0, 0.01, 2.0)
    assert Mw == 46 and n_ref == 12 and sorted(H) == sorted([(c, 0) for c in range(43, 49)] + [(0, c) for c in range(43, 49)])
    assert field_at(H, Mw, 0) == 2 and field_at(H, Mw + 2, 0) == 2 and field_at(H, Mw + 3, 0) == 1 and field_at(H, Mw + 4, 1) == 0
    out, m8, scores = match_pairs(poses, scans, ang, [pair], None, 20.0, 0.01, 2.0, 1, 4, 0, 0.0)
    for i in range(-4, 5):
        for j in range(-4, 5):
            assert scores[0, 0, i + 4, j + 4] == score_scalar(poses, scans, ang, pair, None, 20.0, 0.01, 2.0, 1, i, j, 0, 0.0)
    assert scores[0, 0, 8, 4] == 2 and scores[0, 0, 6, 4] == 1 and scores[0, 0, 5, 4] == 0      # cells 44, 42 and 41 on the x axis
    assert m8[0].tolist() == [0, 3, 0, 2, 0, 2, 12, 0]   # one beam reaches cell 43 at (3, 0) and at (0, 3): the tie goes to the smaller i


def test_displaced_queries_come_back_towards_the_truth(room):
    """Eight queries, 91 beams over 270 degrees cast to 12 m, used in (0.3, 11), each matched against the five neighbouring
    scans at their true poses; guesses off by up to 0.8 of the window on each axis (W = 16 cells of 0.05 m = 0.8 m, 20 steps
    of 0.5 degrees).  The figures this prints are in DESIGN.md 3.18; the assertion is on the medians, refined below half the
    guesses'."""
    poses, scans, ang = room
    rng = np.random.Generator(np.random.PCG64(7))
    q = np.arange(0, 48, 6)
    truth = poses[q]
    span = 0.8 * np.array([0.8, 0.8, 20 * STEP])
    guess = truth + rng.uniform(-1.0, 1.0, (8, 3)) * span
    pairs = np.stack([q, q + 1, q + 6], axis=1)
    out, m8, _ = run(poses, scans, ang, pairs, guess)
    assert np.all(m8[:, 3] >= m8[:, 4]) and np.all(m8[:, 3] <= 2 * m8[:, 5]) and np.all(m8[:, 5] > 40) and np.all(m8[:, 6] > 200)

    def errors(p):
        d = p - truth
        return np.hypot(d[:, 0], d[:, 1]), np.abs((d[:, 2] + math.pi) % (2 * math.pi) - math.pi)
    gt, gh = errors(guess)
    rt, rh = errors(out)
    print("translation: guesses median %.4f max %.4f, refined median %.4f max %.4f" % (np.median(gt), gt.max(), np.median(rt), rt.max()))
    print("heading:     guesses median %.5f max %.5f, refined median %.5f max %.5f" % (np.median(gh), gh.max(), np.median(rh), rh.max()))
    print("fraction:    guesses median %.3f, refined median %.3f" % (np.median(m8[:, 4] / (2.0 * m8[:, 5])), np.median(m8[:, 3] / (2.0 * m8[:, 5]))))
    assert np.median(rt) < 0.5 * np.median(gt)
    assert np.median(rh) < 0.5 * np.median(gh)
