"""Pose refinement without a GPU: the NumPy oracle of tests/refine_oracle.py against its scalar form, against hand cases and
against the locate oracle's scores, and the property the feature is for: in the asymmetric room, perturbed poses come back
towards the truth (DESIGN.md 3.17 has the numbers)."""
import math

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds
from tests.locate_oracle import asym_room, locate
from tests.refine_oracle import refine, refine_one, score_scalar, tie_order, window_reach

QUANTUM, THRESHOLD = 0.1, 1.0
STEP = math.radians(0.25)


def room_scan(cells, x0, y0, cell, pose, angles, max_range=12.0):
    lo, hi = lattice_bounds(int(round(40 / cell)), 3)
    return cast(cells, x0, y0, lo, hi, 1.0 / cell, QUANTUM, THRESHOLD, pose, angles, max_range)[0]


@pytest.fixture(scope="module")
def room():
    cells, x0, y0 = asym_room(0.05)
    return cells, x0, y0, np.linspace(-0.75 * math.pi, 0.75 * math.pi, 181)


def run(cells, x0, y0, poses, ranges, angles, cell=0.05, lo=0.3, hi=11.0, S=4, W=12, R=10, step=STEP):
    return refine(cells, x0, y0, poses, ranges, angles, 1.0 / cell, QUANTUM, THRESHOLD, lo, hi, S, W, R, step)


def test_tie_order():
    order = tie_order(1, 1)
    assert len(order) == 27 and len(set(order)) == 27
    assert order[:5] == [(0, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0)]        # (k, i, j): |k|, then i^2 + j^2, then k, i, j
    assert order[9:12] == [(-1, 0, 0), (1, 0, 0), (-1, -1, 0)] and order[-1] == (1, 1, 1)
    assert tie_order(0, 0) == [(0, 0, 0)]
    assert window_reach(11.0, 20.0, 12, 4) == 225 and window_reach(11.0, 20.0, 13, 4) == 226 and window_reach(0.5, 10.0, 0, 1) == 7


def test_empty_map_returns_the_guess_bit_for_bit():
    cells = np.zeros((50, 60), np.int8)
    ang = np.linspace(-2.0, 2.0, 33)
    guess = np.array([[0.123456789, -1.987654321, 0.777], [-3.3, 2.2, -3.0]])
    rg = np.full((2, 33), 2.5)
    poses, n6, scores = run(cells, -25, -30, guess, rg, ang, W=3, R=2)
    assert poses.tobytes() == guess.tobytes()
    assert n6.tolist() == [[0, 0, 0, 0, 0, 33]] * 2 and not scores.any() and scores.shape == (2, 5, 7, 7)


def test_unused_ranges_are_data():
    cells = np.full((80, 80), 30, np.int8)               # occupied everywhere: F = 2 at every end cell
    ang = np.linspace(-1.0, 1.0, 9)
    rg = np.array([[np.nan, np.inf, -np.inf, 0.0, -1.0, 0.3, 11.0, 0.5, 1.5]])
    poses, n6, scores = run(cells, -40, -40, [[0.01, 0.02, 0.1]], rg, ang, W=2, R=1)
    assert n6[0].tolist() == [0, 0, 0, 4, 4, 2] and np.all(scores == 4)                  # only 0.5 and 1.5 lie in (0.3, 11)
    none = np.full((1, 9), np.nan)
    poses, n6, scores = run(cells, -40, -40, [[0.01, 0.02, 0.1]], none, ang, W=2, R=1)
    assert n6[0].tolist() == [0, 0, 0, 0, 0, 0] and not scores.any() and poses[0].tolist() == [0.01, 0.02, 0.1]


def test_window_zero_is_plain_scoring(room):
    cells, x0, y0, ang = room
    pose = (2.17, -3.36, 2.0)
    r = room_scan(cells, x0, y0, 0.05, pose, ang)
    guess = np.array([[2.19, -3.33, 2.01]])
    poses, n6, scores = run(cells, x0, y0, guess, r[None], ang, W=0, R=0)
    want = score_scalar(cells, x0, y0, guess[0], r, ang, 20.0, QUANTUM, THRESHOLD, 0.3, 11.0, 4, 0, 0, 0, STEP)
    assert scores.shape == (1, 1, 1, 1) and n6[0].tolist() == [0, 0, 0, want, want, int(np.sum((r > 0.3) & (r < 11.0)))]
    assert 0 < want and poses.tobytes() == guess.tobytes()


def test_vector_form_equals_scalar_form(room):
    cells, x0, y0, ang = room
    r = room_scan(cells, x0, y0, 0.05, (-3.05, 5.52, -1.2), ang[::3])
    r[2], r[5] = 0.3, 11.0                               # the bounds themselves: unused
    guess = (-3.0, 5.45, -1.18)
    for S in (1, 2, 4, 8, 16):
        _, n6, scores = run(cells, x0, y0, [guess], r[None], ang[::3], S=S, W=5, R=2)
        for i, j, k in ((0, 0, 0), (-5, 5, -2), (5, -5, 2), (3, 1, 1), (-2, -4, 0), (int(n6[0, 0]), int(n6[0, 1]), int(n6[0, 2]))):
            got = score_scalar(cells, x0, y0, guess, r, ang[::3], 20.0, QUANTUM, THRESHOLD, 0.3, 11.0, S, i, j, k, STEP)
            assert got == scores[0, k + 2, i + 5, j + 5], (S, i, j, k)
        assert n6[0, 3] == scores.max() and n6[0, 4] == scores[0, 2, 5, 5] and n6[0, 3] > 0


def test_one_step_per_cell_scores_like_locate():
    """substeps 1, no rotation, the guess at a cell's centre: candidate (i, j) is the locate oracle's cell (X + i, Y + j) at
    rotation 0, whose end cells are X + floor(0.5 + d inv).  The two roundings agree unless an end point lies within 1e-9 of a
    cell boundary; this scan has no such beam."""
    cells, x0, y0 = asym_room(0.1)
    ang = np.linspace(-0.75 * math.pi, 0.75 * math.pi, 91)
    X, Y = 21, -33
    pose = ((X + 0.5) * 0.1, (Y + 0.5) * 0.1, 0.0)
    r = room_scan(cells, x0, y0, 0.1, (2.1337, -3.2871, 0.0123), ang)   # seen from off the centre: from it, beams end on cell faces
    W = 6
    _, n6, scores = refine(cells, x0, y0, [pose], r[None], ang, 10.0, QUANTUM, THRESHOLD, 1e-3, 11.0, 1, W, 0, 0.0)
    best, _, n_used = locate(cells, x0, y0, (X - W, X + W + 1, Y - W, Y + W + 1), r, ang, 1, 10.0, QUANTUM, THRESHOLD, 1e-3, 11.0)
    assert n_used == n6[0, 5] > 50
    free = best >= 0                                     # locate scores only the cells a robot can stand on
    assert free.sum() > 100 and np.array_equal(scores[0, 0][free], best[free])


def test_a_shift_along_a_wall_ties_and_the_shortest_wins():
    cells = np.zeros((200, 120), np.int8)                # cells X -100 .. 99, Y -20 .. 99; one wall along x at Y = 40
    cells[:, 60] = 30
    x0, y0 = -100, -20
    ang = np.linspace(-0.5, 0.5, 41)
    true = (0.013, 1.0, math.pi / 2)
    r = room_scan(cells, x0, y0, 0.05, true, ang, max_range=5.0)
    assert np.all((r > 0.9) & (r < 1.3))
    guess = np.array([[0.013, 0.9, math.pi / 2]])        # two cells short of the wall
    poses, n6, scores = run(cells, x0, y0, guess, r[None], ang, S=4, W=12, R=0)
    i, j, k, best, at_guess, n_used = n6[0].tolist()
    assert (i, k) == (0, 0) and j > 0 and best == 2 * n_used > at_guess
    assert np.all(scores[0, 0, :, j + 12] == best)                                        # every shift along the wall ties
    assert np.all(scores[0, 0, 12, 12 - j + 1:12 + j] < best)                             # and no shorter move reaches the maximum
    assert poses[0].tolist() == [0.013, 0.9 + float(j) / 80.0, math.pi / 2]
    # the refined pose is a guess that attains the maximum: it stays where it is, bit for bit
    again, n6b, _ = run(cells, x0, y0, poses, r[None], ang, S=4, W=12, R=3)
    assert n6b[0, :3].tolist() == [0, 0, 0] and again.tobytes() == poses.tobytes() and n6b[0, 3] == n6b[0, 4] == best


def test_perturbed_poses_come_back_towards_the_truth(room):
    """12 seeded poses on free cells, 181 beams over 270 degrees cast to 12 m, used in (0.3, 11); guesses off by up to 0.8 of
    the window on each axis (window 12 / 4 cells = 0.15 m, 10 steps of 0.25 degrees).  Measured with this oracle (PCG64 seed 5):
    translation error of the guesses median 0.0816 m, max 0.1562 m, refined median 0.0275 m, max 0.0588 m; heading error of
    the guesses median 0.02082 rad, max 0.03149 rad, refined median 0.00340 rad, max 0.00676 rad.  Single poses may get slightly
    worse in heading: the assertion is on the medians, refined below half the guesses'."""
    cells, x0, y0, ang = room
    rng = np.random.Generator(np.random.PCG64(5))
    truth = []
    while len(truth) < 12:
        x, y = rng.uniform(-7.5, 7.5, 2)
        if cells[int(math.floor(x * 20.0)) - x0, int(math.floor(y * 20.0)) - y0] < 0:
            truth.append((x, y, rng.uniform(-math.pi, math.pi)))
    truth = np.array(truth)
    scans = np.stack([room_scan(cells, x0, y0, 0.05, p, ang) for p in truth])
    span = 0.8 * np.array([0.15, 0.15, 10 * STEP])
    guess = truth + rng.uniform(-1.0, 1.0, (12, 3)) * span
    poses, n6, _ = run(cells, x0, y0, guess, scans, ang)
    assert np.all(n6[:, 3] >= n6[:, 4]) and np.all(n6[:, 3] <= 2 * n6[:, 5]) and np.all(n6[:, 5] > 60)

    def errors(p):
        d = p - truth
        return np.hypot(d[:, 0], d[:, 1]), np.abs((d[:, 2] + math.pi) % (2 * math.pi) - math.pi)
    gt, gh = errors(guess)
    rt, rh = errors(poses)
    print("translation: guesses median %.4f max %.4f, refined median %.4f max %.4f" % (np.median(gt), gt.max(), np.median(rt), rt.max()))
    print("heading:     guesses median %.5f max %.5f, refined median %.5f max %.5f" % (np.median(gh), gh.max(), np.median(rh), rh.max()))
    assert np.median(rt) < 0.5 * np.median(gt)
    assert np.median(rh) < 0.5 * np.median(gh)
