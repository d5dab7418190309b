"""Global localization without a GPU: the NumPy oracle of tests/locate_oracle.py against its scalar form and in an asymmetric
room, and the host half of the feature (thesis_amd/locate.py: hypotheses, allot, seed_particles; ParticleEngine.relocalize
with the oracle behind a stub engine)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds
from tests.locate_oracle import asym_room, locate, locate_scalar
from thesis_amd import locate as loc

CELL, N_ROT, NB, K = 0.1, 360, 181, 8
QUANTUM, THRESHOLD, MIN_R, MAX_R = 0.1, 1.0, 1e-3, 11.0

# The committed pose list.  Six poses chosen without looking at the map; POSES[6] looks into the corner (8, -8) and sees only
# the two walls, which every corner of the room shows alike: its best score (279 of 2 * 169) is shared by four poses, and the
# first of them in the order of `hypotheses` lies 13 m from the truth.  POSES[7] does the same in another corner.
POSES = [(0.33, 0.41, 0.3), (2.17, -3.36, 2.0), (-3.05, 5.52, -1.2), (5.71, 1.13, 3.0), (-1.48, -6.22, 0.9), (6.13, 6.42, -2.5),
         (6.45, -6.55, -0.785), (-6.61, 6.37, 2.3562)]
AMBIGUOUS = 6


def room_scan(cells, x0, y0, cell, pose, angles):
    """What `pose` sees in the raster: the float64 supercover walk of tests/cast_oracle.py (30 m where nothing is met)."""
    lo, hi = lattice_bounds(int(round(40 / cell)), 3)
    return cast(cells, x0, y0, lo, hi, 1.0 / cell, QUANTUM, THRESHOLD, pose, angles, 30.0)[0]


def pose_error(cell3, pose, cell, n_rot):
    """(Chebyshev distance in cells, rotation steps) of a hypothesis cell (X, Y, rot) from a true pose."""
    tx, ty = pose[0] / cell - 0.5, pose[1] / cell - 0.5                  # the robot stands at the centre of its cell
    tr = (pose[2] % (2 * math.pi)) / (2 * math.pi / n_rot)
    dr = abs(cell3[2] - tr)
    return max(abs(cell3[0] - tx), abs(cell3[1] - ty)), min(dr, n_rot - dr)


@pytest.fixture(scope="module")
def room():
    from thesis_amd.datasets import synthetic
    cells, x0, y0 = asym_room(CELL)
    return cells, x0, y0, synthetic.beam_angles(NB)


def test_room_is_asymmetric():
    cells, _, _ = asym_room(CELL)
    assert (cells < 0).any() and (cells > 10).any() and (cells == 0).any()
    assert not any(np.array_equal(cells, q) for q in (np.rot90(cells), np.rot90(cells, 2), cells[::-1], cells[:, ::-1], cells.T))


def test_vector_form_equals_scalar_form(room):
    cells, x0, y0, ang = room
    r = room_scan(cells, x0, y0, CELL, POSES[1], ang[::4])
    r[3], r[7] = 0.0, 11.0                               # unused: not above the minimum, not below the maximum
    box = (-40, 25, 10, 70)
    best, rot, n_used = locate(cells, x0, y0, box, r, ang[::4], 24, 1.0 / CELL, QUANTUM, THRESHOLD, MIN_R, MAX_R)
    assert n_used == int(np.sum((r > MIN_R) & (r < MAX_R))) < len(r)
    picks = [(-40, 10), (24, 69), (-7, 33), (3, 41), (15, 55), (-30, 60), (11, 52), (-1, 12)]      # floor, block shell, inside the block
    got = [locate_scalar(cells, x0, y0, X, Y, r, ang[::4], 24, 1.0 / CELL, QUANTUM, THRESHOLD, MIN_R, MAX_R) for X, Y in picks]
    assert got == [(int(best[X - box[0], Y - box[2]]), int(rot[X - box[0], Y - box[2]])) for X, Y in picks]
    assert any(g == (-1, -1) for g in got) and any(g[0] > 0 for g in got)


def test_box_outside_the_raster_and_no_used_beam(room):
    cells, x0, y0, ang = room
    r = np.full(NB, 30.0)
    box = (x0 + 150, x0 + 230, y0 - 20, y0 + 40)         # partly beyond the raster: unknown there
    best, rot, n_used = locate(cells, x0, y0, box, r, ang, 7, 1.0 / CELL, QUANTUM, THRESHOLD, MIN_R, MAX_R)
    assert n_used == 0
    cand = np.zeros_like(best, dtype=bool)
    cand[:50, 20:] = cells[150:, :40] < 0
    assert cand.any() and np.array_equal(best, np.where(cand, 0, -1)) and np.array_equal(rot, np.where(cand, 0, -1))


def test_every_pose_is_among_the_hypotheses(room):
    cells, x0, y0, ang = room
    box = (x0, x0 + cells.shape[0], y0, y0 + cells.shape[1])
    top1 = 0
    for n, pose in enumerate(POSES):
        r = room_scan(cells, x0, y0, CELL, pose, ang)
        best, rot, n_used = locate(cells, x0, y0, box, r, ang, N_ROT, 1.0 / CELL, QUANTUM, THRESHOLD, MIN_R, MAX_R)
        assert 0 < best.max() <= 2 * n_used
        h = loc.hypotheses(best, rot, box, N_ROT, CELL, k=K, n_used=n_used)
        err = [pose_error(c, pose, CELL, N_ROT) for c in h.cells]
        hit = [i for i, (d, dr) in enumerate(err) if d <= 1.5 and dr <= 1.5]
        print(f"pose {n} {pose}: n_used {n_used}, scores {h.scores.tolist()}, truth at hypothesis {hit}, first is {err[0][0]:.1f} cells / "
              f"{err[0][1]:.1f} steps away")
        assert hit, (pose, h.cells.tolist())
        top1 += hit[0] == 0
        if n == AMBIGUOUS:                               # why k > 1 exists
            assert hit[0] > 0 and h.scores[hit[0]] == h.scores[0] and err[0][0] * CELL > 10.0
    assert top1 >= len(POSES) - 2


# ---- hypotheses --------------------------------------------------------------------------------------------------------------------
def test_hypotheses_order_nms_ties_and_k():
    best = np.full((30, 40), -1, np.int32)
    rot = np.full((30, 40), -1, np.int32)
    for (i, j), (s, r) in {(5, 5): (90, 3), (5, 6): (95, 4), (16, 5): (95, 5), (15, 16): (95, 6), (2, 30): (20, 7), (29, 39): (0, 0),
                           (16, 16): (94, 8)}.items():
        best[i, j], rot[i, j] = s, r
    box = (-10, 20, 100, 140)
    h = loc.hypotheses(best, rot, box, 8, 0.5, k=8, nms_cells=10, n_used=50)
    # 95 three times: X ascending, then Y ascending.  (5, 5) is within 10 cells of (5, 6); (16, 5) is 11 rows from it;
    # (15, 16) is exactly 10 from (5, 6): skipped; (16, 16) is 11 from (5, 6) and (16, 5)
    assert h.cells.tolist() == [[-5, 106, 4], [6, 105, 5], [6, 116, 8], [-8, 130, 7], [19, 139, 0]]
    assert h.scores.tolist() == [95, 95, 94, 20, 0] and h.n_used == 50
    assert np.array_equal(h.poses[:, 0], (h.cells[:, 0] + 0.5) * 0.5) and np.array_equal(h.poses[:, 1], (h.cells[:, 1] + 0.5) * 0.5)
    assert np.array_equal(h.poses[:, 2], h.cells[:, 2] * 6.283185307179586 / 8)
    assert loc.hypotheses(best, rot, box, 8, 0.5, k=2).cells.tolist() == [[-5, 106, 4], [6, 105, 5]]
    assert loc.hypotheses(best, rot, box, 8, 0.5, k=3, nms_cells=0).cells.tolist() == [[-5, 106, 4], [5, 116, 6], [6, 105, 5]]
    empty = loc.hypotheses(np.full((3, 3), -1), np.full((3, 3), -1), (0, 3, 0, 3), 8, 0.5)
    assert empty.poses.shape == (0, 3) and empty.scores.shape == (0,) and empty.cells.shape == (0, 3)


def test_allot():
    assert loc.allot([3, 2, 1], 12).tolist() == [6, 4, 2]              # 1 each, then 9 spare: 4.5, 3, 1.5 -> 4, 3, 1 + the tie's first
    assert loc.allot([300, 1, 1], 10).tolist() == [8, 1, 1]
    assert loc.allot([0, 0, 0], 7).tolist() == [3, 2, 2]
    assert loc.allot([5, 5, 5, 5], 3).tolist() == [1, 1, 1, 0]
    assert loc.allot([], 4).tolist() == []
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(200):
        s = rng.integers(0, 400, size=int(rng.integers(1, 9)))
        P = int(rng.integers(len(s), 300))
        n = loc.allot(s, P)
        assert n.sum() == P and n.min() >= 1
        if s.sum() > 0:                                  # within one particle of the exact share of the spare ones
            assert np.all(np.abs((n - 1) - (P - len(s)) * s / s.sum()) < 1.0)


class StubEngine:
    """locate_scan with the oracle behind it, in the asymmetric room; set_state records what it is given."""
    from thesis_amd.engine import ParticleEngine as _E
    relocalize = _E.relocalize

    def __init__(self, P):
        self.P, self.dim = P, 400
        self.cfg = SimpleNamespace(match_min_range=MIN_R, match_max_range=MAX_R, tile_len_m=40, cell_size=CELL)
        self.cells, self.x0, self.y0 = asym_room(CELL)
        self.state = None

    def locate_scan(self, ranges, angles, particle="best", box=None, n_rot=720, device=False):
        box = box or (self.x0, self.x0 + self.cells.shape[0], self.y0, self.y0 + self.cells.shape[1])
        best, rot, _ = locate(self.cells, self.x0, self.y0, box, ranges, angles, n_rot, 1.0 / CELL, QUANTUM, THRESHOLD, MIN_R, MAX_R)
        return best, rot, tuple(box)

    def set_state(self, poses=None, covs=None, weights=None):
        self.state = (poses, covs, weights)


def test_relocalize_allots_and_jitters(room):
    cells, x0, y0, ang = room
    P, n_rot = 100, 90
    e = StubEngine(P)
    pose = POSES[AMBIGUOUS]
    r = room_scan(cells, x0, y0, CELL, pose, ang)
    h = e.relocalize(r, ang, particle=0, k=5, n_rot=n_rot, seed=4)
    poses, covs, weights = e.state
    assert len(h.poses) == 5 and poses.shape == (P, 3) and covs == 0.0 and weights == 1.0
    assert h.n_used == int(np.sum((r > MIN_R) & (r < MAX_R)))
    n = loc.allot(h.scores, P)
    assert n.sum() == P and n.min() >= 1 and n[0] >= n[-1]
    owner = np.repeat(np.arange(5), n)
    d = poses - h.poses[owner]
    assert np.all(np.abs(d[:, :2]) <= CELL / 2) and np.all(np.abs(d[:, 2]) <= math.pi / n_rot)
    assert np.all(np.floor(poses[:, :2] / CELL) == h.cells[owner, :2])  # each particle inside its hypothesis's cell
    assert d.std(axis=0).min() > 0                                       # jittered at all
    e2 = StubEngine(P)
    e2.relocalize(r, ang, particle=0, k=5, n_rot=n_rot, seed=4)
    assert np.array_equal(e2.state[0], poses)                            # the seed decides
    e2.relocalize(r, ang, particle=0, k=5, n_rot=n_rot, seed=5)
    assert not np.array_equal(e2.state[0], poses)
    assert min(pose_error(c, pose, CELL, n_rot)[0] for c in h.cells) <= 1.5
