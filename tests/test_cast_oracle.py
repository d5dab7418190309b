"""The scan-casting oracle (tests/cast_oracle.py) against the analytic room and on cases built by hand, and
datasets.mapsim.make_log over a stub engine.  No GPU."""
import math

import numpy as np

from tests.cast_oracle import cast, lattice_bounds, room16_cells
from thesis_amd.datasets import synthetic

DIM, R, INV, Q, THR = 800, 3, 800 / 40.0, 0.1, 1.0
LO, HI = lattice_bounds(DIM, R)


def room_poses():
    return synthetic.circle_trajectory(40)[::8].tolist() + [[1.23, -2.2, 2.5], [-6.1, 6.3, -1.0]]


def one(cells, x0, y0, pose, angle, max_range=30.0, lo=LO, hi=HI, inv=INV):
    r, st, _ = cast(cells, x0, y0, lo, hi, inv, Q, THR, pose, [angle], max_range)
    return float(r[0]), int(st[0])


# ---- 1. the analytic room ----------------------------------------------------------------------------------------------------
def test_oracle_equals_the_analytic_room():
    cells, x0, y0 = room16_cells()
    angles = synthetic.beam_angles(1081)
    poses = room_poses()
    assert len(poses) == 8
    worst, steps = 0.0, 0
    for pose in poses:
        r, st, n = cast(cells, x0, y0, LO, HI, INV, Q, THR, pose, angles, 30.0)
        ref = synthetic.cast_scan(pose, angles, None)
        d = np.abs(r - ref)
        worst, steps = max(worst, float(d.max())), steps + n
        assert np.all(st == 1), (pose, np.bincount(st, minlength=3))
        assert np.all(d <= 1e-9), (pose, float(d.max()), int(np.count_nonzero(d > 1e-9)))   # every beam
    print(f"oracle vs analytic room: max |difference| {worst:.3g} m over {8 * 1081} beams, {steps / (8 * 1081):.0f} steps per ray")


# ---- 2. edge cases by construction -------------------------------------------------------------------------------------------
def grid(n=40, x0=-20):
    return np.zeros((n, n), np.int8), x0, x0


def cast_dir(monkeypatch, cells, x0, y0, origin, d, max_range=30.0):
    """One ray from `origin` (in cells: inv = 1) with the direction (dx, dy) = d exactly: no float64 angle has a cosine of
    0 or equal sine and cosine, so the oracle's libm is replaced by exact values (pose angle 0 -> (1, 0), beam -> d)."""
    import tests.cast_oracle as co

    class ExactTrig:
        inf, floor = math.inf, staticmethod(math.floor)
        cos = staticmethod(lambda a: 1.0 if a == 0.0 else d[0])
        sin = staticmethod(lambda a: 0.0 if a == 0.0 else d[1])
    monkeypatch.setattr(co, "math", ExactTrig)
    r, st, steps = co.cast(cells, x0, y0, LO, HI, 1.0, Q, THR, (origin[0], origin[1], 0.0), [1.0], max_range)
    return float(r[0]), int(st[0]), steps


def test_start_cell_occupied_is_range_zero():
    c, x0, y0 = grid()
    c[3 - x0, -2 - y0] = 11
    assert one(c, x0, y0, (3.5 / INV, -1.5 / INV, 0.7), 0.3) == (0.0, 1)


def test_rays_along_an_axis(monkeypatch):
    c, x0, y0 = grid()
    c[10 - x0, :] = 11                                   # walls: the faces met are x = 10, x = -4, y = 9, y = -6
    c[-5 - x0, :] = 11
    c[:, 9 - y0] = 11
    c[:, -7 - y0] = 11
    ox, oy = 2.25, 3.5                                   # exact in binary
    assert cast_dir(monkeypatch, c, x0, y0, (ox, oy), (1.0, 0.0)) == (10 - ox, 1, 8)      # dy == 0
    assert cast_dir(monkeypatch, c, x0, y0, (ox, oy), (-1.0, 0.0)) == (ox + 4, 1, 7)
    assert cast_dir(monkeypatch, c, x0, y0, (ox, oy), (0.0, 1.0)) == (9 - oy, 1, 6)       # dx == 0
    assert cast_dir(monkeypatch, c, x0, y0, (ox, oy), (0.0, -1.0)) == (oy + 6, 1, 10)
    # an origin ON a cell boundary with a zero component: f = 0 there, and 0 * inf must not be formed
    assert cast_dir(monkeypatch, c, x0, y0, (2.0, 3.0), (0.0, 1.0)) == (6.0, 1, 6)
    assert cast_dir(monkeypatch, c, x0, y0, (2.0, 3.0), (1.0, 0.0)) == (8.0, 1, 8)


def test_an_exact_tie_steps_in_y(monkeypatch):
    h = math.sqrt(0.5)
    c, x0, y0 = grid()
    c[1 - x0, 0 - y0] = 11                                # entered only if the tie stepped in x: 1 step
    c[1 - x0, 1 - y0] = 11                                # the walk (0,0) -> (0,1) -> (1,1): 2 steps, the same t
    r, st, steps = cast_dir(monkeypatch, c, x0, y0, (0.5, 0.5), (h, h))
    assert (st, steps) == (1, 2) and r == 0.5 * (1.0 / h)
    c[0 - x0, 1 - y0] = 11                                # and (0,1) itself is what a tie meets first
    assert cast_dir(monkeypatch, c, x0, y0, (0.5, 0.5), (h, h))[1:] == (1, 1)
    # from a cell corner the same holds for every later corner on the diagonal
    c2, _, _ = grid()
    c2[3 - x0, 2 - y0] = 11
    c2[3 - x0, 3 - y0] = 11
    assert cast_dir(monkeypatch, c2, x0, y0, (0.0, 0.0), (h, h))[1:] == (1, 6)            # (2,2) -> (2,3) -> (3,3)


def test_a_diagonal_gap_is_not_passed(monkeypatch):
    h = math.sqrt(0.5)
    c, x0, y0 = grid()
    c[5 - x0, 4 - y0] = 11                                # two cells that touch at the corner (5, 5) only
    c[4 - x0, 5 - y0] = 11
    c[15 - x0, :] = 11                                    # what a ray that slipped through would reach
    c[:, 15 - y0] = 11
    r, st, _ = cast_dir(monkeypatch, c, x0, y0, (3.0, 3.0), (h, h))                       # exactly through the corner
    assert st == 1 and r == 2.0 * (1.0 / h)               # stopped AT the corner, by the cell the y step enters
    for a in np.linspace(0.6, 1.0, 41):                   # a fan of libm directions around the diagonal
        r, st = one(c, x0, y0, (4.05, 4.05, 0.0), float(a), inv=1.0)
        assert st == 1 and r < 2.0, (a, r)


def test_status_0_short_of_a_wall_and_status_2_at_the_lattice_edge():
    c, x0, y0 = grid()
    c[10 - x0, :] = 11
    ox, oy = 2.25, 3.5
    d = (10 - ox) / INV                                   # distance to the wall's face
    assert one(c, x0, y0, (ox / INV, oy / INV, 0.0), 0.0, max_range=d + 1e-6) == (d, 1)
    assert one(c, x0, y0, (ox / INV, oy / INV, 0.0), 0.0, max_range=d - 1e-6) == (d - 1e-6, 0)
    # nothing in the way: the ray leaves the lattice (its last cell is HI - 1) before a long max_range runs out
    assert one(c, x0, y0, (ox / INV, oy / INV, 0.0), math.pi / 2, max_range=1000.0) == (1000.0, 2)
    assert one(c, x0, y0, (ox / INV, oy / INV, 0.0), math.pi / 2, max_range=50.0) == (50.0, 0)
    # an origin outside the lattice, however far, is status 2 at once
    assert one(c, x0, y0, (HI / INV + 0.01, 0.0, 0.0), math.pi) == (30.0, 2)
    assert one(c, x0, y0, (1e300, -1e300, 0.0), 0.0) == (30.0, 2)
    assert one(c, x0, y0, ((LO - 0.5) / INV, 0.0, 0.0), 0.0) == (30.0, 2)
    assert one(c, x0, y0, (LO / INV, 0.0, 0.0), 0.0, max_range=1.0) == (1.0, 0)     # the first lattice cell is inside


def test_threshold_is_strict_and_negative_cells_are_free():
    c, x0, y0 = grid()
    c[5 - x0, :] = 10                                     # exactly the threshold: free
    c[7 - x0, :] = -30
    c[9 - x0, :] = 11
    assert one(c, x0, y0, (0.5, 0.5, 0.0), 0.0, inv=1.0) == (8.5, 1)


# ---- 3. mapsim.make_log over a stub ------------------------------------------------------------------------------------------
class StubEngine:
    """cast_scans with the oracle behind it, in the exact room."""
    def __init__(self):
        self.cells, self.x0, self.y0 = room16_cells()
        self.calls = 0

    def cast_scans(self, poses, angles, particle=None, max_range=None):
        self.calls += 1
        mr = 25.0 if max_range is None else max_range
        return np.stack([cast(self.cells, self.x0, self.y0, LO, HI, INV, Q, THR, p, angles, mr)[0] for p in poses])


def test_mapsim_make_log_over_a_stub():
    from thesis_amd.datasets import mapsim
    e = StubEngine()
    poses = synthetic.circle_trajectory(6)
    ang = synthetic.beam_angles(61)
    a, r, odo, truth = mapsim.make_log(e, 0, poses, ang, period=0.1, seed=3, odo_seed=4, max_range=30.0)
    assert e.calls == 1                                   # one cast for the whole log
    assert a.shape == (61,) and r.shape == (7, 61) and odo.shape == (6, 3) and truth.shape == (7, 3)
    assert np.array_equal(truth, poses) and np.array_equal(a, ang)
    a2, r2, odo2, _ = mapsim.make_log(e, 0, poses, ang, period=0.1, seed=3, odo_seed=4, max_range=30.0)
    assert np.array_equal(r, r2) and np.array_equal(odo, odo2)        # seeds reproduce
    _, r3, odo3, _ = mapsim.make_log(e, 0, poses, ang, period=0.1, seed=5, odo_seed=6, max_range=30.0)
    assert not np.array_equal(r, r3) and not np.array_equal(odo, odo3)
    vel = np.diff(poses, axis=0) / 0.1
    nz = vel != 0
    assert np.all(np.abs(odo[nz] / vel[nz] - 1.0) < 0.06) and np.all(odo[~nz] == 0)   # 1 % noise: six sigma
    assert np.all(r >= 0)
    # noise off: the cast ranges themselves, which are the analytic room's
    _, r0, _, _ = mapsim.make_log(e, 0, poses, ang, noise_sigma=0.0, max_range=30.0)
    ref = np.stack([synthetic.cast_scan(p, ang, None) for p in poses])
    assert np.all(np.abs(r0 - ref) <= 1e-9)
    # the noise is synthetic.make_log's: one PCG64(seed) stream over the scans in order
    rng = np.random.Generator(np.random.PCG64(3))
    want = np.maximum(np.stack([r0[k] + rng.normal(0.0, 0.01, size=61) for k in range(7)]), 0.0)
    assert np.array_equal(r, want)
    # ranges are clipped at 0: a robot standing in a wall reads 0 everywhere, whatever the noise
    _, rw, _, _ = mapsim.make_log(e, 0, np.array([[8.5, 0.0, 0.0], [8.6, 0.0, 0.0]]), ang, max_range=30.0)
    assert np.all(rw >= 0) and np.any(rw == 0)
