"""Scenes of the scan-check tests (tests/test_scancheck_oracle.py on the CPU, tests/test_gpu_scancheck.py on the GPU): the exact
room with its interior known free, poses in and around it, and measured ranges built round the true ones so that every class
and both ends of the hit table are reached."""
import numpy as np

from tests.cast_oracle import cast, room16_cells

CELL = 0.05
INV = 20.0                   # cells per metre at 0.05 m: dim 800 / tile_len 40
QUANTUM, THRESHOLD = 0.1, 1.0
TOL = 2 * CELL               # check_scans' default
MAX_RANGE, MIN_RANGE = 6.0, 0.3
B_CASES = (1, 37, 64, 65, 271)
N_VARIANTS = 20


def known_room(patch=True):
    """(cells, x0, y0): room16_cells() with the interior at -30 (known free) and, with `patch`, one patch of it, 1 <= x < 3 m
    and -8 <= y < -3 m, left at 0 (unknown)."""
    cells, x0, y0 = room16_cells()
    cells = np.where(cells == 0, np.int8(-30), cells).astype(np.int8)
    if patch:
        cells[20 - x0:60 - x0, -160 - y0:-60 - y0] = 0
    return cells, x0, y0


BLOCKER_BOX = (-70, -50, 30, 36)         # a wall of 20 x 6 cells that only one particle's map holds (x -3.5 .. -2.5 m, y 1.5 .. 1.8 m)


def room_poses():
    from thesis_amd.datasets import synthetic
    return np.array(synthetic.circle_trajectory(40)[::8].tolist() + [[1.23, -2.2, 2.5], [-6.1, 6.3, -1.0]])


OUTSIDE_POSE = [1.0e6, -3.0, 0.4]        # its origin lies outside any lattice
WALL_POSE = [8.6, 0.33, 3.0]             # its origin cell is a wall cell


def all_poses():
    """room_poses() and the two special ones [10, 3]."""
    return np.array(room_poses().tolist() + [OUTSIDE_POSE, WALL_POSE])


def paired_poses():
    """Eight of them, the two special ones included: one per particle of the GPU test's engine."""
    return np.array(room_poses()[:6].tolist() + [OUTSIDE_POSE, WALL_POSE])


def true_ranges(cells, x0, y0, lo, hi, poses, angles):
    """[N, B]: the cast oracle's ranges to 30 m, the room's own size whatever the check's max_range."""
    return np.stack([cast(cells, x0, y0, lo, hi, INV, QUANTUM, THRESHOLD, q, angles, 30.0)[0] for q in poses])


def measured_ranges(e, tol=TOL, max_range=MAX_RANGE, min_range=MIN_RANGE):
    """[N, B] built from the true ranges e: variant (b + 3 n) % 20 of
         0 .. 8    e + k tol / 2, k = -4 .. 4
         9 .. 12   nextafter either side of e - tol and of e + tol
         13 .. 18  0, -1, NaN, +inf, -inf, max_range itself
         19        half of min_range
    and, where there are 64 beams or more, a block of 40 consecutive beams shortened by 1.5 m."""
    N, B = e.shape
    var = (np.arange(B)[None, :] + 3 * np.arange(N)[:, None]) % N_VARIANTS
    z = np.empty_like(e)
    for k in range(-4, 5):
        z = np.where(var == k + 4, e + k * tol / 2, z)
    for v, (base, to) in enumerate([(e - tol, -np.inf), (e - tol, np.inf), (e + tol, -np.inf), (e + tol, np.inf)]):
        z = np.where(var == 9 + v, np.nextafter(base, to), z)
    for v, val in enumerate([0.0, -1.0, np.nan, np.inf, -np.inf, max_range, 0.5 * min_range]):
        z = np.where(var == 13 + v, val, z)
    if B >= 64:
        z[:, B // 3:B // 3 + 40] = e[:, B // 3:B // 3 + 40] - 1.5
    return z


def narrow_model():
    """A beam model whose hit table ends inside the tolerance (half_bins 7 < tol * bins_per_cell = 8), so that MATCH beams are
    clamped at both of its ends."""
    from thesis_amd import sensor

    class Cfg:
        cell_size, weight_max_range = CELL, 25.0
    return sensor.beam_model(Cfg, sigma_hit=0.02)
