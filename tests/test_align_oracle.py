"""The alignment oracle (tests/align_oracle.py) against itself, and the host side of an alignment (thesis_amd/align.py): no GPU."""
import math

import numpy as np
import pytest

from tests import align_oracle as ao
from tests import place_oracle as po
from tests.locate_oracle import asym_room
from thesis_amd import align
from thesis_amd.mapio import SourceMap

INV, Q, THR = 10.0, 0.1, 1.0


@pytest.fixture(scope="module")
def room():
    return asym_room(0.1)


def points(seed, n_occ, n_free, reach=6.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-reach, reach, (n_occ, 2)), rng.uniform(-reach, reach, (n_free, 2))


def test_align_equals_align_scalar_and_align_fft(room):
    cells, x0, y0 = room
    occ, free = points(1, 40, 55)
    box = (-30, -12, 25, 58)
    for n_rot, wnd in ((12, (0, 12)), (90, (31, 7))):
        best, rot = ao.align(cells, x0, y0, box, occ, free, n_rot, *wnd, INV, Q, THR)
        assert best.dtype == np.int32 and best.shape == (18, 33) and best.max() > 0
        assert not np.array_equal(best, ao.align(cells, x0, y0, box, occ, None, n_rot, *wnd, INV, Q, THR)[0])      # clashes count
        for X, Y in ((-30, 25), (-13, 57), (-21, 40), (-17, 31)):
            assert ao.align_scalar(cells, x0, y0, X, Y, occ, free, n_rot, *wnd, INV, Q, THR) == (best[X - box[0], Y - box[2]], rot[X - box[0], Y - box[2]])
        fb, fr = ao.align_fft(cells, x0, y0, box, occ, free, n_rot, *wnd, INV, Q, THR)
        assert np.array_equal(fb, best) and np.array_equal(fr, rot)
    # no free points; a box that leaves the raster
    b1 = ao.align(cells, x0, y0, (90, 110, -5, 5), occ, None, 5, 0, 5, INV, Q, THR)
    b2 = ao.align_fft(cells, x0, y0, (90, 110, -5, 5), occ, np.zeros((0, 2)), 5, 0, 5, INV, Q, THR)
    assert np.array_equal(b1[0], b2[0]) and np.array_equal(b1[1], b2[1]) and b1[0].min() >= 0


def test_translation_invariance(room):
    cells, x0, y0 = room
    occ, free = points(2, 30, 30)
    box, (dx, dy) = (-20, 5, 10, 45), (7, -13)
    a = ao.align(cells, x0, y0, box, occ, free, 16, 2, 9, INV, Q, THR)
    b = ao.align(cells, x0 + dx, y0 + dy, (box[0] + dx, box[1] + dx, box[2] + dy, box[3] + dy), occ, free, 16, 2, 9, INV, Q, THR)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_window_is_a_cut_of_the_full_turn(room):
    cells, x0, y0 = room
    occ, free = points(3, 25, 10)
    box = (40, 50, 40, 50)
    parts = [ao.align(cells, x0, y0, box, occ, free, 24, rb, rc, INV, Q, THR) for rb, rc in ((0, 10), (10, 14))]
    full = ao.align(cells, x0, y0, box, occ, free, 24, 0, 24, INV, Q, THR)
    first = parts[0][0] >= parts[1][0]                   # on a tie the smaller rotation
    assert np.array_equal(full[0], np.maximum(parts[0][0], parts[1][0]))
    assert np.array_equal(full[1], np.where(first, parts[0][1], parts[1][1]))


def test_thinning_is_deterministic_and_respects_the_cap():
    rng = np.random.Generator(np.random.PCG64(4))
    cells = rng.choice(np.array([-30, 0, 30], dtype=np.int8), size=(60, 47), p=(0.5, 0.3, 0.2))
    src = SourceMap(cells=cells, cell_size=0.08, quantum=Q)
    n_occ, n_free = int((cells > 10).sum()), int((cells < 0).sum())
    occ, free, anchor = align.points_from_source(src, THR)
    assert (len(occ), len(free)) == (n_occ, n_free) and anchor == (60 * 0.08 / 2, 47 * 0.08 / 2)
    i, j = np.nonzero(cells > 10)                         # row-major
    assert np.array_equal(occ, np.stack([(i + 0.5) * 0.08 - anchor[0], (j + 0.5) * 0.08 - anchor[1]], axis=1))
    for cap in (n_occ + n_free - 1, n_occ + 100, n_occ, n_occ - 1, 100, 1):
        o, f, _ = align.points_from_source(src, THR, max_points=cap)
        o2, f2, _ = align.points_from_source(src, THR, max_points=cap)
        assert np.array_equal(o, o2) and np.array_equal(f, f2) and len(o) + len(f) <= cap and len(o) >= 1
        if cap >= n_occ:
            assert np.array_equal(o, occ)                # the occupied points are kept whole when they fit
            step = -(-n_free // max(cap - n_occ, 1))
            assert np.array_equal(f, free[::step] if cap > n_occ else free[:0])
        else:
            assert np.array_equal(o, occ[::-(-n_occ // cap)]) and len(f) <= cap - len(o)
    with pytest.raises(ValueError):
        align.points_from_source(src, THR, max_points=32768)


def test_pose_of_round_trips_a_known_transform():
    """A source whose frame is moved by a pose that sits exactly on a cell centre and a rotation step: the anchor lands on the
    cell centre, and src.moved(pose_of(...)) is the source in the engine's frame."""
    cs, n_rot, rot, cell = 0.1, 2880, 275, (17, -42)
    src = SourceMap(cells=np.zeros((50, 30), np.int8), cell_size=0.08, origin=(1.25, -0.5, 0.3), quantum=Q)
    _, _, anchor = align.points_from_source(SourceMap(cells=np.full((50, 30), 30, np.int8), cell_size=0.08, quantum=Q), THR)
    assert anchor == (2.0, 1.2)
    pose = align.pose_of(cell, rot, n_rot, cs, anchor, src.origin)
    ox, oy, yaw = src.moved(pose).origin
    th = rot * 2 * math.pi / n_rot
    assert abs(yaw - th) < 1e-12
    for q in ((0.0, 0.0), anchor, (4.0, 2.4), (1.0, 0.3)):   # raster-frame points: R(theta)(q - a) + C
        want = (math.cos(th) * (q[0] - anchor[0]) - math.sin(th) * (q[1] - anchor[1]) + (cell[0] + 0.5) * cs,
                math.sin(th) * (q[0] - anchor[0]) + math.cos(th) * (q[1] - anchor[1]) + (cell[1] + 0.5) * cs)
        got = (ox + math.cos(yaw) * q[0] - math.sin(yaw) * q[1], oy + math.sin(yaw) * q[0] + math.cos(yaw) * q[1])
        assert math.hypot(got[0] - want[0], got[1] - want[1]) < 1e-12
    # through the search: a small asymmetric map resampled into a moved frame is found again
    world = np.zeros((60, 60), np.int8)
    world[5:55, 5:55] = -30
    world[5:55, 5] = world[5:55, 54] = world[5, 5:55] = world[54, 5:55] = 30
    world[20:26, 30:44] = 30
    world[40:44, 12:15] = 30
    true = (0.9, 1.3, 70 * 2 * math.pi / 720)
    origin = (-3.2, -2.4)
    cells, _ = po.resample(world, cs, (0.0, 0.0, 0.0), (80, 80), 0.08, align.compose(true, (origin[0], origin[1], 0.0)), 3)
    part = SourceMap(cells=cells, cell_size=0.08, origin=(origin[0], origin[1], 0.0), quantum=Q)

    def search(occ, free, box, nr, rb, rc):
        return ao.align_fft(world, 0, 0, box, occ, free, nr, rb, rc, INV, Q, THR)
    hyp = align.align_map(search, part, THR, cs, (0, 60, 0, 60), (-600, 600), k=2, n_rot=90, refine=8)
    _, _, a = align.points_from_source(part, THR)
    aw = (origin[0] + a[0], origin[1] + a[1], 0.0)
    rec, tru = align.compose(hyp.poses[0], aw), align.compose(true, aw)
    assert math.hypot(rec[0] - tru[0], rec[1] - tru[1]) <= cs * math.sqrt(2) / 2 + 0.08 and abs(hyp.poses[0][2] - true[2]) <= 2 * math.pi / 90
    assert hyp.scores[0] == hyp.scores.max() and hyp.n_used == int((cells > 10).sum())


def test_refine_window_wraps_past_zero():
    calls = []

    def search(occ, free, box, nr, rb, rc):
        calls.append((box, nr, rb, rc))
        best = np.zeros((box[1] - box[0], box[3] - box[2]), np.int32)
        return best, np.full(best.shape, rb, np.int32)
    assert align.refine_hypothesis(search, None, None, (10, 20, 0), 360, 8, (-50, 50)) == (8, 18, 0, 0)
    assert calls == [((8, 13, 18, 23), 2880, 0, 9), ((8, 13, 18, 23), 2880, 2872, 8)]
    calls.clear()
    align.refine_hypothesis(search, None, None, (49, -50, 359), 360, 8, (-50, 50))
    assert calls == [((47, 50, -50, -47), 2880, 0, 1), ((47, 50, -50, -47), 2880, 2864, 16)]
    calls.clear()
    align.refine_hypothesis(search, None, None, (0, 0, 100), 360, 8, (-50, 50))
    assert calls == [((-2, 3, -2, 3), 2880, 792, 17)]
