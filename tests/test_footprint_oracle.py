"""Footprint checks on the CPU: the helpers of thesis_amd/plan.py that go with ParticleEngine.check_footprints (heading bins,
arc and path headings, the span table of an outline) and the scalar oracle of tests/footprint_oracle.py, held to itself by
properties: a one-cell footprint is the path oracle, a chamfer disc is the clearance, a quarter turn transposes a rectangle, the
padded table covers the true outline, and the seeded fuzz inputs of tests/test_gpu_footprints.py block a fair share."""
import math

import numpy as np
import pytest

from tests import footprint_oracle as FO
from tests import paths_oracle as PO
from tests import travel_oracle as T
from thesis_amd import plan

CELL, INV = 0.05, 20.0
SPEEDS, TURNS = np.repeat([0.2, 0.4], 8), np.tile(np.linspace(-1.5, 1.5, 8), 2)
# (inflate, clear_max, through_unknown, exempt) of the fuzz, here and on the GPU
FUZZ_SETTINGS = ((0, 1, False, -1), (7, 8, False, -1), (20, 21, False, -1), (20, 320, False, -1), (0, 1, True, -1), (7, 8, False, 3), (0, 1, True, 0))


def rectangle(length, width):
    a, b = length / 2.0, width / 2.0
    return np.array([[a, b], [-a, b], [-a, -b], [a, -b]])


def fuzz_table():
    """A rectangle of 9 x 5 cells in 32 bins, unpadded: its bin 0 is the cells -4 .. 4 by -2 .. 2."""
    return plan.footprint_table(rectangle(9 * CELL, 5 * CELL), CELL, 32, pad_m=0.0)


def fuzz_inputs(inv, origin, seed=8):
    """(poses [25, 3], templates [16, 5, 2], headings [16, 5]) of the seeded fuzz, 400 rollouts: each pose's cell in
    [20, 180) x [20, 130) of the fuzz scene whose cell (0, 0) is mosaic cell `origin`, 0.05 .. 0.95 of a cell inside it, any
    heading; sixteen arcs of one second and their headings."""
    rng = np.random.default_rng(seed)
    cell = np.stack([rng.integers(20, 180, size=25), rng.integers(20, 130, size=25)], axis=1) + np.asarray(origin)
    xy = (cell + rng.uniform(0.05, 0.95, size=(25, 2))) / float(inv)
    poses = np.concatenate([xy, rng.uniform(-np.pi, np.pi, size=(25, 1))], axis=1)
    return poses, plan.arc_templates(SPEEDS, TURNS, 1.0, 0.25), plan.arc_headings(TURNS, 1.0, 0.25)


def scene_field(fp, inflate, clear_max, through=False, box=None):
    """The oracle's field over the whole fuzz scene as its own raster, unknown round it."""
    c = PO.fuzz_scene()
    box = box or (0, c.shape[0], 0, c.shape[1])
    g = FO.grow(clear_max, FO.table_reach(fp))
    wide = np.zeros((box[1] - box[0] + 2 * g, box[3] - box[2] + 2 * g), np.int8)
    wide[g - box[0]:g - box[0] + c.shape[0], g - box[2]:g - box[2] + c.shape[1]] = c
    return FO.Field(wide, box, 0.1, 1.0, inflate, clear_max, fp, through)      # walls 30, free -30: any threshold between serves


# ---- the helpers of plan.py ---------------------------------------------------------------------------------------------------------
def test_heading_bins_follow_the_rule():
    H = 8
    step = 2 * math.pi / H
    assert plan.heading_bins([0.0, step, -step, 7 * step, 8 * step, -8 * step, 2 * math.pi, -2 * math.pi, 100 * math.pi], H).tolist() == [0, 1, 7, 7, 0, 0, 0, 0, 0]
    assert plan.heading_bins([0.49 * step, 0.51 * step, -0.49 * step, -0.51 * step, 7.51 * step], H).tolist() == [0, 1, 0, 7, 0]
    assert plan.heading_bins(np.float64(0.5) * (2 * math.pi / 4), 4).tolist() == 1      # the half-bin point goes up: floor(0.5 + 0.5)
    assert plan.heading_bins(-np.float64(0.5) * (2 * math.pi / 4), 4).tolist() == 0     # and so does the negative one: floor(-0.5 + 0.5)
    assert plan.heading_bins(np.linspace(-50, 50, 1001), 1).tolist() == [0] * 1001
    b = plan.heading_bins(np.random.default_rng(1).uniform(-20, 20, size=(5, 7)), 256)
    assert b.shape == (5, 7) and b.dtype == np.int32 and b.min() >= 0 and b.max() <= 255
    for bad in (lambda: plan.heading_bins([0.0], 0), lambda: plan.heading_bins([0.0], 257), lambda: plan.heading_bins([np.nan], 8), lambda: plan.heading_bins([1e10], 8)):
        with pytest.raises(ValueError):
            bad()


def test_arc_and_path_headings():
    hd = plan.arc_headings(TURNS, 2.0, 0.5)
    tm = plan.arc_templates(SPEEDS, TURNS, 2.0, 0.5)
    assert hd.shape == tm.shape[:2] and np.all(hd[:, 0] == 0.0) and np.allclose(hd[:, -1], TURNS * 2.0)
    k = 3                                                                  # the heading of an arc is twice the direction of its chord
    assert np.allclose(np.arctan2(tm[k, 1:, 1], tm[k, 1:, 0]) * 2.0, hd[k, 1:])
    path = np.array([[0, 0], [1, 0], [1, 0], [1, 2], [0, 2.0]])
    assert np.allclose(plan.path_headings(path), [0.0, 0.0, math.pi / 2, math.pi, math.pi])
    assert plan.path_headings([[3.0, 4.0]]).tolist() == [0.0] and plan.path_headings([[0, 0], [0, 0], [0, -1.0]]).tolist() == [0.0, -math.pi / 2, -math.pi / 2]
    with pytest.raises(ValueError):
        plan.path_headings(np.zeros((0, 2)))


def test_footprint_table_shapes_spans_and_limits():
    fp = fuzz_table()
    assert fp.H == 32 and fp.offsets.shape == (33,) and fp.offsets[0] == 0 and fp.offsets[-1] == len(fp.spans) and fp.spans.dtype == np.int32
    assert sorted(map(tuple, plan.footprint_cells(fp, 0).tolist())) == [(i, j) for i in range(-4, 5) for j in range(-2, 3)]
    assert fp.spans[:5].tolist() == [[i, -2, 2] for i in range(-4, 1)]
    wide = plan.footprint_table(rectangle(0.21, 5.04), CELL, 4, pad_m=0.0)       # rows of 101 cells: spans of 64 and 37
    rows = wide.spans[wide.offsets[0]:wide.offsets[1]]
    assert sorted(set((int(r[2]) - int(r[1]) + 1) for r in rows)) == [37, 64] and len(plan.footprint_cells(wide, 0)) == 5 * 101
    padded = plan.footprint_table(rectangle(0.8, 0.5), CELL, 64)
    assert all(len(plan.footprint_cells(padded, b)) > 16 * 10 for b in range(64)) and np.abs(padded.spans).max() <= 14
    with pytest.raises(ValueError, match="127 cells"):
        plan.footprint_table(rectangle(13.0, 0.5), CELL, 8)
    with pytest.raises(ValueError, match="256 spans"):
        plan.footprint_table(rectangle(12.04, 12.04), CELL, 2, pad_m=0.0)      # 241 rows of 241 cells: four spans a row
    for bad in (lambda: plan.footprint_table(rectangle(1, 1)[:2], CELL), lambda: plan.footprint_table(rectangle(1, 1), 0.0), lambda: plan.footprint_table(rectangle(1, 1), CELL, 257)):
        with pytest.raises(ValueError):
            bad()


# ---- the oracle, held to itself ---------------------------------------------------------------------------------------------------------
def test_a_single_cell_footprint_is_the_path_oracle():
    one = plan.Footprint(np.array([[0, 0, 0]], np.int32), np.array([0, 1], np.int32), 1, CELL)
    poses, tm, hd = fuzz_inputs(INV, (0, 0))
    rolls = FO.rollout_cells(poses, tm, hd, 1, INV)
    c = PO.fuzz_scene()
    for inflate, clear_max, through, exempt in FUZZ_SETTINGS[:5]:
        res, steps = FO.check_all(scene_field(one, inflate, clear_max, through), rolls)
        f = PO.Field(np.pad(c, T.margin(clear_max)), (0, c.shape[0], 0, c.shape[1]), 0.1, 1.0, inflate, clear_max, through)
        want, wsteps = f.check_xy(list(plan.place_templates(poses, tm).reshape(-1, 5, 2)), INV)
        assert np.array_equal(res.reshape(-1, 4)[:, 1:], want[:, 1:]) and np.array_equal(steps.reshape(-1), wsteps)
        late = lambda a: np.where(a < 0, 1 << 30, a)
        assert np.all(late(res.reshape(-1, 4)[:, 0]) >= late(want[:, 0]))      # no corner rule here: never sooner than the path's


def test_a_chamfer_disc_is_the_clearance():
    r = 17
    cells = [(dx, dy) for dx in range(-4, 5) for dy in range(-4, 5) if 5 * max(abs(dx), abs(dy)) + 2 * min(abs(dx), abs(dy)) <= r]
    spans = []
    for dx in sorted(set(c[0] for c in cells)):
        ys = [c[1] for c in cells if c[0] == dx]
        spans.append((dx, min(ys), max(ys)))                                # a disc's rows are whole
    H = 3
    fp = plan.Footprint(np.array(spans * H, np.int32), np.arange(H + 1, dtype=np.int32) * len(spans), H, CELL)
    f = scene_field(fp, 0, 40, through=True)
    rng = np.random.default_rng(4)
    hit = 0
    for x, y in zip(rng.integers(0, 200, 600), rng.integers(0, 150, 600)):
        got = f.check([(x, y)], [int(rng.integers(0, H))])
        assert (got[0] == 0) == (f.clear[x, y] <= r) and got[4] == 1
        hit += got[0] == 0
    assert 60 < hit < 540


def test_a_quarter_turn_transposes_a_rectangle():
    for fp in (fuzz_table(), plan.footprint_table(rectangle(0.8, 0.5), CELL, 64)):
        a = set(map(tuple, plan.footprint_cells(fp, 0).tolist()))
        b = set(map(tuple, plan.footprint_cells(fp, fp.H // 4).tolist()))
        assert b == {(y, x) for x, y in a} and a != b
        assert set(map(tuple, plan.footprint_cells(fp, fp.H // 2).tolist())) == a


def test_the_padded_table_covers_the_true_outline():
    """1000 seeded (place in the cell, pose heading, waypoint heading): every point of the true outline, and of its inside, lies in
    a cell of the bin the call would test."""
    rng = np.random.default_rng(12)
    for poly, H in ((rectangle(0.8, 0.5), 64), (np.array([[0.5, 0.0], [-0.2, 0.3], [-0.1, 0.0], [-0.2, -0.3]]), 32)):
        fp = plan.footprint_table(poly, CELL, H)
        have = [set(map(tuple, plan.footprint_cells(fp, b).tolist())) for b in range(H)]
        edge = np.concatenate([np.linspace(p, q, 40) for p, q in zip(poly, np.roll(poly, -1, axis=0))])
        pts = np.concatenate([edge, edge * 0.5, edge * 0.05])
        for _ in range(500):
            e = rng.uniform(-0.5, 0.5, 2) * CELL
            th, ph = rng.uniform(-7.0, 7.0), rng.uniform(-3.2, 3.2)
            b = (int(plan.heading_bins(th, H)) + int(plan.heading_bins(ph, H))) % H
            c, s = math.cos(th + ph), math.sin(th + ph)
            q = np.stack([c * pts[:, 0] - s * pts[:, 1], s * pts[:, 0] + c * pts[:, 1]], axis=1) + e
            cells = set(map(tuple, np.floor(q / CELL + 0.5).astype(np.int64).tolist()))
            assert cells <= have[b], (th, ph, sorted(cells - have[b])[:3])


def test_bins_of_a_walk():
    w = FO.walk_bins([(0, 0), (0, 0), (4, 1), (4, 1), (4, 1), (7, 1), (7, 2)], [1, 2, 3, 4, 5, 6, 7])
    assert [c for c, _ in w] == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (7, 2)]
    assert [b for _, b in w] == [[1, 2], [2], [3], [3], [3, 4, 5], [5], [6], [6], [7]]      # 2 t < n: t = 1 of 4; t = 1 of 3


def test_the_fuzz_inputs_block_a_fair_share_on_the_oracle_alone():
    fp = fuzz_table()
    poses, tm, hd = fuzz_inputs(INV, (0, 0))
    rolls = FO.rollout_cells(poses, tm, hd, fp.H, INV)
    shares = []
    for inflate, clear_max, through, exempt in FUZZ_SETTINGS:
        res, steps = FO.check_all(scene_field(fp, inflate, clear_max, through), rolls, exempt)
        assert res.shape == (25, 16, 4) and steps.shape == (25, 16) and steps.min() >= 1      # all 400, none left out
        shares.append(float((res[..., 0] >= 0).mean()))
    print("blocked shares", [f"{s:.2f}" for s in shares])
    assert all(0.1 <= s <= 0.9 for s in shares), shares
