"""Rollout templates on the CPU (thesis_amd/plan.py: arc_templates, place_templates; the placement rule of rbpf_check_rollouts in
include/rbpf_hip.h): the templates against `rollouts`, the placement against a scalar model in plain Python floats, how far the
two ways to an arc differ, and the seeded fuzz inputs of tests/test_gpu_rollouts.py judged by tests/paths_oracle.py alone."""
import math

import numpy as np
import pytest

from tests import paths_oracle as PO
from tests import travel_oracle as T
from thesis_amd import plan

SETTINGS = ((0, 1), (7, 8), (20, 21), (20, 320))         # (inflate, clear_max), as tests/test_gpu_paths.py
SPEEDS, TURNS = np.repeat([0.2, 0.4], 8), np.tile(np.linspace(-1.5, 1.5, 8), 2)


def fuzz_inputs(inv, origin):
    """(poses [64, 3], templates [16, 5, 2]) of the seeded fuzz: each pose's cell in [20, 180) x [20, 130) of the fuzz scene whose
    cell (0, 0) is mosaic cell `origin`, 0.05 .. 0.95 of a cell inside it, any heading; sixteen arcs of two seconds."""
    rng = np.random.default_rng(5)
    cell = np.stack([rng.integers(20, 180, size=64), rng.integers(20, 130, size=64)], axis=1) + np.asarray(origin)
    xy = (cell + rng.uniform(0.05, 0.95, size=(64, 2))) / float(inv)
    poses = np.concatenate([xy, rng.uniform(-np.pi, np.pi, size=(64, 1))], axis=1)
    return poses, plan.arc_templates(SPEEDS, TURNS, 2.0, 0.5)


def place_scalar(pose, lx, ly):
    """The rule in Python floats, one rounded operation after another."""
    x, y, th = (float(q) for q in pose)
    c, s = math.cos(th), math.sin(th)
    a, b = c * lx, s * ly
    d, e = s * lx, c * ly
    return x + (a - b), y + (d + e)


def test_arc_templates_are_the_rollouts_of_the_zero_pose():
    tm = plan.arc_templates(SPEEDS, TURNS, 2.0, 0.5)
    assert tm.shape == (16, 5, 2) and tm.dtype == np.float64
    assert tm.tobytes() == plan.rollouts(np.zeros(3), SPEEDS, TURNS, 2.0, 0.5).tobytes()
    assert np.all(tm[:, 0] == 0.0) and tm[:, -1, 0].max() > 0.7


def test_place_templates_is_the_scalar_rule():
    rng = np.random.default_rng(17)
    poses = np.concatenate([rng.uniform(-900.0, 900.0, size=(40, 2)), rng.uniform(-np.pi, np.pi, size=(40, 1))], axis=1)
    poses[:4, 2] = [0.0, np.pi / 2, -np.pi, 2.3]
    tm = np.concatenate([plan.arc_templates(SPEEDS, TURNS, 3.0, 0.25), np.zeros((16, 13, 1))], axis=-1)      # a third column is ignored
    got = plan.place_templates(poses, tm)
    assert got.shape == (40, 16, 13, 2)
    for n in range(40):
        for k in range(0, 16, 3):
            for j in range(13):
                want = place_scalar(poses[n], float(tm[k, j, 0]), float(tm[k, j, 1]))
                assert (float(got[n, k, j, 0]), float(got[n, k, j, 1])) == want, (n, k, j)
    assert plan.place_templates(poses[7], tm).tobytes() == got[7].tobytes()
    assert plan.place_templates(np.zeros(3), tm).tobytes() == np.ascontiguousarray(tm[..., :2]).tobytes()      # cos 0 = 1, sin 0 = 0: exact
    for bad in (lambda: plan.place_templates(np.zeros((2, 4)), tm), lambda: plan.place_templates(poses, tm[0]), lambda: plan.place_templates(poses, tm[..., :1])):
        with pytest.raises(ValueError):
            bad()


def test_placed_templates_and_rollouts_agree_to_rounding():
    """rollouts adds the heading inside the cosine, place_templates rotates a finished template: the same arc up to rounding.  Below
    1000 m a coordinate's ulp is 1.2e-13 m and a template of a few metres carries a few 1e-16 relative: 1e-9 m is far outside it."""
    rng = np.random.default_rng(23)
    poses = np.concatenate([rng.uniform(-999.0, 999.0, size=(200, 2)), rng.uniform(-np.pi, np.pi, size=(200, 1))], axis=1)
    a = plan.place_templates(poses, plan.arc_templates(SPEEDS, TURNS, 3.0, 0.25))
    b = plan.rollouts(poses, SPEEDS, TURNS, 3.0, 0.25)
    assert a.shape == b.shape == (200, 16, 13, 2)
    worst = float(np.abs(a - b).max())
    print(f"placed templates against rollouts: largest difference {worst:.3e} m")
    assert worst <= 1e-9
    assert not np.array_equal(a, b)                      # and only to rounding: the placement rule is the specification


def test_the_fuzz_inputs_block_a_fair_share_on_the_oracle_alone():
    """The shares the GPU fuzz asserts, found here without a GPU: the scene as its own raster, unknown round it."""
    inv, c = 20.0, PO.fuzz_scene()
    poses, tm = fuzz_inputs(inv, (0, 0))
    paths = list(plan.place_templates(poses, tm).reshape(-1, 5, 2))
    cells = np.concatenate([T.cells_of(p, inv) for p in paths])
    assert cells.min() >= 0 and cells[:, 0].max() < c.shape[0] and cells[:, 1].max() < c.shape[1]
    box = (0, c.shape[0], 0, c.shape[1])
    shares = []
    for exempt in (False, True):
        for inflate, clear_max in SETTINGS:
            m = T.margin(clear_max)
            f = PO.Field(np.pad(c, m), box, 0.1, 1.0, inflate, clear_max)        # walls 30, free -30: any threshold between serves
            res, steps = f.check_xy(paths, inv, exempt)
            shares.append(float((res[:, 0] >= 0).mean()))
            unknown = float((res[:, 1] >= 0).mean())
            assert len(res) == 64 * 16 and steps.min() >= 1
    print("blocked shares", [f"{s:.2f}" for s in shares], f"unknown on {unknown:.2f} of the paths")
    assert all(0.1 <= s <= 0.9 for s in shares), shares
    assert unknown >= 0.05
