"""thesis_amd/refine.py and rebuild.rebuild_at on the host, on a stand-in engine whose refine_poses, build_map and place_map are
the oracles: chunking, the `particle` modes, the bookkeeping of the rounds, follow() feeding each result forward, and fraction()
where no beam was used."""
import math

import numpy as np
import pytest

from tests.build_oracle import build_map as oracle_build
from tests.refine_oracle import refine as oracle_refine
from tests.test_rebuild import LoggedEngine
from thesis_amd import rebuild, refine
from thesis_amd.engine import ParticleEngine, RefineResult

STEP = math.radians(0.25)


def result(n6, poses=None, scores=None):
    n6 = np.asarray(n6, np.int32).reshape(-1, 6)
    poses = np.zeros((len(n6), 3)) if poses is None else poses
    return RefineResult(poses, n6[:, 0:3], n6[:, 3], n6[:, 4], n6[:, 5], scores, 4, STEP, 0.05)


def test_fraction_and_moved():
    res = result([[0, 0, 0, 10, 10, 8], [1, 0, 0, 6, 2, 4], [0, 0, 0, 0, 0, 0], [0, 0, -2, 7, 7, 20]])
    assert refine.fraction(res).tolist() == [10 / 16, 6 / 8, 0.0, 7 / 40]                 # n_used = 0 gives 0, not a NaN
    assert refine.moved(res).tolist() == [1, 3]
    assert refine.moved(result([[0, 0, 0, 1, 1, 1]])).tolist() == []


class MapEngine:
    """One particle whose map is what place_map was given; refine_poses is the oracle on it."""

    class cfg:
        quantum, occupied_threshold, match_min_range, match_max_range, cell_size, tile_len_m = 0.1, 1.0, 0.1, 2.0, 0.1, 40

    dim = 400

    def __init__(self):
        self.calls, self.placed, self.closed = [], 0, False
        self.cells, self.x0, self.y0 = np.zeros((1, 1), np.int8), 0, 0

    def weights(self):
        return np.array([1.0])

    def place_map(self, src, particle=None):
        assert particle == 0 and src.cell_size == self.cfg.cell_size and src.origin[2] == 0.0
        self.cells = np.array(src.cells)
        self.x0, self.y0 = int(round(src.origin[0] / src.cell_size)), int(round(src.origin[1] / src.cell_size))
        self.placed += 1

    def refine_poses(self, poses, ranges, angles, particle="best", substeps=4, window=12, rotations=10, rot_step=STEP,
                     min_range=None, max_range=None):
        ps = np.asarray(poses, np.float64).reshape(-1, 3)
        rg = np.asarray(ranges, np.float64).reshape(len(ps), -1)
        self.calls.append((len(ps), particle, ps.copy()))
        c = self.cfg
        lo, hi = c.match_min_range if min_range is None else min_range, c.match_max_range if max_range is None else max_range
        out, n6, _ = oracle_refine(self.cells, self.x0, self.y0, ps, rg, angles, self.dim / float(c.tile_len_m), c.quantum,
                                   c.occupied_threshold, lo, hi, substeps, window, rotations, rot_step)
        return RefineResult(out, n6[:, 0:3], n6[:, 3], n6[:, 4], n6[:, 5], None, substeps, rot_step, c.cell_size)

    def close(self):
        self.closed = True


def wall_room():
    """A 4 m square of walls at 0.1 m, and what a sensor sees of it: the distance to the walls along each beam."""
    cells = np.zeros((60, 60), np.int8)                  # cells -30 .. 29 on both axes
    cells[10:51, 10] = cells[10:51, 50] = cells[10, 10:51] = cells[50, 10:51] = 30     # wall cells -20 and 20: faces at -2.0 and 2.1 m
    return cells, -30, -30


def see(pose, angles):
    """Ranges to the inner faces of wall_room from `pose`, exact geometry."""
    x, y, th = pose
    out = []
    for a in angles:
        dx, dy = math.cos(th + a), math.sin(th + a)
        t = [((2.0 if d > 0 else -1.9) - p) / d for p, d in ((x, dx), (y, dy)) if abs(d) > 1e-12]
        out.append(min(q for q in t if q > 0) + 0.05)    # to the middle of the wall cell
    return np.array(out)


def test_follow_feeds_each_result_forward():
    cells, x0, y0 = wall_room()
    e = MapEngine()
    e.cells, e.x0, e.y0 = cells, x0, y0
    ang = np.linspace(-math.pi, math.pi, 48, endpoint=False)
    truth = np.array([[0.1 + 0.04 * t, -0.2 + 0.03 * t, 0.3 + 0.01 * t] for t in range(5)])
    scans = np.stack([see(p, ang) for p in truth])
    search = dict(substeps=2, window=3, rotations=2, rot_step=0.01, max_range=3.5)
    path, frac = refine.follow(e, scans, ang, truth[0] + [0.05, -0.05, 0.01], **search)
    assert path.shape == (5, 3) and frac.shape == (5,) and np.all(frac > 0.5)
    assert [c[0] for c in e.calls] == [1] * 5 and all(c[1] == 0 for c in e.calls)          # "best" resolved once, to an index
    for t in range(1, 5):
        assert e.calls[t][2].tobytes() == path[t - 1:t].tobytes()                          # scan t starts where scan t - 1 ended
    pose, want = truth[0] + [0.05, -0.05, 0.01], []
    for r in scans:                                      # the same loop over the oracle
        pose = oracle_refine(cells, x0, y0, [pose], r[None], ang, 10.0, 0.1, 1.0, 0.1, 3.5, 2, 3, 2, 0.01)[0][0]
        want.append(pose)
    assert path.tobytes() == np.array(want).tobytes()
    assert np.abs(path[-1, :2] - truth[-1, :2]).max() < np.abs(truth[0, :2] + [0.05, -0.05] - truth[-1, :2]).max()
    with pytest.raises(ValueError):
        refine.follow(e, scans, ang, truth[0], device=True)
    with pytest.raises(ValueError):
        refine.follow(e, scans[0], ang, truth[0])


class RunEngine(LoggedEngine):
    """LoggedEngine (tests/test_rebuild.py: records, lineages and the build oracle) with the configuration refine_trajectory reads."""

    class cfg(LoggedEngine.cfg):
        lattice_radius, device, cell_size = 3, 0, 0.05


def scan_log(e, T, B, angles):
    log = rebuild.ScanLog()
    records = [r for r in range(1, T) if r != 4]
    scans = np.stack([see((0.0, 0.0, 0.0), angles) for _ in records]) * 0.4
    for r, s in zip(records, scans):
        log.append(r, s)
    return log, records, scans


def test_rebuild_at_chunks_explicit_poses(monkeypatch):
    e = RunEngine(6)
    ang = np.linspace(-2.0, 2.0, 7)
    rng = np.random.Generator(np.random.PCG64(4))
    poses, scans = rng.uniform(-1.0, 1.0, (5, 3)), rng.uniform(0.2, 1.5, (5, 7))
    monkeypatch.setattr(rebuild, "CHUNK", 2)
    got = rebuild.rebuild_at(e, poses, scans, ang, cell_size=0.1, max_range=1.0)
    box = ParticleEngine.build_box(poses, 10.0, 1.0)
    assert e.calls == [(2, box, False), (2, box, True), (1, box, True)]
    h, s, _ = oracle_build(poses, scans, ang, 10.0, box, 0.0, 1.0)
    assert np.array_equal(got.hits, h) and np.array_equal(got.seen, s) and (got.x0, got.y0) == (box[0], box[2])
    e.calls.clear()
    own = (box[0] - 3, box[1] + 1, box[2], box[3] + 2)
    assert rebuild.rebuild_at(e, poses[:2], scans[:2], ang, cell_size=0.1, max_range=1.0, box=own).hits.shape == (own[1] - own[0], own[3] - own[2])
    assert e.calls == [(2, own, False)]
    with pytest.raises(ValueError):
        rebuild.rebuild_at(e, np.empty((0, 3)), np.empty((0, 7)), ang)


def test_refine_trajectory_rounds_particles_and_chunks(monkeypatch):
    T, B = 9, 24
    e = RunEngine(T)
    e.paths *= 0.05                                      # poses near the origin of wall_room's square, scaled to 0.4
    e.mean = e.paths.mean(axis=0)
    ang = np.linspace(-math.pi, math.pi, B, endpoint=False)
    log, records, scans = scan_log(e, T, B, ang)
    monkeypatch.setattr(refine, "CHUNK", 3)
    search = dict(substeps=2, window=2, rotations=1, rot_step=0.02, min_range=0.1, max_range=1.5)
    for particle, path in (("best", e.paths[1]), (2, e.paths[2]), ("mean", e.mean)):
        me = MapEngine()
        e.calls.clear()
        out = refine.refine_trajectory(e, log, ang, particle=particle, rounds=2, cell_size=0.1, map_engine=me, **search)
        n = len(records)
        assert out.records.tolist() == records and out.poses.shape == (n, 3) and len(out.rounds) == 2
        assert me.placed == 2 and not me.closed                                             # a supplied engine stays open
        assert [c[0] for c in me.calls] == [3, 3, 1] * 2 and all(c[1] == 0 for c in me.calls)
        first = np.concatenate([c[2] for c in me.calls[:3]])
        assert first.tobytes() == np.ascontiguousarray(path[records]).tobytes()             # round 1 starts from the chosen trajectory
        second = np.concatenate([c[2] for c in me.calls[3:]])
        # the same rounds by hand: build, refine against the built map, build again
        box = e.calls[0][1]
        assert all(c[1] == box for c in e.calls) and len(e.calls) == 3
        poses = path[records]
        for rnd in range(2):
            h, s, _ = oracle_build(poses, scans, ang, 10.0, box, 0.0, e.cfg.max_ray_m)
            built = rebuild.BuiltMap(h, s, box[0], box[2], 0.1, 10.0)
            cells = rebuild.to_cells(built, engine=e)
            new, n6, _ = oracle_refine(cells, box[0], box[2], poses, scans, ang, 10.0, 0.1, 1.0, 0.1, 1.5, 2, 2, 1, 0.02)
            r = out.rounds[rnd]
            used = np.maximum(n6[:, 5], 1)
            assert r.moved == int(np.any(n6[:, :3] != 0, axis=1).sum())
            assert r.before == pytest.approx(np.mean(n6[:, 4] / (2.0 * used)), abs=1e-15) and r.after == pytest.approx(np.mean(n6[:, 3] / (2.0 * used)), abs=1e-15)
            assert r.after >= r.before
            poses = new
            if rnd == 0:
                assert second.tobytes() == poses.tobytes()
        assert out.poses.tobytes() == poses.tobytes()
        h, s, _ = oracle_build(poses, scans, ang, 10.0, box, 0.0, e.cfg.max_ray_m)
        assert np.array_equal(out.built.hits, h) and np.array_equal(out.built.seen, s)      # the map the refined poses draw
    with pytest.raises(ValueError):
        refine.refine_trajectory(e, log, ang, particle="worst", map_engine=MapEngine())
    with pytest.raises(ValueError):
        refine.refine_trajectory(e, log, ang, rounds=0, map_engine=MapEngine())
