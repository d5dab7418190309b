"""The event-walk kernel's level walk in runs (kernels_mapev.hip: a work item is a ray and a run of RUN consecutive whole
chunks, the left-over chunks behind a ray's runs are levels of their own) against the oracle.

Every case forces RBPF_MAP_KERNEL=ev and goes through test_gpu_mapev_flagged.run_case: two scans into a few particles,
every tile byte and the read-out at the flagged cells compared with OracleHybridMap.update.  Before the engine runs, each
case works out on the CPU, from the beams' cells, how many steps the walk takes on every ray - the ray's cells (the
Chebyshev distance of the end cell plus one) less the beam's own: its end cell and, when that lies in the end cell's tile,
the cell before it - and asserts that the scene holds the classes of rays it is about:

    steps 0 .. 15 lie in the 16-bit block; behind them nfull = (steps - 16) // 16 whole chunks and a tail of
    (steps - 16) % 16 steps; nfull // RUN runs and nfull % RUN left-over chunks.

GPU only:  python -m pytest tests -m gpu"""
from math import cos, sin

import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests.test_gpu_mapev_flagged import run_case

pytestmark = pytest.mark.gpu

RUN = 2                  # chunks per run (EV_RUN in kernels_mapev.hip)
NEAR, CH = 16, 16        # steps in the 16-bit block, steps per chunk
TILE_M = 40.0


@pytest.fixture()
def ev_engine(monkeypatch):
    monkeypatch.setenv("RBPF_MAP_KERNEL", "ev")
    monkeypatch.delenv("RBPF_EV_GRID", raising=False)
    from thesis_amd import engine
    return engine


def _tile(cell, cs):
    return int(np.floor((cell * cs + TILE_M / 2) / TILE_M))


def walk_steps(pose, ranges, angles, cs):
    """Per beam: steps the walk takes, steep (|dy| > |dx|), sign of dx, sign of dy - from the oracle's own cells."""
    sx, sy = orc.scan_xy(ranges, angles)
    gx, gy = orc.transform(sx, sy, pose)
    x0, y0 = int(pose[0] / cs), int(pose[1] / cs)
    out = []
    for i in range(len(ranges)):
        assert np.hypot(sx[i], sy[i]) <= orc.MAX_RAY_M
        x1, y1 = int(gx[i] / cs), int(gy[i] / cs)
        pts = orc.get_affected_points(x0, y0, x1, y1)
        own = 0
        if pts:
            own = 1
            if len(pts) >= 2 and _tile(pts[-2][0], cs) == _tile(x1, cs) and _tile(pts[-2][1], cs) == _tile(y1, cs):
                own = 2
        out.append((len(pts) - own, abs(y1 - y0) > abs(x1 - x0), x1 > x0, y1 > y0))
    return out


def classes(steps):
    """(nfull, tail) of the rays that leave the 16-bit block."""
    return [((n - NEAR) // CH, (n - NEAR) % CH) for n, *_ in steps if n > NEAR]


def ranges_for(pose, angles, steps, cs):
    """Ranges that give beam i a walk of steps[i] steps from `pose`: the end point lies in the middle (major axis) of the cell
    steps[i] + 1 cells from the start cell (two cells of a ray are the beam's own).  For poses whose cells and rays have
    positive coordinates (int() rounds towards zero)."""
    out = []
    for a, n in zip(angles, steps):
        ux, uy = cos(a + pose[2]), sin(a + pose[2])
        m = 1 if abs(uy) > abs(ux) else 0
        u = (ux, uy)[m]
        k = int(pose[m] / cs) + (1 if u > 0 else -1) * (n + 1)
        assert k > 0
        out.append(((k + 0.5) * cs - pose[m]) / u)
    return np.array(out)


def fan(B, phase=0.0):
    """B beam angles all round, none on an axis or a diagonal."""
    return phase + 0.0137 + 2 * np.pi * np.arange(B) / B


def ladder_steps(copies=2):
    """Every (nfull, tail) with nfull = 0 .. 3 RUN + 1, `copies` times, in an order that gives every direction every length."""
    kinds = [NEAR + CH * f + t for f in range(3 * RUN + 2) for t in range(CH)]
    n = len(kinds) * copies
    return [kinds[(i * 37) % len(kinds)] for i in range(n)]


def check_ladder(pose, ranges, angles, cs):
    st = walk_steps(pose, ranges, angles, cs)
    cl = classes(st)
    assert {f for f, _ in cl} >= set(range(3 * RUN + 2)), "whole-chunk counts 0 .. 3 RUN + 1"
    assert {t for _, t in cl} == set(range(CH)), "every tail length"
    assert {f % RUN for f, _ in cl} == set(range(RUN)) and max(f // RUN for f, _ in cl) >= 3
    assert {(s, dx, dy) for n, s, dx, dy in st if n > NEAR + CH * RUN} == {(s, dx, dy) for s in (False, True) for dx in (False, True)
                                                                          for dy in (False, True)}, "both ray classes, four sign pairs"


LADDER_TH = 0.3
LADDER_POSES = [[8.02, 9.03, LADDER_TH], [8.02, 9.03, LADDER_TH], [8.047, 9.011, LADDER_TH], [17.52, 9.03, LADDER_TH]]   # two sub-cell offsets; a fan across the tile edge x = 20 m


def fan_near_axes(B, th):
    """B beam angles within 0.2 rad of the four axes of the map (a particle at heading th): a ray of n cells is at most 1.02 n cells long."""
    i = np.arange(B)
    return (i // (B // 4)) * (np.pi / 2) - 0.2 + 0.4 * (i % (B // 4) + 0.5) / (B // 4) - th


def ladder_scans(cs, pose, near_axes=False):
    st = ladder_steps()
    ang = fan_near_axes(len(st), pose[2]) if near_axes else fan(len(st))
    st2 = st[5:] + st[:5]
    return [ranges_for(pose, ang, st, cs), ranges_for(pose, ang, st2, cs)], ang


def scaled(poses, cs):
    """The ladder's poses with the cell size: the same cells at another resolution."""
    return [[x * cs / 0.05, y * cs / 0.05, th] for x, y, th in poses]


def test_ladder(ev_engine):
    """Whole-chunk counts 0 .. 3 RUN + 1 with every tail, all round, from two sub-cell offsets and across a tile edge."""
    cs = 0.05
    scans, ang = ladder_scans(cs, LADDER_POSES[0])
    for pose in LADDER_POSES[1:]:
        for r in scans:
            check_ladder(pose, r, ang, cs)
    assert orc.transform(*orc.scan_xy(scans[0], ang), LADDER_POSES[3])[0].max() > TILE_M / 2 + 1.0      # beams end in the next tile
    c = run_case(ev_engine, LADDER_POSES, scans, ang, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
    assert c["map_windows"] == len(LADDER_POSES) * len(scans)            # one window each: the runs of the whole fan


@pytest.mark.parametrize("nfull", [RUN - 1, RUN, RUN + 1, 2 * RUN])
def test_run_boundaries(ev_engine, nfull):
    """All rays with exactly `nfull` whole chunks: no run at all, runs only, a run and a left-over, two runs."""
    cs, B = 0.05, 96
    poses = [[8.02, 9.03, 0.3], [8.02, 9.03, 0.3], [11.02, 6.03, 0.3]]       # whole cells apart: the same rays
    ang = fan(B)
    scans = [ranges_for(poses[0], ang, [NEAR + CH * nfull + (i * 7 + s) % CH for i in range(B)], cs) for s in (0, 5)]
    for pose in poses[1:]:
        for r in scans:
            cl = classes(walk_steps(pose, r, ang, cs))
            assert len(cl) == B and {f for f, _ in cl} == {nfull} and {t for _, t in cl} == set(range(CH))
    c = run_case(ev_engine, poses, scans, ang)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]


def test_no_leftover_beside_most_leftovers(ev_engine):
    """Rays whose whole chunks are runs and nothing else together with rays that leave RUN - 1 chunks behind their runs."""
    cs, B = 0.05, 128
    poses = [[8.02, 9.03, 0.3], [8.02, 9.03, 0.3], [11.02, 6.03, 0.3]]
    ang = fan(B)
    full = [(1 + i % 3) * RUN - (i // 3) % 2 for i in range(B)]              # RUN, 2 RUN, 3 RUN and one chunk less
    scans = [ranges_for(poses[0], ang, [NEAR + CH * f + (i * 5 + s) % CH for i, f in enumerate(full)], cs) for s in (0, 9)]
    for pose in poses[1:]:
        for r in scans:
            cl = classes(walk_steps(pose, r, ang, cs))
            assert {f % RUN for f, _ in cl} == {0, RUN - 1} and {f for f, _ in cl} == set(full)
    c = run_case(ev_engine, poses, scans, ang)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]


@pytest.mark.parametrize("same", [63, 64, 65])
def test_lane_fill(ev_engine, same):
    """63, 64, 65 rays of RUN + 1 whole chunks - one run and one left-over each: the wave-slot arithmetic of a run level and of a
    left-over level at one wave and at two - and one ray of 2 RUN + 1: a second run level that holds one ray."""
    cs = 0.05
    poses = [[8.02, 9.03, 0.3], [8.02, 9.03, 0.3], [11.02, 6.03, 0.3]]
    ang = fan(same + 1)
    scans = [ranges_for(poses[0], ang, [NEAR + CH * (RUN + 1) + (i + s) % CH for i in range(same)] + [NEAR + CH * (2 * RUN + 1) + 3 + s], cs)
             for s in (0, 6)]
    for pose in poses[1:]:
        for r in scans:
            full = sorted(f for f, _ in classes(walk_steps(pose, r, ang, cs)))
            assert full == [RUN + 1] * same + [2 * RUN + 1]
    c = run_case(ev_engine, poses, scans, ang)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]


def test_events_inside_a_run(ev_engine):
    """A short wall in front of a far one, beam by beam: the far rays cross the short beams' end cells in the second and in the
    last chunk of a run (chunks 2 and 2 RUN; one and the same at RUN = 2 apart from the run they belong to)."""
    cs, B = 0.05, 120
    poses = [[8.02, 9.03, 0.3], [8.02, 9.03, 0.3], [8.047, 9.011, 0.3], [11.02, 6.03, 0.3]]
    ang = 0.4 + 0.008 * np.arange(B)                                         # a third of a cell apart at 40 cells
    far = NEAR + CH * (2 * RUN + 1) + 5
    kinds = [NEAR + CH + 6, far, NEAR + CH * (2 * RUN - 1) + 9, far]         # ends in chunk 2, far, ends in chunk 2 RUN, far
    scans = [ranges_for(poses[0], ang, [kinds[i % 4] + s * (i % 3) for i in range(B)], cs) for s in (0, 1)]
    for pose in poses[1:]:
        for r in scans:
            cl = classes(walk_steps(pose, r, ang, cs))
            assert {f for f, _ in cl} >= {1, 2 * RUN - 1, 2 * RUN + 1}
    c = run_case(ev_engine, poses, scans, ang)
    assert c["map_events"] > 0
    assert c["window_fallbacks"] == 0 and c["map_event_overflows"] == 0


def test_strips_cut_runs(ev_engine):
    """0.025 m cells, 181 beams, ranges to 14 m: the fan is walked in strips of rows whose edges cut the rays' runs."""
    cs, B = 0.025, 181
    ang = np.linspace(-2.3, 2.3, B)
    poses = [[0.2, -0.1, 0.4], [0.2, -0.1, 0.4], [0.2, -0.1, 0.4], [-6.33, 2.21, -2.0]]
    scans = [2.0 + 12.0 * ((np.arange(B) * 37 + s) % B) / B for s in (0, 60)]      # a ladder of ranges, shuffled over the fan
    for pose in poses[2:]:
        for r in scans:
            cl = classes(walk_steps(pose, r, ang, cs))
            assert len({f for f, _ in cl}) >= 3 * RUN + 2 and {t for _, t in cl} == set(range(CH)) and {f % RUN for f, _ in cl} == set(range(RUN))
    c = run_case(ev_engine, poses, scans, ang, cell_size=cs, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
    assert c["map_windows"] > len(poses) * len(scans)


def test_ladder_partial_groups(ev_engine):
    """The ladder at 0.1 m cells: dim 400, the last 32-cell group of a tile row holds 16 cells.  (Beams near the axes: the longest
    ray's 145 cells are 14.8 m there, below the 15 m at which a beam is cut.)"""
    cs = 0.1
    poses = scaled(LADDER_POSES, cs)[:3]
    scans, ang = ladder_scans(cs, poses[0], near_axes=True)
    for pose in poses[1:]:
        for r in scans:
            check_ladder(pose, r, ang, cs)
    c = run_case(ev_engine, poses, scans, ang, cell_size=cs, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]


def test_ladder_one_workgroup(ev_engine, monkeypatch):
    """The ladder with one resident workgroup: it takes the particles one after the other, shorter and longer fans in turn -
    nothing of a particle's levels may reach the next."""
    monkeypatch.setenv("RBPF_EV_GRID", "1")
    cs = 0.05
    scans, ang = ladder_scans(cs, LADDER_POSES[0])
    poses = [LADDER_POSES[0], [8.02, 9.03, 1.1], LADDER_POSES[2], [3.31, 4.44, -2.0], LADDER_POSES[3], LADDER_POSES[0]]
    for r in scans:
        check_ladder(LADDER_POSES[2], r, ang, cs)
    c = run_case(ev_engine, poses, scans, ang, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
