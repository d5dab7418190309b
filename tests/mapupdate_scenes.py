"""The scenes of the map-update tier tests (test_gpu_mapray_tiers.py, test_gpu_mapwin_tiers.py) and what each must show in the
census (tests/mapupdate_census.py) to reach its rung.  test_mapupdate_census.py checks every `precondition` on the CPU; the GPU
tests check it again before they launch, so a scene that drifts off its rung fails and does not pass vacuously.

A scene is (poses, scans, angles, cell size): 4 - 5 particles - a duplicated pose, a rotated one, one on the negative side
of the home tile, where the reference's index formula repeats cells - and two scans, the second with ranges a few
millimetres off so that the same cells are met again with non-zero, partly saturated values."""
import functools
from collections import namedtuple

import numpy as np

from tests import mapupdate_census as mc

Scene = namedtuple("Scene", "poses scans angles cs pool_tiles")

NEG = (-12.3, -15.1, 0.3)                                             # negative side of the home tile
POSES_5 = ((0.02, 0.03, 0.0), (0.02, 0.03, 0.0), (3.111, -2.222, 1.0), (-1.26, 0.77, -2.0), NEG)
# cell centres, headings 0 and pi/2: beams at multiples of pi/4 run along the axes and diagonals through the start cell
# (every ray stays at positive coordinates, or at negative ones: int() truncates towards zero, and a fan across 0 is not symmetric)
POSES_AXIS = ((10.025, 10.025, 0.0), (10.025, 10.025, 0.0), (12.025, 11.025, np.pi / 2), (-12.225, -15.075, 0.0))
# a negative-side pose with repeated cells 15 / 16 steps from the start cell on both axes (the block's rim)
RIM_POSE = (-11.62, -11.62, 0.3)
SHIFT = 0.004                                                         # the second scan's ranges


def bundle(n, centre, width=2e-4):
    """n beam angles within `width` rad of `centre`: at a few metres their end points share one cell."""
    return centre + np.linspace(-width / 2, width / 2, n)


def _two(r):
    r = np.asarray(r, dtype=np.float64)
    return [r, r - SHIFT]


def one_bundle(n, rng_m=3.0, centre=0.3):
    return Scene(POSES_5, _two(np.full(n, rng_m)), bundle(n, centre), 0.05, 32)


def bundles(k, off=0.076, per=9, lo=3.17, hi=3.17, width=2e-4, cs=0.05, poses=POSES_5):
    """k bundles of `per` beams round the circle, `off` rad off the axes and diagonals, ranges spread over lo .. hi.  The
    offsets in use were searched so that no bundle straddles a cell border from any of the poses: 0.076 for 56 bundles,
    0.039 for 40, at 3.17 m."""
    cen = off + 2 * np.pi * np.arange(k) / k
    ang = np.concatenate([bundle(per, c, width) for c in cen])
    r = np.repeat(np.linspace(lo, hi, k), per)
    return Scene(poses, _two(r), ang, cs, 64)


def short_fan(B, seed, lo=0.2, hi=0.75):
    """B beams over the full circle with random ranges below NEAR_R cells: every flagged cell is near."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ang = np.linspace(0.0, 2 * np.pi, B, endpoint=False)
    return Scene(POSES_5, [rng.uniform(lo, hi, B), rng.uniform(lo, hi, B)], ang, 0.05, 32)


def near_bundle(n):
    """n beams that end in one cell 10 cells from the sensor (hits n against NSPC)."""
    return Scene(POSES_5, _two(np.full(n, 0.5)), bundle(n, 0.3), 0.05, 32)


def star(per):
    """8 directions x `per` beams of distinct lengths >= 1.2 m from a cell centre: every flagged cell is special.  End cells
    three (axes) / two (diagonals) cells apart, so no pair repeats a cell of the beam before it.  The rays along -x and -y
    have no points (hybridmap.py:278-281): six directions carry events."""
    ang = np.repeat(np.arange(8) * (np.pi / 4), per)
    r = np.tile(1.21 + 0.15 * np.arange(per), 8)
    return Scene(POSES_AXIS, _two(r), ang, 0.05, 32)


def two_tier_bundle():
    """200 beams of 0.5 m and 40 of 3 m in one direction: the counter bound over all rays of the slope buckets fails (240),
    the one over the rays that reach an 8-bit field holds (40)."""
    return Scene(POSES_5, _two(np.concatenate([np.full(200, 0.5), np.full(40, 3.0)])), np.concatenate([bundle(200, 0.3), bundle(40, 0.3)]), 0.05, 32)


def quadrant_fan(B, seed, lo=1.0, hi=5.3, a0=8.0, a1=82.0, pose=(0.1, 0.1, 0.0)):
    """B beams over a0 .. a1 degrees with random ranges: all flagged cells in the first window of the home tile."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ang = np.linspace(np.radians(a0), np.radians(a1), B)
    poses = (pose, pose, (pose[0] + 0.31, pose[1] + 0.17, 0.05), NEG)
    return Scene(poses, [rng.uniform(lo, hi, B), rng.uniform(lo, hi, B)], ang, 0.05, 32)


def rim_scene():
    """Beams from RIM_POSE whose end or nearby storage cell has a source inside the block round the start cell and one on
    its rim (RIM_BEAMS: found by find_rim_beams, pinned by test_mapupdate_census.py)."""
    ang = np.array([a for a, _ in RIM_BEAMS])
    r = np.array([x for _, x in RIM_BEAMS])
    return Scene(POSES_5[:4] + (RIM_POSE,), _two(r), ang, 0.05, 32)


def find_rim_beams(pose=RIM_POSE, n_ang=96, want=8):
    """Search (angle, range) pairs from `pose` that end a beam in a rim storage cell, also with the range SHIFT shorter."""
    out = []
    for a in np.linspace(-np.pi, np.pi, n_ang, endpoint=False):
        for r in np.arange(0.70, 0.95, 0.005):
            if all(any(c.rim for c in mc.census(pose, np.array([rr]), np.array([a])).flagged) for rr in (r, r - SHIFT)):
                out.append((float(a), float(round(r, 3))))
                break
        if len(out) == want:
            break
    return out


# what find_rim_beams() returns (test_mapupdate_census.py checks it still does)
RIM_BEAMS = ((-3.141592653589793, 0.825), (-3.076142806640006, 0.84), (-3.0106929596902186, 0.865), (-2.945243112740431, 0.895),
             (-2.356194490192345, 0.89), (-2.2907446432425576, 0.86), (-2.2252947962927703, 0.84), (-2.159844949342983, 0.82))


@functools.lru_cache(maxsize=None)
def _census(pose, rkey, akey, cs):
    return mc.census(pose, np.frombuffer(rkey), np.frombuffer(akey), cs)


def censuses(scene):
    """[scan][particle] -> Census (shared between particles of one pose, and cached)."""
    a = np.ascontiguousarray(scene.angles, dtype=np.float64)
    return [[_census(tuple(float(v) for v in p), np.ascontiguousarray(r, dtype=np.float64).tobytes(), a.tobytes(), scene.cs)
             for p in scene.poses] for r in scene.scans]


def each(scene):
    return [c for per_scan in censuses(scene) for c in per_scan]


def regular(c):
    """The index map over the scan is a pure offset: every storage cell has one source, at a constant distance."""
    offs = {(a - gx, b - gy) for (cx, cy, a, b), cell in c.cells.items() for gx, gy in cell.sources if (cx, cy) == (0, 0)}
    return all(len(cell.sources) == 1 for cell in c.cells.values()) and len(offs) <= 1


def far_plain(c, lo, hi=10 ** 9):
    """Flagged cells that take the ray kernel's per-pair lists (not near, not special) with lo < events <= hi."""
    return sum(1 for x in c.flagged if not x.near and not x.special and lo < x.events <= hi)


# ---- the cases: scene + what the census must show.  pre(scene) asserts it and returns the figures the GPU assertions use ----

def _sum(scene, f):
    return sum(f(c) for c in each(scene))


def pre_bundle(scene, n, lo=None, hi=None, beyond=None):
    """One bundle: two flagged cells, neither near nor special; where the index map is a pure offset the end cell has n events
    and the cell before it 2 n (n passes + n nearby hits).  lo < events <= hi of some cell / events > beyond of some cell."""
    for c in each(scene):
        assert len(c.flagged) == 2 and not any(x.near or x.special for x in c.flagged)
        assert sorted(x.hits for x in c.flagged) == [n, n]
        if regular(c):
            assert sorted(x.events for x in c.flagged) == [n, 2 * n]
        if lo is not None:
            assert far_plain(c, lo, hi) >= 1
        if beyond is not None:
            assert far_plain(c, beyond) >= 1
    assert sum(regular(c) for c in each(scene)) >= 6 and not all(regular(c) for c in each(scene))
    return {"gt16": _sum(scene, lambda c: far_plain(c, mc.ECAP))}


def pre_pool(scene, k, at_least=None):
    """k bundles of 9: k cells with 17 .. 64 events that take the per-pair lists (at_least: no fewer), nothing near."""
    for c in each(scene):
        n = far_plain(c, mc.ECAP, mc.PCAP)
        assert (n >= at_least) if at_least else (n == k), n
        assert far_plain(c, mc.PCAP) == 0 and not any(x.near for x in c.flagged)
        assert mc.special_far_pairs(c) <= mc.RSPEC
    return {"gt16": _sum(scene, lambda c: far_plain(c, mc.ECAP)), "beyond_pool": _sum(scene, lambda c: max(0, far_plain(c, mc.ECAP) - mc.NPOOL))}


def pre_near(scene, max_hits=None, min_hits=None, inside=None, flagged_max=None):
    """Every flagged cell inside the block round the start cell; bounds on a cell's occupied / nearby hits (against NSPC),
    on the number of cells (against NNEAR, NNEAR + RSLOW)."""
    for c in each(scene):
        assert c.flagged and all(x.inside for x in c.flagged)
        hits = max(x.hits for x in c.flagged)
        assert max_hits is None or hits <= max_hits
        assert min_hits is None or hits >= min_hits
        n = mc.near_inside_cells(c)
        assert inside is None or inside[0] < n <= inside[1], n
        assert flagged_max is None or len(c.flagged) <= flagged_max
    return {"beyond_near": _sum(scene, lambda c: max(0, mc.near_inside_cells(c) - mc.NNEAR))}


def pre_rim(scene):
    per = [sum(x.rim for x in c.flagged) for c in each(scene)]
    assert all(n >= 1 for c, n in zip(each(scene), per) if c.pose == RIM_POSE) and sum(n > 0 for n in per) >= len(scene.scans)
    return {"with_rim": sum(n > 0 for n in per), "rim_cells": sum(per)}


def pre_star(scene, fits):
    for c in each(scene):
        far = [x for x in c.flagged if not x.near]
        assert far and all(x.special for x in far)
        if fits:
            assert mc.special_far_pairs(c) <= mc.RSPEC and max(x.events for x in far) <= mc.ECAP
        else:
            assert mc.special_far_pairs(c) > mc.RSPEC
    assert not all(regular(c) for c in each(scene))
    return {}


def pre_bound(scene, all_rays, far_rays):
    """Rays in one direction (all in the slope buckets of one cell), and those of them that reach an 8-bit field."""
    for c in each(scene):
        steps = [max(abs(e[0][0] - c.start[0]), abs(e[0][1] - c.start[1])) for e in c.ends if e is not None]
        assert len(steps) == all_rays and sum(d >= mc.NEAR_R for d in steps) == far_rays
    return {}


RAY_CASES = {}
for _n in (7, 8, 9, 15, 16, 17):
    RAY_CASES["ecap-%d" % _n] = (functools.partial(one_bundle, _n), functools.partial(pre_bundle, n=_n, lo=mc.ECAP if _n in (9, 17) else None, hi=mc.PCAP))
for _n in (31, 32, 33):
    RAY_CASES["pcap-%d" % _n] = (functools.partial(one_bundle, _n), functools.partial(pre_bundle, n=_n, lo=mc.ECAP, hi=mc.PCAP, beyond=mc.PCAP if _n == 33 else None))
RAY_CASES.update({
    "pool-56": (functools.partial(bundles, 56, 0.076), functools.partial(pre_pool, k=56)),
    "pool-40": (functools.partial(bundles, 40, 0.039), functools.partial(pre_pool, k=40)),
    "near-60": (functools.partial(short_fan, 60, 11, 0.2, 0.7), functools.partial(pre_near, max_hits=mc.NSPC, inside=(0, mc.NNEAR))),
    "near-hits-32": (functools.partial(near_bundle, 32), functools.partial(pre_near, max_hits=mc.NSPC, min_hits=mc.NSPC)),
    "near-hits-33": (functools.partial(near_bundle, 33), functools.partial(pre_near, min_hits=mc.NSPC + 1)),
    "near-300": (functools.partial(short_fan, 300, 17), functools.partial(pre_near, max_hits=mc.NSPC, inside=(mc.NNEAR, mc.NNEAR + mc.RSLOW), flagged_max=mc.NNEAR + mc.RSLOW)),
    "slow-full-720": (functools.partial(short_fan, 720, 13), functools.partial(pre_near, inside=(mc.NNEAR + mc.RSLOW, 10 ** 6))),
    "rim": (rim_scene, pre_rim),
    "special-8x8": (functools.partial(star, 8), functools.partial(pre_star, fits=True)),
    "special-8x44": (functools.partial(star, 44), functools.partial(pre_star, fits=False)),
    "bound-63": (functools.partial(one_bundle, 63), functools.partial(pre_bound, all_rays=mc.HIT_BOUND, far_rays=mc.HIT_BOUND)),
    "bound-64": (functools.partial(one_bundle, 64), functools.partial(pre_bound, all_rays=mc.HIT_BOUND + 1, far_rays=mc.HIT_BOUND + 1)),
    "bound-two-tier": (two_tier_bundle, functools.partial(pre_bound, all_rays=240, far_rays=40)),
    "strips-pool": (functools.partial(bundles, 60, 0.076, lo=9.0, hi=14.0, width=4e-5, cs=0.025, poses=(POSES_5[0], POSES_5[0], POSES_5[2], NEG)),
                    functools.partial(pre_pool, k=60, at_least=56)),
})


# ---- window kernel: the positive-side particles (equalities) and the negative-side ones (bounds) run in engines of their own ----

def split_sides(scene):
    """(scene with the poses whose index map is a pure offset in every scan, scene with the others)."""
    reg = [all(regular(row[i]) for row in censuses(scene)) for i in range(len(scene.poses))]
    pos = scene._replace(poses=tuple(p for p, r in zip(scene.poses, reg) if r))
    neg = scene._replace(poses=tuple(p for p, r in zip(scene.poses, reg) if not r) * 2)
    assert len(set(pos.poses)) >= 2 and len(pos.poses) > len(set(pos.poses)) and neg.poses
    return pos, neg


def window_prediction(scene):
    """(slow, pool) summed over the scene's particles and scans by the window kernel's rules (mc.window_routing)."""
    B = max(len(r) for r in scene.scans)
    r = [mc.window_routing(c, B) for c in each(scene)]
    return sum(x[0] for x in r), sum(x[1] for x in r)


def pre_win(scene, cap=None, nflag=None, both_sides=None, events=None):
    """The largest window's bucket depth / flagged cells within bounds; at least `both_sides` cells above and at or below
    the depth; `events`: event counts some flagged cell must have."""
    B = max(len(r) for r in scene.scans)
    for c in each(scene):
        t = max(mc.window_tables(c, B).values(), key=lambda t: t["nflag"])
        assert cap is None or cap[0] <= t["cap"] <= cap[1], t
        assert nflag is None or nflag[0] < t["nflag"] <= nflag[1], t
        if both_sides:
            assert sum(x.events > t["cap"] for x in c.flagged) >= both_sides <= sum(x.events <= t["cap"] for x in c.flagged)
        if events and regular(c):
            assert sorted(x.events for x in c.flagged) == sorted(events)
    return {}


WIN_CASES = {}
for _n in (4, 8, 9, 32, 33):
    WIN_CASES["bundle-%d" % _n] = (functools.partial(one_bundle, _n), functools.partial(pre_win, cap=(64, 64), events=(_n, 2 * _n)))
WIN_CASES.update({
    "shallow": (functools.partial(quadrant_fan, 200, 21, 1.0, 3.0, 30.0, 60.0), functools.partial(pre_win, cap=(5, 16), both_sides=5)),
    "very-shallow": (functools.partial(quadrant_fan, 700, 22), functools.partial(pre_win, cap=(4, 4), nflag=(1024, mc.NB_MAX))),
    "more-cells-than-ids": (functools.partial(quadrant_fan, 1081, 23), functools.partial(pre_win, cap=(4, 4), nflag=(mc.NB_MAX, 10 ** 6))),
})
