"""thesis_amd/loops.py's appearance path without a GPU: the bookkeeping of candidates_by_appearance over canned search results,
what the descriptors find in the asymmetric room (tests/places_oracle.py), and close_loops on a drifted log over the oracle
stand-ins for describe_scans, match_places and match_pairs."""
import math

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds
from tests.locate_oracle import asym_room
from tests.places_oracle import Descriptors, OracleEngine, as_matches, describe, match_places
from thesis_amd import loops, rebuild, trajectory

SEARCH = dict(window=8, rotations=4, rot_step=math.radians(1.0), cell_size=0.1)


class Canned:
    """describe_scans numbers the scans; match_places answers from a table {query scan: [(reference scan, shift, score)]} with
    n_bits = 50 and weight = 100 everywhere, so that similarity = score / 100."""

    def __init__(self, table):
        self.table, self.asked = table, None

    def describe_scans(self, ranges, angles, rings=24, min_range=None, max_range=None):
        n = len(ranges)
        self.described = (n, rings, min_range, max_range)
        return Descriptors(np.arange(n, dtype=np.uint64)[:, None], np.zeros(n, np.int32), np.zeros(n, np.int32))

    def match_places(self, queries, refs=None, ref_limit=None, k=4):
        qs, rs = [int(q) for q in queries[:, 0]], [int(r) for r in refs[:, 0]]
        self.asked = (qs, rs, [int(x) for x in ref_limit], k)
        out4 = np.zeros((len(qs), k, 4), np.int32)
        out4[:, :, 0] = -1
        out2 = np.full((len(qs), 2), 50, np.int32)
        for m, q in enumerate(qs):
            rows = [(rs.index(r), s, v, 100) for r, s, v in self.table.get(q, []) if r in rs and rs.index(r) < ref_limit[m]][:k]
            out4[m, :len(rows)] = np.array(rows, np.int32).reshape(-1, 4)
            out2[m, 1] = len(rows)
        return as_matches(out4, out2)


def test_candidate_bookkeeping():
    n = 40
    poses = np.stack([np.arange(n) * 0.5, np.arange(n) * -0.25, np.linspace(-3.0, 3.0, n)], axis=1)
    ranges, ang = np.zeros((n, 3)), np.zeros(3)
    table = {30: [(5, 3, 90), (6, 3, 80), (7, 2, 70), (11, 60, 60), (1, 0, 50)],       # 6 and 7 lie within half_run of 5
             36: [(17, 0, 40), (2, 32, 30)], 39: [(0, 63, 20)]}
    e = Canned(table)
    pairs, guesses, sim = loops.candidates_by_appearance(e, poses, ranges, ang, min_gap=10, half_run=2)
    # every scan with an admissible reference is a query: r + 2 < q - 10, so q >= 13 and limit = q - 12
    assert e.asked[0] == list(range(13, n)) and e.asked[1] == list(range(n - 13)) and e.asked[2] == [q - 12 for q in range(13, n)] and e.asked[3] == 4
    assert e.described == (n, 24, None, None)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[30, 3, 8], [36, 15, 20], [39, 0, 3]]      # the run of r = 0 is clipped
    assert sim.tolist() == [0.9, 0.4, 0.2]
    turn = 2.0 * math.pi / 64.0
    want = [[poses[5, 0], poses[5, 1], poses[5, 2] - 3 * turn], [poses[17, 0], poses[17, 1], poses[17, 2]],
            [0.0, 0.0, (poses[0, 2] - 63 * turn + math.pi) % (2.0 * math.pi) - math.pi]]
    assert np.allclose(guesses, want, atol=1e-15) and abs(guesses[2, 2] - (poses[0, 2] + turn)) < 1e-12
    # per_query = 2 asks for 8 and keeps, in rank order, what lies more than half_run from what it has: 5, then 11, not 6 or 7
    pairs, guesses, sim = loops.candidates_by_appearance(e, poses, ranges, ang, min_gap=10, half_run=2, per_query=2)
    assert e.asked[3] == 8 and pairs.tolist() == [[30, 3, 8], [30, 9, 14], [36, 15, 20], [36, 0, 5], [39, 0, 3]]
    assert loops.candidates_by_appearance(e, poses, ranges, ang, 10, half_run=2, per_query=5)[0][:, 0].tolist() == [30, 30, 30, 36, 36, 39] and e.asked[3] == 16
    assert loops.candidates_by_appearance(e, poses, ranges, ang, 10, half_run=0, per_query=5)[0][:, 1].tolist() == [5, 6, 7, 11, 1, 17, 2, 0]
    # min_similarity drops a candidate and lets the next one in
    pairs, _, sim = loops.candidates_by_appearance(e, poses, ranges, ang, 10, half_run=2, min_similarity=0.85)
    assert pairs.tolist() == [[30, 3, 8]] and sim.tolist() == [0.9]
    assert loops.candidates_by_appearance(e, poses, ranges, ang, 10, half_run=2, per_query=2, min_similarity=0.35)[0].tolist() == [[30, 3, 8], [30, 9, 14], [36, 15, 20]]
    # strides: queries 0, 10, .., references 0, 3, ..; the limit counts references
    pairs, _, _ = loops.candidates_by_appearance(e, poses, ranges, ang, 10, half_run=2, stride=10, ref_stride=3, rings=8, max_range=5.0)
    assert e.asked[0] == [20, 30] and e.asked[1] == [0, 3, 6, 9, 12, 15] and e.asked[2] == [3, 6] and e.described == (n, 8, None, 5.0)
    assert pairs.tolist() == [[30, 4, 9]]                # of 5, 6, 7, 11 and 1 only 6 is a reference
    # nothing admissible: no call at all
    e.asked = None
    none = loops.candidates_by_appearance(e, poses, ranges, ang, min_gap=38, half_run=2)
    assert e.asked is None and none[0].shape == (0, 3) and none[0].dtype == np.int32 and none[1].shape == (0, 3) and none[2].shape == (0,)
    for bad in (dict(min_gap=-1), dict(min_gap=3, stride=0), dict(min_gap=3, ref_stride=0), dict(min_gap=3, per_query=0), dict(min_gap=3, half_run=-1)):
        with pytest.raises(ValueError):
            loops.candidates_by_appearance(e, poses, ranges, ang, **bad)


def lap(n, radius, phase, way):
    phi = phase + way * 2.0 * math.pi * np.arange(n) / n
    return np.stack([radius * np.cos(phi), radius * np.sin(phi), phi + way * math.pi / 2], axis=1)


@pytest.fixture(scope="module")
def laps():
    """Three laps in the asymmetric room at 0.1 m, on circles round the origin with the heading tangent: 60 poses at 2.0 m, 40 at
    2.4 m from phase 0.05 rad, 40 at 1.7 m from phase 0.4 rad driven the other way; 181 beams over 270 degrees.
    (truth, scans, angles)."""
    cells, x0, y0 = asym_room(0.1)
    ang = np.linspace(-0.75 * math.pi, 0.75 * math.pi, 181)
    truth = np.concatenate([lap(60, 2.0, 0.0, 1), lap(40, 2.4, 0.05, 1), lap(40, 1.7, 0.4, -1)])
    lo, hi = lattice_bounds(400, 3)
    scans = np.stack([cast(cells, x0, y0, lo, hi, 10.0, 0.1, 1.0, p, ang, 12.0)[0] for p in truth])
    return truth, scans, ang


def test_the_best_reference_is_the_place_and_the_turn_its_heading(laps):
    """Laps 2 and 3 are the queries, lap 1 the references.  Measured with this oracle: the best reference lies within 0.54 m of
    the query's true position for all 80 (asserted: 1.0 m), the implied heading within 4.5 degrees (asserted: one sector and the
    6 degrees between neighbouring references), also for the lap driven the other way."""
    truth, scans, ang = laps
    desc, _ = describe(scans, ang, 24, 0.3, 12.0)
    out4, out2 = match_places(desc[60:], desc[:60], None, 4)
    assert np.all(out2[:, 1] == 4)
    r, s = out4[:, 0, 0], out4[:, 0, 1]
    dist = np.hypot(truth[r, 0] - truth[60:, 0], truth[r, 1] - truth[60:, 1])
    off = np.abs((truth[r, 2] - s * (2.0 * math.pi / 64.0) - truth[60:, 2] + math.pi) % (2.0 * math.pi) - math.pi)
    print("place: max %.3f m; heading: max %.2f degrees" % (dist.max(), math.degrees(off.max())))
    assert dist.max() < 1.0
    assert math.degrees(off.max()) < 360.0 / 64 + 360.0 / 60


# The end-to-end log.  Seen from the circles the room is the same after a quarter turn but for its two blocks, some 14 % of a scan's
# beams, so a scan that has no true revisit among its references finds the quarter-turn alias of its place, with a similarity (up
# to 0.59) and a match fraction (up to 0.88) as high as a true revisit's (from 0.34 and 0.77): no descriptor and no acceptance rule
# tells them apart, and on the whole laps one min_gap cannot both keep the aliases out and leave every scan its true
# place.  So the log is three sweeps over one arc of less than a quarter turn, where no alias exists: lap 2's first 10 scans, lap 1's
# first 15, and the 10 scans of lap 3 over the same arc, driven the other way.  With min_gap + half_run = 9 the first sweep asks
# nothing, and every later scan has its place among its references.
ARC = list(range(60, 70)) + list(range(0, 15)) + [100 + i for i in (33, 34, 35, 36, 37, 38, 39, 0, 1, 2)]
DRIFT = np.array([2.4, -1.8, math.radians(20.0)])        # at the last scan: 3 m, more than radius + window * cell = 1.3 m


def arc_log(laps, drift):
    truth, scans, ang = laps
    truth, scans = truth[ARC], scans[ARC]
    path = truth + np.linspace(0.0, 1.0, len(truth))[:, None] * drift
    e = OracleEngine(cell_size=0.1, min_range=0.3, max_range=12.0, path=np.concatenate([np.zeros((1, 3)), path]))   # record 0 holds no scan
    log = rebuild.ScanLog()
    for k, r in enumerate(scans):
        log.append(k + 1, r)
    return e, log, truth, path, ang


def test_pose_candidates_are_what_they_were(laps):
    e, log, truth, path, ang = arc_log(laps, 0.5 * DRIFT)
    args = dict(min_gap=7, radius=0.5, half_run=2, **SEARCH)
    old = loops.close_loops(e, log, ang, **args)
    new = loops.close_loops(e, log, ang, candidates="pose", **args)
    assert old.rounds == new.rounds and old.rounds[0].accepted > 0 and old.poses.tobytes() == new.poses.tobytes()
    for a, b in zip(old.edges, new.edges):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        loops.close_loops(e, log, ang, candidates="looks", **args)
    # match(guesses=...) hands them to match_pairs; None is the poses
    pairs = loops.candidates(path, 7, 0.5, half_run=2)
    own = loops.match(e, path, laps[1][ARC], ang, pairs, **SEARCH)
    given = loops.match(e, path, laps[1][ARC], ang, pairs, guesses=path[pairs[:, 0]], **SEARCH)
    for a, b in zip(own, given):
        assert np.array_equal(a, b)
    moved = loops.match(e, path, laps[1][ARC], ang, pairs, guesses=path[pairs[:, 0]] + [0.3, 0.0, 0.0], **SEARCH)
    assert not np.array_equal(moved.fraction_guess, own.fraction_guess)
    with pytest.raises(ValueError):
        loops.match(e, path, laps[1][ARC], ang, pairs, guesses=path[:3], **SEARCH)


def test_a_drifted_loop_is_closed_by_appearance(laps):
    """Drift to 3 m and 20 degrees over the 35 scans.  The poses propose 16 pairs and none holds: the identity.  The scans propose
    25, 21 are accepted.  Measured here (trajectory.ate after the rigid fit): 0.8684 m drifted, 0.0678 m closed; asserted: twice
    that, for libm differences between machines, and less than half the drifted error."""
    e, log, truth, path, ang = arc_log(laps, DRIFT)
    args = dict(min_gap=7, radius=0.5, half_run=2, **SEARCH)
    still = loops.close_loops(e, log, ang, candidates="pose", **args)
    assert still.rounds[0].accepted == 0 and len(still.rounds) == 1 and still.poses.tobytes() == path.tobytes()
    closed = loops.close_loops(e, log, ang, candidates="appearance", **args)
    before, after = trajectory.ate(path, truth), trajectory.ate(closed.poses, truth)
    print("pairs %d, accepted %d; ate %.4f m -> %.4f m" % (closed.rounds[0].pairs, closed.rounds[0].accepted, before, after))
    assert closed.rounds[0].accepted > 0 and closed.poses[0].tobytes() == path[0].tobytes()
    assert after < 2 * 0.0678 and after < 0.5 * before
    far = np.hypot(*(truth[closed.edges.q, :2] - truth[closed.edges.r, :2]).T) > 1.0
    assert not (closed.edges.accepted & far).any()
    # both: the pose pairs first, at their own poses, then the appearance pairs no pose pair has; the same accepted edges
    both = loops.close_loops(e, log, ang, candidates="both", **args)
    n_pose, n_look = still.rounds[0].pairs, closed.rounds[0].pairs
    assert both.edges.q[:n_pose].tolist() == still.edges.q.tolist() and np.array_equal(both.edges.fraction[:n_pose], still.edges.fraction)
    have = set(zip(still.edges.q.tolist(), still.edges.r.tolist()))
    fresh = [m for m in range(n_look) if (int(closed.edges.q[m]), int(closed.edges.r[m])) not in have]
    assert both.rounds[0].pairs == n_pose + len(fresh) and both.edges.q[n_pose:].tolist() == closed.edges.q[fresh].tolist()
    assert np.array_equal(both.edges.z[n_pose:], closed.edges.z[fresh]) and both.rounds[0].accepted >= closed.edges.accepted[fresh].sum()
