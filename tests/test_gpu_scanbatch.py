"""The six entry points over a batch of scans (cast, view gain, map building, pose refinement, pair matching, scan description)
through the raw binding, at shapes whose scratch regions are no multiples of 256 bytes: 3 scans or pairs of 5 beams, one
rotation and one translation each way, 2 substeps, a box of 7 x 5 cells.  Every combination of host and device outputs with each
optional output present and absent equals the NumPy oracles of tests/ bit for bit; a second, larger call on the same engine
makes each scratch block grow.  Then which check wins where two arguments are bad at once."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.build_oracle import build_map as oracle_build
from tests.pairs_oracle import match_pairs as oracle_pairs
from tests.places_oracle import describe as oracle_describe
from tests.refine_oracle import refine as oracle_refine
from tests.test_gpu_cast import oracle as oracle_cast
from tests.test_gpu_locate import engine, load_room
from tests.test_gpu_view_gain import oracle as oracle_gain, random_table

pytestmark = pytest.mark.gpu

S, W, R, STEP = 2, 1, 1, math.radians(0.5)
LO, HI, CAST_RANGE, RINGS = 0.3, 6.0, 4.0, 7
DEV = 1                                                  # RBPF_*_DEVICE_OUT of every entry point here
POISON = 77

dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


class Outputs:
    """Poisoned output buffers in host or device memory; absent ones are passed as NULL."""

    def __init__(self, device, **specs):
        self.device, self.bufs = device, {}
        for name, spec in specs.items():
            if spec is None:
                self.bufs[name] = None
            elif device:
                import torch
                self.bufs[name] = torch.full(spec[0], POISON, dtype=getattr(torch, np.dtype(spec[1]).name), device="cuda")
            else:
                self.bufs[name] = np.full(spec[0], POISON, dtype=spec[1])

    def ptr(self, name):
        b = self.bufs[name]
        return None if b is None else C.c_void_p(b.data_ptr() if self.device else b.ctypes.data)

    def get(self, name):
        b = self.bufs[name]
        return b.cpu().numpy() if self.device else b


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def world():
    """The asymmetric room in particle 1 of a two-particle engine; for each size the poses, beams, scans, pairs and guesses, and
    every oracle result, computed once."""
    pytest.importorskip("torch")
    e = engine(2)
    full = load_room(e, particle=1)
    m = e.render_map(1)
    c = e.cfg
    inv, q, thr = e.dim / float(c.tile_len_m), float(c.quantum), float(c.occupied_threshold)
    rng = np.random.Generator(np.random.PCG64(41))
    cases = {}
    for size, (n, nb) in (("small", (3, 5)), ("large", (67, 37))):
        truth = []
        while len(truth) < n:                            # poses on the room's floor
            x, y = rng.uniform(-7.5, 7.5, 2)
            if m.cells[int(math.floor(x * 20.0)) - full[0], int(math.floor(y * 20.0)) - full[2]] < 0:
                truth.append((x, y, rng.uniform(-math.pi, math.pi)))
        truth = np.array(truth)
        ang = np.ascontiguousarray(np.linspace(-2.2, 2.3, nb))
        scans = np.ascontiguousarray(e.cast_scans(truth, ang, particle=1, max_range=12.0))
        scans[0, 1], scans[n - 1, nb - 1] = np.nan, 30.0                   # data, not errors
        guess = np.ascontiguousarray(truth + rng.uniform(-1.0, 1.0, (n, 3)) * [0.04, 0.04, STEP])
        pairs = np.array([[k, (k + 1) % n, (k + 1) % n + 1] for k in range(n)], dtype=np.int32)
        pairs[0] = [0, 0, n]                             # one run of every scan
        pguess = np.ascontiguousarray(truth[pairs[:, 0]] + rng.uniform(-1.0, 1.0, (n, 3)) * [0.04, 0.04, STEP])
        X, Y = int(math.floor(truth[0, 0] * 20.0)), int(math.floor(truth[0, 1] * 20.0))
        box = np.array([X - 3, X + 4, Y - 2, Y + 3], dtype=np.int32) if size == "small" else np.array([X - 40, X + 33, Y - 25, Y + 46], dtype=np.int32)
        tab = random_table(n)
        d = dict(n=n, nb=nb, truth=np.ascontiguousarray(truth), ang=ang, scans=scans, guess=guess, pairs=pairs, pguess=pguess, box=box, tab=tab)
        d["refine"] = oracle_refine(m.cells, m.x0, m.y0, guess, scans, ang, inv, q, thr, LO, HI, S, W, R, STEP)
        d["pairs_ref"] = oracle_pairs(truth, scans, ang, pairs, pguess, 20.0, LO, HI, S, W, R, STEP)
        d["describe"] = oracle_describe(scans, ang, RINGS, LO, HI)
        d["build"] = oracle_build(truth, scans, ang, 20.0, tuple(int(b) for b in box), LO, HI)[:2]
        d["cast"] = oracle_cast(e, 1, truth, ang, CAST_RANGE)[:2]
        d["gain"] = oracle_gain(e, 1, truth, ang, CAST_RANGE, [tab])[0][0]
        cases[size] = d
    assert cases["small"]["refine"][1][:, 3].max() > 0 and cases["small"]["pairs_ref"][1][:, 3].max() > 0
    yield e, cases
    e.close()


SIZES = ("small", "large")                               # in this order: the second call finds its scratch block too small
PRESENT = [(True, False), (False, True), (True, True)]


@pytest.mark.parametrize("device", [False, True])
def test_refine_every_output_combination(world, device):
    e, cases = world
    for size in SIZES:
        d = cases[size]
        n, nk, nw = d["n"], 2 * R + 1, 2 * W + 1
        poses, n6, scores = d["refine"]
        for (with_pose, with_n6) in PRESENT:
            for with_scores in (False, True):
                o = Outputs(device, pose=((n, 3), np.float64) if with_pose else None, n6=((n, 6), np.int32) if with_n6 else None,
                            scores=((n, nk, nw, nw), np.int32) if with_scores else None)
                rc = e._lib.rbpf_refine_poses(e._h, 1, dp(d["guess"]), n, dp(d["scans"]), dp(d["ang"]), d["nb"], LO, HI, S, W, R, STEP,
                                              o.ptr("pose"), o.ptr("n6"), o.ptr("scores"), DEV if device else 0)
                assert rc == 0, (size, with_pose, with_n6, with_scores, e._lib.rbpf_last_error(e._h))
                e.synchronize()
                what = (size, device, with_pose, with_n6, with_scores)
                assert not with_pose or same_bits(o.get("pose"), poses), what
                assert not with_n6 or same_bits(o.get("n6"), n6), what
                assert not with_scores or same_bits(o.get("scores"), scores), what


@pytest.mark.parametrize("device", [False, True])
def test_pairs_every_output_combination(world, device):
    e, cases = world
    for size in SIZES:
        d = cases[size]
        n, nk, nw = d["n"], 2 * R + 1, 2 * W + 1
        poses, m8, scores = d["pairs_ref"]
        assert not m8[:, 7].any()
        for (with_pose, with_m8) in PRESENT:
            for with_scores in (False, True):
                o = Outputs(device, pose=((n, 3), np.float64) if with_pose else None, m8=((n, 8), np.int32) if with_m8 else None,
                            scores=((n, nk, nw, nw), np.int32) if with_scores else None)
                rc = e._lib.rbpf_match_pairs(e._h, dp(d["truth"]), n, dp(d["scans"]), dp(d["ang"]), d["nb"], ip(d["pairs"]), n, dp(d["pguess"]),
                                             20.0, LO, HI, S, W, R, STEP, o.ptr("pose"), o.ptr("m8"), o.ptr("scores"), DEV if device else 0)
                assert rc == 0, (size, with_pose, with_m8, with_scores, e._lib.rbpf_last_error(e._h))
                e.synchronize()
                what = (size, device, with_pose, with_m8, with_scores)
                assert not with_pose or same_bits(o.get("pose"), poses), what
                assert not with_m8 or same_bits(o.get("m8"), m8.astype(np.int32)), what
                assert not with_scores or same_bits(o.get("scores"), scores), what


@pytest.mark.parametrize("device", [False, True])
def test_describe_every_output_combination(world, device):
    e, cases = world
    for size in SIZES:
        d = cases[size]
        n = d["n"]
        desc, info = d["describe"]
        for (with_desc, with_info) in PRESENT:
            o = Outputs(device, desc=((n, RINGS), np.int64) if with_desc else None, info=((n, 2), np.int32) if with_info else None)
            rc = e._lib.rbpf_describe_scans(e._h, dp(d["scans"]), n, dp(d["ang"]), d["nb"], LO, HI, RINGS, o.ptr("desc"), o.ptr("info"),
                                            DEV if device else 0)
            assert rc == 0, (size, with_desc, with_info, e._lib.rbpf_last_error(e._h))
            e.synchronize()
            assert not with_desc or same_bits(o.get("desc").view(np.uint64), desc), (size, device, with_desc, with_info)
            assert not with_info or same_bits(o.get("info"), info), (size, device, with_desc, with_info)


@pytest.mark.parametrize("device", [False, True])
def test_build_every_output_combination(world, device):
    e, cases = world
    for size in SIZES:
        d = cases[size]
        n, box = d["n"], d["box"]
        shape = (int(box[1] - box[0]), int(box[3] - box[2]))
        hits, seen = d["build"]
        assert size != "small" or shape == (7, 5)
        for (with_hits, with_seen) in PRESENT:
            o = Outputs(device, hits=(shape, np.int32) if with_hits else None, seen=(shape, np.int32) if with_seen else None)
            rc = e._lib.rbpf_build_map(e._h, dp(d["truth"]), n, dp(d["scans"]), dp(d["ang"]), d["nb"], 20.0, ip(box), LO, HI, DEV if device else 0,
                                       o.ptr("hits"), o.ptr("seen"))
            assert rc == 0, (size, with_hits, with_seen, e._lib.rbpf_last_error(e._h))
            e.synchronize()
            assert not with_hits or same_bits(o.get("hits"), hits.astype(np.int32)), (size, device, with_hits, with_seen)
            assert not with_seen or same_bits(o.get("seen"), seen.astype(np.int32)), (size, device, with_hits, with_seen)
    assert cases["large"]["build"][0].max() > 0


@pytest.mark.parametrize("device", [False, True])
def test_cast_and_gain_every_output_combination(world, device):
    e, cases = world
    for size in SIZES:
        d = cases[size]
        n, nb = d["n"], d["nb"]
        ranges, status = d["cast"]
        for with_status in (False, True):
            o = Outputs(device, ranges=((n, nb), np.float64), status=((n, nb), np.uint8) if with_status else None)
            rc = e._lib.rbpf_cast_scans(e._h, 1, dp(d["truth"]), n, dp(d["ang"]), nb, CAST_RANGE, DEV if device else 0, o.ptr("ranges"), o.ptr("status"))
            assert rc == 0, (size, with_status, e._lib.rbpf_last_error(e._h))
            e.synchronize()
            assert same_bits(o.get("ranges"), ranges) and (not with_status or same_bits(o.get("status"), status)), (size, device, with_status)
        gain, seen, unknown = d["gain"]
        for with_seen in (False, True):
            for with_unknown in (False, True):
                o = Outputs(device, gain=((n,), np.int64), seen=((n,), np.int32) if with_seen else None, unknown=((n,), np.int32) if with_unknown else None)
                rc = e._lib.rbpf_view_gain(e._h, 1, dp(d["truth"]), n, dp(d["ang"]), nb, CAST_RANGE, ip(d["tab"]), DEV if device else 0,
                                           o.ptr("gain"), o.ptr("seen"), o.ptr("unknown"))
                assert rc == 0, (size, with_seen, with_unknown, e._lib.rbpf_last_error(e._h))
                e.synchronize()
                what = (size, device, with_seen, with_unknown)
                assert same_bits(o.get("gain"), gain), what
                assert not with_seen or same_bits(o.get("seen"), seen), what
                assert not with_unknown or same_bits(o.get("unknown"), unknown), what


# ---- which check wins ---------------------------------------------------------------------------------------------------------------
MAX_MSG, MIN_MSG = "max_range must be finite and > 0", "min_range must be finite and >= 0"
POSES_MSG, ANGLES_MSG = "poses must be finite", "angles must be finite"
MID = " between rbpf_scan_update_begin and rbpf_scan_update_end"


def test_the_first_bad_argument_is_reported():
    from thesis_amd import _lib
    P, NB, N = 3, 16, 4
    e = engine(P, lattice_radius=1)
    load_room(e)
    ang = np.linspace(-2.0, 2.0, NB)
    rg = np.tile(np.linspace(1.0, 6.0, NB), (N, 1))
    poses = np.array([[0.5, 0.4, 0.3], [-1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [0.3, 0.3, 3.0]])
    pairs = np.array([[3, 0, 2], [2, 1, 2]], dtype=np.int32)
    box = np.array([-20, 20, -20, 20], dtype=np.int32)
    tab = random_table(3)
    nan_pose, nan_ang, nan_guess, bad_tab, bad_pairs = poses.copy(), ang.copy(), poses[:2].copy(), tab.copy(), pairs.copy()
    nan_pose[1, 2], nan_ang[7], nan_guess[1, 0], bad_tab[4], bad_pairs[0, 0] = np.nan, np.inf, np.nan, -1, N
    out = np.zeros(1 << 16, np.int64)                    # room for every output
    vp = C.c_void_p(out.ctypes.data)

    def cast(particle=0, p=poses, n=N, a=ang, nb=NB, hi=9.0, flags=0):
        return e._lib.rbpf_cast_scans(e._h, particle, dp(p), n, dp(a), nb, hi, flags, vp, None)

    def gain(p=poses, n=N, a=ang, nb=NB, hi=9.0, t=tab, flags=0):
        return e._lib.rbpf_view_gain(e._h, 0, dp(p), n, dp(a), nb, hi, ip(t), flags, vp, None, None)

    def build(p=poses, n=N, a=ang, nb=NB, inv=20.0, bx=box, lo=0.3, hi=9.0, flags=0):
        return e._lib.rbpf_build_map(e._h, dp(p), n, dp(rg), dp(a), nb, inv, ip(bx), lo, hi, flags, vp, None)

    def refine(particle=0, p=poses, n=N, a=ang, nb=NB, lo=0.3, hi=9.0, s=4, w=2, r=1, step=STEP, flags=0):
        return e._lib.rbpf_refine_poses(e._h, particle, dp(p), n, dp(rg), dp(a), nb, lo, hi, s, w, r, step, vp, None, None, flags)

    def match(p=poses, n=N, a=ang, nb=NB, pr=pairs, m=2, g=None, inv=20.0, lo=0.3, hi=9.0, s=4, w=2, r=1, step=STEP, flags=0):
        return e._lib.rbpf_match_pairs(e._h, dp(p), n, dp(rg), dp(a), nb, ip(pr), m, dp(g), inv, lo, hi, s, w, r, step, vp, None, None, flags)

    def describe(n=N, a=ang, nb=NB, lo=0.3, hi=9.0, rings=6, flags=0):
        return e._lib.rbpf_describe_scans(e._h, dp(rg), n, dp(a), nb, lo, hi, rings, vp, None, flags)

    def expect(rc, code, msg):
        assert rc == code and e._lib.rbpf_last_error(e._h).decode() == msg, (rc, e._lib.rbpf_last_error(e._h), msg)
    EINVAL = _lib.RBPF_EINVAL
    cast_counts = "n_poses >= 0, n_beams >= 1 and n_poses * n_beams < 2^31 are required"
    expect(cast(flags=2, nb=0), EINVAL, "unknown flags")
    expect(cast(particle=P, nb=0), EINVAL, "particle index out of range")
    expect(cast(nb=0, hi=0.0), EINVAL, cast_counts)
    expect(cast(n=-1, p=nan_pose), EINVAL, cast_counts)
    expect(cast(hi=np.nan, p=nan_pose), EINVAL, MAX_MSG)
    expect(cast(p=nan_pose, a=nan_ang), EINVAL, POSES_MSG)
    expect(cast(a=nan_ang), EINVAL, ANGLES_MSG)
    assert cast(n=0, p=nan_pose) == 0                    # no pose is read

    gain_counts = "n_poses >= 1, n_beams >= 1 and n_poses * n_beams < 2^31 are required"
    expect(gain(n=0, hi=-1.0), EINVAL, gain_counts)
    expect(gain(nb=0, p=nan_pose), EINVAL, gain_counts)
    expect(gain(hi=np.inf, a=nan_ang), EINVAL, MAX_MSG)
    expect(gain(p=nan_pose, t=bad_tab), EINVAL, POSES_MSG)
    expect(gain(a=nan_ang, t=bad_tab), EINVAL, ANGLES_MSG)
    expect(gain(t=bad_tab, hi=1000.0), EINVAL, "value_tab entries must lie in 0 .. 2^20")

    build_counts = "n_scans >= 1, n_beams >= 1 and n_scans * n_beams < 2^31 are required"
    expect(build(nb=0, bx=np.array([3, 3, 0, 1], dtype=np.int32)), EINVAL, build_counts)
    expect(build(bx=np.array([3, 3, 0, 1], dtype=np.int32), inv=0.0), EINVAL, "box must have x1 > x0 and y1 > y0")
    expect(build(inv=0.0, hi=0.0), EINVAL, "cells_per_m must be finite and > 0")
    expect(build(hi=0.0, lo=-1.0), EINVAL, MAX_MSG)
    expect(build(lo=-1.0, p=nan_pose), EINVAL, MIN_MSG)
    expect(build(p=nan_pose, a=nan_ang), EINVAL, POSES_MSG)
    expect(build(a=nan_ang, hi=1000.0), EINVAL, ANGLES_MSG)

    scan_counts = "n_scans >= 1, 1 <= n_beams <= 16384 and n_scans * n_beams < 2^31 are required"
    search = ["substeps must be 1, 2, 4, 8 or 16", "0 <= n_trans <= 32 is required", "0 <= n_rot <= 100 is required", "rot_step must be finite and >= 0"]
    expect(refine(flags=2, nb=16385), EINVAL, "unknown flags")
    expect(refine(nb=16385, particle=P), EINVAL, scan_counts)
    expect(refine(particle=P, s=3), EINVAL, "particle index out of range")
    expect(refine(s=3, w=33), EINVAL, search[0])
    expect(refine(w=33, r=101), EINVAL, search[1])
    expect(refine(r=101, step=-1.0), EINVAL, search[2])
    expect(refine(step=np.nan, hi=0.0), EINVAL, search[3])
    expect(refine(hi=0.0, lo=-1.0), EINVAL, MAX_MSG)
    expect(refine(lo=np.nan, p=nan_pose), EINVAL, MIN_MSG)
    expect(refine(p=nan_pose, a=nan_ang), EINVAL, POSES_MSG)
    expect(refine(a=nan_ang, hi=1000.0), EINVAL, ANGLES_MSG)

    pair_counts = "n_scans >= 1, n_pairs >= 1, 1 <= n_beams <= 16384 and n_scans * n_beams < 2^31 are required"
    expect(match(m=0, s=3), EINVAL, pair_counts)
    expect(match(nb=16385, s=3), EINVAL, pair_counts)
    expect(match(s=3, w=33), EINVAL, search[0])
    expect(match(w=-1, r=101), EINVAL, search[1])
    expect(match(r=-1, step=-1.0), EINVAL, search[2])
    expect(match(step=np.inf, inv=0.0), EINVAL, search[3])
    expect(match(inv=0.0, hi=0.0), EINVAL, "cells_per_m must be finite and > 0")
    expect(match(hi=0.0, lo=-1.0), EINVAL, MAX_MSG)
    expect(match(lo=-1.0, p=nan_pose), EINVAL, MIN_MSG)
    expect(match(p=nan_pose, g=nan_guess), EINVAL, POSES_MSG)
    expect(match(g=nan_guess, a=nan_ang), EINVAL, "guesses must be finite")
    expect(match(a=nan_ang, pr=bad_pairs), EINVAL, ANGLES_MSG)
    expect(match(pr=bad_pairs, hi=1000.0), EINVAL, "a pair {q, r0, r1} needs 0 <= q < n_scans and 0 <= r0 < r1 <= n_scans")

    expect(describe(nb=0, rings=0), EINVAL, scan_counts)
    expect(describe(rings=33, hi=0.0), EINVAL, "1 <= n_rings <= 32 is required")
    expect(describe(hi=np.nan, lo=np.nan), EINVAL, MAX_MSG)
    expect(describe(lo=-1.0, a=nan_ang), EINVAL, MIN_MSG)
    expect(describe(a=nan_ang), EINVAL, ANGLES_MSG)

    # between the two halves of a scan update: the state comes after every argument, and rbpf_cast_scans does not look at it
    e.set_scan(rg[0], ang)
    e.map_update(np.zeros((P, 3)))
    e.imu_update("velocity", np.array([0.1, 0.0, 0.0]), 1000.0)
    e.set_scan(rg[1], ang)
    e.scan_update_begin(adj=False)
    for call, what in ((gain, "view gain"), (build, "map building"), (refine, "pose refinement"), (match, "pair matching"), (describe, "scan description")):
        expect(call(a=nan_ang), EINVAL, ANGLES_MSG)
        expect(call(), _lib.RBPF_ESTATE, what + MID)
    for call in (gain, build, refine, match):            # the window limit is an argument check too
        assert call(hi=1000.0) == EINVAL and "needs a window" in e._lib.rbpf_last_error(e._h).decode()
    assert cast() == 0
    e.scan_update_end()
    for call in (cast, gain, build, refine, match, describe):
        assert call() == 0
    e.close()
