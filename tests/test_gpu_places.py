"""Places by appearance on the GPU (rbpf_describe_scans, rbpf_match_places, kernels_places.hip) against the NumPy oracle of
tests/places_oracle.py: descriptors, counts and the k best references of every query bit for bit.  Then the launch shape, the
device tables and outputs, the argument checks, what the calls leave alone, and thesis_amd/loops.py's appearance path on a
run.  No accuracy is asserted here: the GPU result is the oracle's, and tests/test_places_oracle.py and
tests/test_loops_appearance.py carry the accuracy claims."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.places_oracle import OracleEngine, describe, match_places as oracle_places, to_bits, to_words
from tests.test_gpu_locate import engine, load_room, rng_state

pytestmark = pytest.mark.gpu

LO, HI = 0.3, 12.0
NQ, NR = 96, 131                                         # multiples of no tile size: 4 queries a workgroup, 32 references a tile


@pytest.fixture(scope="module")
def eng():
    e = engine(2)
    load_room(e, particle=1)                             # a map nothing here may read
    yield e
    e.close()


def scans_of(B, seed):
    """37 scans of B beams: ranges on both sides of (LO, HI), what is not a range, the ends of the interval, many beams in one
    cell, one scan without a used beam; angles below -pi, above 2 pi and negative."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ang = np.linspace(-1.3 * math.pi, 2.4 * math.pi, B) if B > 1 else np.array([-4.0])
    rg = rng.uniform(-1.0, 14.0, (37, B))
    special = [np.nan, np.inf, -np.inf, 0.0, -2.0, LO, HI, np.nextafter(HI, 0.0), np.nextafter(LO, 1.0), np.nextafter(HI, 20.0)]
    for n in range(0, 37, 5):
        for j, v in enumerate(special):
            rg[n, (n + 3 * j) % B] = v
    rg[7] = 5.0                                          # every beam of a sector in one cell
    rg[8] = np.nextafter(HI, 0.0)                        # the clamp to ring R - 1
    rg[9] = np.where(np.arange(B) % 2 == 0, 0.2, 30.0)   # no used beam
    rg[10] = np.nan
    return rg, ang


def tables(R, seed=5):
    """(queries [96, R], references [131, R]).  References: sparse random images of several densities; 100 .. 109 copies of 0 ..
    9; 110 .. 114 empty; 115 periodic in the sector, 116 the same turned by 3; 117 .. 130 dense.  Queries: 0 .. 59 references
    turned and disturbed; 60 .. 69 empty; 70 periodic; 71 .. 95 dense."""
    rng = np.random.Generator(np.random.PCG64(seed + R))
    rb = np.zeros((NR, R, 64), dtype=bool)
    for r in range(100):
        rb[r] = rng.random((R, 64)) < (0.02, 0.06, 0.15)[r % 3]
    rb[100:110] = rb[0:10]
    rb[115] = to_bits(np.full((1, R), 0x0101010101010101, dtype=np.uint64))[0]
    rb[116] = np.roll(rb[115], 3, axis=-1)
    rb[117:] = rng.random((NR - 117, R, 64)) < 0.5
    qb = np.zeros((NQ, R, 64), dtype=bool)
    for q in range(60):
        src = rb[(7 * q) % 110]
        qb[q] = np.roll(src, -int(rng.integers(0, 64)), axis=-1) ^ (rng.random((R, 64)) < 0.01)
    qb[70] = rb[115]
    qb[71:] = rng.random((NQ - 71, R, 64)) < 0.5
    return to_words(qb), to_words(rb)


def limits(kind):
    return {"none": None, "triangular": np.minimum((np.arange(NQ) * 3) // 2, NR).astype(np.int32), "zero": np.zeros(NQ, np.int32)}[kind]


def assert_same(res, want, what=""):
    out4, out2 = want
    got4 = np.stack([res.ref, res.shift, res.score, res.weight], axis=-1)
    assert got4.shape == out4.shape and got4.dtype == np.int32, (what, got4.shape, out4.shape)
    bad = np.any(got4 != out4, axis=-1)
    if bad.any():
        q, j = (int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} slots differ; first [q, j] = {[q, j]}: got {got4[q, j].tolist()}, oracle {out4[q, j].tolist()}")
    assert np.array_equal(res.n_bits, out2[:, 0]) and np.array_equal(res.count, out2[:, 1]), what


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 70, 181, 1081])
def test_descriptors(eng, B):
    rg, ang = scans_of(B, B)
    for R in (1, 7, 24, 32):
        got = eng.describe_scans(rg, ang, rings=R, min_range=LO, max_range=HI)
        desc, info = describe(rg, ang, R, LO, HI)
        assert got.desc.dtype == np.uint64 and got.desc.shape == (37, R) and np.array_equal(got.desc, desc), (B, R)
        assert np.array_equal(got.n_used, info[:, 0]) and np.array_equal(got.n_bits, info[:, 1]), (B, R)
        assert got.n_used[9] == 0 and got.n_used[10] == 0 and not got.desc[9].any() and got.n_used[8] == B
        assert not got.desc[8, :R - 1].any() and got.desc[8, R - 1] != 0 and got.n_bits[7] <= min(B, 64)
    # the defaults are the configuration's ranges; one output alone is admitted
    own = eng.describe_scans(rg, ang)
    assert np.array_equal(own.desc, describe(rg, ang, 24, float(eng.cfg.match_min_range), float(eng.cfg.match_max_range))[0])
    only = np.full((37, 2), -5, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert eng._lib.rbpf_describe_scans(eng._h, dp(rg), 37, dp(ang), B, LO, HI, 7, None, C.c_void_p(only.ctypes.data), 0) == 0
    assert np.array_equal(only, describe(rg, ang, 7, LO, HI)[1])


@pytest.mark.parametrize("kind", ["none", "triangular", "zero"])
@pytest.mark.parametrize("R", [1, 7, 24, 32])
def test_the_best_references_of_every_query(eng, R, kind):
    qd, rd = tables(R)
    lim = limits(kind)
    for k in (1, 5, 16):
        res = eng.match_places(qd, rd, ref_limit=lim, k=k)
        want = oracle_places(qd, rd, lim, k)
        assert_same(res, want, f"R {R}, {kind}, k {k}")
    if kind == "zero":
        assert not res.count.any() and np.all(res.ref == -1)
        return
    if kind == "none":
        assert res.count[60:70].tolist() == [0] * 10 and not np.isin(res.ref, np.arange(110, 115)).any()   # empty queries, empty references
        assert res.ref[70, 0] == 115 and res.shift[70, 0] == 0                         # eight turns tie: s = 0
        j = res.ref[70].tolist().index(116)
        assert res.shift[70, j] == 61 and res.score[70, j] == res.score[70, 0]         # the copy turned by 3
        if R >= 24:
            assert res.ref[0, :2].tolist() == [0, 100]                                # a copy ranks right behind its original
            assert res.score[71:].max() > 1000                                        # dense images: scores in the thousands
        sim = res.similarity()
        assert sim.shape == (NQ, 16) and 0.0 < sim.max() <= 1.0 and sim[70, 0] == sim[70, 1] and not sim[60].any()
    else:
        assert res.count[0] == 0 and res.count[1] <= 1 and np.all(res.count <= np.minimum(16, lim))   # fewer admitted than k
        assert np.all(res.ref < np.maximum(lim, 1)[:, None])


def test_queries_against_themselves(eng):
    qd, _ = tables(24)
    assert_same(eng.match_places(qd, k=3), oracle_places(qd, qd, None, 3), "one table")
    got = eng.match_places(qd, qd, k=3)
    assert np.all(got.score[:60, 0] > 0) and np.all(got.count[60:70] == 0)


# ---- 2. launch shape -----------------------------------------------------------------------------------------------------------------
def test_the_chunk_length_does_not_show(eng, monkeypatch):
    """RBPF_PLACES_CHUNK sets the references of a (query, chunk) work item; the rank is a strict total order, so the merged
    lists are the same for every chunking.  1 puts every reference in a chunk of its own."""
    qd, rd = tables(24)
    lim = limits("triangular")
    monkeypatch.delenv("RBPF_PLACES_CHUNK", raising=False)
    for use in (None, lim):
        want = oracle_places(qd, rd, use, 5)
        assert_same(eng.match_places(qd, rd, ref_limit=use, k=5), want, "the default chunk")
        for chunk in ("1", "7", "32", "33", "100", "131", "100000"):
            monkeypatch.setenv("RBPF_PLACES_CHUNK", chunk)
            assert_same(eng.match_places(qd, rd, ref_limit=use, k=5), want, f"chunks of {chunk}")
        monkeypatch.delenv("RBPF_PLACES_CHUNK")
    whole = eng.match_places(qd, rd, ref_limit=lim, k=5)
    for q in (0, 1, 37, 70, 95):                         # a query alone gives its row of the batch
        alone = eng.match_places(qd[q], rd, ref_limit=lim[q:q + 1], k=5)
        for name in ("ref", "shift", "score", "weight", "n_bits", "count"):
            assert np.array_equal(getattr(alone, name)[0], getattr(whole, name)[q]), (q, name)


# ---- 3. device tables and outputs ------------------------------------------------------------------------------------------------------
def test_device_tables_and_outputs_equal_the_host_path(eng):
    torch = pytest.importorskip("torch")
    from thesis_amd import _lib
    rg, ang = scans_of(181, 3)
    host = eng.describe_scans(rg, ang, rings=24, min_range=LO, max_range=HI)
    dev = eng.describe_scans(rg, ang, rings=24, min_range=LO, max_range=HI, device=True)
    assert isinstance(dev.desc, torch.Tensor) and dev.desc.device.type == "cuda" and dev.desc.dtype == torch.int64 and dev.n_bits.dtype == torch.int32
    assert np.array_equal(dev.desc.cpu().numpy().view(np.uint64), host.desc)
    assert np.array_equal(dev.n_used.cpu().numpy(), host.n_used) and np.array_equal(dev.n_bits.cpu().numpy(), host.n_bits)
    lim = np.arange(37, dtype=np.int32)
    want = eng.match_places(host.desc, ref_limit=lim, k=4)
    assert_same(want, oracle_places(host.desc, host.desc, lim, 4), "scans")
    for q, r, out in ((dev, None, True), (dev.desc, dev, False), (host, dev.desc, True), (dev, host.desc, False)):
        got = eng.match_places(q, r, ref_limit=lim, k=4, device=out)
        assert isinstance(got.ref, torch.Tensor if out else np.ndarray)
        for name in ("ref", "shift", "score", "weight", "n_bits", "count"):
            a = getattr(got, name)
            assert np.array_equal(a.cpu().numpy() if out else a, getattr(want, name)), name
    assert np.allclose(eng.match_places(dev, ref_limit=lim, k=4, device=True).similarity().cpu().numpy(), want.similarity(), rtol=1e-14, atol=0.0)
    # poisoned buffers: nothing outside the outputs is written; each output alone is admitted
    pad, n, R, k = 64, 37, 24, 4
    bd = torch.full((n * R + 2 * pad,), -77, dtype=torch.int64, device=dev.desc.device)
    bi = torch.full((2 * n + 2 * pad,), -77, dtype=torch.int32, device=dev.desc.device)
    b4 = torch.full((4 * k * n + 2 * pad,), -77, dtype=torch.int32, device=dev.desc.device)
    b2 = torch.full((2 * n + 2 * pad,), -77, dtype=torch.int32, device=dev.desc.device)
    torch.cuda.synchronize()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for do, io in ((C.c_void_p(bd.data_ptr() + 8 * pad), None), (None, C.c_void_p(bi.data_ptr() + 4 * pad))):
        assert eng._lib.rbpf_describe_scans(eng._h, dp(rg), n, dp(ang), 181, LO, HI, R, do, io, _lib.RBPF_PLACES_DEVICE_OUT) == 0
    tab = C.c_void_p(dev.desc.data_ptr())
    for o4, o2 in ((C.c_void_p(b4.data_ptr() + 4 * pad), None), (None, C.c_void_p(b2.data_ptr() + 4 * pad))):
        assert eng._lib.rbpf_match_places(eng._h, tab, n, tab, n, R, lim.ctypes.data_as(C.POINTER(C.c_int32)), k, o4, o2,
                                          _lib.RBPF_PLACES_DEVICE_OUT | _lib.RBPF_PLACES_DEVICE_IN) == 0
    eng.synchronize()
    for buf, body in ((bd, host.desc.view(np.int64)), (bi, np.stack([host.n_used, host.n_bits], axis=1)),
                      (b4, np.stack([want.ref, want.shift, want.score, want.weight], axis=-1)), (b2, np.stack([want.n_bits, want.count], axis=1))):
        t = buf.cpu().numpy()
        assert np.all(t[:pad] == -77) and np.all(t[-pad:] == -77) and np.array_equal(t[pad:-pad], body.reshape(-1))


# ---- 4. arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    P, NB, N, R, K = 3, 16, 4, 6, 3
    e = engine(P, lattice_radius=1)
    ang = np.linspace(-2.0, 2.0, NB)
    rg = np.tile(np.linspace(1.0, 6.0, NB), (N, 1))
    out_d, out_i = np.full((N, R), 7, np.uint64), np.full((N, 2), -9, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def desc(r=rg, n=N, a=ang, nb=NB, lo=0.3, hi=11.0, rings=R, od=out_d, oi=out_i, flags=0):
        return e._lib.rbpf_describe_scans(e._h, dp(r), n, dp(a), nb, lo, hi, rings, vp(od), vp(oi), flags)

    def with_(arr, k, val):
        out = arr.copy()
        out[k] = val
        return out
    cases = dict(no_ranges=dict(r=None), no_angles=dict(a=None), no_outputs=dict(od=None, oi=None), no_scans=dict(n=0), neg_scans=dict(n=-1),
                 no_beams=dict(nb=0), many_beams=dict(nb=16385), huge=dict(n=2 ** 27, nb=16), rings_0=dict(rings=0), rings_33=dict(rings=33),
                 rings_neg=dict(rings=-1), nan_angle=dict(a=with_(ang, 15, np.nan)), inf_angle=dict(a=with_(ang, 5, -np.inf)),
                 min_neg=dict(lo=-0.1), min_nan=dict(lo=np.nan), min_inf=dict(lo=np.inf), max_zero=dict(hi=0.0), max_neg=dict(hi=-1.0),
                 max_inf=dict(hi=np.inf), max_nan=dict(hi=np.nan), flags=dict(flags=2), flags_high=dict(flags=1 << 31))
    for name, kw in cases.items():
        assert desc(**kw) == _lib.RBPF_EINVAL, name
        assert np.all(out_d == 7) and np.all(out_i == -9), name
    assert desc(a=with_(ang, 3, 1e300), r=with_(with_(rg, (3, 3), np.nan), (2, 0), np.inf)) == 0      # any finite angle; NaN and infinite ranges are data
    assert out_i[:, 0].tolist() == [NB, NB, NB - 1, NB - 1]
    assert desc() == 0
    table = out_d.copy()
    out_4, out_2 = np.full((N, K, 4), -11, np.int32), np.full((N, 2), -13, np.int32)
    lim = np.array([4, 0, 2, 4], np.int32)

    def match(q=table, nq=N, r=table, nr=N, rings=R, lm=lim, k=K, o4=out_4, o2=out_2, flags=0):
        return e._lib.rbpf_match_places(e._h, vp(q), nq, vp(r), nr, rings, ip(lm), k, vp(o4), vp(o2), flags)
    cases = dict(no_queries=dict(q=None), no_refs=dict(r=None), no_outputs=dict(o4=None, o2=None), nq_0=dict(nq=0), nq_neg=dict(nq=-1), nr_0=dict(nr=0),
                 nr_neg=dict(nr=-2), huge=dict(nq=2 ** 28, k=8), rings_0=dict(rings=0), rings_33=dict(rings=33), k_0=dict(k=0), k_17=dict(k=17),
                 k_neg=dict(k=-1), limit_neg=dict(lm=with_(lim, 1, -1)), limit_high=dict(lm=with_(lim, 3, N + 1)), flags=dict(flags=4),
                 flags_high=dict(flags=1 << 31))
    for name, kw in cases.items():
        assert match(**kw) == _lib.RBPF_EINVAL, name
        assert np.all(out_4 == -11) and np.all(out_2 == -13), name
    # between the two halves of a scan update
    e.set_scan(rg[0], ang)
    e.map_update(np.zeros((P, 3)))
    e.imu_update("velocity", np.array([0.1, 0.0, 0.0]), 1000.0)
    e.set_scan(rg[1], ang)
    e.scan_update_begin(adj=False)
    out_d[...], out_i[...] = 7, -9
    assert desc() == _lib.RBPF_ESTATE and match() == _lib.RBPF_ESTATE
    assert np.all(out_d == 7) and np.all(out_i == -9) and np.all(out_4 == -11) and np.all(out_2 == -13)
    e.scan_update_end()
    assert desc() == 0 and match() == 0 and np.array_equal(out_d, table)
    assert out_2[:, 1].tolist() == [K, 0, 2, K] and out_4[0, :, 0].tolist() == [0, 1, 2] and out_4[2, 2].tolist() == [-1, 0, 0, 0]
    # more than 4 GiB of scratch: 2^23 queries with a list of 16 entries for each of 2^23 / 256 chunks
    assert match(nq=1 << 23, nr=1 << 23, k=16, o4=None, lm=None) == _lib.RBPF_ENOMEM
    e.close()


# ---- 5. read-only ---------------------------------------------------------------------------------------------------------------------
def test_calls_interleaved_in_a_run_change_nothing():
    from thesis_amd.datasets import synthetic
    P, N, NB = 16, 6, 1081
    ang, ranges, odo, truth = synthetic.make_log(N + 1, NB)
    plain, mixed = engine(P, seed=11), engine(P, seed=11)
    for e in (plain, mixed):
        e.set_scan(ranges[0], ang)
        e.map_update(np.zeros((P, 3)))
    for k in range(N):
        for e in (plain, mixed):
            e.imu_update("velocity", odo[k], 1000.0)
            e.set_scan(ranges[k + 1], ang)
            if e is mixed:
                d = e.describe_scans(ranges[:k + 2], ang, rings=24)
            e.scan_update(adj=False)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)
            if e is mixed:
                found = e.match_places(d, ref_limit=np.arange(k + 2), k=2)
                assert found.count[1:].min() >= 1
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    assert np.array_equal(mixed.render_map(3, box=box).cells, plain.render_map(3, box=box).cells)
    assert mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    assert rng_state(mixed) == rng_state(plain)
    plain.close(); mixed.close()


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------
class OverOracle:
    """The engine with match_pairs, describe_scans and match_places replaced by the oracles."""

    def __init__(self, e):
        self._e = e
        self._o = OracleEngine(float(e.cfg.cell_size), float(e.cfg.match_min_range), float(e.cfg.match_max_range))

    def __getattr__(self, name):
        return getattr(self._e, name)

    def match_pairs(self, *a, **kw):
        return self._o.match_pairs(*a, **kw)

    def describe_scans(self, *a, **kw):
        return self._o.describe_scans(*a, **kw)

    def match_places(self, *a, **kw):
        return self._o.match_places(*a, **kw)


def test_close_loops_by_appearance_equals_the_run_over_the_oracles():
    """A circle of 1 m radius and a quarter more in the loaded asymmetric room; the trajectory gets a drift that grows to 1.2 m
    and 9 degrees, more than radius + window * cell = 0.9 m: the poses propose no pair that holds, the scans do."""
    from thesis_amd import loops, refine
    from thesis_amd.datasets import mapsim, synthetic
    from thesis_amd.slam import ParticleFilter
    room = engine(1, seed=5)
    load_room(room)
    ang = synthetic.beam_angles(121)
    steps = 78
    truth = synthetic.circle_trajectory(steps, radius=1.0, speed=1.0) + np.array([0.33, 0.41, 0.0])
    _, ranges, odo, _ = mapsim.make_log(room, 0, truth, ang)
    room.close()
    pf = ParticleFilter(32, ang, seed=5, history="device", keep_scans=True)
    pf.map_update(ranges[0])
    for k in range(steps):
        pf.imu_update(odo[k], 1000.0)
        pf.map_update(ranges[k + 1])
        pf.resample()
    e = pf.engine
    _, start, _ = refine.scan_poses(e, pf.scans, "best")
    drifted = start + np.linspace(0.0, 1.0, len(start))[:, None] * np.array([1.0, -0.66, math.radians(9.0)])
    args = dict(poses=drifted, min_gap=40, radius=0.5, half_run=2, stride=2, window=8, rotations=4, rot_step=math.radians(1.0), max_range=8.0,
                build_args=dict(max_range=8.0))
    still = loops.close_loops(e, pf.scans, ang, **args)
    assert still.rounds[0].accepted == 0 and still.poses.tobytes() == drifted.tobytes()
    got = loops.close_loops(e, pf.scans, ang, candidates="appearance", **args)
    want = loops.close_loops(OverOracle(e), pf.scans, ang, candidates="appearance", **args)
    assert got.rounds == want.rounds and got.rounds[0].pairs > 8 and got.rounds[0].accepted > 0
    for a, b in zip(got.edges, want.edges):
        assert np.array_equal(a, b)
    assert got.poses.tobytes() == want.poses.tobytes() and got.records.tolist() == pf.scans.records
    assert np.array_equal(got.built.hits, want.built.hits) and np.array_equal(got.built.seen, want.built.seen)
    both = loops.close_loops(e, pf.scans, ang, candidates="both", **args)
    assert got.rounds[0].pairs <= both.rounds[0].pairs <= still.rounds[0].pairs + got.rounds[0].pairs
    if still.rounds[0].pairs == 0:
        assert both.poses.tobytes() == got.poses.tobytes()
    print(f"closed by appearance: {got.rounds[0].pairs} pairs, {got.rounds[0].accepted} accepted, largest move {got.rounds[0].moved:.4f} m; "
          f"fractions {np.round(got.edges.fraction, 2).tolist()}")
    pf.close()
