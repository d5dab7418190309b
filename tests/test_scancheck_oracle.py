"""The scan-check oracle (tests/scancheck_oracle.py) against the cast oracle it shares its ray with, its vectorised form against
the scalar one, and thesis_amd/sensor.py's tables and helpers on the CPU.  The GPU side is tests/test_gpu_scancheck.py."""
import numpy as np
import pytest

from tests import scancheck_oracle as so
from tests import scancheck_scenes as sc
from tests.cast_oracle import cast, lattice_bounds

LO, HI = lattice_bounds(800, 3)
EPS = 1e-9                   # cells: how near a class or bin border a beam may lie before a comparison through e = t / inv skips it


def run_oracle(room, poses, angles, z, model, max_range=sc.MAX_RANGE, min_range=sc.MIN_RANGE, tol=sc.TOL):
    return so.check(lambda n: room, LO, HI, sc.INV, sc.QUANTUM, sc.THRESHOLD, poses, angles, z, max_range, min_range, tol, model)


@pytest.fixture(scope="module")
def room_case():
    """The exact room at 271 beams: the oracle's answer and the cast oracle's, computed once."""
    from thesis_amd.datasets import synthetic
    room = sc.known_room()
    poses, ang, model = sc.all_poses(), synthetic.beam_angles(271), sc.narrow_model()
    z = sc.measured_ranges(sc.true_ranges(*room, LO, HI, poses, ang))
    got = run_oracle(room, poses, ang, z, model)
    casts = [cast(*room, LO, HI, sc.INV, sc.QUANTUM, sc.THRESHOLD, q, ang, sc.MAX_RANGE) for q in poses]
    return dict(room=room, poses=poses, ang=ang, model=model, z=z, got=got, e=np.stack([c[0] for c in casts]), st=np.stack([c[1] for c in casts]))


def test_scene_reaches_every_class_and_both_ends_of_the_hit_table(room_case):
    got, model = room_case["got"], room_case["model"]
    assert set(np.unique(got["classes"]).tolist()) == set(range(8))
    raw = so.raw_bins(got["d"], model)[got["classes"] == so.MATCH]
    assert (raw > model.half_bins).any() and (raw < -model.half_bins).any()
    assert np.array_equal(np.isfinite(got["d"]), (got["classes"] == so.MATCH) | (got["classes"] == so.LONG))


def test_oracle_agrees_with_the_cast_oracle(room_case):
    c = room_case
    z, e, st, cls, d, model = c["z"], c["e"], c["st"], c["got"]["classes"], c["got"]["d"], c["model"]
    ttol = sc.TOL * sc.INV
    with np.errstate(invalid="ignore"):
        skip = ~(z > 0) | (z < sc.MIN_RANGE)
        returned = ~skip & (z < sc.MAX_RANGE)
        noret = ~skip & ~(z < sc.MAX_RANGE)
        above = returned & (st == 1) & (z > e)                       # the wall stands in front of the measured end
        beyond = returned & ((st != 1) | (z + sc.TOL < e - EPS))     # nothing within the measured end plus the tolerance
    assert np.all(cls[skip] == so.SKIP) and skip.sum() > 0
    assert np.all(cls[~skip & (st == 2)] == so.OFF) and np.all((cls == so.OFF) == (~skip & (st == 2)))
    assert np.all(np.isin(cls[above], (so.MATCH, so.LONG))) and above.sum() > 100
    d_e = e * sc.INV - z * sc.INV                                  # d computed from e
    assert np.max(np.abs(d[above] - d_e[above])) < EPS
    clear_of_border = above & (np.abs(d_e + ttol) > EPS)
    assert np.array_equal(cls[clear_of_border] == so.MATCH, d_e[clear_of_border] >= -ttol)
    inside = beyond & (st != 2)
    v_end = end_values(c["room"], c["poses"], c["ang"], z)
    assert np.all(np.isin(cls[inside], (so.SHORT, so.NEW))) and inside.sum() > 100
    assert np.array_equal(cls[inside] == so.SHORT, v_end[inside] < 0)
    assert (cls[inside] == so.SHORT).any() and (cls[inside] == so.NEW).any()
    assert np.array_equal(cls[noret & (st != 2)] == so.MISSING, st[noret & (st != 2)] == 1)
    assert np.all(np.isin(cls[noret & (st != 2)], (so.MISSING, so.CLEAR)))
    # the sums follow from the classes and d
    on_tab = np.isfinite(d)
    q = np.clip(so.raw_bins(np.where(on_tab, d, 0.0), model), -model.half_bins, model.half_bins).astype(int)
    beam_cost = model.class_cost.astype(np.int64)[cls] + np.where(on_tab, model.hit_tab.astype(np.int64)[q + model.half_bins], 0)
    assert np.array_equal(c["got"]["cost"], beam_cost.sum(axis=1))
    assert np.array_equal(c["got"]["counts"], np.stack([(cls == k).sum(axis=1) for k in range(8)], axis=1))
    assert np.array_equal(c["got"]["votes"].sum(axis=1), np.full(len(c["ang"]), len(c["poses"])))


def end_values(room, poses, angles, z):
    cells, x0, y0 = room
    ec = so.end_cells(poses, angles, z, sc.INV)
    i, j = ec[..., 0] - x0, ec[..., 1] - y0
    ok = (i >= 0) & (i < cells.shape[0]) & (j >= 0) & (j < cells.shape[1])
    return np.where(ok, cells[np.clip(i, 0, cells.shape[0] - 1), np.clip(j, 0, cells.shape[1] - 1)], 0)


def test_one_scan_for_every_pose_is_the_scan_repeated(room_case):
    c = room_case
    one = run_oracle(c["room"], c["poses"], c["ang"], c["z"][2], c["model"])
    rep = run_oracle(c["room"], c["poses"], c["ang"], np.repeat(c["z"][2:3], len(c["poses"]), axis=0), c["model"])
    assert all(np.array_equal(one[k], rep[k]) for k in ("cost", "counts", "classes", "votes"))


def test_vectorised_form_equals_the_scalar_one_on_the_room():
    from thesis_amd.datasets import synthetic
    from thesis_amd import sensor
    rng = np.random.Generator(np.random.PCG64(5))
    room = sc.known_room()
    ang = synthetic.beam_angles(181)
    poses = np.concatenate([rng.uniform([-7.5, -7.5, -np.pi], [7.5, 7.5, np.pi], size=(7, 3)), [sc.OUTSIDE_POSE]])
    e30 = sc.true_ranges(*room, LO, HI, poses, ang)
    z = e30 + rng.normal(0.0, 0.08, size=e30.shape)
    z[:, 20:50] -= 1.5
    z[rng.random(z.shape) < 0.05] = np.inf
    z[rng.random(z.shape) < 0.03] = np.nan
    z[rng.random(z.shape) < 0.03] = 0.1

    class Cfg:
        cell_size, weight_max_range = sc.CELL, 25.0
    for model, max_range in ((sensor.beam_model(Cfg), 6.0), (sc.narrow_model(), 30.0)):
        want = run_oracle(room, poses, ang, z, model, max_range=max_range)
        casts = [cast(*room, LO, HI, sc.INV, sc.QUANTUM, sc.THRESHOLD, q, ang, max_range) for q in poses]
        got = so.classify_cast(np.stack([c[0] for c in casts]), np.stack([c[1] for c in casts]), z, sc.INV, max_range, sc.MIN_RANGE, sc.TOL,
                               model, v_end=end_values(room, poses, ang, z))
        for k in ("classes", "cost", "counts", "votes"):
            assert np.array_equal(got[k], want[k]), k
        assert len(np.unique(want["classes"])) >= 6


def test_beam_model_tables():
    from thesis_amd import sensor

    class Cfg:
        cell_size, weight_max_range = 0.05, 25.0
    for kw in ({}, dict(sigma_hit=0.02), dict(sigma_hit=0.2, bins_per_cell=8), dict(z_hit=0.5, z_rand=0.4, scale=1024), dict(z_rand=0.0, sigma_hit=0.01)):
        m = sensor.beam_model(Cfg, **kw)
        t, hb = m.hit_tab, m.half_bins
        assert t.dtype == np.int32 and m.class_cost.dtype == np.int32 and t.shape == (2 * hb + 1,) and m.class_cost.shape == (8,)
        assert 1 <= hb <= 4096 and m.bins_per_cell == kw.get("bins_per_cell", 4) and m.scale == kw.get("scale", 65536)
        assert t.min() >= 0 and t.max() <= 1 << 20 and m.class_cost.min() >= 0 and m.class_cost.max() <= 1 << 20
        assert np.array_equal(t, t[::-1])                              # symmetric
        assert t[hb] == t.min() and np.all(np.diff(t[hb:]) >= 0)       # least at q = 0, non-decreasing in |q|
        assert t[-1] > t[hb]
        assert m.class_cost[sensor.SKIP] == 0 and m.class_cost[sensor.MISSING] > m.class_cost[sensor.CLEAR]
    m = sensor.beam_model(Cfg)
    p0 = 0.85 * 0.09948 + 0.05 * 0.0125 / 25.0                         # bin 0 is +-0.00625 m = +-0.125 sigma: a normal mass of 0.09948
    assert abs(m.hit_tab[m.half_bins] / 65536 + np.log2(p0)) < 0.01    # costs read as bits
    assert m.class_cost[sensor.CLEAR] == round(-65536 * np.log2(0.9))
    assert sensor.beam_model(Cfg, z_rand=0.0, sigma_hit=0.01, z_short=0.0).class_cost[sensor.SHORT] == 1 << 20     # the cap
    with pytest.raises(ValueError):
        sensor.beam_model(Cfg, sigma_hit=0.0)
    with pytest.raises(ValueError):
        sensor.beam_model(Cfg, bins_per_cell=65)


def hand_made(cost, counts, classes=None, votes=None, scale=65536):
    from thesis_amd import sensor
    return sensor.ScanCheck(np.asarray(cost, dtype=np.int64), np.asarray(counts, dtype=np.int32), classes, votes, scale)


def test_scan_check_shares_and_likelihood():
    from thesis_amd import sensor
    chk = hand_made([65536, 0, 3 * 65536], [[2, 6, 0, 2, 0, 0, 0, 0], [10, 0, 0, 0, 0, 0, 0, 0], [0, 5, 1, 1, 1, 0, 1, 1]])
    assert np.array_equal(chk.matched(), [0.75, 0.0, 0.5]) and np.array_equal(chk.share(sensor.SHORT), [0.25, 0.0, 0.1])
    assert np.allclose(chk.log_likelihood(), [-np.log(2.0), 0.0, -3 * np.log(2.0)], rtol=1e-15, atol=0)
    assert (chk.SKIP, chk.MATCH, chk.LONG, chk.SHORT, chk.NEW, chk.OFF, chk.MISSING, chk.CLEAR) == tuple(range(8))
    assert (sensor.SKIP, sensor.MATCH, sensor.LONG, sensor.SHORT, sensor.NEW, sensor.OFF, sensor.MISSING, sensor.CLEAR) == tuple(range(8))


def test_posterior_weights():
    from thesis_amd import sensor
    counts = np.zeros((4, 8), np.int32)
    w = sensor.posterior_weights(hand_made([2 * 65536, 65536, 65536, 4 * 65536], counts))
    assert abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, np.array([0.5, 1.0, 1.0, 0.125]) / 2.625, rtol=1e-15)
    big = hand_made([2 ** 40 + 65536, 2 ** 40, 2 ** 41, 2 ** 40 + 2 * 65536], counts)          # costs of 2^40: no overflow, no NaN
    w = sensor.posterior_weights(big)
    assert np.all(np.isfinite(w)) and abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, np.array([0.5, 1.0, 0.0, 0.25]) / 1.75, rtol=1e-15)
    w = sensor.posterior_weights(big, prior=[1.0, 0.0, 1.0, 2.0])
    assert np.allclose(w, [0.5, 0.0, 0.0, 0.5], rtol=1e-15) and w.dtype == np.float64
    flat = sensor.posterior_weights(big, temperature=2.0)
    assert np.allclose(flat, np.array([0.5 ** 0.5, 1.0, 0.0, 0.5]) / (0.5 ** 0.5 + 1.5), rtol=1e-15)
    assert np.allclose(sensor.posterior_weights(hand_made([65536, 0], counts[:2], scale=32768)), [0.2, 0.8], rtol=1e-15)
    with pytest.raises(ValueError):
        sensor.posterior_weights(big, prior=[0.0, 0.0, 1.0, 0.0] * np.array([1.0, 1.0, 0.0, 1.0]))
    with pytest.raises(ValueError):
        sensor.posterior_weights(big, temperature=0.0)


def test_dynamic_beams_keep_and_lost():
    from thesis_amd import sensor
    rng = np.random.Generator(np.random.PCG64(9))
    N, B = 8, 40
    classes = rng.integers(0, 8, size=(N, B)).astype(np.uint8)
    classes[:, 5] = sensor.SHORT
    classes[:4, 6] = sensor.SHORT                            # exactly half
    classes[4:, 6] = sensor.MATCH
    classes[:3, 7] = sensor.SHORT                            # fewer than half
    classes[3:, 7] = sensor.NEW
    votes = np.stack([(classes == k).sum(axis=0) for k in range(8)], axis=1).astype(np.int32)
    counts = np.stack([(classes == k).sum(axis=1) for k in range(8)], axis=1).astype(np.int32)
    chk = hand_made(np.zeros(N), counts, classes, votes)
    by_votes = sensor.dynamic_beams(chk)
    assert by_votes.dtype == bool and by_votes.shape == (B,) and by_votes[5] and by_votes[6] and not by_votes[7]
    assert np.array_equal(by_votes, votes[:, sensor.SHORT] * 2 >= N)
    assert np.array_equal(sensor.dynamic_beams(chk, weights=np.full(N, 3.0)), by_votes)          # uniform weights: the votes
    assert np.array_equal(sensor.dynamic_beams(chk, min_share=1.0), votes[:, sensor.SHORT] == N)
    w = np.zeros(N)
    w[1] = 1.0
    assert np.array_equal(sensor.dynamic_beams(chk, weights=w), classes[1] == sensor.SHORT)
    with pytest.raises(ValueError):
        sensor.dynamic_beams(hand_made(np.zeros(N), counts, classes, None))
    with pytest.raises(ValueError):
        sensor.dynamic_beams(hand_made(np.zeros(N), counts, None, votes), weights=w)
    ranges, angles = np.arange(B, dtype=np.float64) + 1.0, np.linspace(-1.0, 1.0, B)
    r, a = sensor.keep(ranges, angles, by_votes)
    assert np.array_equal(r, ranges[~by_votes]) and np.array_equal(a, angles[~by_votes]) and len(r) == B - by_votes.sum()
    lo = hand_made([0, 0], [[0, 2, 0, 8, 0, 0, 0, 0], [5, 9, 0, 1, 0, 0, 0, 0]])       # matched 0.2 and 0.9
    assert sensor.lost(lo, weights=[1.0, 0.0]) and not sensor.lost(lo, weights=[0.0, 1.0])
    assert not sensor.lost(lo) and sensor.lost(lo, min_matched=0.56) and not sensor.lost(lo, weights=[1.0, 1.0], min_matched=0.55)
