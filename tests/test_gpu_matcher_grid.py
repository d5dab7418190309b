"""The scan matcher's grid stage (match_kernel) against its CPU restatement, oracle/matcher_oracle.py grid_search.

Pose bit for bit, score exactly, covariance to rtol 1e-12 (its sums run in another order and use the device's exp).  The
sines and cosines come from the device (ParticleEngine.native_sincosf), so every beam position is the kernel's own.
Every engine runs with ndt_refine=0: with the NDT stage on, its pose may replace the grid one (that stage on the same
paths: tests/test_gpu_matcher_ndt.py, which borrows the helpers below)."""
import numpy as np
import pytest

from oracle import matcher_oracle as mo

pytestmark = pytest.mark.gpu

PI = np.pi


def rot(th):
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, -s], [s, c]])


@pytest.fixture(scope="module")
def eng():
    from thesis_amd.engine import ParticleEngine
    e = ParticleEngine(2, max_beams=4095, ndt_refine=0)
    yield e
    e.close()


def room(half, mcs, rng=None, clutter=0, thick=2, centre=(0.0, 0.0)):
    """Cell-corner points of a square room of half-width `half` metres, walls `thick` cells, optional clutter."""
    k = int(round(half / mcs))
    line = np.arange(-k, k + 1)
    pts = []
    for t in range(thick):
        for s in (-1, 1):
            pts += [np.stack([np.full_like(line, s * (k + t)), line], 1), np.stack([line, np.full_like(line, s * (k + t))], 1)]
    p = np.unique(np.concatenate(pts), axis=0).astype(np.float64)
    if clutter:
        p = np.concatenate([p, rng.integers(-k + 3, k - 3, size=(clutter, 2)).astype(np.float64)])
    return p * mcs + np.asarray(centre)


def seen_from(ref, pose, guess_th=0.0):
    """ref points as a sensor at `pose` sees them, expressed in the rotation of a guess with heading guess_th."""
    return (ref - np.asarray(pose[:2])) @ rot(pose[2] - guess_th)


def check_twin(eng, curr, ref, guess, cpm, rng3, sincos="device"):
    from thesis_amd.engine import match_scan
    sc = eng.native_sincosf if sincos == "device" else mo.np_sincos
    pose, cov, score = match_scan(eng, curr, ref, guess, cpm, rng3)
    wp, wc, ws, r = mo.match_scan_oracle(curr, ref, guess, cpm, rng3, sincos=sc)
    assert np.array_equal(pose, wp), (pose, wp)
    assert score == ws, (score, ws)
    np.testing.assert_allclose(cov, wc, rtol=1e-12, atol=1e-17)
    assert not r["edge_effect"]
    return pose, cov, score, r


@pytest.mark.parametrize("cpm", [10, 20, 40])
@pytest.mark.parametrize("off", [(0.21, -0.13, 0.07), (-0.36, 0.27, -0.31)])
def test_twin_resolutions(eng, cpm, off):
    """W = 11 / 21 / 21 (40 cells/m runs at ds = 2): the non-DPP dilation; pi/6 rotations in groups (n_groups > 1)."""
    rng = np.random.Generator(np.random.PCG64(cpm))
    mcs = 1.0 / cpm
    ref = room(4.0, mcs, rng, clutter=300)
    guess = np.array([0.03, -0.02, 0.4])
    curr = seen_from(ref, guess + off, guess[2])[rng.permutation(len(ref))[:1500]]
    _, _, _, r = check_twin(eng, curr, ref, guess, cpm, [0.7, 0.7, PI / 6])
    assert r["N"] // 32 in (11, 21) and r["nr"] > 1


def test_twin_translation_only_needs_no_device_sincos(eng):
    """Heading 0 and a rotation range below d0: only rotation 0 is valid, so the CPU's sin/cos (0 and 1) are exact and
    the oracle is checked without the device entry."""
    mcs = 0.05
    ref = room(3.0, mcs, thick=1)
    for shift in [(3, -2), (-9, 5), (0, 0), (13, 13)]:
        curr = ref[::2] - np.array(shift) * mcs
        pose, cov, score, r = check_twin(eng, curr, ref, [0.0, 0.0, 0.0], 20, [0.7, 0.7, 0.003], sincos="cpu")
        assert r["ncr"] == 0 and np.array_equal(pose, [shift[0] * mcs, shift[1] * mcs, 0.0])


@pytest.mark.parametrize("rng3", [(0.9, 0.9, 0.2), (1.5, 0.4, 0.2), (0.4, 1.5, 0.1)])
def test_twin_wide_windows(eng, rng3):
    """nty > 8 (several passes of 8 y translations, NP > 1) and ntx > 7 (several t0 passes)."""
    rng = np.random.Generator(np.random.PCG64(7))
    ref = room(5.0, 0.05, rng, clutter=400)
    curr = seen_from(ref, (0.6 * rng3[0], -0.7 * rng3[1], 0.05))[::3]
    _, _, _, r = check_twin(eng, curr, ref, [0.0, 0.0, 0.0], 20, list(rng3))
    assert r["NP"] > 1 or r["ntx"] > 7


def test_twin_coarse_candidate_index_past_16_bits(eng):
    """pose_range (3, 3, pi/6) at 20 cells/m: 79 rotations x 29 x 29 = 66 439 coarse candidates.  The optimum lies in
    the last rotation (+0.515 rad), whose indices are all >= 65 536: a 16-bit key would decode it as a rotation near
    -0.52 rad."""
    rng = np.random.Generator(np.random.PCG64(5))
    ref = room(6.0, 0.05, rng, clutter=300)
    ref = np.concatenate([ref, room(2.0, 0.05, centre=(1.3, -2.1))])
    true = (0.35, -0.2, 0.515)
    curr = seen_from(ref, true)[::2]
    pose, cov, score, r = check_twin(eng, curr, ref, [0.0, 0.0, 0.0], 20, [3.0, 3.0, PI / 6])
    assert r["nr"] * r["ntx"] * r["nty"] == 66439
    assert np.all(np.isfinite(cov)) and abs(pose[2] - true[2]) < 0.01 and abs(pose[0] - true[0]) < 0.06


@pytest.mark.parametrize("guess", [(0.0249, 0.0751, PI - 0.01), (-0.0251, -0.0749, -PI + 0.02), (13.337, -7.613, 3.1),
                                   (-0.0125, 0.0375, -3.14159)])
def test_twin_guess_rounding(eng, guess):
    """Guesses at non-integer cell offsets of both parities and headings near +-pi: remainder() and the float fx / fy."""
    rng = np.random.Generator(np.random.PCG64(3))
    ref = room(4.0, 0.05, rng, clutter=200, centre=guess[:2])
    curr = seen_from(ref, np.array(guess) + [0.11, -0.07, 0.04], guess[2])[::2]
    check_twin(eng, curr, ref, list(guess), 20, [0.7, 0.7, PI / 6])


def test_twin_exact_ties(eng):
    """A symmetric room seen from its centre: many candidates share the best score at both levels and the tie-break rules
    decide the answer."""
    ref = room(3.0, 0.05, thick=2)
    curr = ref[::4].copy()
    pose, _, _, r = check_twin(eng, curr, ref, [0.0, 0.0, 0.0], 20, [0.7, 0.7, PI / 6])
    assert (r["fine"] == r["best"]).sum() > 1 and (r["coarse"] == r["coarse"].max()).sum() > 1


@pytest.mark.parametrize("cpm", [10, 20])
def test_twin_region_edges(eng, cpm):
    """Curr points beyond 15 m, ref points at the 15 m edge, a wide window: the pass drops at the region edge and the
    zero pad rows change no score."""
    rng = np.random.Generator(np.random.PCG64(cpm + 1))
    a = np.linspace(-PI, PI, 3000, endpoint=False)
    ref = np.concatenate([np.stack([14.98 * np.cos(a), 14.98 * np.sin(a)], 1), room(3.0, 1.0 / cpm)])
    curr = np.concatenate([seen_from(ref, (0.4, -0.3, 0.02))[::2], rng.uniform(-19, 19, size=(800, 2))])
    check_twin(eng, curr, ref, [0.0, 0.0, 0.0], cpm, [1.5, 1.5, 0.2])


def test_twin_more_than_2880_beams(eng):
    """4000 beams: the fine level's 120-beam byte-lane chunks run more than 6 times per slice."""
    rng = np.random.Generator(np.random.PCG64(8))
    ref = room(5.0, 0.05, rng, clutter=4000)
    curr = seen_from(ref, (0.2, 0.1, -0.05))[rng.permutation(len(ref))[:4000]]
    assert len(curr) == 4000
    check_twin(eng, curr, ref, [0.0, 0.0, 0.0], 20, [0.7, 0.7, PI / 6])


def test_twin_empty_field(eng):
    """No overlap: pose at the guess, NaN covariance, score 0."""
    rng = np.random.Generator(np.random.PCG64(3))
    curr = rng.uniform(-5, 5, size=(100, 2))
    for ref in (rng.uniform(40, 45, size=(50, 2)), np.zeros((0, 2))):
        pose, cov, score, r = check_twin(eng, curr, ref, [0.5, -0.5, 0.2], 20, [0.5, 0.5, PI / 6])
        assert np.isnan(cov).all() and score == 0.0 and not r["ok"]


def test_twin_fuzz(eng):
    """150 seeded problems (rooms, offsets, windows, resolutions), compared exactly.  Prints how often the two-level
    search misses the best full-resolution score of an exhaustive search over the whole window (every 4th beam)."""
    rng = np.random.Generator(np.random.PCG64(2024))
    gaps = []
    for i in range(150):
        cpm = int(rng.choice([10, 20, 40]))
        mcs = 1.0 / cpm
        ref = room(rng.uniform(1.5, 5.0), mcs, rng, clutter=int(rng.integers(0, 200)), thick=int(rng.integers(1, 3)))
        win = [rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.02, PI / 6)]
        guess = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-PI, PI)])
        off = np.array([rng.uniform(-0.8, 0.8) * win[0], rng.uniform(-0.8, 0.8) * win[1], rng.uniform(-0.8, 0.8) * win[2]])
        curr = seen_from(ref, guess + off, guess[2])
        curr = curr[rng.permutation(len(curr))[:int(rng.integers(50, 1500))]]
        _, _, _, r = check_twin(eng, curr, ref, guess, cpm, win)
        if r["ok"] and i % 3 == 0:                       # the exhaustive search is slow: every third problem
            occ, ox, oy = mo.rasterise_fast(ref, guess, r["mcs"], r["N"], 0.5, 15.0)
            bx, by = mo.beams_f32(curr, r["mcs"])
            ex, _ = mo.exhaustive_best(occ, ox, oy, bx, by, guess, win, r["mcs"], r["d0"], 0.5, eng.native_sincosf)
            gaps.append(ex - r["best"])
    gaps = np.array(gaps)
    print(f"two-level vs exhaustive: {np.count_nonzero(gaps > 0)} of {len(gaps)} problems below the exhaustive best; "
          f"gap mean {gaps.mean():.2f}, max {gaps.max()} (fine-level score units)")
    assert np.all(gaps >= 0)


# ---- particle path: rbpf_scan_update_begin's built-in matcher, read back with match_results -----------------------------
def mapped_engine(P, poses, cs=0.05, B=1081, n_scans=3, ndt_refine=0, **kw):
    from thesis_amd.engine import ParticleEngine
    from thesis_amd.datasets import synthetic
    ang = synthetic.beam_angles(B)
    rng = np.random.Generator(np.random.PCG64(11))
    e = ParticleEngine(P, max_beams=B, cell_size=cs, pool_tiles=8 * P, ndt_refine=ndt_refine, **kw)
    for _ in range(n_scans):
        e.set_scan(synthetic.cast_scan((0.0, 0.0, 0.0), ang, rng), ang)
        e.map_update(poses)
    return e, ang, rng


def oracle_particle(e, p, x, y, pose, cov, adj, last=None, sincos=None):
    """The grid stage's oracle for particle p.  The dict also carries what the NDT stage's oracle needs (occ, origin,
    beams, window, mcs, pose).  sincos: the device's (e.native_sincosf) unless given."""
    cfg = e.cfg
    N, ds, mcs, d0, ncr = mo.match_geometry(cfg.cell_size, cfg.match_max_range)
    beams = mo.select_beams(x, y, cfg.match_min_range, cfg.match_max_range, adj)
    bx, by = mo.beams_f32(beams, mcs)
    rx, ry = mo.window_from_cov(cov[0, 0], cov[1, 1])
    if adj:
        occ, ox, oy = mo.rasterise_fast(last, pose, mcs, N, 0.0, cfg.match_max_range)
    else:
        tiles = dict(e.tiles(p))
        occ, ox, oy = mo.field_from_tiles(tiles, pose, N, ds, mcs, cfg.cell_size, float(cfg.tile_len_m), cfg.lattice_radius,
                                          int(np.floor(cfg.occupied_threshold / cfg.quantum + 1e-9)))
    r = mo.grid_search(occ, ox, oy, bx, by, pose, (rx, ry, PI / 6), mcs, d0, ncr, 0.0, sincos or e.native_sincosf)
    r.update(N=N, ds=ds, mcs=mcs, occ=occ, ox=ox, oy=oy, bx=bx, by=by, window=(rx, ry, PI / 6), pose=np.array(pose, dtype=np.float64))
    return r


def check_particles(e, x, y, adj=False, last=None, refresh=False):
    poses, covs = e.poses(), e.covs()
    pre = [oracle_particle(e, p, x, y, poses[p], covs[p], adj, last) for p in range(e.P)]
    e.set_scan_xy(x, y)
    if adj and refresh:
        e.scan_update_begin(adj=True, last_scan_xy=None)
    else:
        e.scan_update_begin(adj=adj, last_scan_xy=last)
    got = e.match_results()
    e.scan_update_end()
    for p in range(e.P):
        w = pre[p]["out"]
        assert np.array_equal(got[p, :3], w[:3]), (p, got[p, :3], w[:3])
        assert got[p, 12] == w[12], (p, got[p, 12], w[12])
        np.testing.assert_allclose(got[p, 3:12], w[3:12], rtol=1e-12, atol=1e-17)
        assert not pre[p]["edge_effect"]
    return pre, got


def scan_xy_at(pose, rng, B=1081):
    from thesis_amd.datasets import synthetic
    from oracle import rbpf_oracle as orc
    ang = synthetic.beam_angles(B)
    r = synthetic.cast_scan(pose, ang, rng)
    return orc.scan_xy(r, ang)


@pytest.mark.parametrize("cs,W", [(0.05, 16), (0.025, 16), (0.1, 8)])
def test_particle_path_own_map(cs, W):
    """adj = 0 (mode 0): the field staged from the particle's own map, window from its covariance.  0.05 m: W = 16, the
    DPP dilation; 0.025 m: ds = 2 staging; 0.1 m: W = 8."""
    P = 4
    poses = np.zeros((P, 3))
    e, ang, rng = mapped_engine(P, poses, cs=cs)
    try:
        e.set_state(poses=[[0.08, -0.05, 0.03], [-0.1, 0.12, -0.04], [0.0, 0.0, 0.0], [0.2, 0.2, 0.1]],
                    covs=[np.diag([1e-4, 4e-5, 1e-5]), np.diag([1e-6, 1e-6, 1e-6]), np.diag([4e-4, 4e-4, 1e-4]),
                          np.diag([2e-5, 3e-4, 1e-5])])
        x, y = scan_xy_at((0.0, 0.0, 0.0), rng)
        pre, got = check_particles(e, x, y)
        assert pre[0]["N"] // 32 == W and all(np.isfinite(got[:, 3]))
    finally:
        e.close()


def test_particle_path_max_range_15():
    """match_max_range = 15 m at 0.05 m: mode 0 with W = 21 (no DPP dilation)."""
    e, ang, rng = mapped_engine(3, np.zeros((3, 3)), match_max_range=15.0)
    try:
        e.set_state(poses=[[0.05, -0.1, 0.02], [-0.15, 0.0, -0.05], [0.1, 0.1, 0.0]], covs=np.diag([1e-4, 1e-4, 1e-5]))
        x, y = scan_xy_at((0.0, 0.0, 0.0), rng)
        pre, _ = check_particles(e, x, y)
        assert pre[0]["N"] // 32 == 21
    finally:
        e.close()


def seam_engine(ndt_refine=0):
    """Four particles on the negative side of a tile and across the tile seams at +-20 m, each with a two-scan map of a
    lobed room round it; returns the engine and the scan (x, y) to match."""
    poses = np.array([[-11.0, -12.5, 0.3], [-19.6, -3.2, -1.2], [19.9, 20.3, 2.0], [-0.3, 19.8, 1.0]])
    P = len(poses)
    from thesis_amd.engine import ParticleEngine
    from thesis_amd.datasets import synthetic
    from oracle import rbpf_oracle as orc
    ang = synthetic.beam_angles(1081)
    rng = np.random.Generator(np.random.PCG64(4))
    e = ParticleEngine(P, max_beams=1081, pool_tiles=64, ndt_refine=ndt_refine)
    try:
        for k in range(2):
            r = 5.0 + 2.0 * np.sin(3 * ang + k) + rng.normal(0, 0.01, 1081)
            e.set_scan(r, ang)
            e.map_update(poses)
        e.set_state(poses=poses + [0.08, -0.05, 0.02], covs=np.diag([4e-5, 4e-5, 1e-5]))
    except Exception:
        e.close()
        raise
    x, y = orc.scan_xy(5.0 + 2.0 * np.sin(3 * ang + 1), ang)
    return e, x, y


def test_particle_path_negative_side_and_tile_seam():
    """Particles on the negative side of a tile and across the tile seams at +-20 m: the index map's defect columns and
    slow words, against the reference's write formula."""
    e, x, y = seam_engine()
    try:
        check_particles(e, x, y)
    finally:
        e.close()


@pytest.mark.parametrize("refresh", [False, True])
def test_particle_path_adjacent_scan(refresh):
    """adj = 1 (mode 1): the previous scan rasterised with cell_off 0 and the match_max_range (11 m) filter, from the host
    list or from the device-resident scan of refresh_last_scan."""
    from oracle import rbpf_oracle as orc
    P = 3
    true0 = np.array([0.5, -0.3, 0.2])
    e, ang, rng = mapped_engine(P, np.broadcast_to(true0, (P, 3)))
    try:
        x0, y0 = scan_xy_at(true0, rng)
        gx, gy = orc.transform(x0, y0, tuple(true0))
        last = np.stack([gx, gy], axis=1)
        if refresh:
            e.set_state(poses=true0)
            e.set_scan_xy(x0, y0)
            e.refresh_last_scan(0)
        e.set_state(poses=[[0.8, -0.1, 0.3], [0.75, -0.2, 0.25], [0.9, 0.0, 0.35]], covs=np.diag([1e-4, 1e-4, 1e-5]))
        x, y = scan_xy_at((0.8, -0.1, 0.3), rng)
        check_particles(e, x, y, adj=True, last=last, refresh=refresh)
    finally:
        e.close()


def test_particle_path_duplicates_after_resample():
    """After a resample that leaves duplicates the matcher runs once per group; match_results reports the
    representative's row for every copy, and each row equals the oracle's for that particle."""
    P = 6
    e, ang, rng = mapped_engine(P, np.zeros((P, 3)))
    try:
        e.set_state(poses=[[0.05 * i, -0.03 * i, 0.01 * i] for i in range(P)], covs=np.diag([1e-4, 1e-4, 1e-5]),
                    weights=[300.0, 0, 0, 299.0, 0, 0])
        did, idx = e.resample(0.37)
        assert did and len(set(idx.tolist())) < P
        before = e.counters()["match_shared"]
        x, y = scan_xy_at((0.0, 0.0, 0.0), rng)
        check_particles(e, x, y)
        assert e.counters()["match_shared"] > before
    finally:
        e.close()


def test_particle_path_empty_map_and_state_errors():
    """An empty map: every row takes the NaN branch (pose at the guess, score 0).  match_results refuses after a
    match_override."""
    from thesis_amd.engine import ParticleEngine, RbpfError
    from thesis_amd.datasets import synthetic
    ang = synthetic.beam_angles(361, PI)
    e = ParticleEngine(3, max_beams=361, ndt_refine=0)
    try:
        with pytest.raises(RbpfError):
            e.match_results()
        e.set_state(poses=[0.1, 0.2, 0.05])
        from oracle import rbpf_oracle as orc
        x, y = orc.scan_xy(synthetic.cast_scan((0, 0, 0), ang, None), ang)
        pre, got = check_particles(e, x, y)
        assert np.isnan(got[:, 3:12]).all() and np.all(got[:, 12] == 0.0)
        e.scan_update(match_override=got)
        with pytest.raises(RbpfError):
            e.match_results()
    finally:
        e.close()
