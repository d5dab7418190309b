"""Pose refinement on the GPU (rbpf_refine_poses, kernels_refine.hip) against the NumPy oracle of tests/refine_oracle.py run
on the rendered maps: the whole score volume, out_n6 and out_pose_n3 bit for bit.  Then what the call leaves alone, its device
outputs, its argument checks, and the loops of thesis_amd/refine.py on a run.  No accuracy is asserted here: the GPU result is
the oracle's, and tests/test_refine_oracle.py carries the accuracy claim."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.cast_oracle import cast, lattice_bounds
from tests.refine_oracle import refine as oracle_refine
from tests.test_gpu_locate import built_engine, engine, load_room, raster, rng_state, seam_maps

pytestmark = pytest.mark.gpu

STEP = math.radians(0.25)


def oracle(e, p, poses, ranges, angles, lo=None, hi=None, S=4, W=12, R=10, step=STEP):
    """The oracle on render_map(p): (poses, n6, scores)."""
    m = e.render_map(p)
    c = e.cfg
    lo = float(c.match_min_range) if lo is None else lo
    hi = float(c.match_max_range) if hi is None else hi
    return oracle_refine(m.cells, m.x0, m.y0, poses, ranges, angles, e.dim / float(c.tile_len_m), float(c.quantum),
                         float(c.occupied_threshold), lo, hi, S, W, R, step)


def gpu(e, p, poses, ranges, angles, lo=None, hi=None, S=4, W=12, R=10, step=STEP, **kw):
    return e.refine_poses(poses, ranges, angles, particle=p, substeps=S, window=W, rotations=R, rot_step=step, min_range=lo,
                          max_range=hi, return_scores=True, **kw)


def assert_same(res, want, what=""):
    poses, n6, scores = want
    got6 = np.concatenate([res.index, res.score[:, None], res.score_guess[:, None], res.n_used[:, None]], axis=1)
    assert res.scores.shape == scores.shape and res.scores.dtype == np.int32, (what, res.scores.shape, scores.shape)
    bad = res.scores != scores
    if bad.any():
        k = tuple(int(q) for q in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: scores differ in {int(bad.sum())} of {bad.size} candidates; first [n, k, i, j] = {k}: got {res.scores[k]}, oracle {scores[k]}")
    assert np.array_equal(got6, n6), (what, got6[np.any(got6 != n6, axis=1)][:4], n6[np.any(got6 != n6, axis=1)][:4])
    assert res.poses.dtype == np.float64 and res.poses.tobytes() == poses.tobytes(), (what, res.poses - poses)


def scans_at(e, p, poses, angles, max_range=12.0):
    return e.cast_scans(np.asarray(poses, dtype=np.float64), angles, particle=p, max_range=max_range)


def both(e, p, poses, ranges, angles, what, **kw):
    res = gpu(e, p, poses, ranges, angles, **kw)
    want = oracle(e, p, poses, ranges, angles, **kw)
    assert_same(res, want, what)
    return res


@pytest.fixture(scope="module")
def room():
    """The asymmetric room in particle 1 of a two-particle engine, 12 poses on its floor and their scans of 181 beams."""
    e = engine(2)
    full = load_room(e, particle=1)
    ang = np.linspace(-0.75 * math.pi, 0.75 * math.pi, 181)
    rng = np.random.Generator(np.random.PCG64(5))
    cells = e.render_map(1).cells
    truth = []
    while len(truth) < 12:
        x, y = rng.uniform(-7.5, 7.5, 2)
        if cells[int(math.floor(x * 20.0)) - full[0], int(math.floor(y * 20.0)) - full[2]] < 0:
            truth.append((x, y, rng.uniform(-math.pi, math.pi)))
    truth = np.array(truth)
    scans = scans_at(e, 1, truth, ang)
    guess = truth + rng.uniform(-1.0, 1.0, (12, 3)) * 0.8 * np.array([0.15, 0.15, 10 * STEP])
    yield e, ang, truth, scans, guess
    e.close()


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------------
def test_one_scan_of_61_beams(room):
    e, ang, truth, scans, guess = room
    a61 = ang[::3]
    assert len(a61) == 61
    res = both(e, 1, guess[3], scans[3, ::3], a61, "61 beams", S=4, W=5, R=3)
    assert res.scores.shape == (1, 7, 11, 11) and res.score[0] >= res.score_guess[0] > 0 and res.n_used[0] > 30
    assert (res.substeps, res.rot_step, res.cell_size) == (4, STEP, 0.05)
    # particle 0 holds no map: every score is 0 and the guess stays
    empty = gpu(e, 0, guess[3], scans[3, ::3], a61, S=4, W=5, R=3)
    assert not empty.scores.any() and empty.index.tolist() == [[0, 0, 0]] and empty.poses.tobytes() == guess[3].tobytes()
    assert empty.n_used[0] == res.n_used[0]


def odd_ranges(scans):
    r = scans.copy()
    r[0, :9] = [np.nan, np.inf, -np.inf, 0.0, -2.0, 0.3, 11.0, 0.2999, 11.0001]      # none of them is used in (0.3, 11)
    r[5, :] = np.nan                                     # a scan without a used beam
    r[7, ::2] = 30.0
    return r


@pytest.mark.parametrize("S,W,R", [(4, 12, 10), (1, 3, 2), (2, 7, 1), (8, 12, 2), (16, 9, 3), (4, 0, 4), (4, 6, 0), (2, 0, 0),
                                   (1, 32, 1), (4, 1, 100)])
def test_a_batch_with_odd_ranges(room, S, W, R):
    e, ang, truth, scans, guess = room
    r = odd_ranges(scans)
    res = both(e, 1, guess, r, ang, f"S {S}, W {W}, R {R}", lo=0.3, hi=11.0, S=S, W=W, R=R)
    assert res.n_used[5] == 0 and res.index[5].tolist() == [0, 0, 0] and res.score[5] == 0
    assert res.n_used[0] == int(np.sum((r[0] > 0.3) & (r[0] < 11.0))) and np.all(res.score <= 2 * res.n_used) and np.all(res.score >= res.score_guess)
    assert res.score.max() > 100


def test_launch_shapes_agree(room, monkeypatch):
    """A scan alone has its rotations split over workgroups, one each; a large batch packs several into one (RBPF_REFINE_KPW
    sets the number here, as a batch this small would get one as well).  Every shape gives the same rows."""
    e, ang, truth, scans, guess = room
    r = odd_ranges(scans)
    kw = dict(lo=0.3, hi=11.0, S=4, W=12, R=10)
    monkeypatch.delenv("RBPF_REFINE_KPW", raising=False)
    whole = gpu(e, 1, guess, r, ang, **kw)
    for n in (0, 5, 11):
        alone = gpu(e, 1, guess[n], r[n], ang, **kw)
        assert np.array_equal(alone.scores[0], whole.scores[n]) and alone.poses.tobytes() == whole.poses[n].tobytes()
        assert alone.index.tolist() == [whole.index[n].tolist()] and alone.score[0] == whole.score[n] and alone.n_used[0] == whole.n_used[n]
    want = oracle(e, 1, guess, r, ang, **kw)
    for kpw in ("5", "2", "16"):                         # 5: what a full batch gets at this window; 21 rotations in runs of 5, 2 and 16
        monkeypatch.setenv("RBPF_REFINE_KPW", kpw)
        assert_same(gpu(e, 1, guess, r, ang, **kw), want, f"{kpw} rotations per workgroup")
    # more tasks than lanes (65 x 9 per rotation) and more beams than the table holds: several passes, several chunks
    monkeypatch.setenv("RBPF_REFINE_KPW", "3")
    a_many = np.linspace(-math.pi, math.pi, 1500, endpoint=False)
    r_many = scans_at(e, 1, truth[:2], a_many)
    both(e, 1, guess[:2], r_many, a_many, "3 rotations per workgroup, 1500 beams, W 32", lo=0.3, hi=11.0, S=2, W=32, R=2)


# ---- 2. lattice and seams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.1])
def test_seams_missing_tiles_and_the_lattice_edge(cs):
    rng = np.random.Generator(np.random.PCG64(int(round(1000 * cs)) + 2))
    e = engine(2, cs=cs, pool_tiles=24, lattice_radius=1)
    seam_maps(e, rng)
    e.load_map(raster(e, (-5, 5, -5, 5), np.full((10, 10), 30, np.int8)), particle=0)     # another map, which must not be seen
    h = e.dim // 2
    last = e.dim + h                                     # lattice_radius 1: mosaic cells [-last, last)
    corner = rng.integers(-30, 31, size=(50, 45)).astype(np.int8)
    e.load_map(raster(e, (last - 50, last, -last, -last + 45), corner), particle=1)       # the lattice's last cells
    inv = e.dim / float(e.cfg.tile_len_m)
    ang = rng.uniform(-np.pi, np.pi, 97)
    edge = last / inv
    guess = np.array([[(h + 3.3) / inv, (h - 2.6) / inv, 0.4], [(-h - 20.2) / inv, (-h - 10.7) / inv, -2.0], [0.31 / inv, 0.77 / inv, 3.0],
                      [(last - 10.4) / inv, (-last + 5.3) / inv, 1.0], [edge + 2.0, edge + 2.0, 0.0], [-edge - 30.0, 0.0, 0.5]])
    r = rng.uniform(0.0, 70.0 / inv, (6, 97))            # end points up to 70 cells away: over the seams into the other rasters
    r[:, :5] = rng.uniform(4.0, 7.0, (6, 5))
    res = both(e, 1, guess, r, ang, f"cs {cs}", lo=0.0, hi=6.0, S=4, W=6, R=2, step=0.01)
    assert res.score[:4].min() > 0 and res.score[5] == 0 and (res.index[:3] != 0).any()   # the last window lies outside the lattice
    e.close()


# ---- 3. 0.025 m ---------------------------------------------------------------------------------------------------------------------
def test_cell_size_0025_at_the_window_limit():
    from thesis_amd.engine import RbpfError
    rng = np.random.Generator(np.random.PCG64(26))
    e = engine(2, cs=0.025, pool_tiles=24, lattice_radius=1)
    seam_maps(e, rng)
    h = e.dim // 2
    most = e.refine_max_range(4, 12)
    # 16384 + (2 Mw + 1) WW 8 <= 163776 bytes admits Mw <= 367 = ceil(max_range * 40) + ceil(W / S) + 2
    for S, W, reach in ((4, 12, 362), (1, 0, 365), (1, 32, 333), (16, 1, 364)):
        m = e.refine_max_range(S, W)
        assert abs(m - reach / 40.0) < 1e-12 and math.ceil(m * 40.0) == reach
    ang = rng.uniform(-np.pi, np.pi, 181)
    r = rng.uniform(0.0, 3.0, (2, 181))
    r[:, :60] = rng.uniform(8.0, 9.2, (2, 60))           # end points up to the window's rim, some beyond max_range
    guess = np.array([[(h + 1.4) / 40.0, (h - 7.7) / 40.0, 0.3], [(-h + 9.1) / 40.0, (-h - 3.2) / 40.0, 2.0]])
    res = both(e, 1, guess, r, ang, "0.025 m at the limit", lo=0.1, hi=most, S=4, W=12, R=1)
    assert res.score.min() > 0 and res.n_used.min() > 120
    for beyond in (most + 1e-9, 11.0):
        with pytest.raises(RbpfError) as err:
            e.refine_poses(guess, r, ang, particle=1, max_range=beyond)
        assert err.value.code == -1 and "9.05" in str(err.value) and "362" in str(err.value)
    e.close()


# ---- 4. a map the filter built ------------------------------------------------------------------------------------------------------
def test_built_maps_best_and_index():
    e, ang, ranges, truth = built_engine(P=3, steps=12)
    rng = np.random.Generator(np.random.PCG64(8))
    a = ang[::6]
    guess = truth[[3, 7, 11]] + rng.uniform(-1.0, 1.0, (3, 3)) * [0.1, 0.1, 0.02]
    r = ranges[[3, 7, 11]][:, ::6]
    res2 = both(e, 2, guess, r, a, "built map, particle 2", S=4, W=8, R=4)
    res0 = both(e, 0, guess, r, a, "built map, particle 0", S=4, W=8, R=4)
    assert not np.array_equal(res2.scores, res0.scores)                   # the particles hold different maps
    best = int(np.argmax(e.weights()))
    got = e.refine_poses(guess, r, a, substeps=4, window=8, rotations=4, return_scores=True)      # particle="best"
    assert_same(got, oracle(e, best, guess, r, a, S=4, W=8, R=4), "best")
    with pytest.raises(ValueError):
        e.refine_poses(guess, r, a, particle="worst")
    with pytest.raises(ValueError):
        e.refine_poses(guess, r[:2], a)
    e.close()


# ---- 5. the tie rule ----------------------------------------------------------------------------------------------------------------
def test_ties_keep_the_guess_and_take_the_shortest_move():
    e = engine(1)
    cells = np.zeros((200, 120), np.int8)
    cells[:, 60] = 30                                    # one wall along x at Y = 40
    e.load_map(raster(e, (-100, 100, -20, 100), cells))
    ang = np.linspace(-0.5, 0.5, 41)
    true = (0.013, 1.0, math.pi / 2)
    lo_, hi_ = lattice_bounds(e.dim, 3)
    r = cast(cells, -100, -20, lo_, hi_, 20.0, 0.1, 1.0, true, ang, 5.0)[0]
    guess = np.array([[0.013, 0.9, math.pi / 2]])
    res = both(e, 0, guess, r[None], ang, "one wall", lo=0.3, hi=11.0, S=4, W=12, R=0)
    i, j, k = res.index[0].tolist()
    assert (i, k) == (0, 0) and j > 0 and res.score[0] == 2 * res.n_used[0] > res.score_guess[0]
    assert np.all(res.scores[0, 0, :, j + 12] == res.score[0])             # a shift along the wall ties: the shortest one wins
    again = both(e, 0, res.poses, r[None], ang, "at the maximum", lo=0.3, hi=11.0, S=4, W=12, R=3)
    assert again.index.tolist() == [[0, 0, 0]] and again.poses.tobytes() == res.poses.tobytes() and again.score[0] == again.score_guess[0]
    e.close()


# ---- 6. device outputs --------------------------------------------------------------------------------------------------------------
def test_device_outputs_equal_host_outputs(room):
    torch = pytest.importorskip("torch")
    from thesis_amd import _lib
    e, ang, truth, scans, guess = room
    kw = dict(lo=0.3, hi=11.0, S=4, W=4, R=2)
    host = gpu(e, 1, guess, scans, ang, **kw)
    dev = gpu(e, 1, guess, scans, ang, device=True, **kw)
    assert isinstance(dev.poses, torch.Tensor) and dev.poses.device.type == "cuda" and dev.poses.dtype == torch.float64
    assert dev.scores.dtype == torch.int32 and dev.index.shape == (12, 3)
    for name in ("poses", "index", "score", "score_guess", "n_used", "scores"):
        assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(host, name)), name
    plain = e.refine_poses(guess, scans, ang, particle=1, substeps=4, window=4, rotations=2, min_range=0.3, max_range=11.0, device=True)
    assert plain.scores is None and torch.equal(plain.poses, dev.poses) and torch.equal(plain.score, dev.score)
    # poisoned buffers: nothing outside the outputs is written; out_pose_n3 alone and out_n6 alone are both admitted
    pad, n = 64, 12
    bp = torch.full((3 * n + 2 * pad,), -77.0, dtype=torch.float64, device=dev.poses.device)
    b6 = torch.full((6 * n + 2 * pad,), -77, dtype=torch.int32, device=dev.poses.device)
    torch.cuda.synchronize()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    g, r = np.ascontiguousarray(guess), np.ascontiguousarray(scans)
    for po, no in ((C.c_void_p(bp.data_ptr() + 8 * pad), None), (None, C.c_void_p(b6.data_ptr() + 4 * pad))):
        rc = e._lib.rbpf_refine_poses(e._h, 1, dp(g), n, dp(r), dp(ang), len(ang), 0.3, 11.0, 4, 4, 2, STEP, po, no, None, _lib.RBPF_REFINE_DEVICE_OUT)
        assert rc == 0
    e.synchronize()
    tp, t6 = bp.cpu().numpy(), b6.cpu().numpy()
    assert np.all(tp[:pad] == -77.0) and np.all(tp[-pad:] == -77.0) and tp[pad:-pad].tobytes() == host.poses.tobytes()
    assert np.all(t6[:pad] == -77) and np.all(t6[-pad:] == -77)
    assert np.array_equal(t6[pad:-pad].reshape(n, 6)[:, :3], host.index) and np.array_equal(t6[pad:-pad].reshape(n, 6)[:, 3], host.score)
    # on a borrowed stream that is torch's current one, no extra synchronisation is needed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = gpu(e, 1, guess, scans, ang, device=True, **kw)
        total = int(d2.scores.sum())                     # consumed by torch in stream order
        same = torch.equal(d2.poses, dev.poses) and torch.equal(d2.scores, dev.scores) and total == int(host.scores.sum())
        e.release_stream()
    assert same


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    P, NB, N = 3, 16, 2
    e = engine(P, lattice_radius=1)
    load_room(e)
    ang = np.linspace(-2.0, 2.0, NB)
    rg = np.tile(np.linspace(1.0, 6.0, NB), (N, 1))
    poses = np.array([[0.5, 0.4, 0.3], [-1.0, 2.0, 1.0]])
    out_p, out_6, out_s = np.full((N, 3), -7.0), np.full((N, 6), -9, np.int32), np.full((N, 3, 5, 5), -11, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(particle=0, p=poses, n=N, r=rg, a=ang, nb=NB, lo=0.3, hi=11.0, S=4, W=2, R=1, step=STEP, op=out_p, o6=out_6, sc=out_s, flags=0):
        return e._lib.rbpf_refine_poses(e._h, particle, dp(p), n, dp(r), dp(a), nb, lo, hi, S, W, R, step, vp(op), vp(o6), vp(sc), flags)

    def with_(arr, k, val):
        out = arr.copy()
        out[k] = val
        return out
    inv = e.dim / float(e.cfg.tile_len_m)
    far = 2.0 ** 30 / (inv * 4)                           # (|g| + max_range) * invS + W reaches 2^30
    cases = dict(particle_high=dict(particle=P), particle_all=dict(particle=-1), no_poses=dict(p=None), no_ranges=dict(r=None),
                 no_angles=dict(a=None), no_outputs=dict(op=None, o6=None), no_scans=dict(n=0), neg_scans=dict(n=-1), no_beams=dict(nb=0),
                 many_beams=dict(nb=16385), huge=dict(n=2 ** 27, nb=16), substeps_0=dict(S=0), substeps_3=dict(S=3), substeps_32=dict(S=32),
                 window_neg=dict(W=-1), window_33=dict(W=33), rot_neg=dict(R=-1), rot_101=dict(R=101), step_neg=dict(step=-0.01),
                 step_nan=dict(step=np.nan), step_inf=dict(step=np.inf), nan_pose=dict(p=with_(poses, (1, 2), np.nan)),
                 inf_pose=dict(p=with_(poses, (0, 0), np.inf)), nan_angle=dict(a=with_(ang, 15, np.nan)), inf_angle=dict(a=with_(ang, 5, -np.inf)),
                 min_neg=dict(lo=-0.1), min_nan=dict(lo=np.nan), max_zero=dict(hi=0.0), max_neg=dict(hi=-1.0), max_inf=dict(hi=np.inf),
                 max_nan=dict(hi=np.nan), far_x=dict(p=with_(poses, (1, 0), far)), far_y=dict(p=with_(poses, (0, 1), -far)),
                 flags=dict(flags=2), flags_high=dict(flags=1 << 31), window_limit=dict(hi=e.refine_max_range(4, 2) + 0.05))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert np.all(out_p == -7.0) and np.all(out_6 == -9) and np.all(out_s == -11), name
    # NaN and infinite ranges are data
    assert call(r=with_(with_(rg, (0, 3), np.nan), (1, 0), np.inf)) == 0 and out_6[0, 5] == NB - 1 and out_6[1, 5] == NB - 1
    out_p[...], out_6[...], out_s[...] = -7.0, -9, -11
    # between the two halves of a scan update
    e.set_scan(rg[0], ang)
    e.map_update(np.zeros((P, 3)))
    e.imu_update("velocity", np.array([0.1, 0.0, 0.0]), 1000.0)
    e.set_scan(rg[1], ang)
    e.scan_update_begin(adj=False)
    assert call() == _lib.RBPF_ESTATE
    assert np.all(out_p == -7.0) and np.all(out_6 == -9) and np.all(out_s == -11)
    e.scan_update_end()
    assert call() == 0 and np.all(out_6[:, 5] == NB)
    # more than 4 GiB of scratch: a score volume of 2^17 scans at the widest search
    big_n = 1 << 17
    assert call(p=np.zeros((big_n, 3)), n=big_n, r=np.ones((big_n, 1)), a=np.zeros(1), nb=1, W=32, R=100, sc=out_s, op=None) == _lib.RBPF_ENOMEM
    e.close()


# ---- 8. read-only ---------------------------------------------------------------------------------------------------------------------
def test_refinements_interleaved_in_a_run_change_nothing():
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
                e.refine_poses(truth[k:k + 2], ranges[k:k + 2], ang, particle=k % P, window=4, rotations=2)
            e.scan_update(adj=False)
            if k == 2:
                w = e.weights()
                w[1] += 250.0
                e.set_state(weights=w)
            e.resample(0.37)                             # an explicit u: the duplicate groups after it are used by the next match
            if e is mixed:
                e.refine_poses(truth[k + 1], ranges[k + 1], ang, particle="best", substeps=2, window=3, rotations=1, return_scores=True)
    np.testing.assert_array_equal(mixed.poses(), plain.poses())
    np.testing.assert_array_equal(mixed.weights(), plain.weights())
    box = plain.map_extent(None)
    assert mixed.map_extent(None) == box
    assert np.array_equal(mixed.render_map(3, box=box).cells, plain.render_map(3, box=box).cells)
    assert mixed.counters()["match_shared"] == plain.counters()["match_shared"]
    assert rng_state(mixed) == rng_state(plain)
    plain.close(); mixed.close()


# ---- 9. end to end --------------------------------------------------------------------------------------------------------------------
def test_a_run_refined_at_half_the_cell_size():
    from thesis_amd import rebuild, refine
    from thesis_amd.datasets import synthetic
    from thesis_amd.slam import ParticleFilter
    steps, nb = 30, 121
    ang, ranges, odo, truth = synthetic.make_log(steps, nb)
    pf = ParticleFilter(64, ang, seed=5, history="device", keep_scans=True)
    pf.map_update(ranges[0])
    for k in range(steps):
        pf.imu_update(odo[k], 1000.0)
        pf.map_update(ranges[k + 1])
        pf.resample()
    e = pf.engine
    search = dict(substeps=4, window=8, rotations=4, max_range=8.0)
    out = refine.refine_trajectory(e, pf.scans, ang, particle="best", rounds=1, cell_size=0.025, build_args=dict(max_range=8.0), **search)
    assert out.records.tolist() == pf.scans.records and out.poses.shape == (steps + 1, 3) and len(out.rounds) == 1
    rnd = out.rounds[0]
    assert 0.0 < rnd.before <= rnd.after <= 1.0 and 0 <= rnd.moved <= steps + 1
    box = (out.built.x0, out.built.x0 + out.built.hits.shape[0], out.built.y0, out.built.y0 + out.built.hits.shape[1])
    again = e.build_map(out.poses, ranges, ang, cell_size=0.025, box=box, max_range=8.0)
    assert np.array_equal(again.hits, out.built.hits) and np.array_equal(again.seen, out.built.seen) and out.built.cell_size == 0.025
    # the same round by hand in an engine of our own: every scan scores at least what its guess scored
    start = e.trajectory("best")[pf.scans.records]
    me = engine(1, cs=0.025, pool_tiles=16)
    me.place_map(rebuild.as_source(rebuild.rebuild_at(e, start, ranges, ang, cell_size=0.025, box=box, max_range=8.0), engine=e), particle=0)
    res = me.refine_poses(start, ranges, ang, particle=0, **search)
    assert np.all(res.score >= res.score_guess) and res.poses.tobytes() == out.poses.tobytes()
    assert rnd.moved == len(refine.moved(res)) and rnd.after == float(np.mean(refine.fraction(res)))
    print(f"refined run: fraction {rnd.before:.4f} -> {rnd.after:.4f}, {rnd.moved} of {steps + 1} scans moved")
    me.close()
    pf.close()


def test_follow_in_the_loaded_room_equals_the_oracle_loop():
    from thesis_amd import refine
    from thesis_amd.datasets import mapsim, synthetic
    e = engine(1, seed=5)
    load_room(e)
    ang = synthetic.beam_angles(181)
    truth = synthetic.circle_trajectory(8) + np.array([0.33, 0.41, 0.0])
    _, ranges, odo, _ = mapsim.make_log(e, 0, truth, ang)
    step = np.abs(np.diff(truth, axis=0)).max(axis=0)
    search = dict(substeps=2, window=int(math.ceil(step[:2].max() * 40.0)) + 2, rotations=int(math.ceil(step[2] / 0.01)) + 1, rot_step=0.01)
    path, frac = refine.follow(e, ranges, ang, truth[0], particle="best", **search)
    pose, want = truth[0], []
    for r in ranges:
        pose = oracle(e, 0, [pose], r[None], ang, S=search["substeps"], W=search["window"], R=search["rotations"], step=0.01)[0][0]
        want.append(pose)
    assert path.shape == (len(ranges), 3) and path.tobytes() == np.array(want).tobytes() and np.all(frac > 0.3)
    e.close()
