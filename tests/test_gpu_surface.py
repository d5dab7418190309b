"""Score surfaces on the GPU (rbpf_score_surface, kernels_surface.hip) against the NumPy oracle of tests/surface_oracle.py: every
record and count bit for bit.  Then the three ways in and out, the surfaces of match_pairs and refine_poses, what the call
leaves alone and its argument checks.  What the numbers mean is asserted on the oracle's figures: the GPU's are pinned to them."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import surface_oracle as so
from tests import surface_scenes as scenes
from tests.test_gpu_locate import engine, load_room, rng_state

pytestmark = pytest.mark.gpu


def records(surf):
    """The library's [N, K, 16] records back from a ScoreSurface."""
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
    idx, sc, size, mom = host(surf.index), host(surf.score), host(surf.size), host(surf.moments)
    return np.concatenate([idx, sc[..., None], size[..., None], mom, np.zeros_like(sc)[..., None]], axis=2), host(surf.count)


def both(e, V, drop, ex, K, what=""):
    surf = e.score_surface(V, drop=drop, exclude=ex, peaks=K)
    rec, cnt = records(surf)
    want, want_cnt = so.surface(V, drop, ex[0], ex[1], K)
    assert rec.dtype == np.int64 and rec.shape == want.shape and cnt.dtype == np.int32
    assert np.array_equal(cnt, want_cnt), (what, cnt, want_cnt)
    bad = np.argwhere(rec != want)
    assert not len(bad), (what, bad[0], rec[tuple(bad[0][:2])] if len(bad) else None, want[tuple(bad[0][:2])] if len(bad) else None)
    # scores do not increase over the peaks; the peak is in its plateau; sum w >= |T|
    for n in range(len(V)):
        c = int(cnt[n])
        assert c >= 1 and np.all(np.diff(rec[n, :c, 3]) <= 0) and np.all(rec[n, :c, 4] >= 1) and np.all(rec[n, :c, 5] >= rec[n, :c, 4])
        assert not rec[n, c:].any()
    return rec, cnt


def volume(rng, N, R, W, top=40):
    return rng.integers(0, top + 1, size=(N, 2 * R + 1, 2 * W + 1, 2 * W + 1)).astype(np.int32)


@pytest.fixture(scope="module")
def eng():
    e = engine(2)
    load_room(e, particle=1)                             # a map nothing here may read or change
    yield e
    e.close()


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------------
def test_one_candidate(eng):
    rec, cnt = both(eng, np.array([[[[17]]]], dtype=np.int32), [4], (1, 1), 3)
    assert cnt.tolist() == [1] and rec[0, 0].tolist() == [0, 0, 0, 17, 1, 5] + [0] * 10


@pytest.mark.parametrize("R,W", [(0, 1), (1, 0), (3, 5), (2, 32), (100, 1)])
def test_three_items_with_their_own_drops(eng, R, W):
    V = volume(np.random.Generator(np.random.PCG64(100 * R + W)), 3, R, W)
    assert V[0].size % 64 != 0
    both(eng, V, [0, 5, 17], (max(1, W // 3), max(1, R // 3)), 3, f"R {R}, W {W}")


def test_the_eight_largest_keys(eng):
    V = volume(np.random.Generator(np.random.PCG64(8)), 2, 2, 4, top=6)      # few values: the tie order decides most places
    rec, cnt = both(eng, V, [0, 2], (0, 0), 8)
    rank = so.tie_rank(4, 2)
    for n in range(2):
        order = np.lexsort((rank.reshape(-1), -V[n].reshape(-1).astype(np.int64)))[:8]
        k, i, j = np.unravel_index(order, V[n].shape)
        assert rec[n, :, :3].tolist() == np.stack([i - 4, j - 4, k - 2], axis=1).tolist() and cnt[n] == 8


def test_an_exclusion_over_the_whole_volume(eng):
    V = volume(np.random.Generator(np.random.PCG64(9)), 2, 3, 4)
    rec, cnt = both(eng, V, [3, 40], (8, 6), 8)
    assert cnt.tolist() == [1, 1] and not rec[:, 1:].any()


def test_a_peak_in_a_corner(eng):
    V = volume(np.random.Generator(np.random.PCG64(10)), 1, 3, 5, top=9)
    V[0, 0, 0, 10] = 100                                 # k = -3, i = -5, j = 5: the box is clipped on three sides
    rec, _ = both(eng, V, [100], (2, 1), 2)             # the floor is 0: the whole clipped box
    assert rec[0, 0, :4].tolist() == [-5, 5, -3, 100] and rec[0, 0, 4] == 2 * 3 * 3


def test_overlapping_boxes(eng):
    V = np.random.Generator(np.random.PCG64(11)).integers(30, 46, size=(1, 5, 11, 11)).astype(np.int32)
    V[0, 2, 5, 5], V[0, 2, 8, 5], V[0, 3, 5, 8] = 50, 49, 48   # (0, 0, 0), (3, 0, 0) and (0, 3, 1): each outside the others' boxes, the boxes overlap
    rec, cnt = both(eng, V, [20], (2, 1), 4)
    assert rec[0, :3, :3].tolist() == [[0, 0, 0], [3, 0, 0], [0, 3, 1]]
    assert rec[0, 0, 4] == 75 and rec[0, 1, 4] == 75 - 30    # every cell is within 20 of 50 and of 49: the second plateau lost i = 1, 2 to the first


def test_constant_volume_at_the_bound_of_the_sums(eng):
    V = np.full((1, 201, 65, 65), 32768, dtype=np.int32)     # R = 100, W = 32; every pass is one tie
    rec, cnt = both(eng, V, [32768], (64, 200), 2, "one box")
    assert cnt.tolist() == [1] and rec[0, 0, :6].tolist() == [0, 0, 0, 32768, V.size, V.size * 32769]
    rec, cnt = both(eng, V, [32768], (21, 66), 8, "eight boxes")
    assert cnt.tolist() == [8] and rec[0, 0, :3].tolist() == [0, 0, 0]


# ---- 2. the ways in and out ------------------------------------------------------------------------------------------------------------
def test_host_and_device_volumes_and_outputs_agree(eng):
    import torch
    V = volume(np.random.Generator(np.random.PCG64(12)), 5, 3, 5)
    drop = np.array([0, 3, 9, 20, 41], dtype=np.int32)
    host = eng.score_surface(V, drop=drop, exclude=(2, 1), peaks=3)
    dev = torch.device("cuda", int(eng.cfg.device))
    tV = torch.from_numpy(V).to(dev)
    mixed = eng.score_surface(tV, drop=drop, exclude=(2, 1), peaks=3)
    device = eng.score_surface(tV, drop=drop, exclude=(2, 1), peaks=3, device=True)
    assert isinstance(mixed.index, np.ndarray) and hasattr(device.index, "data_ptr") and device.index.device == dev
    want = records(host)
    for other in (mixed, device):
        got = records(other)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert np.array_equal(np.asarray(other.drop.cpu() if hasattr(other.drop, "cpu") else other.drop), drop)
    # raw, with out_count NULL and guard words round the device records
    from thesis_amd import _lib
    pad = 32
    buf = torch.full((2 * pad + 5 * 3 * 16,), -77, dtype=torch.int64, device=dev)
    tdrop = torch.from_numpy(drop).to(dev)
    torch.cuda.synchronize()
    rc = eng._lib.rbpf_score_surface(eng._h, C.c_void_p(tV.data_ptr()), 5, 3, 5, C.c_void_p(tdrop.data_ptr()), 2, 1, 3,
                                     C.c_void_p(buf.data_ptr() + 8 * pad), None, _lib.RBPF_SURFACE_DEVICE_IN | _lib.RBPF_SURFACE_DEVICE_OUT)
    assert rc == 0
    eng.synchronize()
    t = buf.cpu().numpy()
    assert np.all(t[:pad] == -77) and np.all(t[-pad:] == -77) and t[pad:-pad].tobytes() == want[0].tobytes()


# ---- 3. the searches' own volumes ---------------------------------------------------------------------------------------------------------
def scene_surface(scene):
    """The oracle's surface of a scene's pair with the engine's defaults: drop = floor(0.05 * 2 n_used), exclusion a quarter
    of the window's width, two peaks.  Returns (records [2, 16], count, m8, volume)."""
    _, m8, V = scenes.oracle_volume(scene)
    s = scene[4]
    drop = int(math.floor(0.05 * (2 * int(m8[5]))))
    rec, cnt = so.surface_one(V, drop, max(1, -(-s["window"] // 2)), max(1, -(-s["rotations"] // 2)), 2)
    return rec, cnt, m8, V


@pytest.mark.parametrize("name", ["corridor", "room", "room_off_centre"])
def test_the_surface_of_a_pair_match(eng, name):
    scene = {"corridor": scenes.corridor, "room": scenes.room, "room_off_centre": lambda: scenes.room((0.5, 0.3))}[name]()
    poses, ranges, angles, pair, search = scene
    assert len(angles) < 100 and (2 * search["rotations"] + 1) * (2 * search["window"] + 1) ** 2 < 2000
    want, want_cnt, m8, V = scene_surface(scene)
    for device in (False, True):
        res = eng.match_pairs(poses, ranges, angles, pair, return_scores=True, device=device, **search)
        surf = eng.score_surface(res)
        rec, cnt = records(surf)
        index, score = (np.asarray(a.cpu()) if device else a for a in (res.index, res.score))
        assert rec[0, 0, :3].tolist() == index[0].tolist() and rec[0, 0, 3] == score[0]      # peak 0 is the search's own best
        assert np.array_equal(rec[0], want) and cnt.tolist() == [want_cnt]
        assert (surf.substeps, surf.rot_step, surf.cell_size) == (search["substeps"], search["rot_step"], search["cell_size"])
    assert np.array_equal(np.asarray(res.scores.cpu())[0], V)


def test_what_the_scenes_say():
    """On the oracle's numbers, to which the test above pins the GPU's."""
    from thesis_amd.engine import ScoreSurface
    def surface(scene):
        rec, cnt, _, _ = scene_surface(scene)
        s = scene[4]
        return ScoreSurface.from_records(rec[None], np.array([cnt], np.int32), np.zeros(1, np.int32), s["substeps"], s["rot_step"], s["cell_size"])
    C2 = surface(scenes.corridor()).second_moment(0)[0]
    # the corridor runs along x: the plateau's second moment is 195 / 52 = 3.75 step^2 = 0.0375 m^2 along it and exactly 0 across it
    assert C2[0, 0] > C2[1, 1] and C2[1, 1] == 0.0
    # the runner-up a quarter turn away scores 157 of 168 = 0.935 at the centre of the room, 80 of 173 = 0.462 off it
    assert surface(scenes.room()).ambiguity()[0] > surface(scenes.room((0.5, 0.3))).ambiguity()[0]


def test_the_surface_of_a_refinement(eng):
    from tests.test_gpu_refine import oracle as refine_oracle
    ang = np.linspace(-0.75 * math.pi, 0.75 * math.pi, 61)
    truth = np.array([[1.0, 1.5, 0.3], [-2.0, 1.0, -1.0]])
    scans = eng.cast_scans(truth, ang, particle=1, max_range=12.0)
    guess = truth + np.array([[0.03, -0.02, 0.004], [-0.04, 0.01, -0.006]])
    kw = dict(S=2, W=5, R=4)
    res = eng.refine_poses(guess, scans, ang, particle=1, substeps=2, window=5, rotations=4, rot_step=math.radians(0.25), return_scores=True)
    surf = eng.score_surface(res, peaks=3)
    rec, cnt = records(surf)
    _, n6, V = refine_oracle(eng, 1, guess, scans, ang, **kw)
    assert np.array_equal(res.scores, V)
    drop = np.floor(0.05 * (2 * n6[:, 5]).astype(np.float64)).astype(np.int64)
    want, want_cnt = so.surface(V, drop, 3, 2, 3)
    assert np.array_equal(rec, want) and np.array_equal(cnt, want_cnt) and np.array_equal(surf.drop, drop)
    assert np.array_equal(rec[:, 0, :3], res.index) and np.array_equal(rec[:, 0, 3], res.score)
    assert np.allclose(surf.poses(guess)[:, 0], res.poses, rtol=0, atol=1e-12)


# ---- 4. what it leaves alone, and what it refuses -----------------------------------------------------------------------------------------
def test_the_engine_is_unchanged(eng):
    def state():
        return eng.poses(), eng.weights(), eng.counters(), rng_state(eng), eng.render_map(1).cells
    before = state()
    eng.score_surface(volume(np.random.Generator(np.random.PCG64(13)), 4, 2, 3), drop=3, peaks=4)
    for a, b in zip(before, state()):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_bad_arguments_write_nothing():
    from thesis_amd import _lib
    P, NB = 3, 16
    e = engine(P, lattice_radius=1)
    N, R, W, K = 2, 1, 2, 3
    V = volume(np.random.Generator(np.random.PCG64(14)), N, R, W)
    drop = np.array([1, 2], dtype=np.int32)
    out, cnt = np.full((N, K, 16), -7, np.int64), np.full(N, -9, np.int32)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(v=V, n=N, r=R, w=W, d=drop, et=1, er=1, k=K, o=out, c=cnt, flags=0):
        return e._lib.rbpf_score_surface(e._h, vp(v), n, r, w, vp(d), et, er, k, vp(o), vp(c), flags)

    def with_(arr, k, val):
        res = arr.copy()
        res[k] = val
        return res
    cases = dict(no_scores=dict(v=None), no_out=dict(o=None), no_items=dict(n=0), neg_items=dict(n=-1), rot_neg=dict(r=-1), rot_101=dict(r=101),
                 window_neg=dict(w=-1), window_33=dict(w=33), ex_t_neg=dict(et=-1), ex_t_65=dict(et=65), ex_r_neg=dict(er=-1), ex_r_201=dict(er=201),
                 no_peaks=dict(k=0), neg_peaks=dict(k=-1), nine_peaks=dict(k=9), flags=dict(flags=4), flags_high=dict(flags=1 << 31),
                 huge=dict(n=2529, r=100, w=32, flags=_lib.RBPF_SURFACE_DEVICE_IN),      # 2529 * 201 * 65^2 >= 2^31, refused before a read
                 drop_neg=dict(d=with_(drop, 1, -1)), drop_high=dict(d=with_(drop, 0, 32769)),
                 score_neg=dict(v=with_(V, (1, 2, 4, 4), -1)), score_high=dict(v=with_(V, (0, 0, 0, 0), 32769)))
    for name, kw in cases.items():
        assert call(**kw) == _lib.RBPF_EINVAL, name
        assert np.all(out == -7) and np.all(cnt == -9), name
    # the ends of the ranges are fine; out_count and drop_n may be NULL
    assert call(v=with_(with_(V, (0, 0, 0, 0), 32768), (1, 1, 1, 1), 0), d=with_(drop, 0, 32768), et=64, er=200, k=8,
                o=np.empty((N, 8, 16), np.int64)) == 0
    assert cnt.tolist() == [1, 1]                        # that box holds the whole volume
    cnt[...] = -9
    assert call(c=None, d=None) == 0 and np.all(cnt == -9)
    want, _ = so.surface(V, None, 1, 1, K)
    assert np.array_equal(out, want)
    out[...] = -7
    # between the two halves of a scan update
    ang = np.linspace(-2.0, 2.0, NB)
    rg = np.tile(np.linspace(1.0, 6.0, NB), (2, 1))
    e.set_scan(rg[0], ang)
    e.map_update(np.zeros((P, 3)))
    e.imu_update("velocity", np.array([0.1, 0.0, 0.0]), 1000.0)
    e.set_scan(rg[1], ang)
    e.scan_update_begin(adj=False)
    assert call() == _lib.RBPF_ESTATE
    assert np.all(out == -7) and np.all(cnt == -9)
    e.scan_update_end()
    assert call() == 0 and np.array_equal(out, so.surface(V, drop, 1, 1, K)[0])
    e.close()
