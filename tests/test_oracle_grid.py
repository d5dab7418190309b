"""The grid stage's CPU oracle (oracle/matcher_oracle.py, grid_search) pinned to itself: the vectorised search against a
literal per-candidate loop, the mode-0 field against a rasterised one, and a known offset.  No GPU."""
from math import floor

import numpy as np
import pytest

from oracle import matcher_oracle as mo

F32 = np.float32


def room(half_cells, mcs, rng=None, clutter=0, thick=2):
    """Cell-corner points of a square room (walls `thick` cells thick) plus optional clutter points."""
    k = half_cells
    line = np.arange(-k, k + 1)
    pts = []
    for t in range(thick):
        for s in (-1, 1):
            pts += [np.stack([np.full_like(line, s * (k + t)), line], 1), np.stack([line, np.full_like(line, s * (k + t))], 1)]
    p = np.unique(np.concatenate(pts), axis=0).astype(np.float64)
    if clutter:
        p = np.concatenate([p, rng.integers(-k + 2, k - 2, size=(clutter, 2)).astype(np.float64)])
    return p * mcs


def literal_search(occ, ox, oy, bx, by, guess, rng3, mcs, d0, ncr, cell_off, sincos=mo.np_sincos):
    """One candidate and one beam at a time, straight from the kernel's comment block: the coarse and fine tables."""
    N = occ.shape[0]
    NC = N // 4

    def occ_at(u, w):
        return 0 <= u < N and 0 <= w < N and bool(occ[u, w])

    def dil_at(u, w):
        return any(occ_at(u + a, w + b) for a in (-1, 0, 1) for b in (-1, 0, 1))

    def crs_at(cu, cw):
        if not (0 <= cu < NC and 0 <= cw < NC):
            return 0
        return int(any(dil_at(4 * cu + a, 4 * cw + b) for a in range(4) for b in range(4)))

    fx = F32(guess[0] / mcs - ox + cell_off)
    fy = F32(guess[1] / mcs - oy + cell_off)
    from math import remainder
    gthf = F32(remainder(guess[2], 6.283185307179586))
    rxc, ryc = rng3[0] / mcs, rng3[1] / mcs
    ktx = max(int(np.ceil(rxc / 4)) - 1, 0)
    kty = max(int(np.ceil(ryc / 4)) - 1, 0)
    ntx, nty, nr = 2 * ktx + 1, 2 * kty + 1, 2 * ncr + 1
    S = np.zeros((nr, ntx, nty), dtype=np.int64)
    for ir in range(nr):
        a = F32(gthf + F32((ir - ncr) * 4.0 * d0))
        sn, cs = (v[0] for v in sincos(np.array([a], dtype=F32)))
        for itx in range(ntx):
            for iy in range(nty):
                ps, j = divmod(iy, 8)
                ty0 = F32(fy + F32((ps * 8 - kty) * 4))
                for b in range(0, len(bx), 8):
                    ex = F32(F32(cs * bx[b]) - F32(sn * by[b])) + fx
                    ey = F32(F32(sn * bx[b]) + F32(cs * by[b])) + ty0
                    S[ir, itx, iy] += crs_at(floor(ex) // 4 + itx - ktx, floor(ey) // 4 + j)
    return S


def problem(seed, cells_per_m=20, win=(0.5, 0.5, 0.3), off=(0.3, -0.2, 0.05), n_beams=240):
    rng = np.random.Generator(np.random.PCG64(seed))
    mcs = 1.0 / cells_per_m
    ref = room(int(2.0 / mcs), mcs, rng, clutter=40)
    dx, dy, dth = off
    c, s = np.cos(dth), np.sin(dth)
    curr = ((ref - [dx, dy]) @ np.array([[c, -s], [s, c]]))[rng.permutation(len(ref))[:n_beams]]
    return curr, ref


@pytest.mark.parametrize("seed,win,off", [(1, (0.5, 0.5, 0.3), (0.3, -0.2, 0.05)),
                                          (2, (0.3, 0.9, 0.05), (0.0, 0.0, 0.0)),        # ties: symmetric room, no offset
                                          (3, (0.2, 0.2, 0.4), (-0.1, 0.15, -0.2))])
def test_vectorised_coarse_level_equals_literal_loop(seed, win, off):
    curr, ref = problem(seed, win=win, off=off)
    guess = (0.013, -0.027, 0.01)
    N, ds, mcs, d0, ncr = mo.twin_geometry(20, win)
    ncr = min(ncr, 3)                                   # a few rotations keep the literal loop short
    occ, ox, oy = mo.rasterise_fast(ref, guess, mcs, N, 0.5, 15.0)
    bx, by = mo.beams_f32(curr, mcs)
    r = mo.grid_search(occ, ox, oy, bx, by, guess, win, mcs, d0, ncr, 0.5)
    S = literal_search(occ, ox, oy, bx, by, guess, win, mcs, d0, ncr, 0.5)
    assert np.array_equal(r["coarse"], S)


def test_fine_level_and_ties_equal_a_literal_loop():
    """The fine table, the window rule (-1 outside) and both tie-break rules, one candidate at a time."""
    curr, ref = problem(5, win=(0.4, 0.4, 0.2), off=(0.0, 0.0, 0.0))
    guess = (0.0, 0.0, 0.0)
    win = (0.4, 0.4, 0.02)
    N, ds, mcs, d0, ncr = mo.twin_geometry(20, win)
    occ, ox, oy = mo.rasterise_fast(ref, guess, mcs, N, 0.5, 15.0)
    bx, by = mo.beams_f32(curr, mcs)
    r = mo.grid_search(occ, ox, oy, bx, by, guess, win, mcs, d0, ncr, 0.5)
    hit = occ.astype(int) + mo.dilate(occ)
    cir, ctx, cty = r["coarse_best"]
    fx, fy, gthf = r["fx"], r["fy"], r["gthf"]
    F = np.zeros((9, 9, 9), dtype=np.int64)
    for a in range(9):
        ang = F32(gthf + F32((cir * 4 + a - 4) * d0))
        sn, cs = (v[0] for v in mo.np_sincos(np.array([ang], dtype=F32)))
        for b in range(9):
            for c in range(9):
                dth, dx, dy = (cir * 4 + a - 4) * d0, ctx + b - 4, cty + c - 4
                if not (abs(dth) < win[2] and abs(dx) < win[0] / mcs and abs(dy) < win[1] / mcs):
                    F[a, b, c] = -1
                    continue
                tx, ty0 = F32(fx + F32(dx)), F32(fy + F32(cty - 4))
                for k in range(0, len(bx), 4):
                    u = floor(F32(F32(cs * bx[k]) - F32(sn * by[k])) + tx)
                    w = floor(F32(F32(sn * bx[k]) + F32(cs * by[k])) + ty0) + c
                    if 0 <= u < N and 0 <= w < N:
                        F[a, b, c] += hit[u, w]
    assert np.array_equal(r["fine"], F)
    best = F.max()
    cands = [(((cir * 4 + a - 4) ** 2 + (ctx + b - 4) ** 2 + (cty + c - 4) ** 2), (a * 9 + b) * 9 + c, (a, b, c))
             for a, b, c in zip(*np.nonzero(F == best))]
    assert len(cands) > 1, "the problem was meant to have ties"
    a, b, c = min(cands)[2]
    assert r["out"][0] == guess[0] + (ctx + b - 4) * mcs and r["out"][1] == guess[1] + (cty + c - 4) * mcs
    assert r["out"][2] == guess[2] + (cir * 4 + a - 4) * d0


def test_kernel_edge_drops_are_harmless_for_fields_inside_max_range():
    """Ref points on the 15 m circle, beams everywhere: the kernel's drop of whole passes at the region edge never removes
    a hit, at every twin resolution."""
    rng = np.random.Generator(np.random.PCG64(9))
    for cpm in (10, 20, 40):
        ang = np.linspace(-np.pi, np.pi, 4000, endpoint=False)
        ref = np.stack([14.999 * np.cos(ang), 14.999 * np.sin(ang)], 1)
        curr = rng.uniform(-17, 17, size=(1600, 2))
        win = (1.5, 1.5, 0.1)
        for guess in ((0.0, 0.0, 0.0), (0.037, -0.061, 1.0)):
            _, _, _, r = mo.match_scan_oracle(curr, ref, guess, cpm, win)
            assert not r["edge_effect"], (cpm, guess)


def test_mode0_field_from_tiles_equals_rasterised_points():
    """A set_tile-style dict built from points by the reference's write formula, read back through field_from_tiles,
    equals the points rasterised straight into the region (ds = 1 and ds = 2; negative side and a tile seam)."""
    from oracle import rbpf_oracle as orc
    rng = np.random.Generator(np.random.PCG64(4))
    for cs, mcs_ds in ((0.05, 1), (0.025, 2)):
        dim, tile = int(round(40 / cs)), 40.0
        for centre in ((-19.3, -6.2), (19.7, 0.4)):
            g = rng.integers(-200, 200, size=(3000, 2)) + np.round(np.array(centre) / cs).astype(int)
            tiles = {}
            for gx, gy in g:
                px, py = gx * cs, gy * cs
                cx, cy = orc.map_centre_1d(px, tile), orc.map_centre_1d(py, tile)
                t = tiles.setdefault((cx, cy), np.zeros((dim, dim), dtype=np.int8))
                t[orc.set_index(px - cx, cs, dim), orc.set_index(py - cy, cs, dim)] = 30
            N, ds, mcs, d0, _ = mo.match_geometry(cs, 11.0)
            assert ds == mcs_ds
            occ, ox, oy = mo.field_from_tiles(tiles, (centre[0], centre[1], 0.0), N, ds, mcs, cs, tile, 3)
            want = np.zeros_like(occ)
            u, w = np.floor_divide(g[:, 0], ds) - ox, np.floor_divide(g[:, 1], ds) - oy
            ins = (u >= 0) & (u < N) & (w >= 0) & (w < N)
            want[u[ins], w[ins]] = True
            # the formula stores a few columns one cell lower (two global indices share a cell): such a cell reads as
            # occupied at both indices; everywhere else the field is the points themselves
            def key(gi):
                pos = gi * cs
                c = orc.map_centre_1d(pos, tile)
                return c, orc.set_index(pos - c, cs, dim)
            written = {(key(a), key(b)) for a, b in g}
            extra = np.argwhere(occ & ~want)
            assert not (want & ~occ).any()
            for eu, ew in extra:
                gis = [((eu + ox) * ds + i, (ew + oy) * ds + j) for i in range(ds) for j in range(ds)]
                assert any((key(a), key(b)) in written for a, b in gis)


@pytest.mark.parametrize("cells_per_m", [10, 20])
@pytest.mark.parametrize("shift", [(3, -2), (-6, 5), (0, 0)])
def test_known_offset_recovered_exactly_at_heading_zero(cells_per_m, shift):
    mcs = 1.0 / cells_per_m
    ref = room(int(3.0 / mcs), mcs, thick=1)           # one-cell walls: the true offset is the only full score
    curr = ref[::2] - np.array(shift) * mcs
    pose, cov, score, r = mo.match_scan_oracle(curr, ref, (0.0, 0.0, 0.0), cells_per_m, (0.7, 0.7, 0.01))
    assert r["ncr"] == 0 and np.all(np.isfinite(cov))
    assert pose[0] == shift[0] * mcs and pose[1] == shift[1] * mcs and pose[2] == 0.0
    assert score == len(curr)                        # every beam on an occupied cell: 2 per beam, halved


def test_empty_field_takes_the_failure_branch():
    pose, cov, score, r = mo.match_scan_oracle(np.ones((50, 2)), np.zeros((0, 2)), (1.0, 2.0, 0.5), 20, (0.5, 0.5, 0.5))
    assert np.isnan(cov).all() and score == 0.0 and not r["ok"]


def test_particle_window_equals_reference_pose_range():
    """match_frame_from's translation window is robot.py:62-65 (orc.pose_range_from_cov); the rotation range is
    hybridmap.py:249's pi/6, not pose_range[2]."""
    from oracle import rbpf_oracle as orc
    rng = np.random.Generator(np.random.PCG64(2))
    for _ in range(200):
        c = np.diag(rng.uniform(0, 0.01, 3) ** 2)
        assert mo.window_from_cov(c[0, 0], c[1, 1]) == tuple(orc.pose_range_from_cov(c)[:2])


def test_geometry_of_the_twin():
    """40 cells/m runs at ds = 2, mcs = 0.05; the overflow configuration has 66 439 coarse candidates."""
    assert mo.twin_geometry(40, (0.7, 0.7, np.pi / 6))[:3] == (672, 2, 0.05)
    N, ds, mcs, d0, ncr = mo.twin_geometry(20, (3.0, 3.0, np.pi / 6))
    assert (N, ds, ncr) == (672, 1, 39)
    assert (2 * ncr + 1) * 29 * 29 == 66439
    assert mo.twin_geometry(10, (0.7, 0.7, np.pi / 6))[:2] == (352, 1)
