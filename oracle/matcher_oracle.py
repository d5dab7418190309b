"""CPU oracle for the NDT refinement stage of the scan matcher (matchScanCustom.m:32-50).

TEST INFRASTRUCTURE ONLY (see oracle/rbpf_oracle.py): nothing in ``thesis_amd/`` imports this.

**Parity unpinned.**  The reference calls MathWorks Navigation Toolbox R2021a ``matchScans`` (closed source, absent
from the reference tree, no recorded outputs).  What is restated here is the *published* algorithm that function
documents -- the Normal Distributions Transform of Biber & Strasser, "The Normal Distributions Transform: A New
Approach to Laser Scan Matching", IROS 2003 -- with the parameters the reference's call site fixes
(``'CellSize', 0.1``, ``'MaxIterations', 500``, matchScanCustom.m:36-37):

* the reference cloud is the set of occupied matcher cells (centres), binned into four overlapping grids of
  ``nc x nc`` matcher cells shifted by half an NDT cell (paper section III);
* a grid cell with at least 3 points carries their mean and sample covariance; the smaller eigenvalue is raised to
  0.001 times the larger one (paper section III, singular-covariance guard);
* score(p) = sum over points and grids of exp(-0.5 d' C^-1 d), d = T(p) x - mean (paper eq. 3);
* Newton's method on -score with the analytic gradient and Hessian (paper section V), made robust with a
  Levenberg-Marquardt damping term (the paper: "H is replaced by H + lambda I" when not positive definite).

The HIP stage (``kernels_match.hip``, ``ndt_*``) follows exactly these steps; this file is its checker.
Coordinates: region-relative matcher-cell units, exactly as the kernel holds them.
"""
from __future__ import annotations

from math import floor

import numpy as np

NDT_CELL_M = 0.1          # matchScanCustom.m:37
NDT_MAX_ITER = 500        # matchScanCustom.m:36
NDT_MIN_POINTS = 3
NDT_EIG_FLOOR = 1e-3
LAM0, LAM_MIN, LAM_MAX = 1e-3, 1e-7, 1e7
TOL_T, TOL_R = 1e-2, 2e-4     # convergence: proposed step below 0.01 cells (0.5 mm at 0.05 m) and 2e-4 rad
LAM_UP, LAM_DOWN = 100.0, 0.1  # damping after a rejected / an accepted trial


def _cell_stats(occ: np.ndarray, u0: np.ndarray, w0: np.ndarray, nc: int):
    """Mean and inverse covariance of the occupied cell centres inside the nc x nc blocks at (u0, w0)."""
    N = occ.shape[0]
    n = np.zeros(len(u0), dtype=np.int64)
    sx = np.zeros_like(n); sy = np.zeros_like(n); sxx = np.zeros_like(n); sxy = np.zeros_like(n); syy = np.zeros_like(n)
    for i in range(nc):
        for j in range(nc):
            uu, ww = u0 + i, w0 + j
            inside = (uu >= 0) & (uu < N) & (ww >= 0) & (ww < N)
            bit = np.zeros(len(u0), dtype=bool)
            bit[inside] = occ[uu[inside], ww[inside]]
            n += bit; sx += bit * i; sy += bit * j; sxx += bit * (i * i); sxy += bit * (i * j); syy += bit * (j * j)
    ok = n >= NDT_MIN_POINTS
    nn = np.where(ok, n, 3).astype(np.float64)
    mx, my = sx / nn, sy / nn
    a = (sxx - sx * mx) / (nn - 1.0)
    b = (sxy - sx * my) / (nn - 1.0)
    c = (syy - sy * my) / (nn - 1.0)
    half_tr = 0.5 * (a + c)
    disc = np.sqrt(0.25 * (a - c) * (a - c) + b * b)
    l1, l2 = half_tr + disc, half_tr - disc
    fix = ok & (l2 < NDT_EIG_FLOOR * l1)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(fix, (NDT_EIG_FLOOR * l1 - l2) / (l1 - l2), 0.0)
    k = np.where(np.isfinite(k), k, 0.0)
    a2 = a + k * (l1 - a); b2 = b + k * (-b); c2 = c + k * (l1 - c)
    det = a2 * c2 - b2 * b2
    det = np.where(ok, det, 1.0)
    B00, B01, B11 = c2 / det, -b2 / det, a2 / det
    return ok, u0 + 0.5 + mx, w0 + 0.5 + my, B00, B01, B11


def ndt_eval(occ: np.ndarray, pts: np.ndarray, p, nc: int, ox: int, oy: int, single: bool = False):
    """f = -score, gradient (3), Hessian (6: xx xy xt yy yt tt) at p = (tx, ty, theta).

    ``single``: the kernel's hot form for nc == 2 -- the offset from the cell mean is formed from the point's float32
    position inside its matcher cell, everything after it in float32 (sums in float64)."""
    tx, ty, th = p
    sn, cs = np.sin(th), np.cos(th)
    bx, by = pts[:, 0], pts[:, 1]
    rx, ry = cs * bx - sn * by, sn * bx + cs * by
    ex, ey = rx + tx, ry + ty
    u, w = np.floor(ex).astype(np.int64), np.floor(ey).astype(np.int64)
    N = occ.shape[0]
    live = (u >= 0) & (u < N) & (w >= 0) & (w < N)
    m = np.zeros(10)
    h = nc // 2
    for g in range(4):
        gx, gy = (h if g & 1 else 0), (h if g & 2 else 0)
        u0 = u - np.mod(u + ox - gx, nc)
        w0 = w - np.mod(w + oy - gy, nc)
        ok, qx, qy, B00, B01, B11 = _cell_stats(occ, u0, w0, nc)
        ok &= live
        dx, dy = ex - qx, ey - qy
        if single:
            # the kernel's form: position inside the matcher cell (float64 -> float32) plus the cell's offset inside the NDT
            # cell, minus the table's float32 "0.5 + mean"; the terms are float32 (the kernel fuses multiply-adds and uses
            # the hardware exponential: agreement to ~1e-7, not bit for bit)
            f32 = np.float32
            fx, fy = (ex - np.floor(ex)).astype(f32), (ey - np.floor(ey)).astype(f32)
            dx = (fx + (u - u0).astype(f32)) - (qx - u0).astype(f32)
            dy = (fy + (w - w0).astype(f32)) - (qy - w0).astype(f32)
            B00, B01, B11 = B00.astype(f32), B01.astype(f32), B11.astype(f32)
            rx, ry = rx.astype(f32), ry.astype(f32)
            e0, e1 = B00 * dx + B01 * dy, B01 * dx + B11 * dy
            s = np.where(ok, np.exp(f32(-0.5) * (dx * e0 + dy * e1)), f32(0.0))
        else:
            e0, e1 = B00 * dx + B01 * dy, B01 * dx + B11 * dy
            s = np.where(ok, np.exp(-0.5 * (dx * e0 + dy * e1)), 0.0)
        c0, c1, c2 = e0, e1, e0 * (-ry) + e1 * rx
        bj0, bj1 = B00 * (-ry) + B01 * rx, B01 * (-ry) + B11 * rx
        f64 = np.float64
        m[0] -= s.sum(dtype=f64)
        m[1] += (s * c0).sum(dtype=f64); m[2] += (s * c1).sum(dtype=f64); m[3] += (s * c2).sum(dtype=f64)
        m[4] += (s * (-c0 * c0 + B00)).sum(dtype=f64)
        m[5] += (s * (-c0 * c1 + B01)).sum(dtype=f64)
        m[6] += (s * (-c0 * c2 + bj0)).sum(dtype=f64)
        m[7] += (s * (-c1 * c1 + B11)).sum(dtype=f64)
        m[8] += (s * (-c1 * c2 + bj1)).sum(dtype=f64)
        m[9] += (s * (-c2 * c2 + (-ry) * bj0 + rx * bj1 + e0 * (-rx) + e1 * (-ry))).sum(dtype=f64)
        if single:
            rx, ry = rx.astype(f64), ry.astype(f64)
    return m


def _lm_step(m, lam):
    """Solve (H + lam * diag(|H_ii| + 1e-12)) d = -g by Cholesky; None when the damped matrix is not positive definite."""
    g = m[1:4]
    A = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    for i in range(3):
        A[i, i] += lam * (abs(A[i, i]) + 1e-12)
    l00 = A[0, 0]
    if not l00 > 0:
        return None
    l00 = np.sqrt(l00)
    l10, l20 = A[1, 0] / l00, A[2, 0] / l00
    d1 = A[1, 1] - l10 * l10
    if not d1 > 0:
        return None
    l11 = np.sqrt(d1)
    l21 = (A[2, 1] - l20 * l10) / l11
    d2 = A[2, 2] - l20 * l20 - l21 * l21
    if not d2 > 0:
        return None
    l22 = np.sqrt(d2)
    y0 = -g[0] / l00
    y1 = (-g[1] - l10 * y0) / l11
    y2 = (-g[2] - l20 * y0 - l21 * y1) / l22
    x2 = y2 / l22
    x1 = (y1 - l21 * x2) / l11
    x0 = (y0 - l10 * x1 - l20 * x2) / l00
    return np.array([x0, x1, x2])


NDT_STRIDE = 1            # points used by the ascent (1: all); the returned score always covers all points


def ndt_refine(occ: np.ndarray, pts_all: np.ndarray, start, nc: int, ox: int, oy: int, max_iter: int = NDT_MAX_ITER,
               single: bool = None, stride: int = NDT_STRIDE):
    """Damped Newton ascent of the NDT score from ``start``; returns (pose, score over all points, evaluations)."""
    single = (nc == 2) if single is None else single
    pts = pts_all[::stride]
    p = np.array(start, dtype=np.float64)
    cur = ndt_eval(occ, pts, p, nc, ox, oy, single)
    evals, lam = 1, LAM0
    while evals <= max_iter:
        d = None
        while d is None and lam <= LAM_MAX:
            d = _lm_step(cur, lam)
            if d is None:
                lam *= 10.0
        if d is None:
            break
        if max(abs(d[0]), abs(d[1])) < TOL_T and abs(d[2]) < TOL_R:
            break
        trial = ndt_eval(occ, pts, p + d, nc, ox, oy, single)
        evals += 1
        if trial[0] < cur[0]:
            p = p + d
            cur = trial
            lam = max(lam * LAM_DOWN, LAM_MIN)
        else:
            lam *= LAM_UP
            if lam > LAM_MAX:
                break
    return p, -ndt_eval(occ, pts_all, p, nc, ox, oy, single)[0], evals


def rasterise(ref_xy: np.ndarray, guess, mcs: float, N: int, cell_off: float, max_range: float):
    """Occupancy of the matcher region from reference points, as the kernel's mode-1 field stage does."""
    ox = int(floor(guess[0] / mcs)) - N // 2
    oy = int(floor(guess[1] / mcs)) - N // 2
    occ = np.zeros((N, N), dtype=bool)
    for rx, ry in np.asarray(ref_xy, dtype=np.float64).reshape(-1, 2):
        dx, dy = rx - guess[0], ry - guess[1]
        if not (np.sqrt(dx * dx + dy * dy) < max_range):
            continue
        u = int(floor(rx / mcs + cell_off)) - ox
        w = int(floor(ry / mcs + cell_off)) - oy
        if 0 <= u < N and 0 <= w < N:
            occ[u, w] = True
    return occ, ox, oy


def beams_in_cells(curr_xy: np.ndarray, mcs: float) -> np.ndarray:
    """Sensor-frame points in matcher-cell units, with the kernel's float32 staging."""
    c = np.asarray(curr_xy, dtype=np.float64).reshape(-1, 2).astype(np.float32)
    inv = np.float32(1.0 / mcs)
    return (c * inv).astype(np.float64)


# ==== grid stage (kernels_match.hip, match_kernel) =====================================================================
# A restatement of the correlative search from the comment block at the top of kernels_match.hip, not of the kernel's
# data layout.  The library is compiled with -ffp-contract=off -fno-fast-math, so every float32 beam position below is
# formed with the kernel's operations in the kernel's order and the comparison can be bit for bit.  The one value the
# CPU cannot reproduce is the device's __sincosf (hardware sine / cosine): ``sincos`` is a callable, float32 in and
# (sin, cos) float32 out; GPU tests pass the device's own values (ParticleEngine.native_sincosf).
#
# Region edges.  The intended rule is that a position outside the N x N region scores 0.  The kernel instead drops a beam
# for a whole pass of 8 coarse y translations when its first column cw0 < 0 (columns past N/4 read zero bits), and for
# all 9 fine y translations when w0 < 0 or w0 + 8 >= N.  ``kernel_edges=True`` applies those drops; grid_search reports
# whether they changed any score.

M_COARSE = 4              # coarse cell = 4 fine cells, coarse rotation step = 4 d0
M_FINE = 4                # fine level: -4..4 rotation steps / cells around the coarse optimum
TWIN_MAX_RANGE = 15.0     # matchScanCustom.m:11 (rbpf_match_scan)
PI = 3.141592653589793
F32 = np.float32


def match_geometry(cell_size: float, max_range: float):
    """match_geometry (kernels_match.hip): region edge N, matcher cell ds map cells of mcs metres, fine rotation step d0,
    coarse rotations ncr on each side of the particle path's pi/6 window."""
    ds = 1
    while True:
        mcs = cell_size * ds
        half = int(np.ceil((max_range + 0.5 + 0.7) / mcs)) + 2
        N = ((2 * half + 31) // 32) * 32
        if 2 * N * (N // 32) * 4 <= 120 * 1024 or ds >= 8:
            break
        ds *= 2
    d0 = mcs / max_range
    return N, ds, mcs, d0, coarse_rotations(PI / 6, d0)


def coarse_rotations(rot: float, d0: float) -> int:
    """Largest k with k * 4 d0 < |rot| (match_geometry; rbpf_match_scan takes it from pose_range[2])."""
    rot = abs(rot)
    k = int(floor(rot / (M_COARSE * d0)))
    if k * M_COARSE * d0 >= rot:
        k -= 1
    return max(k, 0)


def twin_geometry(cells_per_m: int, pose_range):
    """rbpf_match_scan: MaxRange 15 m; the coarse rotations come from pose_range[2]."""
    N, ds, mcs, d0, _ = match_geometry(1.0 / cells_per_m, TWIN_MAX_RANGE)
    return N, ds, mcs, d0, coarse_rotations(pose_range[2], d0)


def region_origin(guess, mcs: float, N: int):
    """match_frame_from: the region's first matcher cell."""
    return int(floor(guess[0] / mcs)) - N // 2, int(floor(guess[1] / mcs)) - N // 2


def window_from_cov(c00: float, c11: float):
    """match_frame_from on the particle path (robot.py:62-65): translation half-widths from the covariance."""
    p0, p1 = np.sqrt(c00) * 30.0, np.sqrt(c11) * 30.0
    return max(min(4 * p0, 0.7), 0.1), max(min(4 * p1, 0.7), 0.1)


def np_sincos(x):
    """CPU default for the device's __sincosf: float32-rounded sin / cos of the float32 angles."""
    x = np.asarray(x, dtype=F32).astype(np.float64)
    return np.sin(x).astype(F32), np.cos(x).astype(F32)


def field_from_tiles(tiles, guess, N: int, ds: int, mcs: float, cell_size: float, tile_len: float, R: int,
                     thr: int = 10):
    """Mode 0: occupancy of the region from one particle's tiles {(cx, cy): int8 cells [x][y]} (lattice values > thr
    quanta, gridmap.py:153).  A map cell with global index g lies at g * cell_size and is addressed by the reference's
    write formula: tile = map_centre_1d, cell = set_index of the offset from the tile centre.  A matcher cell is occupied
    if any of its ds x ds map cells is; cells of absent tiles or outside the lattice are free."""
    from oracle import rbpf_oracle as orc
    ox, oy = region_origin(guess, mcs, N)
    dim = next(iter(tiles.values())).shape[0] if tiles else 0

    def axis(o):
        lat, idx = np.full(N * ds, -99999), np.zeros(N * ds, dtype=np.int64)
        for i in range(N * ds):
            pos = (o * ds + i) * cell_size
            c = orc.map_centre_1d(pos, tile_len)
            if not (pos < c + tile_len / 2 and pos >= c - tile_len / 2):
                continue
            l = int(round(c / tile_len))
            if -R <= l <= R:
                lat[i], idx[i] = l, orc.set_index(pos - c, cell_size, dim)
        return lat, idx

    lx, ix = axis(ox)
    ly, iy = axis(oy)
    fine = np.zeros((N * ds, N * ds), dtype=bool)
    for (cx, cy), cells in tiles.items():
        a, b = int(round(cx / tile_len)), int(round(cy / tile_len))
        rows, cols = np.nonzero(lx == a)[0], np.nonzero(ly == b)[0]
        if len(rows) and len(cols):
            fine[np.ix_(rows, cols)] = cells[np.ix_(ix[rows], iy[cols])] > thr
    occ = fine.reshape(N, ds, N, ds).any(axis=(1, 3))
    return occ, ox, oy


def rasterise_fast(ref_xy, guess, mcs: float, N: int, cell_off: float, max_range: float):
    """rasterise, vectorised (same operations per point)."""
    ox, oy = region_origin(guess, mcs, N)
    p = np.asarray(ref_xy, dtype=np.float64).reshape(-1, 2)
    dx, dy = p[:, 0] - guess[0], p[:, 1] - guess[1]
    keep = np.sqrt(dx * dx + dy * dy) < max_range
    u = np.floor(p[keep, 0] / mcs + cell_off).astype(np.int64) - ox
    w = np.floor(p[keep, 1] / mcs + cell_off).astype(np.int64) - oy
    inside = (u >= 0) & (u < N) & (w >= 0) & (w < N)
    occ = np.zeros((N, N), dtype=bool)
    occ[u[inside], w[inside]] = True
    return occ, ox, oy


def dilate(occ: np.ndarray) -> np.ndarray:
    """3x3 dilation (the cell itself included), nothing beyond the region."""
    N = occ.shape[0]
    p = np.zeros((N + 2, N + 2), dtype=bool)
    p[1:-1, 1:-1] = occ
    out = np.zeros_like(occ)
    for a in range(3):
        for b in range(3):
            out |= p[a:a + N, b:b + N]
    return out


def beams_f32(xy, mcs: float):
    """Beams in matcher cells as the kernel stages them: float32 metres times float32(1 / mcs)."""
    c = np.asarray(xy, dtype=np.float64).reshape(-1, 2).astype(F32)
    inv = F32(1.0 / mcs)
    return c[:, 0] * inv, c[:, 1] * inv


def _gather(field, u, w):
    N = field.shape[0]
    u, w = np.broadcast_arrays(u, w)
    inside = (u >= 0) & (u < N) & (w >= 0) & (w < N)
    out = np.zeros(u.shape, dtype=np.int64)
    out[inside] = field[u[inside], w[inside]]
    return out


def grid_search(occ, ox, oy, bx, by, guess, rng3, mcs, d0, ncr, cell_off, sincos=np_sincos, kernel_edges=False):
    """The grid stage for one problem.  occ: bool [N][N] region occupancy; bx, by: float32 beams in matcher cells (all
    selected beams, in order); guess: (x, y, theta); rng3: (rx, ry, rotation range) in metres / radians.
    Returns a dict: out (13: pose, cov row-major, score, as match_kernel writes d_match), ok, the coarse / fine score
    tables and the winners, and ``edge_effect``: whether the kernel's edge drops change any score."""
    N = occ.shape[0]
    NC = N // M_COARSE
    dil = dilate(occ)
    hit = occ.astype(np.int64) + dil                                  # 2 occupied, 1 dilated only
    crs = dil.reshape(NC, M_COARSE, NC, M_COARSE).any(axis=(1, 3)).astype(np.int64)   # 4x4 max-pool of the dilated field
    nb = len(bx)
    gx, gy, gth = float(guess[0]), float(guess[1]), float(guess[2])
    fx = F32(gx / mcs - float(ox) + cell_off)
    fy = F32(gy / mcs - float(oy) + cell_off)
    gthf = F32(_ieee_remainder(gth, 6.283185307179586))
    rxc, ryc = rng3[0] / mcs, rng3[1] / mcs
    ktx = max(int(np.ceil(rxc / M_COARSE)) - 1, 0)                  # largest k with 4k < range (at least 0)
    kty = max(int(np.ceil(ryc / M_COARSE)) - 1, 0)
    ntx, nty, nr = 2 * ktx + 1, 2 * kty + 1, 2 * ncr + 1
    NP = (nty + 7) // 8

    # ---- coarse: every 8th beam, rotation gthf + (float)(k * 4 d0), one float y offset per pass of 8 translations
    cx, cy = bx[::8], by[::8]
    ang = np.array([gthf + F32((ir - ncr) * 4.0 * d0) for ir in range(nr)], dtype=F32)
    sn, cs = sincos(ang)
    S = np.zeros((nr, ntx, NP * 8), dtype=np.int64)
    S_k = np.zeros_like(S)
    tx = np.arange(ntx) - ktx
    for ir in range(nr):
        ex = (cs[ir] * cx - sn[ir] * cy) + fx
        row = (np.floor(ex).astype(np.int64) >> 2)[:, None] + tx[None, :]              # [beam, x translation]
        ey0 = sn[ir] * cx + cs[ir] * cy
        for ps in range(NP):
            ty0 = F32(fy + F32((ps * 8 - kty) * M_COARSE))
            cw0 = np.floor(ey0 + ty0).astype(np.int64) >> 2
            col = cw0[:, None] + np.arange(8)[None, :]                                     # [beam, y translation]
            v = _gather(crs, row[:, :, None], col[:, None, :])                             # [beam, x, y]
            S[ir, :, ps * 8:ps * 8 + 8] = v.sum(axis=0)
            drop = cw0 < 0
            S_k[ir, :, ps * 8:ps * 8 + 8] = v[~drop].sum(axis=0)
    S, S_k = S[:, :, :nty], S_k[:, :, :nty]
    Sc = S_k if kernel_edges else S
    best_c = Sc.max()
    ir_, ix_, iy_ = np.nonzero(Sc == best_c)
    dist = (ir_ - ncr) ** 2 + (ix_ - ktx) ** 2 + (iy_ - kty) ** 2
    cnd = (ir_ * ntx + ix_) * nty + iy_
    k = np.lexsort((cnd, dist))[0]
    cir, ctx, cty = int(ir_[k]) - ncr, (int(ix_[k]) - ktx) * M_COARSE, (int(iy_[k]) - kty) * M_COARSE

    # ---- fine: every 4th beam, 9 x 9 x 9 around the coarse winner, hits occ + dil
    fxb, fyb = bx[::4], by[::4]
    FT = 2 * M_FINE + 1
    F = np.zeros((FT, FT, FT), dtype=np.int64)
    F_k = np.zeros_like(F)
    fang = np.array([gthf + F32((cir * M_COARSE + r) * d0) for r in range(-M_FINE, M_FINE + 1)], dtype=F32)
    fsn, fcs = sincos(fang)
    ty0 = F32(fy + F32(cty - M_FINE))
    for a in range(FT):
        ey = (fsn[a] * fxb + fcs[a] * fyb) + ty0
        w0 = np.floor(ey).astype(np.int64)
        exr = fcs[a] * fxb - fsn[a] * fyb
        for b in range(FT):
            u = np.floor(exr + F32(fx + F32(ctx + b - M_FINE))).astype(np.int64)
            v = _gather(hit, u[:, None], w0[:, None] + np.arange(FT)[None, :])
            F[a, b] = v.sum(axis=0)
            keep = (u >= 0) & (u < N) & (w0 >= 0) & (w0 + 8 < N)
            F_k[a, b] = v[keep].sum(axis=0)
    r_ = np.arange(-M_FINE, M_FINE + 1)
    DTH = (cir * M_COARSE + r_)[:, None, None] * d0
    DX = (ctx + r_)[None, :, None]
    DY = (cty + r_)[None, None, :]
    inwin = (np.abs(DTH) < rng3[2]) & (np.abs(DX.astype(np.float64)) < rxc) & (np.abs(DY.astype(np.float64)) < ryc)
    inwin = np.broadcast_to(inwin, F.shape)
    F = np.where(inwin, F, -1)
    F_k = np.where(inwin, F_k, -1)
    Fs = F_k if kernel_edges else F
    best = int(Fs.max())
    a_, b_, c_ = np.nonzero(Fs == best)
    fd = (cir * M_COARSE + a_ - M_FINE) ** 2 + (ctx + b_ - M_FINE) ** 2 + (cty + c_ - M_FINE) ** 2
    fc = (a_ * FT + b_) * FT + c_
    k = np.lexsort((fc, fd))[0]
    fa, fb, fcc = int(a_[k]), int(b_[k]), int(c_[k])
    bth = float(cir * M_COARSE + fa - M_FINE) * d0
    bdx = float(ctx + fb - M_FINE) * mcs
    bdy = float(cty + fcc - M_FINE) * mcs

    # ---- full score over all beams at the chosen pose (double sincos, cast to float)
    sd, cd = F32(np.sin(gth + bth)), F32(np.cos(gth + bth))
    tx1, ty1 = F32(fx + F32(bdx / mcs)), F32(fy + F32(bdy / mcs))
    ex = (cd * bx - sd * by) + tx1
    ey = (sd * bx + cd * by) + ty1
    full = int(_gather(hit, np.floor(ex).astype(np.int64), np.floor(ey).astype(np.int64)).sum())

    # ---- covariance: second moments of exp((s - best) / tau) over the fine candidates in the window, plus a floor
    out = np.empty(13)
    out[0], out[1], out[2] = gx + bdx, gy + bdy, gth + bth
    ok = best > 0 and nb > 0
    if not ok:
        out[3:12] = np.nan
        out[12] = 0.0
    else:
        tau = max(1.0, 0.02 * float((nb + 3) // 4) * 2.0)
        m = Fs >= 0
        w = np.exp((Fs[m] - best).astype(np.float64) / tau)
        e = np.stack([np.broadcast_to(DX * mcs, F.shape)[m].astype(np.float64) - bdx,
                      np.broadcast_to(DY * mcs, F.shape)[m].astype(np.float64) - bdy,
                      np.broadcast_to(DTH, F.shape)[m] - bth])
        sw = w.sum()
        mu = (e * w).sum(axis=1) / sw
        c = (e[:, None, :] * e[None, :, :] * w).sum(axis=2) / sw - mu[:, None] * mu[None, :]
        fl_t, fl_r = mcs * mcs / 16.0, d0 * d0 / 16.0
        for i, fl in enumerate((fl_t, fl_t, fl_r)):
            c[i, i] = max(c[i, i], 0.0) + fl
        out[3:12] = c.reshape(-1)
        out[12] = 0.5 * full
    return {"out": out, "ok": ok, "coarse": S, "fine": F, "coarse_best": (cir, ctx, cty), "best": best,
            "full_score": full, "bdx": bdx, "bdy": bdy, "bth": bth,
            "fx": fx, "fy": fy, "gthf": gthf, "ntx": ntx, "nty": nty, "nr": nr, "NP": NP,
            "edge_effect": bool((S != S_k).any() or (F != F_k).any())}


def _ieee_remainder(x: float, y: float) -> float:
    from math import remainder
    return remainder(x, y)


def ndt_cells(mcs: float) -> int:
    """ndt_cells (kernels_match.hip): the NDT cell edge of 0.1 m in matcher cells; below 2 the stage stays off."""
    return int(floor(NDT_CELL_M / mcs + 0.5))


def ndt_stage(occ, ox, oy, pts, r, guess, window, mcs, cell_off, nc, mode):
    """The second matcher stage as ndt_kernel composes it around ndt_refine (matchScanCustom.m:32-57).  occ, ox, oy: the
    region's occupancy and origin; pts: beams_in_cells(...); r: grid_search's dict; window: (rx, ry, rotation range) in
    metres / radians; mode: ndt_refine (1: the reference's acceptance rule, 2: every valid pose is taken).
    Returns a dict: row (13, what match_results reports), entered, valid, accepted, evals, score, margin
    (2 * score / grid score: the acceptance rule is margin > 1) and, if entered, start / pose (region cells) and dd (the
    pose's offset from the guess, metres / radians)."""
    from math import remainder
    row = np.array(r["out"], dtype=np.float64)
    res = {"row": row, "entered": False, "valid": False, "accepted": False, "evals": 0, "score": 0.0, "margin": 0.0}
    if not (r["ok"] and len(pts) > 0 and nc >= 2):
        return res
    gx, gy, gth = float(guess[0]), float(guess[1]), float(guess[2])
    X0 = gx / mcs - float(ox) + cell_off
    Y0 = gy / mcs - float(oy) + cell_off
    start = (X0 + r["bdx"] / mcs, Y0 + r["bdy"] / mcs, gth + r["bth"])
    p, score, evals = ndt_refine(occ, pts, start, nc, ox, oy)
    ddx, ddy, ddt = (p[0] - X0) * mcs, (p[1] - Y0) * mcs, p[2] - gth
    valid = (abs(ddx) < window[0] and abs(ddy) < window[1] and abs(remainder(ddt, 6.283185307179586)) < window[2]
             and (gx + ddx != 0.0 or gy + ddy != 0.0 or gth + ddt != 0.0))
    grid_score = 0.5 * float(r["full_score"])
    accepted = bool(valid and (mode == 2 or 2.0 * score > grid_score))
    if accepted:
        row[0], row[1], row[2], row[12] = gx + ddx, gy + ddy, gth + ddt, score
    res.update(entered=True, valid=bool(valid), accepted=accepted, evals=int(evals), score=float(score),
               margin=(2.0 * score / grid_score if grid_score > 0 else np.inf), start=start, pose=p, dd=(ddx, ddy, ddt))
    return res


def twin_gate(out13, guess, pose_range):
    """rbpf_match_scan's validity gate (matchScanCustom.m:19,52-57): pose, cov (NaN if invalid), score (0 if invalid)."""
    from math import fmod
    dth = fmod(out13[2] - guess[2] + PI, 2 * PI)
    if dth < 0:
        dth += 2 * PI
    dth -= PI
    valid = (abs(out13[0] - guess[0]) < abs(pose_range[0]) and abs(out13[1] - guess[1]) < abs(pose_range[1])
             and abs(dth) < abs(pose_range[2]) and not np.isnan(out13[3]))
    cov = out13[3:12].reshape(3, 3) if valid else np.full((3, 3), np.nan)
    return out13[:3].copy(), cov.copy(), (out13[12] if valid else 0.0)


def match_scan_oracle(curr_xy, ref_xy, guess, cells_per_m, pose_range, sincos=np_sincos, kernel_edges=False):
    """rbpf_match_scan restated: (pose, cov, score, detail dict)."""
    N, ds, mcs, d0, ncr = twin_geometry(cells_per_m, pose_range)
    occ, ox, oy = rasterise_fast(ref_xy, guess, mcs, N, 0.5, TWIN_MAX_RANGE)
    bx, by = beams_f32(curr_xy, mcs)
    r = grid_search(occ, ox, oy, bx, by, guess, (pose_range[0], pose_range[1], pose_range[2]), mcs, d0, ncr, 0.5,
                    sincos, kernel_edges)
    r.update(N=N, ds=ds, mcs=mcs, d0=d0, ncr=ncr)
    pose, cov, score = twin_gate(r["out"], guess, pose_range)
    return pose, cov, score, r


def select_beams(x, y, min_range: float, max_range: float, adj: bool):
    """rbpf_set_scan's compaction (order kept): BF_MATCH 1e-3 < r < max, BF_MATCH_ADJ r < max."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = np.sqrt(x * x + y * y)
    keep = (d < max_range) if adj else ((d < max_range) & (d > min_range))
    return np.stack([x[keep], y[keep]], axis=1)


def exhaustive_best(occ, ox, oy, bx, by, guess, rng3, mcs, d0, cell_off, sincos=np_sincos):
    """Full-resolution search over the whole window with every 4th beam (the fine level's scores everywhere): the best
    score and its pose offset (cells, cells, rotation steps).  For measuring the two-level search's gap."""
    N = occ.shape[0]
    hit = occ.astype(np.int64) + dilate(occ)
    fx = F32(guess[0] / mcs - float(ox) + cell_off)
    fy = F32(guess[1] / mcs - float(oy) + cell_off)
    gthf = F32(_ieee_remainder(float(guess[2]), 6.283185307179586))
    kx = int(np.ceil(rng3[0] / mcs)) - 1
    ky = int(np.ceil(rng3[1] / mcs)) - 1
    kr = int(np.ceil(rng3[2] / d0)) - 1
    fxb, fyb = bx[::4], by[::4]
    rs = np.arange(-kr, kr + 1)
    sn, cs = sincos(np.array([gthf + F32(r * d0) for r in rs], dtype=F32))
    best, arg = -1, None
    for i, r in enumerate(rs):
        exr = cs[i] * fxb - sn[i] * fyb
        eyr = sn[i] * fxb + cs[i] * fyb
        for dx in range(-kx, kx + 1):
            u = np.floor(exr + F32(fx + F32(dx))).astype(np.int64)
            w0 = np.floor(eyr + F32(fy + F32(-ky))).astype(np.int64)
            v = _gather(hit, u[:, None], w0[:, None] + np.arange(2 * ky + 1)[None, :]).sum(axis=0)
            j = int(v.argmax())
            if v[j] > best:
                best, arg = int(v[j]), (dx, j - ky, int(r))
    return best, arg
