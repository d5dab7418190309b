"""The NDT refinement restatement (oracle/matcher_oracle.py; matchScanCustom.m:32-37, parity unpinned against MATLAB):
its analytic derivatives are the derivatives of its score, and the damped Newton ascent converges on a known pose.
Then the general form (NDT cells of 3, 4 and 5 matcher cells) on its own -- derivatives, anchoring of the grids to the
global cell index -- and the preconditions of the adjacent-scan cases that tests/test_gpu_matcher_ndt.py runs on the
device (tests/ndt_scenes.py): each enters the stage, decides clearly and is stable in the reference."""
import numpy as np
import pytest

from oracle import matcher_oracle as mo
from tests import ndt_scenes as scenes


def room(N=672, half=100, thick=2):
    occ = np.zeros((N, N), dtype=bool)
    c = N // 2
    for t in range(thick):
        occ[c - half - t, c - half:c + half + 1] = True
        occ[c + half + t, c - half:c + half + 1] = True
        occ[c - half:c + half + 1, c - half - t] = True
        occ[c - half:c + half + 1, c + half + t] = True
    ang = np.linspace(-np.pi, np.pi, 720, endpoint=False) + 0.0123
    d = half + 0.5
    r = d / np.maximum(np.abs(np.cos(ang)), np.abs(np.sin(ang)))
    return occ, np.stack([r * np.cos(ang), r * np.sin(ang)], 1), c + 0.5


def test_gradient_and_hessian_are_derivatives_of_the_score():
    occ, pts, c = room()
    p = np.array([c + 0.31, c - 0.22, 0.003])
    m = mo.ndt_eval(occ, pts, p, 2, 17, -5)
    H = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    for k, h in enumerate((1e-6, 1e-6, 1e-8)):
        e = np.zeros(3); e[k] = h
        up, dn = mo.ndt_eval(occ, pts, p + e, 2, 17, -5), mo.ndt_eval(occ, pts, p - e, 2, 17, -5)
        assert abs((up[0] - dn[0]) / (2 * h) - m[1 + k]) < 1e-5 * max(1.0, abs(m[1 + k]))
        assert np.allclose((up[1:4] - dn[1:4]) / (2 * h), H[k], rtol=1e-4, atol=1e-3 * np.abs(H).max())


def test_cells_with_fewer_than_three_points_carry_no_gaussian():
    occ = np.zeros((64, 64), dtype=bool)
    occ[10, 10] = occ[10, 11] = True                     # two points in every NDT cell that holds them
    pts = np.array([[0.0, 0.0]])
    assert mo.ndt_eval(occ, pts, (10.5, 10.5, 0.0), 2, 0, 0)[0] == 0.0
    occ[11, 10] = True                                   # three points: the grids that hold all three respond
    assert mo.ndt_eval(occ, pts, (10.5, 10.5, 0.0), 2, 0, 0)[0] < 0.0


def test_collinear_points_get_the_eigenvalue_floor():
    occ = np.zeros((64, 64), dtype=bool)
    occ[8, 8:12] = True                                  # four collinear points inside one 4x4 NDT cell
    ok, qx, qy, B00, B01, B11 = mo._cell_stats(occ, np.array([8]), np.array([8]), 4)
    assert ok[0] and np.isfinite([B00[0], B01[0], B11[0]]).all()
    cov = np.linalg.inv(np.array([[B00[0], B01[0]], [B01[0], B11[0]]]))
    ev = np.linalg.eigvalsh(cov)
    assert np.isclose(ev[0] / ev[1], mo.NDT_EIG_FLOOR, rtol=1e-9)


def test_newton_ascent_recovers_the_pose():
    occ, pts, c = room()
    for start in ((c + 0.6, c - 0.4, 0.004), (c - 0.7, c + 0.7, -0.003), (c, c, 0.0)):
        p, score, evals = mo.ndt_refine(occ, pts, start, 2, 0, 0)
        assert abs(p[0] - c) < 0.05 and abs(p[1] - c) < 0.05 and abs(p[2]) < 1e-3
        assert evals < 60 and score > 0.9 * -mo.ndt_eval(occ, pts, (c, c, 0.0), 2, 0, 0, True)[0]


# ---- the general form (nc != 2: ndt_point in kernels_match.hip), checked before anything is compared with it --------
ORIGINS = [(17, -5), (-244, -259), (-1, 7), (0, 0)]           # region origins: residues mod nc differ, two lie on the negative side
EPS = np.finfo(np.float64).eps


def _hess(m):
    return np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])


@pytest.mark.parametrize("nc", [3, 4, 5])
def test_general_form_derivatives_by_central_differences(nc):
    """Gradient and all six Hessian entries of ndt_eval's general form against central differences with steps of 1e-6
    cells and 1e-8 rad.  The allowance is what the difference quotient itself can deliver, nothing measured from the
    result:

    * truncation: h^2 / 6 times the next derivative in the step's direction.  For the quotient of f that is d H_kk / d p_k,
      for the quotient of g_j it is d^2 H_jk / d p_k^2; both are taken from the analytic Hessian at p -+ 1000 h, doubled
      for the terms of higher order;
    * rounding: a beam's cell coordinates (magnitude up to C = 2 N cells: position and cell mean) carry eps * C of rounding,
      which moves a term by its derivative; a term's own arithmetic carries a few eps (16 allowed: the exponent's argument
      reaches 10).  Summed with the terms' absolute values (per beam) and divided by h.
    The step itself is taken as it is representable round p (p +- h rounds at 6e-14 of 1e-6)."""
    occ, pts, c = room()
    pts = pts[::4]
    p = np.array([c + 0.31, c - 0.22, 0.003])
    C = 2.0 * occ.shape[0]
    assert len({(ox % nc, oy % nc) for ox, oy in ORIGINS}) >= 3 and sum(ox < 0 and oy < 0 for ox, oy in ORIGINS) >= 1
    worst = 0.0
    for ox, oy in ORIGINS:
        def ev(q):
            return mo.ndt_eval(occ, pts, q, nc, ox, oy)
        m = ev(p)
        H = _hess(m)
        per = np.abs(np.array([mo.ndt_eval(occ, pts[i:i + 1], p, nc, ox, oy) for i in range(len(pts))])).sum(axis=0)
        assert m[0] < -10.0 and per[0] >= -m[0] * (1 - 1e-12)                    # the scene has Gaussians under its beams
        Ag, AH = per[1:4], _hess(per)
        for k, h in enumerate((1e-6, 1e-6, 1e-8)):
            e = np.zeros(3); e[k] = h
            up_p, dn_p = p + e, p - e
            h_eff = 0.5 * (up_p[k] - dn_p[k])
            up, dn = ev(up_p), ev(dn_p)
            Hp, Hm = _hess(ev(p + 1000 * e)), _hess(ev(p - 1000 * e))
            d = 1000 * h
            tol_f = 2 * h * h / 6 * abs(Hp[k, k] - Hm[k, k]) / (2 * d) + EPS * (C * (Ag[0] + Ag[1]) + 16 * per[0]) / h
            err_f = abs((up[0] - dn[0]) / (2 * h_eff) - m[1 + k])
            assert err_f <= tol_f, (nc, ox, oy, k, err_f, tol_f)
            tol_g = 2 * h * h / 6 * np.abs(Hp[:, k] - 2 * H[:, k] + Hm[:, k]) / (d * d) + EPS * (C * (AH[:, 0] + AH[:, 1]) + 16 * Ag) / h
            err_g = np.abs((up[1:4] - dn[1:4]) / (2 * h_eff) - H[k])
            assert np.all(err_g <= tol_g), (nc, ox, oy, k, err_g, tol_g)
            # the allowance is tight enough to mean something: 1e-4 of the size of the terms it guards
            assert tol_f <= 1e-4 * Ag[k] and np.all(tol_g <= 1e-4 * AH[k].max())
            worst = max(worst, err_f / tol_f, float((err_g / tol_g).max()))
    print(f"nc {nc}: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("mcs", [0.03125, 3.0 / 128, 5.0 / 256])            # nc = 3, 4, 5; all exact in binary
def test_ndt_grids_are_anchored_to_the_global_cell_index(mcs):
    """Shifting the reference points and the guess together by k * nc matcher cells changes nothing: pose relative to
    the guess, score and evaluation count bit for bit.  A shift by one cell moves the grids over the points and does."""
    nc = mo.ndt_cells(mcs)
    assert nc == {0.03125: 3, 3.0 / 128: 4, 5.0 / 256: 5}[mcs]
    N, max_range = 256, 3.5
    k = np.arange(-96, 97)
    layers = [np.stack([k, np.full_like(k, s * t)], 1) for s in (-1, 1) for t in (96, 97)]                 # a room, walls two cells thick,
    layers += [np.stack([np.full_like(k, s * t), k], 1) for s in (-1, 1) for t in (96, 97)]
    layers += [np.stack([k[::2], k[::2] // 3 + 20 + t], 1) for t in (0, 1)]                                # and a slanted wall, on the lattice
    wall = np.unique(np.concatenate(layers), axis=0).astype(np.float64) * mcs
    guess = np.array([5.0 / 1024, -3.0 / 1024, 0.0])
    th = 0.002
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    pts = mo.beams_in_cells(((wall[::3] + 0.5 * mcs) - [0.37 * mcs, 0.55 * mcs]) @ R, mcs)

    def run(shift_cells):
        sh = np.array([shift_cells[0] * mcs, shift_cells[1] * mcs, 0.0])
        g = guess + sh
        occ, ox, oy = mo.rasterise(wall + sh[:2], g, mcs, N, 0.0, max_range)
        X0, Y0 = g[0] / mcs - ox, g[1] / mcs - oy
        pose, score, evals = mo.ndt_refine(occ, pts, (X0, Y0, 0.0), nc, ox, oy)
        return np.array([pose[0] - X0, pose[1] - Y0, pose[2]]), score, evals, occ.sum()

    base = run((0, 0))
    assert base[2] > 1 and base[1] > 10.0 and np.abs(base[0][:2]).max() > 0.3            # the ascent moved
    for sh in [(nc, 0), (0, -nc), (-7 * nc, 4 * nc), (40 * nc, 40 * nc)]:
        got = run(sh)
        assert np.array_equal(got[0], base[0]) and got[1] == base[1] and got[2] == base[2] and got[3] == base[3], sh
    for sh in [(1, 0), (0, 1), (-1, -1)]:
        got = run(sh)
        assert got[3] == base[3]                                   # the same field ...
        assert got[1] != base[1] and not np.array_equal(got[0], base[0]), sh       # ... under other grids


# ---- preconditions of the mode-1 cases of tests/test_gpu_matcher_ndt.py (tests/ndt_scenes.py) -----------------------
@pytest.mark.parametrize("name", list(scenes.CASES))
def test_gpu_cases_enter_the_stage_decide_clearly_and_are_stable(name):
    """Every adjacent-scan case the GPU test runs, here with NumPy's sines and cosines: the geometry is the one the case is
    meant for, every particle enters the stage, the acceptance margin 2 * ndtScore / gridScore is away from 1 by more
    than 1e-3 (window rejections: the pose leaves the window), the outcome is the intended one, and feeding the beams in
    reverse order -- another summation order, nothing else -- leaves the evaluation count and the decisions unchanged and
    the pose and score within 1 / 64 of the nc == 2 bound (what the 64-fold margin of the nc != 2 bound may use up)."""
    c = scenes.CASES[name]
    N, ds, mcs, _, _ = mo.match_geometry(c.cell_size, c.max_range)
    assert (N, ds, mo.ndt_cells(mcs), int(np.floor(0.1 / mcs + 0.5))) == (c.N, c.ds, c.nc, c.nc)
    for p, (r, a, b) in enumerate(scenes.cpu_solution(name)):
        assert a["entered"] and b["entered"] and not r["edge_effect"]
        want = scenes.expected(c, p)
        if want == "window":
            assert not a["valid"] and not a["accepted"] and a["margin"] > 1 + 1e-3        # the score alone would have taken it
            assert max(abs(a["dd"][0]) - r["window"][0], abs(a["dd"][1]) - r["window"][1]) > 1e-3 * mcs     # clearly outside
        else:
            assert a["valid"] and abs(a["margin"] - 1.0) > 1e-3, (p, a["margin"])
            assert a["accepted"] == (want == "accept"), (p, a["margin"])
        assert (a["evals"], a["valid"], a["accepted"]) == (b["evals"], b["valid"], b["accepted"])
        dp = np.abs(a["pose"] - b["pose"]) * [mcs, mcs, 1.0]
        assert dp.max() <= scenes.NC2_POSE_TOL / scenes.GENERAL_MARGIN
        assert abs(a["score"] - b["score"]) <= scenes.NC2_SCORE_RTOL / scenes.GENERAL_MARGIN * max(abs(a["score"]), 1e-300)
        if not a["accepted"]:
            assert np.array_equal(a["row"], r["out"], equal_nan=True)


def test_general_form_bound_is_far_below_the_nc2_bound():
    """The nc != 2 tolerance the GPU test uses: 64 times the reference's sensitivity to the beams' order, floored at 1e-12."""
    dp, ds = scenes.order_sensitivity(scenes.GENERAL)
    bp, bs = scenes.general_bounds(scenes.GENERAL)
    print(f"order sensitivity: pose {dp:.3e} m/rad, score {ds:.3e} relative; bounds {bp:.3e}, {bs:.3e}")
    assert 1e-12 <= bp <= 1e-9 and 1e-12 <= bs <= 1e-9


def test_general_cases_cover_negative_cells_and_several_grid_phases():
    """In every nc != 2 case the beams at the start pose land on both sides of global cell 0 on either axis (the kernel's
    fix-up of C++'s % for negative operands runs, and its plain branch too) and the particles' region origins have
    different residues mod nc."""
    for name in scenes.GENERAL:
        c = scenes.CASES[name]
        sol = scenes.cpu_solution(name)
        assert len({(r["ox"] % c.nc, r["oy"] % c.nc) for r, _, _ in sol}) == len(sol)
        for r, a, _ in sol:
            assert scenes.negative_and_positive_cells(r, a, c.nc)
