"""The scan matcher's second stage (ndt_kernel) against its CPU restatement, oracle/matcher_oracle.py ndt_stage, on
every path that reaches it: the particle path over the particle's own map (mode 0, also at ds = 2), across tile seams and
on the negative side of the map, over the previous scan (mode 1, cell_off 0, from the host list and from
refresh_last_scan), the general form for NDT cells of 3, 4 and 5 matcher cells (nc != 2), the acceptance rule and the
window gate rejecting, beams at and beyond the region's edge, 1 / 2 / 3 / 257 beams, duplicates after a resample.

Per particle: the oracle's row (grid_search, then ndt_stage) against the row match_results reports.  A row the stage
does not rewrite must be the grid row: pose and score exact, covariance to rtol 1e-12, as tests/test_gpu_matcher_grid.py
has it; the covariance of a rewritten row stays the grid one.  The counters must move by what the oracle says: ndt_runs by
the particles that entered (duplicates once), ndt_accepted by those it accepted, ndt_evaluations by the sum of its
evaluation counts -- one flipped "trial < current" decision changes that sum.

Tolerances of a rewritten pose (metres / radians, absolute) and score (relative):

* nc == 2 (float32 terms, hardware exponential): 1e-6 and 1e-6, the bound of test_ndt_stage_equals_oracle
  (tests/test_gpu_matcher.py), which held over the 800 rooms of tests/test_gpu_fuzz.py.
* nc != 2 (float64 throughout): computed here from the reference, not fixed: 64 times the worst difference of the oracle
  with itself when the beams are fed in reverse order (summation order only) over the nc != 2 adjacent-scan cases of
  tests/ndt_scenes.py, at least 1e-12.  Measured: pose 0 (bit for bit), score 2.4e-16 relative, so both bounds are the
  floor, 1e-12 -- 700 units in the last place of a pose of 300 cells of 0.025 m.  tests/test_oracle_ndt.py checks on the
  CPU that the cases are stable and decisive in the reference.

Sines and cosines of the grid stage come from the device (ParticleEngine.native_sincosf), as in the grid tests.  Parity
with MATLAB's matchScans stays unpinned, as everywhere in the matcher (oracle/matcher_oracle.py)."""
import numpy as np
import pytest

from oracle import matcher_oracle as mo
from tests import ndt_scenes as scenes
from tests.test_gpu_matcher_grid import mapped_engine, oracle_particle, room, scan_xy_at, seam_engine, seen_from

pytestmark = pytest.mark.gpu

PI = np.pi
COUNTERS = ("ndt_runs", "ndt_accepted", "ndt_evaluations")


@pytest.fixture(scope="module")
def largest_nc():
    """The nc >= 5 case: 40/2048 m cells (nc = 5) unless rbpf_create refuses that cell size, then 0.0125 m (nc = 8)."""
    from thesis_amd.engine import ParticleEngine, RbpfError
    c = scenes.CASES["nc5"]
    try:
        ParticleEngine(1, cell_size=c.cell_size, match_max_range=c.max_range, pool_tiles=2).close()
        return "nc5"
    except RbpfError:
        return "nc8"


@pytest.fixture(scope="module")
def general_tol(largest_nc):
    """(pose, relative score) bound of the nc != 2 cases, from the reference's own sensitivity (see the module docstring)."""
    names = ("nc4", "nc3", largest_nc)
    dp, ds = scenes.order_sensitivity(names)
    bp, bs = scenes.general_bounds(names)
    print(f"nc != 2: order sensitivity pose {dp:.3e}, score {ds:.3e}; bounds {bp:.3e}, {bs:.3e}")
    return bp, bs


def tolerances(nc, general_tol):
    return (scenes.NC2_POSE_TOL, scenes.NC2_SCORE_RTOL) if nc == 2 else general_tol


def compare_row(got, grid, st, tol, tag):
    """One 13-row against the oracle: st is ndt_stage's dict, grid the grid stage's row."""
    tp, ts = tol
    np.testing.assert_allclose(got[3:12], grid[3:12], rtol=1e-12, atol=1e-17)
    if st["accepted"]:
        w = st["row"]
        dp, dsc = np.abs(got[:3] - w[:3]).max(), abs(got[12] - w[12]) / abs(w[12])
        print(f"{tag}: accepted, evals {st['evals']}, margin {st['margin']:.4f}, pose diff {dp:.3e}, score diff {dsc:.3e} (bounds {tp:.1e}, {ts:.1e})")
        assert dp <= tp and dsc <= ts, (tag, got[:3], w[:3], got[12], w[12])
    else:
        print(f"{tag}: grid row, entered {st['entered']}, valid {st['valid']}, evals {st['evals']}, margin {st['margin']:.4f}")
        assert np.array_equal(got[:3], grid[:3]) and got[12] == grid[12], (tag, got[:3], grid[:3], got[12], grid[12])


def assert_decisive(st, mode, tag):
    """A case whose acceptance hangs on the last digits of the score tests the rounding, not the stage: replace it."""
    if st["entered"] and st["valid"] and mode == 1:
        assert abs(st["margin"] - 1.0) > 1e-3, (tag, st["margin"])


def check_stage(e, x, y, general_tol, adj=False, last=None, refresh=False, groups=None, tag=""):
    """check_particles of the grid tests, extended by the stage: every particle's row and the three counters.
    groups: the ancestor of every particle after a resample (duplicates run once); returns the stage dicts."""
    poses, covs = e.poses(), e.covs()
    mode = e.cfg.ndt_refine
    pre = [oracle_particle(e, p, x, y, poses[p], covs[p], adj, last) for p in range(e.P)]
    nc = mo.ndt_cells(pre[0]["mcs"])
    sts = [scenes.stage(r, nc, mode) for r in pre]
    before = e.counters()
    e.set_scan_xy(x, y)
    e.scan_update_begin(adj=adj, last_scan_xy=None if (adj and refresh) else last)
    got = e.match_results()
    e.scan_update_end()
    after = e.counters()
    for p in range(e.P):
        assert not pre[p]["edge_effect"]
        assert_decisive(sts[p], mode, f"{tag} p{p}")
        compare_row(got[p], pre[p]["out"], sts[p], tolerances(nc, general_tol), f"{tag} p{p}")
    reps = range(e.P) if groups is None else sorted({groups.index(a) for a in groups})     # the first copy of every ancestor
    want = (sum(sts[p]["entered"] for p in reps), sum(sts[p]["accepted"] for p in reps), sum(sts[p]["evals"] for p in reps))
    delta = tuple(int(after[k] - before[k]) for k in COUNTERS)
    assert delta == want, (tag, dict(zip(COUNTERS, delta)), want)
    return pre, sts, got


# ---- 1. own map, shipped geometry -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs,mode", [(0.05, 1), (0.025, 1), (0.05, 2)])
def test_own_map_shipped_geometry(cs, mode, general_tol):
    """Mode 0, N = 512 (W = 16), nc = 2, cell_off 0; 0.025 m maps run at ds = 2.  Four windows from four covariances, the
    smallest 0.1 m; once with ndt_refine = 2 (every valid pose is taken)."""
    P = 4
    e, ang, rng = mapped_engine(P, np.zeros((P, 3)), cs=cs, ndt_refine=mode)
    try:
        e.set_state(poses=[[0.08, -0.05, 0.03], [-0.04, 0.03, -0.02], [0.0, 0.0, 0.0], [0.2, 0.2, 0.1]],
                    covs=[np.diag([1e-5, 4e-5, 1e-5]), np.diag([1e-7, 1e-7, 1e-6]), np.diag([4e-4, 4e-4, 1e-4]),
                          np.diag([2e-5, 3e-4, 1e-5])])
        x, y = scan_xy_at((0.0, 0.0, 0.0), rng)
        pre, sts, _ = check_stage(e, x, y, general_tol, tag=f"own map {cs} mode {mode}")
        assert (pre[0]["N"], pre[0]["ds"], mo.ndt_cells(pre[0]["mcs"])) == (512, 1 if cs == 0.05 else 2, 2)
        assert min(min(r["window"][:2]) for r in pre) == 0.1 and len({r["window"][:2] for r in pre}) == 4
        assert all(s["entered"] for s in sts)
    finally:
        e.close()


# ---- 2. negative side and tile seams ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_negative_side_and_tile_seams(mode, general_tol):
    """The poses of test_particle_path_negative_side_and_tile_seam with the stage on.  Their maps hold two scans: walls one
    cell thick, so the reference's rule (mode 1) rejects and the rows must stay the grid rows; mode 2 takes every valid
    pose, so the stage's own poses across the seams are compared as well.  A particle whose grid stage finds no overlap
    does not enter."""
    e, x, y = seam_engine(ndt_refine=mode)
    try:
        pre, sts, _ = check_stage(e, x, y, general_tol, tag=f"seams mode {mode}")
        assert [s["entered"] for s in sts] == [r["ok"] for r in pre] and sum(s["entered"] for s in sts) >= 3
        assert mode == 1 or sum(s["accepted"] for s in sts) >= 3
    finally:
        e.close()


# ---- 3. / 4. / 5. adjacent scan: shipped geometry, the general form, rejections ----------------------------------------
def run_adjacent(name, general_tol, refresh=False):
    """One case of tests/ndt_scenes.py on the device (mode 1: no map is read)."""
    from thesis_amd.engine import ParticleEngine
    c = scenes.CASES[name]
    N, ds, mcs, _, _ = mo.match_geometry(c.cell_size, c.max_range)
    assert (N, ds, mo.ndt_cells(mcs), int(np.floor(0.1 / mcs + 0.5))) == (c.N, c.ds, c.nc, c.nc)
    (x0, y0), last, (x, y) = scenes.scans(name)
    P = len(c.poses)
    e = ParticleEngine(P, max_beams=1081, cell_size=c.cell_size, match_max_range=c.max_range, pool_tiles=8 * P, ndt_refine=c.mode)
    try:
        if refresh:
            assert c.thin == 1
            e.set_state(poses=c.true0)
            e.set_scan_xy(x0, y0)
            e.refresh_last_scan(0)
        e.set_state(poses=np.array(c.poses), covs=scenes.covariances(c))
        pre, sts, got = check_stage(e, x, y, general_tol, adj=True, last=last, refresh=refresh, tag=name + (" refreshed" if refresh else ""))
        assert pre[0]["N"] == c.N
        for p, (r, s) in enumerate(zip(pre, sts)):
            want = scenes.expected(c, p)
            assert s["entered"] and s["accepted"] == (want == "accept") and s["valid"] == (want != "window"), (name, p, want)
        return pre, sts, got
    finally:
        e.close()


@pytest.mark.parametrize("refresh", [False, True])
def test_adjacent_scan_shipped_geometry(refresh, general_tol):
    """Mode 1 at 0.05 m: N = 512, nc = 2, cell_off 0, windows 0.7 / 0.1 / 0.7 m; two particles are taken, the third is
    rejected by 2 * ndtScore > gridScore.  The previous scan from the host list and from refresh_last_scan."""
    run_adjacent("adjacent", general_tol, refresh)


@pytest.mark.parametrize("which", ["nc4", "nc3", "largest"])
def test_general_form_adjacent_scan(which, largest_nc, general_tol):
    """ndt_point, the branch for nc != 2, in mode 1: (0.025 m, 5 m) nc = 4, W = 16; (0.03125 m, 9 m) nc = 3, W = 21;
    (40/2048 m, 5 m) nc = 5, W = 20 -- replaced by (0.0125 m, 2.5 m), nc = 8, W = 19, only if rbpf_create refuses 40/2048 m.
    The particles sit on both sides of the origin: at the start pose the operands of the kernel's two % take both signs on
    either axis, and the region origins have four different residue pairs mod nc."""
    name = largest_nc if which == "largest" else which
    c = scenes.CASES[name]
    assert c.nc >= 5 if which == "largest" else c.nc == int(which[2:])
    pre, sts, _ = run_adjacent(name, general_tol)
    assert pre[0]["N"] // 32 == {"nc4": 16, "nc3": 21, "nc5": 20, "nc8": 19}[name]
    assert len({(r["ox"] % c.nc, r["oy"] % c.nc) for r in pre}) == len(pre)
    assert all(scenes.negative_and_positive_cells(r, s, c.nc) for r, s in zip(pre, sts))


def lobed_scan(max_range, ang, rng):
    """Ranges of the three-lobed room of tests/ndt_scenes.py seen from the origin."""
    return 0.5 * max_range * (1.0 + 0.3 * np.sin(3 * ang + 0.4)) + rng.normal(0, 0.004, ang.shape)


@pytest.mark.parametrize("name", ["nc4", "nc3"])
def test_general_form_own_map(name, general_tol):
    """The same two configurations in mode 0: the field from the particle's own tiles (three scans of the lobed room)."""
    from thesis_amd.engine import ParticleEngine
    from thesis_amd.datasets import synthetic
    from oracle import rbpf_oracle as orc
    c = scenes.CASES[name]
    N, ds, mcs, _, _ = mo.match_geometry(c.cell_size, c.max_range)
    assert (N, ds, mo.ndt_cells(mcs), int(np.floor(0.1 / mcs + 0.5))) == (c.N, c.ds, c.nc, c.nc)
    P = len(c.poses)
    ang = synthetic.beam_angles(1081)
    rng = np.random.Generator(np.random.PCG64(c.nc))
    e = ParticleEngine(P, max_beams=1081, cell_size=c.cell_size, match_max_range=c.max_range, pool_tiles=8 * P, ndt_refine=1)
    try:
        for _ in range(3):
            e.set_scan(lobed_scan(c.max_range, ang, rng), ang)
            e.map_update(np.zeros((P, 3)))
        poses = np.array(c.poses) - [0.0, 0.0, 0.1]                       # headings round 0, where the map was drawn from
        e.set_state(poses=poses, covs=scenes.covariances(c))
        x, y = orc.scan_xy(lobed_scan(c.max_range, ang, rng), ang)
        pre, sts, _ = check_stage(e, x, y, general_tol, tag=name + " own map")
        assert all(s["entered"] for s in sts) and any(s["accepted"] for s in sts)
        assert len({(r["ox"] % c.nc, r["oy"] % c.nc) for r in pre}) == P
        assert all(scenes.negative_and_positive_cells(r, s, c.nc) for r, s in zip(pre, sts))
    finally:
        e.close()


@pytest.mark.parametrize("name", ["thin", "window"])
def test_rejections_leave_the_grid_row(name, general_tol):
    """thin: every seventh point of the previous scan makes the field, no NDT cell holds three points, the score rule
    rejects.  window: the truth lies 0.13 m from the particle, outside its 0.1 m window; the ascent leaves the window and
    the validity gate rejects a pose the score rule would have taken.  Either way the row is the grid row and
    ndt_accepted does not move (check_stage compares all three counters)."""
    _, sts, _ = run_adjacent(name, general_tol)
    assert not any(s["accepted"] for s in sts)
    if name == "window":
        assert all(s["margin"] > 1.0 and not s["valid"] for s in sts)


# ---- 6. / 7. the stateless twin at 20 cells/m: region edge, beam counts -------------------------------------------------
@pytest.fixture(scope="module")
def eng_twin():
    from thesis_amd.engine import ParticleEngine
    e = ParticleEngine(1, max_beams=4095, ndt_refine=2)
    yield e
    e.close()


def twin_oracle(curr, ref, guess, cpm, rng3, mode, sincos):
    """rbpf_match_scan with the stage on, restated: (grid dict, stage dict, (occ, ox, oy))."""
    _, _, _, r = mo.match_scan_oracle(curr, ref, guess, cpm, rng3, sincos=sincos)
    occ, ox, oy = mo.rasterise_fast(ref, guess, r["mcs"], r["N"], 0.5, mo.TWIN_MAX_RANGE)
    st = mo.ndt_stage(occ, ox, oy, mo.beams_in_cells(curr, r["mcs"]), r, guess, rng3, r["mcs"], 0.5, mo.ndt_cells(r["mcs"]), mode)
    return r, st, (occ, ox, oy)


def check_twin_stage(e, curr, ref, guess, cpm, rng3, tag):
    from thesis_amd.engine import match_scan
    mode = e.cfg.ndt_refine
    before = e.counters()
    pose, cov, score = match_scan(e, curr, ref, guess, cpm, rng3)
    after = e.counters()
    r, st, field = twin_oracle(curr, ref, guess, cpm, rng3, mode, e.native_sincosf)
    assert not r["edge_effect"]
    assert_decisive(st, mode, tag)
    gp, gc, gs = mo.twin_gate(r["out"], guess, rng3)
    wp, wc, ws = mo.twin_gate(st["row"], guess, rng3)
    assert np.array_equal(np.isnan(cov), np.isnan(wc))
    delta = tuple(int(after[k] - before[k]) for k in COUNTERS)
    print(f"{tag}: evaluations {delta[2]}, oracle {st['evals']}")
    compare_row(np.concatenate([pose, cov.reshape(-1), [score]]), np.concatenate([gp, gc.reshape(-1), [gs]]),
                dict(st, row=np.concatenate([wp, wc.reshape(-1), [ws]])), tolerances(mo.ndt_cells(r["mcs"]), None), tag)
    assert delta == (int(st["entered"]), int(st["accepted"]), st["evals"]), (tag, delta, st["evals"])
    return r, st, field


def test_region_edge_hot_form(eng_twin):
    """The scene of test_twin_region_edges (reference points on the 14.98 m circle, current points out to 19 m) plus four
    ladders of points across the region's four edges, with the stage on: beams outside the region take the hot form's
    `inside == false` lane, beams in rows / columns 0 and N - 1 read the zero border of its field copy."""
    cpm, mcs = 20, 0.05
    rng = np.random.Generator(np.random.PCG64(cpm + 1))
    a = np.linspace(-PI, PI, 3000, endpoint=False)
    ref = np.concatenate([np.stack([14.98 * np.cos(a), 14.98 * np.sin(a)], 1), room(3.0, mcs)])
    true = (0.4, -0.3, 0.02)
    t, s = np.arange(-0.15, 0.15, 0.006), np.linspace(-6.0, 6.0, 50)
    ladders = np.concatenate([np.stack([e + t, s], 1) for e in (-16.8, 16.8)] + [np.stack([s, e + t], 1) for e in (-16.8, 16.8)])
    curr = np.concatenate([seen_from(ref, true)[::2], rng.uniform(-19, 19, size=(800, 2)), seen_from(ladders, true)])
    r, st, (occ, ox, oy) = check_twin_stage(eng_twin, curr, ref, [0.0, 0.0, 0.0], cpm, [1.5, 1.5, 0.2], "region edge")
    N = r["N"]
    assert N == 672 and st["entered"]
    pts = mo.beams_in_cells(curr, mcs)
    u, w = scenes.beam_cells({"bx": pts[:, 0], "by": pts[:, 1]}, st)
    outside = (u < 0) | (u >= N) | (w < 0) | (w >= N)
    assert outside.sum() >= 20 and (u[~outside] == 0).any() and (u[~outside] == N - 1).any() and (w[~outside] == 0).any() and (w[~outside] == N - 1).any()
    assert (u < 0).any() and (u >= N).any() and (w < 0).any() and (w >= N).any()


def nudge_response(curr, ref, guess, cpm, rng3, mode, sincos, st):
    """The beams are staged in float32: the problem is stated to one unit in the last place of their coordinates.  Both
    nudges by that unit, through the oracle: (largest nudge in metres, largest move of the pose, evaluation counts)."""
    c32 = np.asarray(curr, dtype=np.float32)
    size, move, evals = 0.0, 0.0, set()
    for sgn in (-1.0, 1.0):
        nudged = np.nextafter(c32, np.float32(sgn * np.inf)).astype(np.float64)
        _, b, _ = twin_oracle(nudged, ref, guess, cpm, rng3, mode, sincos)
        size = max(size, float(np.abs(nudged - c32).max()))
        move = max(move, float(np.abs(b["row"][:3] - st["row"][:3]).max()))
        evals.add(b["evals"])
    return size, move, evals


@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_beam_counts(eng_twin, n):
    """1 to 3 beams: the Hessian is singular (one point fixes two of three directions), the damped matrix is refused as not
    positive definite and the damping climbs (to 1e3 with seed 18, 11 evaluations).  257 beams: one more than the kernel's
    threads, lane 0 takes a second beam.

    A singular problem can also be ILL-POSED: where the ascent runs on with the damping at its floor, the step along
    the free direction is rounding noise divided by rounding noise.  Such a case has no answer to compare with - the
    reference itself is unstable, and the rule of tests/test_oracle_ndt.py applies: replace it.  The criterion is the
    reference's alone: nudging every beam coordinate by one float32 unit in the last place (2.4e-7 or 4.8e-7 m here: the precision
    the problem is stated in, and the size of the rounding by which kernel and oracle differ) must leave the evaluation
    count unchanged and move the reference's pose by no more than the bound it is compared at, 1e-6.  Seeds 18, 25 and 28
    move it by 5e-7 to 8e-7 with 1 to 3 beams and by 3e-7 with 257.  Seed 41, tried first, does not qualify: with 1, 2 or
    3 beams (one of them under a Gaussian) the reference moves by 1.9e-2 m and runs 5 or 9 evaluations instead of 10; the
    kernel's pose there differs from the oracle's by 1.5e-4 m and its score by 2.6e-7 relative."""
    mcs = 0.05
    for seed in (18, 25, 28):
        rng = np.random.Generator(np.random.PCG64(seed))
        ref = room(4.0, mcs, rng, clutter=200)
        guess = np.array([0.03, -0.02, 0.1])
        seen = seen_from(ref, guess + [0.11, -0.07, 0.03], guess[2])
        curr = seen[rng.permutation(len(seen))[:n]]
        assert len(curr) == n
        rng3 = [0.7, 0.7, PI / 6]
        r, st, _ = check_twin_stage(eng_twin, curr, ref, guess, 20, rng3, f"{n} beams, seed {seed}")
        assert st["entered"] and st["evals"] >= 2
        size, move, evals = nudge_response(curr, ref, guess, 20, rng3, 2, eng_twin.native_sincosf, st)
        print(f"{n} beams, seed {seed}: nudge {size:.2e} m moves the reference by {move:.2e}, evaluations {sorted(evals)}")
        assert evals == {st["evals"]} and move <= scenes.NC2_POSE_TOL, (seed, size, move, evals)


# ---- 8. duplicates after a resample -------------------------------------------------------------------------------------
def test_duplicates_after_resample(general_tol):
    """The stage runs once per group of exact copies; every copy reports its representative's row, and that row is the
    oracle's for the copy."""
    P = 6
    e, ang, rng = mapped_engine(P, np.zeros((P, 3)), ndt_refine=1)
    try:
        e.set_state(poses=[[0.05 * i, -0.03 * i, 0.01 * i] for i in range(P)], covs=np.diag([1e-4, 1e-4, 1e-5]),
                    weights=[300.0, 0, 0, 299.0, 0, 0])
        did, idx = e.resample(0.37)
        assert did and len(set(idx.tolist())) < P
        x, y = scan_xy_at((0.0, 0.0, 0.0), rng)
        _, sts, got = check_stage(e, x, y, general_tol, groups=idx.tolist(), tag="duplicates")
        assert all(s["entered"] for s in sts)
        for p in range(P):
            assert np.array_equal(got[p], got[idx.tolist().index(idx[p])], equal_nan=True)
    finally:
        e.close()
