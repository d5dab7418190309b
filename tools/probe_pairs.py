"""match_pairs beside what there was for the job before it ("Measured").

  python tools/probe_pairs.py [pairs] [--no-yardsticks]
  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_pairs.py 1000 --no-yardsticks

The bench scene (synthetic.make_log at bench.PERIOD_S, 1081 beams), 2000 scans: the circle is walked 37 times, so every scan
from the third lap on has earlier scans beside it.  `pairs` pairs (default 1000) from loops.candidates at the true poses
(min_gap 50, radius 0.5 m, runs of 11); the guesses are the queries' true poses plus seeded noise of up to 0.8 of the search
window on each axis (window 16 cells, 20 rotations of 0.5 degrees: the defaults).  At 0.05 m and at 0.1 m, wall time round a
synchronise, REPS calls after a warm-up:
  batch      match_pairs of all pairs in one call, device outputs
  one pair   the same for the first pair alone: its 41 rotations go to 41 workgroups
  parent     what the parent commit offers for the same pairs: per pair one build_map of the run, one place_map of it into a
             one-particle engine of that cell size and one refine_poses of the query there with the same window, on 40 pairs and
             scaled.  Its field is the log-odds map of the run thresholded (a hit that later beams pass through can be carved
             away, a cell needs occ > threshold), not the end points themselves: a DIFFERENT field, and the line after it counts
             the pairs of the 40 whose best candidate agrees
Under rocprofv3 the trace holds the kernels' own times: REPS + 1 dispatches of pairs_field_kernel and pairs_search_kernel per
line above (the first of each a warm-up), after one that prints the result."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS, SCANS = 5, 1081, 2000


def timed(fn, sync, reps=REPS):
    fn()
    sync()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def show(name, ms, scale=1.0):
    ms = [m * scale for m in ms]
    print(f"  {name:10s} min {min(ms):10.3f}  median {float(np.median(ms)):10.3f}  max {max(ms):10.3f} ms", flush=True)
    return float(np.median(ms))


def main():
    import bench
    from thesis_amd import loops, rebuild
    from thesis_amd.datasets import synthetic
    from thesis_amd.engine import ParticleEngine
    from thesis_amd.refine import _map_engine
    m = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1000
    yardsticks = "--no-yardsticks" not in sys.argv
    ang, ranges, _, truth = synthetic.make_log(SCANS - 1, BEAMS, period=bench.PERIOD_S)
    truth, ranges = np.ascontiguousarray(truth[:SCANS]), np.ascontiguousarray(ranges[:SCANS])
    pairs = loops.candidates(truth, min_gap=50, radius=0.5, half_run=5)[:m]
    m = len(pairs)
    step = float(np.radians(0.5))
    rng = np.random.Generator(np.random.PCG64(7))
    true_q = truth[pairs[:, 0]]
    guess = true_q + rng.uniform(-1.0, 1.0, (m, 3)) * 0.8 * np.array([0.8, 0.8, 20 * step])
    e = ParticleEngine(1, max_beams=BEAMS, pool_tiles=16)
    err = lambda p: (float(np.median(np.hypot(p[:, 0] - true_q[:, 0], p[:, 1] - true_q[:, 1]))),
                     float(np.median(np.abs((p[:, 2] - true_q[:, 2] + np.pi) % (2 * np.pi) - np.pi))))
    for cs in (0.05, 0.1):
        guess_cs = true_q + (guess - true_q) * [cs / 0.05, cs / 0.05, 1.0]       # the same share of the window at either cell size
        res = e.match_pairs(truth, ranges, ang, pairs, guess_cs, cell_size=cs)
        frac = res.score / (2.0 * np.maximum(res.n_used, 1))
        print(f"cell {cs} m: {m} pairs over {SCANS} scans of {BEAMS} beams, runs of {int(np.median(pairs[:, 2] - pairs[:, 1]))}, {REPS} timed calls each; "
              f"median fraction {float(np.median(res.score_guess / (2.0 * np.maximum(res.n_used, 1)))):.3f} -> {float(np.median(frac)):.3f}; median error "
              f"{err(guess_cs)[0]:.4f} m / {err(guess_cs)[1]:.5f} rad -> {err(res.poses)[0]:.4f} m / {err(res.poses)[1]:.5f} rad")
        t_batch = show("batch", timed(lambda: e.match_pairs(truth, ranges, ang, pairs, guess_cs, cell_size=cs, device=True), e.synchronize))
        show("one pair", timed(lambda: e.match_pairs(truth, ranges, ang, pairs[0], guess_cs[0], cell_size=cs, device=True), e.synchronize))
        if not yardsticks:
            continue
        sub = np.linspace(0, m - 1, min(m, 40)).astype(int)
        box = e.build_box(truth, 1.0 / cs, float(e.cfg.max_ray_m))
        me = _map_engine(e, box, cs, BEAMS)
        found = []

        def parent():
            found.clear()
            for k in sub:
                q, r0, r1 = (int(v) for v in pairs[k])
                built = e.build_map(truth[r0:r1], ranges[r0:r1], ang, cell_size=cs, box=box)
                me.place_map(rebuild.as_source(built, engine=e), particle=0)
                found.append(me.refine_poses(guess_cs[k], ranges[q], ang, particle=0, substeps=1, window=16, rotations=20, rot_step=step))
        t_par = show("parent", timed(parent, lambda: (e.synchronize(), me.synchronize()), reps=2), scale=m / len(sub))
        same = sum(int(np.array_equal(f.index[0], res.index[k])) for f, k in zip(found, sub))
        d = np.concatenate([f.poses for f in found]) - true_q[sub]
        print(f"  parent / batch = {t_par / t_batch:.0f}; {same} of {len(sub)} pairs have the same best candidate; the parent path's median error on them "
              f"{float(np.median(np.hypot(d[:, 0], d[:, 1]))):.4f} m / {float(np.median(np.abs((d[:, 2] + np.pi) % (2 * np.pi) - np.pi))):.5f} rad")
        me.close()
    e.close()


if __name__ == "__main__":
    main()
