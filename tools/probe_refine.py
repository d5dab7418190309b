"""refine_poses beside what there was for the job before it ("Measured").

  python tools/probe_refine.py [scans] [--no-yardsticks]
  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_refine.py 2000 --no-yardsticks

The bench scene (synthetic.make_log at bench.PERIOD_S, 1081 beams), `scans` records (default 2000).  The map is the one those
scans draw from their true poses (build_map at the engine's 0.05 m, loaded into a one-particle engine); the guesses are the true
poses plus seeded noise of up to 0.8 of the search window on each axis.  Wall time round a synchronise, REPS calls after a
warm-up:
  batch      refine_poses of all scans in one call, the defaults (substeps 4, window 12, 10 rotations of 0.25 degrees), device
             outputs
  one scan   the same for the first scan alone: its 21 rotations go to 21 workgroups
  locate     what the parent commit offers: one locate_scan per scan over the box of the same extent round the guess's cell
             (7 x 7 cells, 720 headings), on a subsample and scaled to all scans.  Its answer is quantised to cell centres and
             half-degree headings and searches the full turn: a DIFFERENT answer
  oracle     tests/refine_oracle.py (NumPy) on a subsample, scaled
Under rocprofv3 the trace holds the kernels' own times: REPS + 1 dispatches of refine_search_kernel per line above (the first of
each a warm-up), after one that prints the result."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS = 5, 1081


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
    from thesis_amd import rebuild, refine
    from thesis_amd.datasets import synthetic
    from thesis_amd.engine import ParticleEngine
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 2000
    yardsticks = "--no-yardsticks" not in sys.argv
    ang, ranges, _, truth = synthetic.make_log(n - 1, BEAMS, period=bench.PERIOD_S)
    truth, ranges = np.ascontiguousarray(truth[:n]), np.ascontiguousarray(ranges[:n])
    e = ParticleEngine(1, max_beams=BEAMS, pool_tiles=16)
    e.load_map(rebuild.as_raster(e.build_map(truth, ranges, ang), engine=e), particle=0)
    rng = np.random.Generator(np.random.PCG64(7))
    step = float(np.radians(0.25))
    guess = truth + rng.uniform(-1.0, 1.0, (n, 3)) * 0.8 * np.array([0.15, 0.15, 10 * step])
    res = e.refine_poses(guess, ranges, ang, particle=0)
    err = lambda p: (float(np.median(np.hypot(p[:, 0] - truth[:, 0], p[:, 1] - truth[:, 1]))),
                     float(np.median(np.abs((p[:, 2] - truth[:, 2] + np.pi) % (2 * np.pi) - np.pi))))
    print(f"{n} scans of {BEAMS} beams, {REPS} timed calls each; {len(refine.moved(res))} scans moved, mean fraction "
          f"{float(np.mean(res.score_guess / (2.0 * np.maximum(res.n_used, 1)))):.4f} -> {float(np.mean(refine.fraction(res))):.4f}; median error "
          f"{err(guess)[0]:.4f} m / {err(guess)[1]:.5f} rad -> {err(res.poses)[0]:.4f} m / {err(res.poses)[1]:.5f} rad")
    t_batch = show("batch", timed(lambda: e.refine_poses(guess, ranges, ang, particle=0, device=True), e.synchronize))
    show("one scan", timed(lambda: e.refine_poses(guess[0], ranges[0], ang, particle=0, device=True), e.synchronize))
    if yardsticks:
        sub = np.linspace(0, n - 1, min(n, 40)).astype(int)
        inv = e.dim / float(e.cfg.tile_len_m)

        def locate_all():
            for k in sub:
                X, Y = int(np.floor(guess[k, 0] * inv)), int(np.floor(guess[k, 1] * inv))
                e.locate_scan(ranges[k], ang, particle=0, box=(X - 3, X + 4, Y - 3, Y + 4), n_rot=720, device=True)
        t_loc = show("locate", timed(locate_all, e.synchronize), scale=n / len(sub))
        from tests.refine_oracle import refine as oracle
        m = e.render_map(0)
        few = sub[:3]
        c = e.cfg
        t_or = show("oracle", timed(lambda: oracle(m.cells, m.x0, m.y0, guess[few], ranges[few], ang, inv, float(c.quantum), float(c.occupied_threshold),
                                                   float(c.match_min_range), float(c.match_max_range), 4, 12, 10, step), lambda: None, reps=2),
                    scale=n / len(few))
        print(f"  locate / batch = {t_loc / t_batch:.1f}   oracle / batch = {t_or / t_batch:.0f}")
    e.close()


if __name__ == "__main__":
    main()
