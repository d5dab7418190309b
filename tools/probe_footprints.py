"""check_footprints on the bench scene beside check_rollouts and beside the host path it replaces ("Measured").

  python tools/probe_footprints.py [P] [steps]                 (wall times)
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/probe_footprints.py [P] [steps] --no-host
  python tools/probe_footprints.py --report OUT/.../kt_kernel_trace.csv

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and takes two cases with a 0.8 m x 0.5 m footprint in 64
heading bins:  (a) ROLLOUTS arcs of 13 waypoints from every particle's own pose, each in its own particle's map;  (b) the same arcs
from the first 1024 particle poses in the best particle's map.  Each case calls check_footprints and check_rollouts of the same
inputs alternately, REPS + 1 times each (the first is a warm-up), and prints the wall time round each call as minimum / median /
maximum.  The host path is what a caller without the entry point would do: render_map and travel_cost(...).clearance read back,
every rollout walked in NumPy and the covered cells looked up (tests/footprint_oracle.py with travel_cost's clearance in place of
its own).  It is timed over HOST rows only - particles in (a), poses in (b) - and scaled to the case, and its first_blocked is
asserted equal to the device's on those rows.  --report prints the trace's dispatches per kernel and case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, RADIUS, ROLLOUTS, HOST, CLEAR_MAX = 5, 0.25, 256, 64, 60
CASES = ("(a)", "(b)")


def report(path):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("check_footprints_kernel", "check_rollouts_kernel"):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if kernel in r["Kernel_Name"]]
        print(f"{len(ms)} dispatches of {kernel}")
        per = REPS + 2                                   # the warm-up, REPS timed calls, the call whose results are compared
        for k, what in enumerate(CASES):
            v = ms[k * per + 1:k * per + 1 + REPS]
            if v:
                print(f"  {what}: min {min(v):.4f}  median {float(np.median(v)):.4f}  max {max(v):.4f} ms per dispatch")


def spread(t):
    return f"min {min(t):.3f} median {float(np.median(t)):.3f} max {max(t):.3f} ms"


def alternate(new, old):
    tn, to = [], []
    for k in range(REPS + 1):
        for f, t in ((new, tn), (old, to)):
            t0 = time.perf_counter()
            f()
            t.append((time.perf_counter() - t0) * 1e3)
    return tn[1:], to[1:]


def host_first_blocked(e, particle, poses, tm, hd, fp, inflate):
    """first_blocked [len(poses), K] of the poses in one particle's map by the host path."""
    from tests import footprint_oracle as FO
    inv = e.dim / float(e.cfg.tile_len_m)
    rolls = FO.rollout_cells(poses, tm, hd, fp.H, inv)
    box = FO.box_of(rolls)
    wide = e.render_map(particle, box=FO.grown_box(box, CLEAR_MAX, FO.table_reach(fp))).cells
    f = FO.Field(np.zeros_like(wide), box, float(e.cfg.quantum), float(e.cfg.occupied_threshold), inflate, CLEAR_MAX, fp)
    f.v = wide.astype(np.int64)
    f.blocked = f.v >= 0
    f.clear = e.travel_cost(poses[0, :2], particle=particle, box=box, radius_m=RADIUS, clear_max=CLEAR_MAX).clearance.astype(np.int64)
    return FO.check_all(f, rolls)[0][..., 0]


def main(P, steps, host):
    from probe_paths import scene                      # beside this file: the bench scene, as that probe builds it
    from thesis_amd import plan
    e = scene(P, steps).e
    poses = e.poses()
    v, w = np.meshgrid(np.linspace(0.1, 1.0, 16), np.linspace(-1.0, 1.0, 16))
    tm, hd = plan.arc_templates(v.ravel(), w.ravel(), 6.0, 0.5), plan.arc_headings(w.ravel(), 6.0, 0.5)      # [256, 13, 2], [256, 13]
    a, b = 0.4, 0.25
    fp = plan.footprint_table(np.array([[a, b], [-a, b], [-a, -b], [a, -b]]), float(e.cfg.tile_len_m) / e.dim, 64)
    best = int(np.argmax(e.weights()))
    print(f"P {P}, {steps} steps, inscribed radius {RADIUS} m, {ROLLOUTS} templates of {tm.shape[1]} waypoints, {len(fp.spans)} spans in {fp.H} bins")
    for what, ps, particle in zip(CASES, (poses, poses[:1024]), (None, best)):
        kw = dict(particle=particle, radius_m=RADIUS, clear_max=CLEAR_MAX)
        new = lambda: e.check_footprints(ps, tm, hd, fp, **kw)
        old = lambda: e.check_rollouts(ps, tm, **kw)
        tn, to = alternate(new, old)
        chk, ref = new(), old()
        assert np.array_equal(chk.min_clearance, ref.min_clearance) and np.array_equal(chk.steps, ref.steps), what
        print(f"{what} {len(ps)} poses, {int(chk.steps.sum())} steps, clear share {chk.clear.mean():.3f} (as discs of the inscribed radius: {ref.clear.mean():.3f})")
        print(f"{what} check_footprints: {spread(tn)}")
        print(f"{what} check_rollouts:   {spread(to)}")
        if host:
            n = min(HOST, len(ps))
            t0 = time.perf_counter()
            if particle is None:
                got = np.concatenate([host_first_blocked(e, p, ps[p:p + 1], tm, hd, fp, chk.inflate) for p in range(n)])
            else:
                got = host_first_blocked(e, particle, ps[:n], tm, hd, fp, chk.inflate)
            t_host = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(got, chk.first_blocked[:n]), what
            print(f"{what} host path over {n} of {len(ps)} rows: {t_host:.0f} ms, first_blocked equal to the device's; scaled to all rows: {t_host * len(ps) / n:.0f} ms")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        args = [a for a in sys.argv[1:] if not a.startswith("--")]
        main(int(args[0]) if len(args) > 0 else 4096, int(args[1]) if len(args) > 1 else 25, "--no-host" not in sys.argv)
