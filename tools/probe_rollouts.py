"""check_rollouts on the bench scene against check_paths of the placed templates ("Measured").

  python tools/probe_rollouts.py [P] [steps]                 (wall times)
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/probe_rollouts.py [P] [steps]
  python tools/probe_rollouts.py --report OUT/.../kt_kernel_trace.csv

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and takes three cases:  (b) of tools/probe_paths.py,
ROLLOUTS arcs of 13 waypoints from every particle's own pose, each in its own particle's map;  (one map, 1024) the same arcs from
the first 1024 particle poses in the best particle's map;  (one map, P) from all of them.  Each case first asserts that
check_rollouts equals check_paths of plan.place_templates, all five fields, then calls the two alternately, REPS + 1 times each
(the first is a warm-up), and prints the wall time round each call as minimum / median / maximum.  plan.place_templates, which
the old call needs first, is timed on its own.  --report prints the same of the trace's dispatches per kernel and case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS, RADIUS, ROLLOUTS = 5, 1081, 0.2, 256
CASES = ("(b)", "(one map, 1024)", "(one map, P)")


def report(path):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("check_rollouts_kernel", "check_paths_kernel"):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if kernel in r["Kernel_Name"]]
        print(f"{len(ms)} dispatches of {kernel}")
        per = REPS + 2                                   # the comparison's call, the warm-up, REPS timed calls
        for k, what in enumerate(CASES):
            v = ms[k * per + 2:(k + 1) * per]
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


def main(P, steps):
    from probe_paths import scene                      # beside this file: the bench scene, as that probe builds it
    from thesis_amd import plan
    e = scene(P, steps).e
    poses = e.poses()
    v, w = np.meshgrid(np.linspace(0.1, 1.0, 16), np.linspace(-1.0, 1.0, 16))
    tm = plan.arc_templates(v.ravel(), w.ravel(), 6.0, 0.5)                 # [256, 13, 2]
    best = int(np.argmax(e.weights()))
    print(f"P {P}, {steps} steps, radius {RADIUS} m, {ROLLOUTS} templates of {tm.shape[1]} waypoints")
    for what, ps, particle in zip(CASES, (poses, poses[:1024], poses), (None, best, best)):
        t0 = time.perf_counter()
        arcs = plan.place_templates(ps, tm)
        t_place = (time.perf_counter() - t0) * 1e3
        own = particle is None
        paths = arcs if own else arcs.reshape((-1,) + arcs.shape[2:])
        new = lambda: e.check_rollouts(ps, tm, particle=particle, radius_m=RADIUS)
        old = lambda: e.check_paths(paths, particle=particle, radius_m=RADIUS, own=own)
        a, b = new(), old()
        for x, y in zip(a[:5], b[:5]):
            assert np.array_equal(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)), what
        tn, to = alternate(new, old)
        print(f"{what} {len(ps)} poses, {int(a.steps.sum())} steps, clear share {a.clear.mean():.3f}; equal to check_paths of the placed templates")
        print(f"{what} check_rollouts: {spread(tn)}")
        print(f"{what} check_paths:    {spread(to)}   (place_templates before it, once: {t_place:.1f} ms)")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 25)
