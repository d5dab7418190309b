"""view_gain's kernel beside cast_scans_kernel on the same rays and maps ("Measured").

  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_gain.py [P] [steps]
  python tools/probe_gain.py --report OUT/.../kt_kernel_trace.csv

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and then dispatches, REPS + 1 times each (the first
is a warm-up):  (a) view_gain of 64 poses x 1081 beams x 15 m in particle 0's map, then cast_scans of the same rays;
(b) view_gain of 8 poses in every particle's map, then the same rays as 8 cast_scans calls (pose j in particle n's map for
all n).  --report splits the trace's dispatches of the two kernels in that order and prints min / median / max per case."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, NA, NB_POSES, BEAMS, RANGE = 5, 64, 8, 1081, 15.0


def report(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if k in r["Kernel_Name"]]
          for k in ("view_gain_kernel", "cast_scans_kernel")}
    g, c = ms["view_gain_kernel"], ms["cast_scans_kernel"]
    assert len(g) == 2 * (REPS + 1) and len(c) == (REPS + 1) * (1 + NB_POSES), (len(g), len(c))
    cb = c[REPS + 1:]
    cases = {"(a) gain": g[1:REPS + 1], "(a) cast": c[1:REPS + 1], "(b) gain": g[REPS + 2:],
             "(b) cast, 8 dispatches": [sum(cb[NB_POSES * k:NB_POSES * (k + 1)]) for k in range(1, REPS + 1)]}
    for name, v in cases.items():
        print(f"{name:26s} min {min(v):8.3f}  median {float(np.median(v)):8.3f}  max {max(v):8.3f} ms  ({len(v)} dispatches)")


def main():
    import bench
    from thesis_amd.datasets import synthetic
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    r = bench.Runner(P, BEAMS, 0.05, synthetic.make_log(steps + 2, BEAMS, period=bench.PERIOD_S))
    for _ in range(steps):
        r.step()
    e = r.e
    e.synchronize()
    ang = synthetic.beam_angles(BEAMS)
    rng = np.random.Generator(np.random.PCG64(9))
    here = r.true_poses[steps]
    pa = here + rng.normal(0, [1.5, 1.5, 1.0], size=(NA, 3))
    pb = here + rng.normal(0, [1.5, 1.5, 1.0], size=(NB_POSES, 3))
    for _ in range(REPS + 1):
        ga = e.view_gain(pa, ang, particle=0, max_range=RANGE, device=True)
    for _ in range(REPS + 1):
        e.cast_scans(pa, ang, particle=0, max_range=RANGE, device=True)
    for _ in range(REPS + 1):
        gb = e.view_gain(pb, ang, particle=None, max_range=RANGE, device=True)
    for _ in range(REPS + 1):
        for j in range(NB_POSES):
            e.cast_scans(np.broadcast_to(pb[j], (P, 3)), ang, particle=None, max_range=RANGE, device=True)
    e.synchronize()
    sa, sb = ga.seen.cpu().numpy(), gb.seen.cpu().numpy()
    print(f"P {P}, {steps} steps: (a) seen per pose {sa.min()} .. {sa.max()}, mean {sa.mean():.0f}; unknown share "
          f"{ga.unknown.sum().item() / sa.sum():.3f}; (b) seen mean {sb.mean():.0f}, unknown share {gb.unknown.sum().item() / sb.sum():.3f}")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        main()
