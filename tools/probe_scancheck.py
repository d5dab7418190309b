"""check_scans on the bench scene ("Measured").

  python tools/probe_scancheck.py [P] [steps]                    (wall times)
  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_scancheck.py [P] [steps]
  python tools/probe_scancheck.py --report OUT/.../kt_kernel_trace.csv

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and then calls, REPS + 1 times each (the first is a
warm-up):  (a) check_scans of the current scan at every particle's own pose (particle=None, P x 1081 rays), with NumPy outputs
and with device=True;  (b) check_scans of the current scan at POSES_B poses scattered round the best particle's, in that
particle's map.  Each is set against the path it replaces: cast_scans with NumPy outputs and the vectorised NumPy
classification of tests/scancheck_oracle.py on the ranges and statuses read back - for (b) with the map rendered and the cells
at the measured ends looked up, for (a) without (4096 renders; SHORT and NEW stay one class there, which flatters the
yardstick) - and the results are compared.  --report prints min / median / max of the trace's check_scans_kernel and
cast_scans_kernel dispatches per case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS, POSES_B = 5, 1081, 64


def report(path):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for kernel, cases in (("check_scans_kernel", ("(a) with classes and votes", "(a) cost and counts alone", "(a) device outputs", "(b)")),
                          ("cast_scans_kernel", ("(a)", "(b)"))):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if kernel in r["Kernel_Name"]]
        print(f"{len(ms)} dispatches of {kernel}")
        for k, what in enumerate(cases):
            v = ms[k * (REPS + 1):(k + 1) * (REPS + 1)][1:]
            if v:
                print(f"  {what}: min {min(v):.4f}  median {float(np.median(v)):.4f}  max {max(v):.4f} ms per dispatch")


def scene(P, steps):
    import bench
    from thesis_amd.datasets import synthetic
    r = bench.Runner(P, BEAMS, 0.05, synthetic.make_log(steps + 2, BEAMS, period=bench.PERIOD_S))
    for _ in range(steps):
        r.step()
    r.e.synchronize()
    return r


def timed(f):
    t = []
    for k in range(REPS + 1):
        t0 = time.perf_counter()
        out = f()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, t[1:]


def spread(t):
    return f"min {min(t):.3f} median {float(np.median(t)):.3f} max {max(t):.3f} ms"


def merged(classes):
    from thesis_amd import sensor
    return np.where(classes == sensor.SHORT, sensor.NEW, classes)


def main(P, steps):
    from tests import scancheck_oracle as so
    from thesis_amd import sensor
    r = scene(P, steps)
    e = r.e
    ang, scan = r.angles, r.ranges[r.frame]
    inv = e.dim / float(e.cfg.tile_len_m)
    mr, tol, model = float(e.cfg.weight_max_range), 2 * float(e.cfg.cell_size), sensor.beam_model(e.cfg)
    poses = e.poses()
    names = ", ".join(f"{n} {{}}" for n in sensor.CLASS_NAMES)
    print(f"P {P}, {steps} steps, {BEAMS} beams, max_range {mr} m, tol {tol} m")
    # (a) the current scan at every particle's own pose
    a, wa = timed(lambda: e.check_scans(poses, scan, ang, return_classes=True, return_votes=True))
    _, wa0 = timed(lambda: e.check_scans(poses, scan, ang))
    print(f"(a) {P} x {BEAMS} rays, classes " + names.format(*a.counts.sum(axis=0)) + f"; matched {a.matched().mean():.4f}, "
          f"{int(sensor.dynamic_beams(a).sum())} dynamic beams")
    print(f"(a) check_scans, NumPy outputs with classes and votes: {spread(wa)}; cost and counts alone: {spread(wa0)}")
    try:
        import torch
        def on_device():
            out = e.check_scans(poses, scan, ang, device=True, return_classes=True, return_votes=True)
            torch.cuda.synchronize()
            return out
        d, wd = timed(on_device)
        print(f"(a) check_scans, device=True: {spread(wd)}; equal to the NumPy outputs: "
              f"{all(np.array_equal(getattr(d, k).cpu().numpy(), getattr(a, k)) for k in ('cost', 'counts', 'classes', 'votes'))}")
    except ImportError:
        print("(a) device=True: torch is not installed")

    def yard_a():
        e_r, e_s = e.cast_scans(poses, ang, max_range=mr, return_status=True)
        return so.classify_cast(e_r, e_s, scan, inv, mr, 0.0, tol, model)
    ya, wya = timed(yard_a)
    diff = int((ya["classes"] != merged(a.classes)).sum())
    print(f"(a) yardstick (cast_scans read back + NumPy classification, SHORT and NEW one class): {spread(wya)}; rays whose class "
          f"differs from check_scans with SHORT and NEW merged: {diff} of {a.classes.size}")
    # (b) POSES_B poses in the best particle's map
    k = int(np.argmax(e.weights()))
    rng = np.random.Generator(np.random.PCG64(31))
    fan = poses[k] + rng.normal(0, [1.0, 1.0, 0.5], size=(POSES_B, 3))
    b, wb = timed(lambda: e.check_scans(fan, scan, ang, particle=k, return_classes=True, return_votes=True))
    print(f"(b) {POSES_B} x {BEAMS} rays in particle {k}'s map, classes " + names.format(*b.counts.sum(axis=0)) + f": {spread(wb)}")

    def yard_b():
        e_r, e_s = e.cast_scans(fan, ang, particle=k, max_range=mr, return_status=True)
        m = e.render_map(k)
        ec = so.end_cells(fan, ang, scan, inv)
        i, j = ec[..., 0] - m.x0, ec[..., 1] - m.y0
        ok = (i >= 0) & (i < m.cells.shape[0]) & (j >= 0) & (j < m.cells.shape[1])
        v_end = np.where(ok, m.cells[np.clip(i, 0, m.cells.shape[0] - 1), np.clip(j, 0, m.cells.shape[1] - 1)], 0)
        return so.classify_cast(e_r, e_s, scan, inv, mr, 0.0, tol, model, v_end=v_end)
    yb, wyb = timed(yard_b)
    print(f"(b) yardstick (cast_scans + render_map read back, NumPy classification): {spread(wyb)}; rays whose class differs: "
          f"{int((yb['classes'] != b.classes).sum())} of {b.classes.size}; equal cost: {np.array_equal(yb['cost'], b.cost)}, counts: "
          f"{np.array_equal(yb['counts'], b.counts)}, votes: {np.array_equal(yb['votes'], b.votes)}")
    w = sensor.posterior_weights(b, temperature=float(BEAMS))
    print(f"(b) posterior weights at temperature {BEAMS}: the best pose lies {float(np.hypot(*(fan[int(np.argmax(w))][:2] - poses[k][:2]))):.3f} m "
          f"from the particle's own; lost: {sensor.lost(b, weights=w)}")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 25)
