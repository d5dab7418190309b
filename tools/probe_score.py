"""score_maps on the bench scene ("Measured").

  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_score.py [P] [steps]
  python tools/probe_score.py --report OUT/.../kt_kernel_trace.csv

The run builds the bench scene (bench.Runner, P particles, `steps` steps), renders the best particle's map over map_extent(None)
as the reference and then calls, REPS + 1 times each (the first is a warm-up), score_maps with tol 1:  (a) of particle 0;  (b) of
every particle.  It prints the wall time of the calls, the bytes a call of (b) reads (the blocks that are not left early, counted
from the extents of SAMPLE particles) and the yardstick: the host path these calls replace, render_map(p) and a vectorised NumPy
confusion count, timed on SAMPLE particles and scaled to P.  --report sums the trace's dispatches of the two kernels per call
and prints min / median / max per case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, SAMPLE, BEAMS, TOL = 5, 64, 1081, 1
KERNELS = ("score_ref_kernel", "score_maps_kernel")


def report(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []                                            # one per reference kernel
    for r in rows:
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        if name == "score_ref_kernel":
            calls.append({k: 0.0 for k in KERNELS})
        calls[-1][name] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    assert len(calls) == 2 * (REPS + 1), len(calls)
    for what, cs in (("(a) one particle", calls[1:REPS + 1]), ("(b) every particle", calls[REPS + 2:])):
        for k in KERNELS:
            v = [c[k] for c in cs]
            print(f"{what:20s} {k:18s} min {min(v):9.4f}  median {float(np.median(v)):9.4f}  max {max(v):9.4f} ms per call")


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


def host_confusion(cells, ref, thr):
    """The nine class pairs and the l1 of one rendered map against the reference, vectorised NumPy."""
    cv = np.where(cells < 0, 0, np.where(cells > thr, 2, 1))
    cr = np.where(ref < 0, 0, np.where(ref > thr, 2, 1))
    n = np.bincount((3 * cv + cr).ravel(), minlength=9)
    return n, int(np.abs(cells.astype(np.int16) - ref).sum())


def main(P, steps):
    r = scene(P, steps)
    e = r.e
    box = e.map_extent(None)
    nx, ny = box[1] - box[0], box[3] - box[2]
    ref = e.render_map("best", box=box).cells
    sa, wa = timed(lambda: e.score_maps(ref, particle=0, box=box, tol_cells=TOL))
    sb, wb = timed(lambda: e.score_maps(ref, box=box, tol_cells=TOL))
    nbx, nby = (nx + 63) // 64, (ny + 63) // 64
    sample = np.linspace(0, P - 1, min(SAMPLE, P)).astype(int)
    full = []                                             # blocks of a particle whose window meets its extent: not left early
    for p in sample:
        x = e.map_extent(int(p)) or (0, 0, 0, 0)
        bi = [i for i in range(nbx) if box[0] + 64 * i - TOL < x[1] and box[0] + 64 * i + 64 + TOL > x[0]]
        bj = [j for j in range(nby) if box[2] + 64 * j - TOL < x[3] and box[2] + 64 * j + 64 + TOL > x[2]]
        full.append(len(bi) * len(bj))
    per_block = 4096 + (64 + 2 * TOL) * 16                # int8 cells, occupancy words of the window
    map_bytes = float(np.mean(full)) * P * per_block
    print(f"P {P}, {steps} steps, tol {TOL}; box {box} = {nx} x {ny} cells, {nbx * nby} blocks")
    print(f"(a) wall min {min(wa):.3f} median {float(np.median(wa)):.3f} max {max(wa):.3f} ms;  f1 {float(sa.f1()):.4f}")
    print(f"(b) wall min {min(wb):.3f} median {float(np.median(wb)):.3f} max {max(wb):.3f} ms;  {float(np.mean(full)):.1f} of {nbx * nby} blocks per "
          f"particle take the full path (from {len(sample)} extents): {map_bytes / 1e6:.1f} MB of tile rows and occupancy words, and "
          f"{float(np.mean(full)) * P * 4096 / 1e6:.1f} MB of reference cells (cache hits past the first particle; the raster is {nx * ny / 1e6:.2f} MB)")
    thr = int(round(float(e.cfg.occupied_threshold) / float(e.cfg.quantum)))
    t0 = time.perf_counter()
    same = True
    for p in sample:
        n, l1 = host_confusion(e.render_map(int(p), box=box).cells, ref, thr)
        same = same and np.array_equal(n, sb.n[p].ravel()) and l1 == int(sb.l1[p])
    dt = (time.perf_counter() - t0) * 1e3
    print(f"host path (render_map(p) + NumPy confusion and l1, no hits): {dt:.1f} ms for {len(sample)} particles = {dt / len(sample):.3f} ms each, "
          f"{dt / len(sample) * P:.0f} ms scaled to {P}; equal to score_maps: {same}")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 25)
