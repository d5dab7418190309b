"""frontier_regions on the bench scene ("Measured").

  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_frontier.py [P] [steps]
  python tools/probe_frontier.py --report OUT/.../kt_kernel_trace.csv

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and then calls, REPS + 1 times each (the first is a
warm-up):  (a) frontier_regions of particle 0 over its whole extent, labels and table to the host;  (b) frontier_regions of every
particle, MAX_REGIONS rows each.  It prints the wall time of the calls, their rounds and block runs (frontier_stats), |F| and the
region counts, and the wall time of the host path the call replaces on particle 0: render_map + explore.frontier_cells + the
labelling of tests/frontier_oracle.py, and whether the labels agree.  --report sums the trace's dispatches of the kernels per
call and prints min / median / max per case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, MAX_REGIONS, BEAMS = 5, 64, 1081
KERNELS = ("frontier_mask_kernel", "frontier_label_kernel", "frontier_reduce_kernel", "frontier_select_kernel", "frontier_moment_kernel",
           "frontier_rep_kernel", "frontier_finish_kernel", "frontier_label_out_kernel")


def report(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seg = []                                              # one segment per mask kernel: a batch of particles
    for r in rows:
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        if name == "frontier_mask_kernel":
            seg.append({k: 0.0 for k in KERNELS} | {"rounds": 0})
        seg[-1][name] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        seg[-1]["rounds"] += name == "frontier_label_kernel"
    a = [c for c in seg if c["frontier_label_out_kernel"] > 0.0]
    b = [c for c in seg if c["frontier_label_out_kernel"] == 0.0]
    assert len(a) == REPS + 1 and len(b) % (REPS + 1) == 0, (len(a), len(b))
    nb = len(b) // (REPS + 1)                             # batches per call of (b)
    calls_b = [{k: sum(c[k] for c in b[nb * q:nb * (q + 1)]) for k in b[0]} for q in range(REPS + 1)]
    for what, calls in (("(a)", a[1:]), (f"(b) {nb} batch(es)", calls_b[1:])):
        for k in KERNELS:
            v = [c[k] for c in calls]
            print(f"{what:16s} {k:26s} min {min(v):9.3f}  median {float(np.median(v)):9.3f}  max {max(v):9.3f} ms per call"
                  + (f"  ({calls[0]['rounds']} dispatches)" if k == "frontier_label_kernel" else ""))


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


def main(P, steps):
    from tests import frontier_oracle as F
    from thesis_amd import explore
    e = scene(P, steps).e
    fa, wa = timed(lambda: e.frontier_regions(0, clearance_cells=0, max_regions=MAX_REGIONS))
    sa = e.frontier_stats()
    fb, wb = timed(lambda: e.frontier_regions(None, clearance_cells=0, max_regions=MAX_REGIONS, labels=False))
    sb = e.frontier_stats()
    nx, ny = fa.label.shape
    print(f"P {P}, {steps} steps, clearance 0, {MAX_REGIONS} rows")
    print(f"(a) box {fa.box} = {nx} x {ny} cells, {sa['blocks']} blocks: {sa['rounds']} rounds, {sa['block_runs']} block runs beside "
          f"{sa['blocks'] * sa['rounds']} (blocks x rounds); |F| {fa.counts[0]}, {fa.counts[1]} regions, {fa.counts[2]} kept, largest "
          f"{fa.regions['size'][0]}; wall min {min(wa):.3f} median {float(np.median(wa)):.3f} max {max(wa):.3f} ms")
    print(f"(b) box {fb.box}, {P} particles, {sb['blocks']} (particle, block) pairs: {sb['rounds']} rounds, {sb['block_runs']} block runs "
          f"beside {sb['blocks'] * sb['rounds']}; |F| {fb.counts[:, 0].min()} .. {fb.counts[:, 0].max()}, regions {fb.counts[:, 1].min()} .. "
          f"{fb.counts[:, 1].max()}; wall min {min(wb):.3f} median {float(np.median(wb)):.3f} max {max(wb):.3f} ms, "
          f"{float(np.median(wb)) / P * 1e3:.1f} us per particle")

    def host():
        m = e.render_map(0)
        f = explore.frontier_cells(m)
        mask = np.zeros(np.asarray(m.cells).shape, bool)
        mask[f[:, 0] - m.x0, f[:, 1] - m.y0] = True
        return F.components(mask)[0]
    label, wh = timed(host)
    import platform
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), platform.machine())
    print(f"host: Python {platform.python_version()}, NumPy {np.__version__}, {cpu}")
    print(f"host path on particle 0 (render_map + explore.frontier_cells + the oracle's labelling): wall min {min(wh):.3f} median "
          f"{float(np.median(wh)):.3f} ms; labels equal: {np.array_equal(label, fa.label)}; (b) per particle is "
          f"{float(np.median(wh)) / (float(np.median(wb)) / P):.0f} times faster")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 25)
