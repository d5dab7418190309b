"""travel_cost on the bench scene ("Measured").

  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_travel.py [P] [steps]
  python tools/probe_travel.py --report OUT/.../kt_kernel_trace.csv
  python tools/probe_travel.py --reads [P] [steps]          (no profiler: wall time against the rounds queued per host read)

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and then calls, REPS + 1 times each (the first is a
warm-up):  (a) travel_cost of particle 0 over its whole extent from its own pose, robot radius RADIUS;  (b) travel_cost of
GOALS goals in every particle's map, each particle's own pose as its start.  It prints the wall time of the calls, their rounds
and block runs (travel_stats) and, for (a), the wall time of tests/travel_oracle.py on the same raster and whether the two
agree.  --report sums the trace's dispatches of the three kernels per call and prints min / median / max per case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, GOALS, BEAMS, RADIUS = 5, 64, 1081, 0.2
KERNELS = ("travel_mask_kernel", "travel_relax_kernel", "travel_cost_kernel", "travel_goal_kernel")


def report(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seg = []                                              # one segment per mask kernel: a batch of particles
    for r in rows:
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        if name == "travel_mask_kernel":
            seg.append({k: 0.0 for k in KERNELS} | {"rounds": 0})
        seg[-1][name] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        seg[-1]["rounds"] += name == "travel_relax_kernel"
    a = [c for c in seg if c["travel_cost_kernel"] > 0.0]
    b = [c for c in seg if c["travel_cost_kernel"] == 0.0]
    assert len(a) == REPS + 1 and len(b) % (REPS + 1) == 0, (len(a), len(b))
    nb = len(b) // (REPS + 1)                             # batches per call of (b)
    calls_b = [{k: sum(c[k] for c in b[nb * q:nb * (q + 1)]) for k in b[0]} for q in range(REPS + 1)]
    for what, calls in (("(a)", a[1:]), (f"(b) {nb} batch(es)", calls_b[1:])):
        for k in ("travel_mask_kernel", "travel_relax_kernel", "travel_cost_kernel", "travel_goal_kernel"):
            v = [c[k] for c in calls]
            print(f"{what:16s} {k:20s} min {min(v):9.3f}  median {float(np.median(v)):9.3f}  max {max(v):9.3f} ms per call"
                  + (f"  ({calls[0]['rounds']} dispatches)" if k == "travel_relax_kernel" else ""))


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


def main(P, steps, reads):
    r = scene(P, steps)
    e = r.e
    poses = e.poses()
    rng = np.random.Generator(np.random.PCG64(9))
    goals = r.true_poses[steps][:2] + rng.normal(0, 2.5, size=(GOALS, 2))
    case_a = lambda: e.travel_cost(poses[0, :2], particle=0, radius_m=RADIUS)
    case_b = lambda: e.travel_cost(poses[:, :2], goals, particle=None, radius_m=RADIUS)
    if reads:
        for q in (1, 2, 4, 8, 16, 32):
            os.environ["RBPF_TRAVEL_ROUNDS_PER_READ"] = str(q)
            (ta, wa), (tb, wb) = timed(case_a), timed(case_b)
            print(f"rounds per read {q:2d}: (a) {ta.rounds:4d} rounds, wall min {min(wa):8.3f} median {float(np.median(wa)):8.3f} ms;  "
                  f"(b) {tb.rounds:5d} rounds, wall min {min(wb):9.3f} median {float(np.median(wb)):9.3f} ms", flush=True)
        e.close()
        return
    ta, wa = timed(case_a)
    sa = e.travel_stats()
    tb, wb = timed(case_b)
    sb = e.travel_stats()
    nx, ny = ta.cost.shape
    print(f"P {P}, {steps} steps, radius {RADIUS} m (inflate {ta.inflate})")
    print(f"(a) box {ta.box} = {nx} x {ny} cells, {sa['blocks']} blocks: {sa['rounds']} rounds, {sa['block_runs']} block runs beside "
          f"{sa['blocks'] * sa['rounds']} (blocks x rounds); {(ta.cost >= 0).sum()} cells reached, largest cost {ta.cost.max()}; "
          f"wall min {min(wa):.3f} median {float(np.median(wa)):.3f} max {max(wa):.3f} ms")
    print(f"(b) box {tb.box}, {GOALS} goals x {P} particles, {sb['blocks']} (particle, block) pairs: {sb['rounds']} rounds, {sb['block_runs']} "
          f"block runs beside {sb['blocks'] * sb['rounds']}; reached share {(tb.goal_cost >= 0).mean():.3f}; "
          f"wall min {min(wb):.3f} median {float(np.median(wb)):.3f} max {max(wb):.3f} ms")
    from tests import travel_oracle as T
    grown = e.render_map(0, box=T.grown_box(ta.box, ta.clear_max)).cells
    t0 = time.perf_counter()
    want = T.travel(grown, ta.box, ta.inv, float(e.cfg.quantum), float(e.cfg.occupied_threshold), [poses[0, :2]], None, ta.inflate, ta.clear_max)
    print(f"(a) tests/travel_oracle.py on the same raster: {(time.perf_counter() - t0) * 1e3:.0f} ms; equal: "
          f"{np.array_equal(want[0], ta.cost) and np.array_equal(want[1], ta.clearance)}")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        args = [a for a in sys.argv[1:] if a != "--reads"]
        main(int(args[0]) if args else 4096, int(args[1]) if len(args) > 1 else 25, "--reads" in sys.argv)
