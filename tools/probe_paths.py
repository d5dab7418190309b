"""check_paths on the bench scene ("Measured").

  python tools/probe_paths.py [P] [steps]                    (wall times)
  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_paths.py [P] [steps]
  python tools/probe_paths.py --report OUT/.../kt_kernel_trace.csv

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and then calls, REPS + 1 times each (the first is a
warm-up):  (a) check_paths of ROLLOUTS_A rollouts of 61 waypoints from particle 0's pose in particle 0's map, robot radius
RADIUS;  (b) check_paths(particle=None, own=True) of ROLLOUTS_B rollouts of 13 waypoints from every particle's own pose;
(c) plan.shortcut_in of one plan.path_to path across the room.  Each is set against the host path it replaces: travel_cost's
clearance raster read back and sampled along plan.path_cells in NumPy - for (b) over HOST_B particles, scaled to P - and the
results are compared.  --report prints min / median / max of the trace's check_paths_kernel dispatches per case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS, RADIUS, ROLLOUTS_A, ROLLOUTS_B, HOST_B = 5, 1081, 0.2, 1024, 256, 64


def report(path):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "check_paths_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    print(f"{len(ms)} dispatches of check_paths_kernel")
    for what, sel in (("(a)", slice(0, REPS + 1)), ("(b)", slice(REPS + 1, 2 * (REPS + 1)))):
        v = ms[sel][1:]
        print(f"{what}: min {min(v):.4f}  median {float(np.median(v)):.4f}  max {max(v):.4f} ms per dispatch")
    v = ms[2 * (REPS + 1):]
    if v:
        print(f"(c) {len(v)} dispatches: sum {sum(v):.4f} ms, {sum(v) / (REPS + 1):.4f} ms per shortcut_in")


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


def host_check(e, paths, particle, start, radius_m):
    """first_blocked of every path by the host path: the clearance and cost rasters of travel_cost read back, sampled along
    plan.path_cells.  A cell carries the robot if it is in T: known free with clearance > inflate (the cost raster of a
    travel_cost from that very cell would say so; here the int8 map is read back for it)."""
    from thesis_amd import plan
    tr = e.travel_cost(start, particle=particle, radius_m=radius_m)
    v = e.render_map(particle, box=tr.box).cells
    ok = (v < 0) & (tr.clearance > tr.inflate)
    x0, x1, y0, y1 = tr.box
    out = np.full(len(paths), -1, np.int32)
    for k, p in enumerate(paths):
        c = plan.path_cells(p, tr.inv)
        inside = (c[:, 0] >= x0) & (c[:, 0] < x1) & (c[:, 1] >= y0) & (c[:, 1] < y1)
        good = np.zeros(len(c), bool)
        good[inside] = ok[c[inside, 0] - x0, c[inside, 1] - y0]
        d = np.diff(c, axis=0)
        diag = np.flatnonzero((d[:, 0] != 0) & (d[:, 1] != 0)) + 1          # no corner is cut
        side = lambda a: np.where((a[:, 0] >= x0) & (a[:, 0] < x1) & (a[:, 1] >= y0) & (a[:, 1] < y1),
                                  ok[np.clip(a[:, 0] - x0, 0, x1 - x0 - 1), np.clip(a[:, 1] - y0, 0, y1 - y0 - 1)], False)
        good[diag] &= side(np.stack([c[diag, 0], c[diag - 1, 1]], 1)) & side(np.stack([c[diag - 1, 0], c[diag, 1]], 1))
        bad = np.flatnonzero(~good)
        if len(bad):
            out[k] = bad[0]
    return out


def main(P, steps):
    from thesis_amd import plan
    r = scene(P, steps)
    e = r.e
    poses = e.poses()
    v, w = np.meshgrid(np.linspace(0.1, 1.0, 32), np.linspace(-1.0, 1.0, 32))
    arcs_a = plan.rollouts(poses[0], v.ravel(), w.ravel(), 6.0, 0.1)        # [1024, 61, 2]
    v, w = np.meshgrid(np.linspace(0.1, 1.0, 16), np.linspace(-1.0, 1.0, 16))
    arcs_b = plan.rollouts(poses, v.ravel(), w.ravel(), 6.0, 0.5)           # [P, 256, 13, 2]
    print(f"P {P}, {steps} steps, radius {RADIUS} m")
    a, wa = timed(lambda: e.check_paths(arcs_a, particle=0, radius_m=RADIUS))
    ha, wha = timed(lambda: host_check(e, arcs_a, 0, poses[0, :2], RADIUS))
    print(f"(a) {ROLLOUTS_A} rollouts, {int(a.steps.sum())} steps ({a.steps.min()} .. {a.steps.max()}), clear share {a.clear.mean():.3f}: {spread(wa)}")
    print(f"(a) host path (travel_cost clearance + render_map read back, NumPy walk): {spread(wha)}; equal first_blocked: {np.array_equal(ha, a.first_blocked)}")
    b, wb = timed(lambda: e.check_paths(arcs_b, particle=None, radius_m=RADIUS, own=True))
    print(f"(b) {P} x {ROLLOUTS_B} rollouts, {int(b.steps.sum())} steps, clear share {b.clear.mean():.3f}: {spread(wb)}")
    n = min(HOST_B, P)
    t0 = time.perf_counter()
    hb = np.stack([host_check(e, arcs_b[p], p, poses[p, :2], RADIUS) for p in range(n)])
    tb = (time.perf_counter() - t0) * 1e3
    print(f"(b) host path over {n} particles, one pass: {tb:.0f} ms, scaled to {P}: {tb * P / n:.0f} ms (extrapolated); equal first_blocked: "
          f"{np.array_equal(hb, b.first_blocked[:n])}")
    k = int(np.argmax(e.weights()))
    start = poses[k, :2]
    tr = e.travel_cost(start, particle=k, radius_m=RADIUS)
    far = np.argwhere(tr.cost == tr.cost.max())[0]
    goal = (far + [tr.box[0] + 0.5, tr.box[2] + 0.5]) * tr.cell
    path = plan.path_to(tr, goal)
    short, wc = timed(lambda: plan.shortcut_in(e, path, particle=k, radius_m=RADIUS))
    length = lambda q: float(np.hypot(*np.diff(q, axis=0).T).sum())
    print(f"(c) path of {len(path)} cells, {length(path):.2f} m -> {len(short)} waypoints, {length(short):.2f} m: {spread(wc)}")

    def host_clear(legs):
        return host_check(e, legs, k, start, RADIUS) < 0
    hshort, whc = timed(lambda: plan.shortcut(path, host_clear))
    print(f"(c) host path: {spread(whc)}; equal chain: {np.array_equal(hshort, short)}")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 25)
