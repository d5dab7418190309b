"""local_map on the bench scene beside the host path it replaces ("Measured").

  python tools/probe_local.py [P] [steps] [--no-host]         (wall times)
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/probe_local.py [P] [steps] --no-host
  python tools/probe_local.py --report OUT/.../kt_kernel_trace.csv [P]

The run builds the bench scene (bench.Runner, P particles, `steps` steps) and takes four cases, all with 2 x 2 samples a cell and
the weights the resample draws from:  (own 128) a 6.4 m window at 0.05 m from every particle's own pose in its own map;  (one
map 128) the same poses in the best particle's map;  (own 64) and (own 256) windows of 3.2 m and 12.8 m.  Each case calls
local_map REPS + 1 times (the first is a warm-up) with NumPy outputs and again with device=True, and prints the wall time round
each call as minimum / median / maximum.  The host path: render_map(particle=p, box=the window's square) read back and the
vectorised NumPy resampling of tests/local_oracle.py, one particle at a time over HOST_ROWS particles, its crops asserted equal
to the device's, its time scaled to all P and labelled so.  --report prints the trace's dispatches per kernel and case."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, SAMPLES, HOST_ROWS = 7, 2, 64
CASES = (("(own 128)", 6.4, True), ("(one map 128)", 6.4, False), ("(own 64)", 3.2, True), ("(own 256)", 12.8, True))
KERNELS = ("local_crop_kernel", "local_fuse_kernel", "local_reduce_kernel")


def batches(P, n):
    """Launches of each kernel in one call: the batch rule of thesis_amd/csrc/rbpf_localbatch.h (crops in scratch, 256 MiB)."""
    pad = lambda b, q: (b + q - 1) // q * q
    cells = pad(n * n, 16)
    size = lambda k: pad(k * cells, 256) + pad((k + 63) // 64 * cells * 20, 256)
    k = P
    while k > 1 and size(k) > 256 << 20:
        k = (k // 2 + 63) // 64 * 64 if k > 64 else k // 2
    return (P + k - 1) // k


def report(path, P):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for kernel in KERNELS:
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if kernel in r["Kernel_Name"]]
        print(f"{len(ms)} dispatches of {kernel}")
        at = 0
        for what, size_m, own in CASES:
            nb = batches(P, int(np.ceil(size_m / 0.05 - 1e-9)))
            calls = [sum(ms[at + c * nb:at + (c + 1) * nb]) for c in range(2 * (REPS + 1))]     # NumPy outputs, then device outputs
            at += 2 * (REPS + 1) * nb
            v = [x for k, x in enumerate(calls) if k % (REPS + 1)]       # without the two warm-ups
            print(f"  {what}: min {min(v):.4f}  median {float(np.median(v)):.4f}  max {max(v):.4f} ms per call, {nb} dispatches a call")


def spread(t):
    return f"min {min(t):.3f} median {float(np.median(t)):.3f} max {max(t):.3f} ms"


def timed(f):
    t = []
    for k in range(REPS + 1):
        t0 = time.perf_counter()
        out = f()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, t[1:]


def host_path(e, poses, rows, n, cell, wq):
    """What a user can do today: one rendered box per particle, read back, resampled in NumPy; returns (crops, ms)."""
    from tests import local_oracle as LO
    inv = e.dim / float(e.cfg.tile_len_m)
    reach = LO.reach(n, cell, (0.0, 0.0), inv)
    t0 = time.perf_counter()
    crops = []
    for p in rows:
        X, Y = int(np.floor(poses[p, 0] * inv)), int(np.floor(poses[p, 1] * inv))
        m = e.render_map(p, box=(X - reach, X + reach + 1, Y - reach, Y + reach + 1))
        crops.append(LO.crop(m.cells, m.x0, m.y0, poses[p], n, SAMPLES, cell, (0.0, 0.0), inv))
    crops = np.stack(crops)
    LO.fuse(crops, wq[rows], float(e.cfg.occupied_threshold) / float(e.cfg.quantum))
    return crops, (time.perf_counter() - t0) * 1e3


def main(P, steps, host):
    from probe_paths import scene                      # beside this file: the bench scene, as that probe builds it
    from thesis_amd.local import quantise_weights
    from thesis_amd.mapio import resample_weights
    e = scene(P, steps).e
    poses, cell = e.poses(), float(e.cfg.cell_size)
    best = int(np.argmax(e.weights()))
    wq = quantise_weights(resample_weights(e.weights()))
    print(f"P {P}, {steps} steps, cell {cell} m, {SAMPLES} x {SAMPLES} samples a cell, weights of the resample ({int((wq > 0).sum())} poses with weight)")
    for what, size_m, own in CASES:
        kw = dict(particle=None if own else best, size_m=size_m, samples=SAMPLES)
        lm, t_np = timed(lambda: e.local_map(poses, **kw))
        dv, t_dev = timed(lambda: e.local_map(poses, device=True, **kw))
        n = lm.occ_w.shape[0]
        assert np.array_equal(dv.sum_wv.cpu().numpy(), lm.sum_wv) and np.array_equal(dv.occ_w.cpu().numpy(), lm.occ_w)
        split = float(((lm.occ_w > 0) & (lm.occ_w < lm.total)).mean())
        print(f"{what} {len(poses)} poses, n {n}: occupied for some of the weight in {split:.3f} of the cells, for all of it in {float((lm.occ_w == lm.total).mean()):.3f}")
        print(f"{what} local_map, NumPy outputs:  {spread(t_np)}")
        print(f"{what} local_map, device outputs: {spread(t_dev)}")
        if host and own:
            rows = np.arange(0, P, max(1, P // HOST_ROWS))[:HOST_ROWS]
            crops, ms = host_path(e, poses, rows, n, cell, wq)
            dev = e.local_map(poses, crops=True, **kw).crops
            assert np.array_equal(crops, dev[rows]), what
            print(f"{what} host path over {len(rows)} of {P} particles: {ms:.0f} ms, crops equal to the device's; extrapolated to all {P}: {ms * P / len(rows):.0f} ms")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--report":
        report(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
    else:
        args = [a for a in sys.argv[1:] if not a.startswith("--")]
        main(int(args[0]) if args else 4096, int(args[1]) if len(args) > 1 else 25, "--no-host" not in sys.argv)
