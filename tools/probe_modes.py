"""Pose modes against the host path they replace ("Measured").

  python tools/probe_modes.py [step ...]          steps: bench blobs big track (default: all, in this order)

Every step runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the probe.
  bench   the bench scene (bench.Runner, 4096 particles, 1081 beams) after 100 steps
  blobs   4096 particles in 8 seeded Gaussian blobs, set through set_state
  big     65536 particles in 8 blobs on an engine of one small tile per particle
          each: the wall time of pose_modes (host outputs, with labels, and device outputs followed by a synchronise), of
          estimate(), and of the host path: poses() + weights() and a vectorised NumPy clustering (host_modes below); REPS + 1
          calls each, the first a warm-up; and whether the two label vectors agree
  track   the bench scene with 2000 records: trajectory_modes against lineage() read back and host_modes per record"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS = 5, 1081
LIMITS = {"bench": 240, "blobs": 120, "big": 240, "track": 420}      # seconds
BIN_XY, N_TH = 0.5, 36


def timed(f):
    t = []
    for _ in range(REPS + 1):
        t0 = time.perf_counter()
        out = f()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, t[1:]


def mmm(v):
    return f"min {min(v):.3f} median {float(np.median(v)):.3f} max {max(v):.3f}"


def host_modes(poses, w, bin_xy=BIN_XY, n_th=N_TH):
    """int32 [P]: the label of DESIGN.md 3.21 (the smallest contributing index of the particle's mode, -1 outside), vectorised:
    bins packed into int64 keys, np.unique, then minimum labels passed along the 13 forward neighbour offsets until none changes."""
    inv, kth = 1.0 / bin_xy, n_th / 6.283185307179586
    f = poses * np.array([inv, inv, kth])
    ok = np.isfinite(w) & (w > 0) & np.isfinite(poses).all(axis=1) & (np.abs(f[:, 0]) < 2.0 ** 23) & (np.abs(f[:, 1]) < 2.0 ** 23) & (np.abs(f[:, 2]) < 2.0 ** 40)
    idx = np.nonzero(ok)[0]
    label = np.full(len(poses), -1, dtype=np.int32)
    if not len(idx):
        return label
    b = np.floor(f[idx]).astype(np.int64)
    b[:, 2] %= n_th
    pack = lambda x, y, t: ((x + (1 << 23)) << 36) | ((y + (1 << 23)) << 12) | t
    keys, inverse = np.unique(pack(b[:, 0], b[:, 1], b[:, 2]), return_inverse=True)
    root = np.full(len(keys), len(poses), dtype=np.int64)
    np.minimum.at(root, inverse, idx)
    x, y, t = (keys >> 36) - (1 << 23), ((keys >> 12) & 0xffffff) - (1 << 23), keys & 0xfff
    pairs = []
    for n in range(14, 27):
        dx, dy, dt = n // 9 - 1, (n // 3) % 3 - 1, n % 3 - 1
        nk = pack(x + dx, y + dy, (t + dt) % n_th)
        at = np.minimum(np.searchsorted(keys, nk), len(keys) - 1)
        hit = np.nonzero(keys[at] == nk)[0]
        pairs.append(np.stack([hit, at[hit]]))
    a, c = np.concatenate(pairs, axis=1)
    while True:
        m = np.minimum(root[a], root[c])
        new = root.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, c, m)
        if np.array_equal(new, root):
            break
        root = new
    label[idx] = root[inverse]
    return label


def blob_cloud(P, seed=7):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-20.0, 20.0, size=(8, 3))
    centres[:, 2] = rng.uniform(-3.0, 3.0, size=8)
    return centres[rng.integers(0, 8, size=P)] + rng.normal(scale=[0.2, 0.2, 0.05], size=(P, 3)), rng.uniform(0.5, 1.5, size=P)


def report(e, what):
    import torch  # noqa: F401  (device outputs)
    m, t = timed(lambda: e.pose_modes(labels=True))
    print(f"{what}: P {e.P}, {m.count} modes in {m.bins} bins, {m.used} particles used, shares {np.round(m.share[:4], 4).tolist()}")
    print(f"  pose_modes, host outputs, labels   {mmm(t)} ms")
    _, t = timed(lambda: e.pose_modes())
    print(f"  pose_modes, host outputs           {mmm(t)} ms")
    _, t = timed(lambda: (e.pose_modes(labels=True, device=True), e.synchronize()))
    print(f"  pose_modes, device outputs + sync  {mmm(t)} ms")
    _, t = timed(lambda: e.estimate())
    print(f"  estimate                           {mmm(t)} ms")
    from thesis_amd.mapio import resample_weights
    (poses, w), tr = timed(lambda: (e.poses(), resample_weights(e.weights())))
    lab, tc = timed(lambda: host_modes(poses, w))
    print(f"  host path: poses() + weights()     {mmm(tr)} ms")
    print(f"             NumPy clustering        {mmm(tc)} ms; labels equal the device's: {bool(np.array_equal(lab, m.labels))}")


def state_only_engine(P):
    from thesis_amd.engine import ParticleEngine
    return ParticleEngine(P, cell_size=0.1, pool_tiles=P + 8, max_beams=16)


def step_bench():
    import bench
    from thesis_amd.datasets import synthetic
    r = bench.Runner(4096, BEAMS, 0.05, synthetic.make_log(104, BEAMS, period=bench.PERIOD_S))
    for _ in range(100):
        r.step()
    r.e.synchronize()
    report(r.e, "bench scene after 100 steps")
    r.e.close()


def step_blobs(P=4096):
    e = state_only_engine(P)
    poses, w = blob_cloud(P)
    e.set_state(poses=poses, weights=w)
    report(e, "8 blobs")
    e.close()


def step_track(records=2000):
    import bench
    from thesis_amd.datasets import synthetic
    from thesis_amd.mapio import resample_weights
    r = bench.Runner(4096, BEAMS, 0.05, synthetic.make_log(records // 2 + 4, BEAMS, period=bench.PERIOD_S))
    e = r.e
    e.track(records, imu=True, scan=True)
    for _ in range(records // 2 - 1):
        r.step()
    e.record()
    e.synchronize()
    assert e.track_info()["n_records"] == records
    tm, t = timed(lambda: e.trajectory_modes())
    print(f"trajectory_modes over {records} records, P {e.P}: {mmm(t)} ms; modes at records 0, 1/4, 1/2, 3/4, last: "
          f"{[int(tm.count[k]) for k in (0, records // 4, records // 2, 3 * records // 4, records - 1)]}")
    w = resample_weights(e.weights())

    def host():
        pose = e.lineage()[1]
        labels = (host_modes(pose[k], w) for k in range(0, records, 20))
        return np.array([len(np.unique(lab[lab >= 0])) for lab in labels])
    t0 = time.perf_counter()
    counts = host()
    dt = (time.perf_counter() - t0) * 1e3
    print(f"host path: lineage() read back + NumPy clustering of every 20th record {dt:.1f} ms, i.e. {dt * 20:.0f} ms for all (scaled); "
          f"counts equal the device's: {bool(np.array_equal(counts, tm.count[::20]))}")
    e.close()


STEPS = {"bench": step_bench, "blobs": step_blobs, "big": lambda: step_blobs(65536), "track": step_track}

if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        STEPS[sys.argv[2]]()
        sys.exit(0)
    for name in sys.argv[1:] or list(STEPS):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], timeout=LIMITS[name]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {name} ended with {rc}: stopping")
            sys.exit(rc)
