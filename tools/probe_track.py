"""The trajectory log on the bench scene ("Measured").

  python tools/probe_track.py [P] [records]

Builds the bench scene (bench.Runner, P particles, 1081 beams) and prints
  1. the step time (host clock over BLOCK steps ending in a synchronise) with tracking off, with scan=True and with imu=True,
     scan=True: ROUNDS rounds, the three settings alternating inside each, so that all of them meet the same stretch of the run;
     min / median / max over the rounds is the scatter a difference has to beat.  (The tracking-off time against the parent
     commit's is bench.py's business: run both builds' bench.py alternately.)
  2. with `records` records in the log (imu=True, scan=True over records / 2 steps): the wall time of lineage (all P, indices
     only and with poses, host and device outputs), trajectory("best"), trajectory_summary and estimate, REPS + 1 calls each
     (the first is a warm-up);
  3. the host path these replace, i.e. what ParticleFilter(history="host") costs: poses() after each of the two updates of a
     step and the ancestors of a resample read back, and a vectorised NumPy walk over the read-back tables;
     and whether that walk and the device's lineage agree."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS, WARM, BLOCK, ROUNDS = 5, 1081, 20, 20, 7
SETTINGS = (("off", None), ("scan", dict(imu=False, scan=True)), ("imu+scan", dict(imu=True, scan=True)))


def timed(f):
    t = []
    for _ in range(REPS + 1):
        t0 = time.perf_counter()
        out = f()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, t[1:]


def mmm(v):
    return f"min {min(v):.3f} median {float(np.median(v)):.3f} max {max(v):.3f}"


def main(P, records):
    import bench
    from thesis_amd.datasets import synthetic
    steps_read = records // 2
    n_steps = WARM + len(SETTINGS) * ROUNDS * BLOCK + steps_read
    r = bench.Runner(P, BEAMS, 0.05, synthetic.make_log(n_steps + 2, BEAMS, period=bench.PERIOD_S))
    e = r.e
    for _ in range(WARM):
        r.step()
    e.synchronize()
    per = {name: [] for name, _ in SETTINGS}
    for _ in range(ROUNDS):
        for name, kw in SETTINGS:
            if kw is not None:
                e.track(2 * BLOCK + 1, **kw)
            e.synchronize()
            t0 = time.perf_counter()
            for _ in range(BLOCK):
                r.step()
            e.synchronize()
            per[name].append((time.perf_counter() - t0) * 1e3 / BLOCK)
            if kw is not None:
                assert e.track_info()["dropped"] == 0
                e.untrack()
    print(f"P {P}, {BEAMS} beams; step time in ms over blocks of {BLOCK} steps, {ROUNDS} rounds, settings alternating")
    for name, _ in SETTINGS:
        print(f"  tracking {name:9s} {mmm(per[name])}")

    e.track(records, imu=True, scan=True)
    for _ in range(steps_read - 1):
        r.step()
    e.record()
    e.synchronize()
    info = e.track_info()
    assert info["n_records"] == records and info["dropped"] == 0, info
    nb = int(e._lib.rbpf_track_record_bytes(e._h))
    print(f"{records} records of {nb} bytes ({records * nb / 1e6:.1f} MB)")
    (idx, _), t = timed(lambda: e.lineage(poses=False))
    print(f"  lineage, all P, indices        {mmm(t)} ms")
    (_, pose), t = timed(lambda: e.lineage())
    print(f"  lineage, all P, with poses     {mmm(t)} ms")
    _, t = timed(lambda: (e.lineage(device=True), e.synchronize()))
    print(f"  the same, device outputs       {mmm(t)} ms")
    _, t = timed(lambda: e.trajectory("best"))
    print(f"  trajectory('best')             {mmm(t)} ms")
    s, t = timed(lambda: e.trajectory_summary())
    print(f"  trajectory_summary             {mmm(t)} ms")
    _, t = timed(lambda: e.estimate())
    print(f"  estimate                       {mmm(t)} ms")
    alive = s.n_alive
    print(f"  distinct ancestors at records 0, 1/4, 1/2, 3/4, last: {[int(alive[k]) for k in (0, records // 4, records // 2, 3 * records // 4, records - 1)]}")

    # the host path: what history="host" reads back per step, and its walk
    _, tp = timed(lambda: e.poses())
    _, tr = timed(lambda: e.resample(0.5))
    print(f"host path per step: 2 x poses() {2 * float(np.median(tp)):.3f} ms + the ancestors read back with the resample "
          f"{float(np.median(tr)):.3f} ms (resample_async returns without waiting)")
    blob = np.empty(records * nb + 4 * P, dtype=np.uint8)
    e._check(e._lib.rbpf_track_export(e._h, 0, records, blob.ctypes.data))
    rec = blob[:records * nb].reshape(records, nb)
    xyz = np.ascontiguousarray(rec[:, :24 * P]).view(np.float64).reshape(records, 3, P)
    parent = np.ascontiguousarray(rec[:, 24 * P + 128:28 * P + 128]).view(np.int32).reshape(records, P)
    pending = blob[records * nb:].view(np.int32)

    def walk():
        out_i, out_p = np.empty((records, P), dtype=np.int32), np.empty((records, P, 3))
        cur = pending.copy()
        for t in range(records - 1, -1, -1):
            out_i[t] = cur
            out_p[t] = xyz[t][:, cur].T
            cur = parent[t][cur]
        return out_i, out_p
    (hi, hp), t = timed(walk)
    lin = e.lineage()
    print(f"host walk over the read-back tables (vectorised NumPy, all P, with poses) {mmm(t)} ms; equal to the device's lineage: "
          f"{bool(np.array_equal(hi, lin[0]) and np.array_equal(hp.view(np.uint64), lin[1].view(np.uint64)))}")
    e.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 2000)
