"""describe_scans, match_places and loops.candidates_by_appearance timed ("Measured").

  python tools/probe_places.py [--no-oracle]
  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_places.py --no-oracle

The bench scene (synthetic.make_log at bench.PERIOD_S, 1081 beams), 2000 scans: the circle is walked 37 times.  10 000 scans are
the same log five times over.  24 rings, k = 4, triangular limits (query q admits the references r < q - 55: min_gap 50 and
runs of 11).  Wall time round a synchronise, REPS calls after a warm-up:
  describe   describe_scans of all scans in one call, host ranges in (8 bytes a beam cross the bus), device outputs
  search     match_places of the device table against itself, device outputs: the field, search and merge kernels
  whole      loops.candidates_by_appearance: describe, search with host tables and outputs, and the host's bookkeeping
  oracle     tests/places_oracle.py on ORACLE_Q queries spread over the log against every reference any of them admits, scaled
             to all the queries by the number of (query, reference) pairs; its result is compared with the GPU's on those queries"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS, SCANS, ORACLE_Q = 5, 1081, 2000, 100


def timed(fn, sync, reps=REPS):
    fn()
    sync()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def show(name, ms, scale=1.0):
    ms = [m * scale for m in ms]
    print(f"  {name:10s} min {min(ms):10.3f}  median {float(np.median(ms)):10.3f}  max {max(ms):10.3f} ms", flush=True)
    return float(np.median(ms))


def main():
    import bench
    from thesis_amd import loops
    from thesis_amd.datasets import synthetic
    from thesis_amd.engine import ParticleEngine
    ang, ranges, _, truth = synthetic.make_log(SCANS - 1, BEAMS, period=bench.PERIOD_S)
    truth, ranges = np.ascontiguousarray(truth[:SCANS]), np.ascontiguousarray(ranges[:SCANS])
    e = ParticleEngine(1, max_beams=BEAMS, pool_tiles=16)
    for times in (1, 5):
        rg, ps = np.tile(ranges, (times, 1)), np.tile(truth, (times, 1))
        n = len(rg)
        limit = np.maximum(np.arange(n) - 55, 0).astype(np.int32)
        pairs_n = int(limit.sum())
        host = e.describe_scans(rg, ang)
        found = e.match_places(host, ref_limit=limit, k=4)
        sim = found.similarity()[:, 0]
        print(f"{n} scans of {BEAMS} beams, 24 rings, k 4, {pairs_n} (query, reference) pairs, {REPS} timed calls each; median bits a scan "
              f"{int(np.median(host.n_bits))}, median best similarity {float(np.median(sim[limit > 0])):.3f}")
        show("describe", timed(lambda: e.describe_scans(rg, ang, device=True), e.synchronize))
        dev = e.describe_scans(rg, ang, device=True)
        t_search = show("search", timed(lambda: e.match_places(dev, ref_limit=limit, k=4, device=True), e.synchronize))
        print(f"  {pairs_n / t_search / 1e6:.2f} G pairs/s, {64 * pairs_n / t_search / 1e6:.1f} G turns/s")
        show("whole", timed(lambda: loops.candidates_by_appearance(e, ps, rg, ang, min_gap=50, half_run=5), e.synchronize, reps=3))
        if "--no-oracle" in sys.argv:
            continue
        from tests.places_oracle import match_places as oracle
        some = np.flatnonzero(limit > 0)
        qs = some[np.linspace(0, len(some) - 1, ORACLE_Q).astype(int)]
        refs = int(limit[qs].max())
        t = time.perf_counter()
        out4, out2 = oracle(host.desc[qs], host.desc[:refs], limit[qs], 4)
        ms = (time.perf_counter() - t) * 1e3
        same = np.array_equal(out4[..., 0], found.ref[qs]) and np.array_equal(out4[..., 1], found.shift[qs]) and np.array_equal(out4[..., 2], found.score[qs])
        t_or = show("oracle", [ms], scale=pairs_n / (len(qs) * refs))
        print(f"  oracle / search = {t_or / t_search:.0f} ({len(qs)} queries x {refs} references took {ms:.0f} ms); the same result: {same}")
    e.close()


if __name__ == "__main__":
    main()
