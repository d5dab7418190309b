"""build_map beside the only path that did the same job before it: one map update per scan ("Measured").

  python tools/probe_build.py [scans] [--no-replay]
  rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- python tools/probe_build.py 2000 --no-replay

The bench scene (synthetic.make_log at bench.PERIOD_S, 1081 beams), `scans` records (default 2000) at their true poses.  Wall
time round a synchronise, REPS calls after a warm-up, for two outputs: the engine's 0.05 m cells to 15 m, and 0.025 m cells to
12.7 m (15 m would be a window of more than 1024 cells there).  Per output:
  build      build_map of all scans in one call, device outputs
  seen only  the same, via the C entry point with hits = NULL: no second bitmap phase
  one row    the same in a box of one row of cells through the middle: every ray is walked and ORed into LDS, next to nothing is
             swept or added - what is left when the atomics are taken away
  replay     a one-particle engine of that cell size: set_scan + map_update(pose) per scan, one launch each
The two draw DIFFERENT maps (per-scan sets of a supercover walk against clamped Bresenham adds); the comparison is of the time to
get a map of the log at all.  Under rocprofv3 the trace holds build_map_kernel's own times, REPS + 1 dispatches per line above in
that order (the first of each a warm-up), after one dispatch that prints the counts."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS = 5, 1081


def timed(fn, sync):
    fn()
    sync()
    out = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def show(name, ms):
    print(f"  {name:10s} min {min(ms):9.3f}  median {float(np.median(ms)):9.3f}  max {max(ms):9.3f} ms", flush=True)
    return float(np.median(ms))


def main():
    import bench
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    from thesis_amd.engine import ParticleEngine
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 2000
    with_replay = "--no-replay" not in sys.argv
    ang, ranges, _, poses = synthetic.make_log(n - 1, BEAMS, period=bench.PERIOD_S)
    poses, ranges = np.ascontiguousarray(poses[:n]), np.ascontiguousarray(ranges[:n])
    print(f"{n} scans of {BEAMS} beams, {REPS} timed calls each")
    for cs, mr in ((0.05, 15.0), (0.025, 12.7)):
        e = ParticleEngine(1, max_beams=BEAMS, cell_size=cs, pool_tiles=16, max_ray_m=mr)
        box = e.build_box(poses, 1.0 / cs if cs != 0.05 else e.dim / float(e.cfg.tile_len_m), mr)
        size = None if cs == 0.05 else cs
        got = e.build_map(poses, ranges, ang, cell_size=size, box=box, max_range=mr, device=True)
        print(f"cell {cs} m, max_range {mr} m, box {got.hits.shape}: {int((got.seen > 0).sum())} cells seen, {int((got.hits > 0).sum())} hit, "
              f"{int(got.seen.sum())} + {int(got.hits.sum())} adds")
        t_build = show("build", timed(lambda: e.build_map(poses, ranges, ang, cell_size=size, box=box, max_range=mr, device=True), e.synchronize))
        b4 = np.array(box, np.int32)
        dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
        seen_only = lambda: e._check(e._lib.rbpf_build_map(e._h, dp(poses), n, dp(ranges), dp(ang), BEAMS, got.cells_per_m, ip(b4), 0.0, mr,
                                                          _lib.RBPF_BUILD_DEVICE_OUT, None, C.c_void_p(got.seen.data_ptr())))
        show("seen only", timed(seen_only, e.synchronize))
        mid = (box[0] + box[1]) // 2
        show("one row", timed(lambda: e.build_map(poses, ranges, ang, cell_size=size, box=(mid, mid + 1, box[2], box[3]), max_range=mr, device=True),
                              e.synchronize))

        def replay():
            for k in range(n):
                e.set_scan(ranges[k], ang)
                e.map_update(poses[k:k + 1])
        if with_replay:
            t_replay = show("replay", timed(replay, e.synchronize))
            print(f"  replay / build = {t_replay / t_build:.1f}")
        e.close()


if __name__ == "__main__":
    main()
