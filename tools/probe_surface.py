"""score_surface beside what there was for the job before it ("Measured").

  python tools/probe_surface.py [pairs] [--no-yardsticks]
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/probe_surface.py 1000 --no-yardsticks

The scene and the pairs of tools/probe_pairs.py at 0.05 m: 2000 scans of 1081 beams, `pairs` pairs (default 1000), window 16,
20 rotations of 0.5 degrees; two peaks, drop 5 % of 2 n_used, the default exclusion box.  Wall time round a synchronise, REPS
calls after a warm-up:
  search     match_pairs(device=True) alone, no volume: what the loop closer paid before
  volume     match_pairs(device=True, return_scores=True): the search writing its volume to device memory
  both       that, followed by score_surface with host outputs: what loops.match_informed runs per batch
  surface    score_surface alone on the device volume, host outputs
  parent     what the parent commit offers: match_pairs(return_scores=True) into host arrays, then the same quantities by a
             vectorised NumPy pass (numpy_surface below, chunks of 100 pairs); its two halves are also timed alone
The NumPy pass and the GPU must agree on every record before anything is timed.  Under rocprofv3 the trace holds
surface_kernel's own time: 2 REPS + 3 dispatches."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS, BEAMS, SCANS = 5, 1081, 2000


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


def show(name, ms):
    print(f"  {name:10s} min {min(ms):10.3f}  median {float(np.median(ms)):10.3f}  max {max(ms):10.3f} ms", flush=True)
    return float(np.median(ms))


def numpy_surface(V, drop, ex_t, ex_r, K, chunk=100):
    """rbpf_score_surface's records [N, K, 16] and counts [N] by vectorised NumPy, `chunk` items at a time."""
    N, nk, nw, _ = V.shape
    R, W, ncand = nk // 2, nw // 2, nk * nw * nw
    kk, ii, jj = (a.reshape(-1) for a in np.meshgrid(np.arange(-R, R + 1), np.arange(-W, W + 1), np.arange(-W, W + 1), indexing="ij"))
    rank = np.empty(ncand, dtype=np.int64)
    rank[np.lexsort((jj, ii, kk, ii * ii + jj * jj, np.abs(kk)))] = np.arange(ncand)
    rec, cnt = np.zeros((N, K, 16), dtype=np.int64), np.zeros(N, dtype=np.int32)
    for n0 in range(0, N, chunk):
        v = V[n0:n0 + chunk].reshape(-1, ncand).astype(np.int64)
        n = len(v)
        rows = np.arange(n)
        merit = v * ncand + (ncand - 1 - rank)
        free = np.ones(v.shape, dtype=bool)
        dr = np.asarray(drop[n0:n0 + chunk], dtype=np.int64)
        for p in range(K):
            live = free.any(axis=1)
            at = np.argmax(np.where(free, merit, -1), axis=1)
            pi, pj, pk, sp = ii[at], jj[at], kk[at], v[rows, at]
            di, dj, dk = ii[None] - pi[:, None], jj[None] - pj[:, None], kk[None] - pk[:, None]
            box = (np.abs(di) <= ex_t) & (np.abs(dj) <= ex_t) & (np.abs(dk) <= ex_r)
            w = np.where(free & box & (v >= (sp - dr)[:, None]), v - (sp - dr)[:, None] + 1, 0)
            cols = [pi, pj, pk, sp, (w > 0).sum(axis=1), w.sum(axis=1), (w * di).sum(axis=1), (w * dj).sum(axis=1), (w * dk).sum(axis=1),
                    (w * di * di).sum(axis=1), (w * di * dj).sum(axis=1), (w * di * dk).sum(axis=1), (w * dj * dj).sum(axis=1),
                    (w * dj * dk).sum(axis=1), (w * dk * dk).sum(axis=1), np.zeros(n, np.int64)]
            rec[n0:n0 + n, p] = np.where(live[:, None], np.stack(cols, axis=1), 0)
            cnt[n0:n0 + n] += live
            free &= ~box
    return rec, cnt


def main():
    import bench
    from thesis_amd import loops
    from thesis_amd.datasets import synthetic
    from thesis_amd.engine import ParticleEngine
    m = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1000
    yardsticks = "--no-yardsticks" not in sys.argv
    ang, ranges, _, truth = synthetic.make_log(SCANS - 1, BEAMS, period=bench.PERIOD_S)
    truth, ranges = np.ascontiguousarray(truth[:SCANS]), np.ascontiguousarray(ranges[:SCANS])
    pairs = loops.candidates(truth, min_gap=50, radius=0.5, half_run=5)[:m]
    m = len(pairs)
    step = float(np.radians(0.5))
    rng = np.random.Generator(np.random.PCG64(7))
    guess = truth[pairs[:, 0]] + rng.uniform(-1.0, 1.0, (m, 3)) * 0.8 * np.array([0.8, 0.8, 20 * step])
    e = ParticleEngine(1, max_beams=BEAMS, pool_tiles=16)
    search = lambda **kw: e.match_pairs(truth, ranges, ang, pairs, guess, **kw)
    res = search(device=True, return_scores=True)
    surf = e.score_surface(res)
    ex = e.surface_exclusion(16, 20)
    amb, c2 = surf.ambiguity(), surf.second_moment(0)
    print(f"{m} pairs over {SCANS} scans of {BEAMS} beams, volume {tuple(res.scores.shape[1:])} = {res.scores[0].numel() * 4 / 1024:.0f} KiB a pair, "
          f"exclusion {ex}, two peaks, drop 5 %: median drop {int(np.median(surf.drop))}, median plateau {int(np.median(surf.size[:, 0]))} cells, "
          f"median sigma {float(np.median(np.sqrt(c2[:, 0, 0]))):.4f} / {float(np.median(np.sqrt(c2[:, 1, 1]))):.4f} m / "
          f"{float(np.median(np.sqrt(c2[:, 2, 2]))):.5f} rad, median ambiguity {float(np.median(amb)):.3f}, {int((amb > 0.9).sum())} pairs above 0.9; "
          f"{REPS} timed calls each")
    t_search = show("search", timed(lambda: search(device=True), e.synchronize))
    show("volume", timed(lambda: search(device=True, return_scores=True), e.synchronize))
    t_both = show("both", timed(lambda: e.score_surface(search(device=True, return_scores=True)), e.synchronize))
    t_surf = show("surface", timed(lambda: e.score_surface(res), e.synchronize))
    print(f"  both / search = {t_both / t_search:.2f}; surface / search = {t_surf / t_search:.2f}")
    if yardsticks:
        host = search(return_scores=True)
        drop = np.asarray(surf.drop)
        rec, cnt = numpy_surface(host.scores, drop, ex[0], ex[1], 2)
        got = np.concatenate([surf.index, surf.score[..., None], surf.size[..., None], surf.moments, np.zeros_like(surf.score)[..., None]], axis=2)
        assert np.array_equal(rec, got) and np.array_equal(cnt, surf.count), "the NumPy pass and the GPU disagree"

        def parent():
            h = search(return_scores=True)
            numpy_surface(h.scores, np.floor(0.05 * (2 * h.n_used.astype(np.int64)).astype(np.float64)).astype(np.int64), ex[0], ex[1], 2)
        t_par = show("parent", timed(parent, e.synchronize, reps=2))
        show("  to host", timed(lambda: search(return_scores=True), e.synchronize, reps=2))
        show("  numpy", timed(lambda: numpy_surface(host.scores, drop, ex[0], ex[1], 2), lambda: None, reps=2))
        print(f"  parent / both = {t_par / t_both:.1f}")
    e.close()


if __name__ == "__main__":
    main()
