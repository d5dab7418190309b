"""Scalar restatement of the scan-check specification (include/rbpf_hip.h: rbpf_check_scans), written from the
specification and not from the kernel, in the manner of tests/cast_oracle.py: plain Python floats are IEEE float64 and math.cos /
math.sin are the libm the library's host code calls, so the GPU tests compare bit for bit.  classify_cast is the other way to the
same answer, the one a user had before the kernel: NumPy on the ranges and statuses cast_scans returns."""
import math

import numpy as np

SKIP, MATCH, LONG, SHORT, NEW, OFF, MISSING, CLEAR = range(8)


def check_pose(cells, x0, y0, lo, hi, inv, quantum, occupied_threshold, pose, angles, ranges, max_range, min_range, tol, model):
    """One pose in one rendered map.  cells[X - x0][Y - y0]: int8 lattice values, 0 outside the raster; [lo, hi) the lattice's
    mosaic cells (cast_oracle.lattice_bounds); inv = dim / tile_len; model: hit_tab, class_cost, half_bins, bins_per_cell.
    Returns (classes [B] uint8, cost int, counts [8] int32, d [B] float64: t - tz of a MATCH or LONG beam, NaN elsewhere, steps)."""
    x, y, th = (float(q) for q in pose)
    c, s = math.cos(th), math.sin(th)
    ox, oy = x * inv, y * inv
    tmax, ttol = max_range * inv, tol * inv
    nxc, nyc = cells.shape
    rows = cells.tolist()
    hit_tab, class_cost = [int(q) for q in model.hit_tab], [int(q) for q in model.class_cost]
    hb, bpc = int(model.half_bins), int(model.bins_per_cell)
    B = len(angles)
    classes, dd, cost, steps = np.zeros(B, np.uint8), np.full(B, np.nan), 0, 0

    def value(X, Y):
        i, j = X - x0, Y - y0
        return rows[i][j] if 0 <= i < nxc and 0 <= j < nyc else 0

    for b, a in enumerate(angles):
        z = float(ranges[b])
        if not (z > 0) or z < min_range:
            continue                                         # SKIP: no walk, class cost below
        returned = z < max_range
        tz = z * inv
        tlim = min(tz + ttol, tmax) if returned else tmax
        ca, sa = math.cos(a), math.sin(a)
        dx, dy = c * ca - s * sa, s * ca + c * sa
        fX, fY = math.floor(ox), math.floor(oy)
        st, t, E = 2, 0.0, None
        if lo <= fX < hi and lo <= fY < hi:
            X, Y = int(fX), int(fY)
            sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
            tdx = 1.0 / abs(dx) if dx != 0 else math.inf
            tdy = 1.0 / abs(dy) if dy != 0 else math.inf
            fx = (X + 1) - ox if dx > 0 else ox - X
            fy = (Y + 1) - oy if dy > 0 else oy - Y
            nx = ny = 0
            while True:
                if not (lo <= X < hi and lo <= Y < hi):
                    st = 2
                    break
                if t <= tz:
                    E = (X, Y)                               # the last tested cell entered at or before the measured end
                if value(X, Y) * quantum > occupied_threshold:
                    st = 1
                    break
                tmx = (nx + fx) * tdx if dx != 0 else math.inf
                tmy = (ny + fy) * tdy if dy != 0 else math.inf
                if tmx < tmy:
                    t, nx, X = tmx, nx + 1, X + sx
                else:
                    t, ny, Y = tmy, ny + 1, Y + sy
                steps += 1
                if t > tlim:
                    st = 0
                    break
        if st == 2:
            cls = OFF
        elif not returned:
            cls = MISSING if st == 1 else CLEAR
        elif st == 1:
            d = t - tz
            cls = MATCH if d >= -ttol else LONG
            q = math.floor(d * bpc + 0.5)
            cost += hit_tab[max(-hb, min(hb, q)) + hb]
            dd[b] = d
        else:
            cls = SHORT if value(*E) < 0 else NEW
        classes[b] = cls
    counts = np.bincount(classes, minlength=8).astype(np.int32)
    cost += sum(int(counts[k]) * class_cost[k] for k in range(8))
    return classes, cost, counts, dd, steps


def check(maps, lo, hi, inv, quantum, occupied_threshold, poses, angles, ranges, max_range, min_range, tol, model):
    """Every pose: maps(n) -> (cells, x0, y0) is the rendered map pose n is checked in, ranges [1 | N][B].  Returns a dict of
    cost int64 [N], counts int32 [N, 8], classes uint8 [N, B], votes int32 [B, 8], d float64 [N, B] and steps."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1, len(angles))
    out = [check_pose(*maps(n), lo, hi, inv, quantum, occupied_threshold, q, angles, ranges[n if len(ranges) > 1 else 0],
                      max_range, min_range, tol, model) for n, q in enumerate(poses)]
    classes = np.stack([o[0] for o in out])
    votes = np.stack([(classes == k).sum(axis=0) for k in range(8)], axis=1).astype(np.int32)
    return dict(cost=np.array([o[1] for o in out], dtype=np.int64), counts=np.stack([o[2] for o in out]), classes=classes, votes=votes,
                d=np.stack([o[3] for o in out]), steps=sum(o[4] for o in out))


def raw_bins(d, model):
    """floor(d * bins_per_cell + 0.5) before the clamp, NaN where d is."""
    return np.floor(np.asarray(d) * int(model.bins_per_cell) + 0.5)


def end_cells(poses, angles, ranges, inv):
    """int64 [N, B, 2]: the mosaic cell that holds the point at the measured range of every beam (0, 0 where that is not
    finite), for classify_cast's v_end.  It is the specification's E unless that point lies within rounding of a cell border."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    z = np.broadcast_to(np.asarray(ranges, dtype=np.float64).reshape(-1, len(angles)), (len(poses), len(angles)))
    th = poses[:, 2:3] + np.asarray(angles, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        px = (poses[:, 0:1] + z * np.cos(th)) * inv
        py = (poses[:, 1:2] + z * np.sin(th)) * inv
    ok = np.isfinite(px) & np.isfinite(py) & (np.abs(px) < 2.0 ** 40) & (np.abs(py) < 2.0 ** 40)
    return np.stack([np.floor(np.where(ok, px, 0.0)), np.floor(np.where(ok, py, 0.0))], axis=2).astype(np.int64)


def classify_cast(cast_ranges, cast_status, ranges, inv, max_range, min_range, tol, model, v_end=None):
    """The classes and sums from a cast of the same poses and beams to `max_range` (cast_scans with return_status), vectorised:
    a hit of the cast at range e is a hit of the check iff e * inv <= tlim, with d = e * inv - tz.  v_end [N, B]: the lattice
    value at each beam's measured end (end_cells); None leaves every beam without a hit NEW.  Two things differ from the
    specification: e * inv is the entry parameter t only up to rounding (e = t / inv), so a beam within an ulp of a class or bin
    border may fall the other side; and a cast that left the lattice (status 2) is OFF here whatever the measured range, where
    the specification says OFF only if the ray leaves the lattice within tlim.  Returns the dict of check() without d and steps."""
    e, st = np.asarray(cast_ranges, dtype=np.float64), np.asarray(cast_status)
    z = np.broadcast_to(np.asarray(ranges, dtype=np.float64).reshape(-1, e.shape[1]), e.shape)
    hb, bpc = int(model.half_bins), int(model.bins_per_cell)
    with np.errstate(invalid="ignore"):
        tz, ttol, tmax = z * inv, tol * inv, max_range * inv
        skip = ~(z > 0) | (z < min_range)
        returned = z < max_range
        tlim = np.where(returned, np.minimum(tz + ttol, tmax), tmax)
        te = e * inv
        hit = (st == 1) & (te <= tlim)
        d = te - tz
        free_end = np.zeros(e.shape, bool) if v_end is None else np.asarray(v_end) < 0
        classes = np.where(returned, np.where(hit, np.where(d >= -ttol, MATCH, LONG), np.where(free_end, SHORT, NEW)),
                           np.where(hit, MISSING, CLEAR))
        classes = np.where(st == 2, OFF, classes)
        classes = np.where(skip, SKIP, classes).astype(np.uint8)
        on_tab = (classes == MATCH) | (classes == LONG)
        q = np.clip(np.floor(np.where(on_tab, d, 0.0) * bpc + 0.5), -hb, hb).astype(np.int64)
    beam_cost = np.asarray(model.class_cost, dtype=np.int64)[classes] + np.where(on_tab, np.asarray(model.hit_tab, dtype=np.int64)[q + hb], 0)
    counts = np.stack([(classes == k).sum(axis=1) for k in range(8)], axis=1).astype(np.int32)
    votes = np.stack([(classes == k).sum(axis=0) for k in range(8)], axis=1).astype(np.int32)
    return dict(cost=beam_cost.sum(axis=1), counts=counts, classes=classes, votes=votes)
