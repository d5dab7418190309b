"""Paths from a travel-cost field (ParticleEngine.travel_cost; include/rbpf_hip.h, rbpf_travel_cost).  Host side,
NumPy only: the field is the work of the GPU, a path is a walk down it.  Below that, what goes with ParticleEngine.check_paths
(rbpf_check_paths): the result type, the cells of a walk, any-angle shortcuts, velocity rollouts and their ranking,
and with ParticleEngine.check_rollouts (rbpf_check_rollouts): rollout templates and their placement at poses, and
with ParticleEngine.check_footprints (rbpf_check_footprints): heading bins and the span table of a footprint."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

AXIAL, DIAGONAL = 5, 7
# the order in which path_to tries the neighbours of a cell
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


class Travel(NamedTuple):
    cost: Optional[np.ndarray]       # int32 [x1-x0, y1-y0] chamfer units (5 per axial step), -1 unreachable; None with particle=None
    clearance: Optional[np.ndarray]  # uint16 [x1-x0, y1-y0] min(chamfer distance to the nearest occupied cell, clear_max); None likewise
    goal_cost: Optional[np.ndarray]  # int32 [n_goals], or [P, n_goals] with particle=None; None without goals
    rounds: int                      # relaxation rounds launched (a diagnostic)
    box: tuple                       # (x0, x1, y0, y1) in mosaic cells
    cell: float                      # metres per cell (tile_len / dim)
    inv: float                       # cells per metre as the engine forms it (dim / tile_len): a point lies in cell floor(x * inv)
    inflate: int                     # cells of T have clearance > inflate
    clear_max: int


def cost_metres(cost, cell: float):
    """Chamfer units -> metres (float64), NaN where the cost is -1."""
    c = np.asarray(cost)
    return np.where(c >= 0, c.astype(np.float64) * (float(cell) / AXIAL), np.nan)


def path_to(travel: Travel, goal_xy):
    """[k, 2] cell centres in metres from a start cell to the cell of `goal_xy` (metres), or None where its cost is -1 or it lies
    outside the box.  Walks down the field: from c to the first neighbour n, in the order of NEIGHBOURS, with cost[n] >= 0 and
    cost[n] + w == cost[c] (w = 5 axial, 7 diagonal; for a diagonal both side cells must have cost >= 0).  Such a
    neighbour exists wherever cost > 0: a traversable cell next to a reached one is reached, so cost >= 0 stands for "in T"."""
    cost = np.asarray(travel.cost)
    x0, _, y0, _ = travel.box
    g = np.floor(np.asarray(goal_xy, dtype=np.float64)[:2] * np.float64(travel.inv))
    i, j = int(g[0]) - x0, int(g[1]) - y0
    nx, ny = cost.shape
    if not (0 <= i < nx and 0 <= j < ny) or cost[i, j] < 0:
        return None
    cells = [(i, j)]
    while cost[i, j] > 0:
        for di, dj in NEIGHBOURS:
            a, b = i + di, j + dj
            if not (0 <= a < nx and 0 <= b < ny) or cost[a, b] < 0:
                continue
            if di and dj and (cost[a, j] < 0 or cost[i, b] < 0):
                continue
            if int(cost[a, b]) + (DIAGONAL if di and dj else AXIAL) == int(cost[i, j]):
                i, j = a, b
                break
        else:
            raise ValueError(f"cost field is no fixed point at cell {(i + x0, j + y0)}")
        cells.append((i, j))
    out = np.array(cells[::-1], dtype=np.float64) + np.array([x0 + 0.5, y0 + 0.5])
    return out * float(travel.cell)


# ---- path checks (ParticleEngine.check_paths; include/rbpf_hip.h, rbpf_check_paths) -----------------------------
def _host(a):
    """A result as numpy, wherever it lives."""
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class PathCheck(NamedTuple):
    first_blocked: np.ndarray        # int32 [K], or [P, K]: the least blocked step of each path, -1 if none
    first_unknown: np.ndarray        # int32 likewise: the least step on an unknown cell (lattice value 0), -1 if none
    min_clearance: np.ndarray        # int32 likewise: min over the path's cells of min(chamfer distance to an occupied cell, clear_max)
    n_unknown: np.ndarray            # int32 likewise: steps on unknown cells
    steps: np.ndarray                # int32 [K] (with own=True [P, K]): steps of each path, 1 + the sum of its segments' max(|dX|, |dY|);
                                     # from check_rollouts [N, K] as every field, and a tensor as they are with device=True
    cell: float                      # metres per cell
    inflate: int                     # a cell carries the robot if its clearance exceeds inflate
    clear_max: int

    @property
    def clear(self):
        """bool, the shape of first_blocked: no step of the path is blocked."""
        return self.first_blocked < 0

    def p_clear(self, weights=None):
        """float64 [K]: the share of the particles in whose map each path is clear, weighted by `weights` [P] (non-negative,
        normalised here; default: equal).  For one particle's result it is clear as 0.0 / 1.0."""
        c = _host(self.first_blocked) < 0
        if c.ndim == 1:
            return c.astype(np.float64)
        w = np.full(c.shape[0], 1.0) if weights is None else np.asarray(weights, dtype=np.float64)
        if w.shape != (c.shape[0],) or not np.all(w >= 0) or not w.sum() > 0:
            raise ValueError("weights must be [P], non-negative and not all zero")
        return (w / w.sum()) @ c.astype(np.float64)

    def clearance_metres(self):
        """min_clearance in metres (float64): chamfer units are a fifth of a cell."""
        return _host(self.min_clearance).astype(np.float64) * (float(self.cell) / AXIAL)


def walk_cells(cells):
    """int64 [S, 2]: the walk of rbpf_check_paths through the waypoint cells `cells` [m, 2], in its closed form: a segment from A
    to B with n = max(|dX|, |dY|) adds the steps t = 1 .. n, the major coordinate moving by one a step and the minor one by
    floor((2 t a + n) / (2 n)), a its whole change.  S = 1 + the sum of n."""
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    out = [c[:1]]
    for A, B in zip(c[:-1], c[1:]):
        d = B - A
        a = np.abs(d)
        n = int(a.max())
        if n == 0:
            continue
        t = np.arange(1, n + 1, dtype=np.int64)
        major = 0 if a[0] >= a[1] else 1
        minor = 1 - major
        seg = np.empty((n, 2), np.int64)
        seg[:, major] = A[major] + (-1 if d[major] < 0 else 1) * t
        seg[:, minor] = A[minor] + (-1 if d[minor] < 0 else 1) * ((2 * t * a[minor] + n) // (2 * n))
        out.append(seg)
    return np.concatenate(out)


def path_cells(path, inv: float):
    """int64 [S, 2]: the cells rbpf_check_paths walks along `path` [m, 2+] (metres; a point lies in cell floor(x * inv)), step by
    step: row s is the place of a first_blocked or first_unknown of s."""
    p = np.asarray(path, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] < 2 or len(p) < 1:
        raise ValueError("path must be [m, 2+] with m >= 1")
    return walk_cells(np.floor(p[:, :2] * np.float64(inv)).astype(np.int64))


def shortcut(path, segments_clear, lookahead: int = 64):
    """Any-angle smoothing of `path` [n, 2+] (e.g. the cell path of path_to): the chain of its waypoints from the first to the
    last of least Euclidean length whose legs are all clear; ties go to fewer waypoints, then to the lower waypoint index.
    `segments_clear(legs) -> bool [len(legs)]` is asked once, for the straight legs path[i] -> path[j] of all pairs
    0 < j - i <= lookahead, each a [2, 2] polyline.  Returns the chain [k, 2]; ValueError where no chain of clear legs joins
    the ends (the path itself does not check clear)."""
    p = np.asarray(path, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] < 2 or len(p) < 1:
        raise ValueError("path must be [n, 2+] with n >= 1")
    p = p[:, :2]
    n, look = len(p), max(1, int(lookahead))
    if n == 1:
        return p.copy()
    pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, min(i + look, n - 1) + 1)]
    ok = np.asarray(segments_clear([p[[i, j]] for i, j in pairs]), dtype=bool)
    if ok.shape != (len(pairs),):
        raise ValueError("segments_clear must return one bool per leg")
    best = [(0.0, 0, -1)] + [None] * (n - 1)              # (length, waypoints so far, predecessor)
    for (i, j), good in zip(pairs, ok):                   # pairs in the order of i: every best[i] is final when it is read
        if not good or best[i] is None:
            continue
        cand = (best[i][0] + float(np.hypot(*(p[j] - p[i]))), best[i][1] + 1)
        # lengths within rounding of each other (collinear waypoints) are a tie: sums of square roots are not exact
        tie = best[j] is not None and abs(cand[0] - best[j][0]) <= 1e-12 * max(cand[0], best[j][0])
        if best[j] is None or (cand[1] < best[j][1] if tie else cand[0] < best[j][0]):
            best[j] = cand + (i,)
    if best[-1] is None:
        raise ValueError("no chain of clear legs joins the ends of the path")
    chain, k = [], n - 1
    while k >= 0:
        chain.append(k)
        k = best[k][2]
    return p[chain[::-1]]


def shortcut_in(engine, path, particle="best", radius_m: float = 0.0, min_share: float = 1.0, weights=None, lookahead: int = 64,
                through_unknown: bool = False, start_exempt: bool = True):
    """shortcut(path) with the legs checked by engine.check_paths in the map of `particle`, or with particle=None in every
    particle's: a leg is clear if its share PathCheck.p_clear(weights) reaches `min_share`.  start_exempt holds for the legs that
    leave the path's first waypoint, as it would for the path itself; they are checked in a call of their own."""
    p0 = np.asarray(path, dtype=np.float64)[0, :2]

    def clear(legs):
        ok = np.zeros(len(legs), dtype=bool)
        first = np.array([start_exempt and np.array_equal(leg[0], p0) for leg in legs], dtype=bool)
        for exempt in (False, True):
            idx = np.flatnonzero(first == exempt)
            if len(idx):
                chk = engine.check_paths(np.stack([legs[k] for k in idx]), particle=particle, radius_m=radius_m,
                                         through_unknown=through_unknown, start_exempt=exempt)
                ok[idx] = chk.p_clear(weights) >= float(min_share)
        return ok

    return shortcut(path, clear, lookahead)


def rollouts(poses, speeds, turn_rates, horizon_s: float, dt: float):
    """Constant-(v, w) arcs from `poses` ([3] or [P, 3]: x, y, theta) in closed form: [K, M, 2] for one pose, [P, K, M, 2] for
    [P, 3], rollout k driving speeds[k] (m/s) and turn_rates[k] (rad/s) for M = round(horizon_s / dt) + 1 points at t = 0, dt, ...
    The point at t is the chord of the arc: x + v t sinc(w t / 2) cos(theta + w t / 2), and y with sin: exact, and the straight
    line at w = 0."""
    ps = np.asarray(poses, dtype=np.float64)
    v, w = np.asarray(speeds, dtype=np.float64).reshape(-1), np.asarray(turn_rates, dtype=np.float64).reshape(-1)
    if ps.shape[-1] != 3 or ps.ndim not in (1, 2) or v.shape != w.shape or not dt > 0 or not horizon_s >= 0:
        raise ValueError("poses must be [3] or [P, 3], speeds and turn_rates [K], dt > 0 and horizon_s >= 0")
    t = np.arange(int(round(float(horizon_s) / float(dt))) + 1, dtype=np.float64) * float(dt)
    half = 0.5 * w[:, None] * t[None, :]                                   # [K, M]
    chord = v[:, None] * t[None, :] * np.sinc(half / np.pi)                # numpy's sinc(x) is sin(pi x) / (pi x)
    q = ps.reshape(-1, 3)
    ang = q[:, None, None, 2] + half[None]
    out = np.stack([q[:, None, None, 0] + chord[None] * np.cos(ang), q[:, None, None, 1] + chord[None] * np.sin(ang)], axis=-1)
    return out[0] if ps.ndim == 1 else out


def arc_templates(speeds, turn_rates, horizon_s: float, dt: float):
    """[K, M, 2]: the constant-(v, w) arcs of `rollouts` in the robot's frame, i.e. rollouts(np.zeros(3), ...): what
    ParticleEngine.check_rollouts places at every pose on the GPU."""
    return rollouts(np.zeros(3), speeds, turn_rates, horizon_s, dt)


def place_templates(poses, templates):
    """[N, K, M, 2] (one pose [3]: [K, M, 2]): `templates` [K, M, 2+] placed at `poses` [N, 3] by the rule of rbpf_check_rollouts
    (include/rbpf_hip.h), which this states in NumPy: c = math.cos(theta) and s = math.sin(theta) once per pose, then
    wx = x + (c * lx - s * ly) and wy = y + (s * lx + c * ly), every operation a float64 operation rounded on its own, in this
    order.  The cells floor(w * inv) of the result are therefore the cells the device walks, bit for bit, and
    check_paths(place_templates(...)) is what check_rollouts(...) returns.  rollouts(poses, ...) adds the heading inside the
    cosine instead of rotating a finished template, so it agrees with placed arc_templates only to rounding."""
    import math
    ps = np.asarray(poses, dtype=np.float64)
    tm = np.asarray(templates, dtype=np.float64)
    if ps.shape[-1] != 3 or ps.ndim not in (1, 2) or tm.ndim != 3 or tm.shape[2] < 2:
        raise ValueError("poses must be [3] or [N, 3] and templates [K, M, 2+]")
    q = ps.reshape(-1, 3)
    c = np.array([math.cos(th) for th in q[:, 2]], dtype=np.float64)[:, None, None]
    s = np.array([math.sin(th) for th in q[:, 2]], dtype=np.float64)[:, None, None]
    lx, ly = tm[None, :, :, 0], tm[None, :, :, 1]
    out = np.stack([q[:, 0, None, None] + (c * lx - s * ly), q[:, 1, None, None] + (s * lx + c * ly)], axis=-1)
    return out[0] if ps.ndim == 1 else out


def rank_rollouts(check: PathCheck, end_cost=None, weights=None, min_p_clear: float = 0.95, clearance_weight: float = 0.0):
    """The rollouts of `check` ([K], or [P, K] from particle=None or own=True) worth driving, best first, as indices into K: those
    with p_clear(weights) >= min_p_clear, ordered by the least expected end_cost - clearance_weight * expected min_clearance
    (both in chamfer units), or without `end_cost` by the largest expected min_clearance; ties go to the lower index.  `end_cost`
    ([K] or [P, K]) is the cost at the arcs' ends, e.g. the goal_cost of a travel_cost whose START is the goal; -1 (no way)
    counts as infinite."""
    fb = _host(check.first_blocked)
    many = fb.ndim == 2
    w = None
    if many:
        w = np.full(fb.shape[0], 1.0) if weights is None else np.asarray(weights, dtype=np.float64)
        w = w / w.sum()
    # over the particles that carry weight: an infinite cost in a particle of weight 0 must not turn the mean into 0 * inf
    mean = lambda a: (w[w > 0] @ a[w > 0]) if many and a.ndim == 2 else a
    p = check.p_clear(weights)
    clearance = mean(_host(check.min_clearance).astype(np.float64))
    if end_cost is None:
        score = -clearance
    else:
        c = _host(end_cost).astype(np.float64)
        score = mean(np.where(c < 0, np.inf, c)) - float(clearance_weight) * clearance
    keep = np.flatnonzero(p >= float(min_p_clear))
    return keep[np.argsort(score[keep], kind="stable")]


# ---- footprint checks (ParticleEngine.check_footprints; include/rbpf_hip.h, rbpf_check_footprints) --------------
def heading_bins(angles, H: int):
    """int32, the shape of `angles`: the heading bin of each angle (radians) among H, by the rule of rbpf_check_footprints:
    floor(angle * (H / (2 pi)) + 0.5) mod H in float64 and in this order, reduced into 0 .. H - 1 for negative angles.  An angle
    whose |angle * H / (2 pi)| reaches 2^31 (or is not finite) is a ValueError."""
    H = int(H)
    if not 1 <= H <= 256:
        raise ValueError("1 <= H <= 256 is required")
    q = np.asarray(angles, dtype=np.float64) * np.float64(H / (2.0 * np.pi))
    if not np.all(np.abs(q) < 2147483648.0):
        raise ValueError("|angle * H / (2 pi)| < 2^31 is required")
    return (np.floor(q + 0.5).astype(np.int64) % H).astype(np.int32)


def arc_headings(turn_rates, horizon_s: float, dt: float):
    """[K, M]: the heading w t of the constant-(v, w) arcs of arc_templates at their M points t = 0, dt, ..., in the robot's frame:
    the `headings` that go with arc_templates(speeds, turn_rates, horizon_s, dt) into ParticleEngine.check_footprints."""
    w = np.asarray(turn_rates, dtype=np.float64).reshape(-1)
    if not dt > 0 or not horizon_s >= 0:
        raise ValueError("dt > 0 and horizon_s >= 0 are required")
    t = np.arange(int(round(float(horizon_s) / float(dt))) + 1, dtype=np.float64) * float(dt)
    return w[:, None] * t[None, :]


def path_headings(path):
    """[m]: a heading for every waypoint of the world path `path` [m, 2+] from its segments: waypoint j looks along the segment
    to waypoint j + 1, the last waypoint repeats the one before it, and a segment of no length keeps the heading before it (0
    where there is none).  With the path as a template at the pose (0, 0, 0), check_footprints drives it in every map."""
    p = np.asarray(path, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] < 2 or len(p) < 1:
        raise ValueError("path must be [m, 2+] with m >= 1")
    out, last = np.zeros(len(p)), 0.0
    for j in range(len(p) - 1):
        dx, dy = p[j + 1, 0] - p[j, 0], p[j + 1, 1] - p[j, 1]
        if dx != 0.0 or dy != 0.0:
            last = float(np.arctan2(dy, dx))
        out[j] = last
    out[-1] = last
    return out


class Footprint(NamedTuple):
    spans: np.ndarray                # int32 [S, 3]: (dx, y0, y1), the cells (dx, y0 .. y1) relative to the cell the robot's centre stands on
    offsets: np.ndarray              # int32 [H + 1]: bin b holds spans[offsets[b]:offsets[b + 1]]
    H: int                           # heading bins; bin b stands for the heading 2 pi b / H
    cell: float                      # metres per cell the table was cut for


FOOTPRINT_MAX_OFFSET, FOOTPRINT_MAX_SPANS, FOOTPRINT_MAX_WIDTH = 127, 256, 64


def _polygon_distance(poly, px, py):
    """Distance of the points (px, py) to the polygon `poly` [n, 2]: 0 inside (even-odd rule), else to the nearest edge."""
    a, b = poly, np.roll(poly, -1, axis=0)
    best = np.full(px.shape, np.inf)
    inside = np.zeros(px.shape, dtype=bool)
    for (ax, ay), (bx, by) in zip(a, b):
        ex, ey = bx - ax, by - ay
        ll = ex * ex + ey * ey
        t = np.clip(((px - ax) * ex + (py - ay) * ey) / ll, 0.0, 1.0) if ll > 0 else np.zeros(px.shape)
        best = np.minimum(best, np.hypot(px - (ax + t * ex), py - (ay + t * ey)))
        if ay != by:
            cross = ((ay > py) != (by > py)) & (px < ax + (py - ay) * (ex / (by - ay)))
            inside ^= cross
    return np.where(inside, 0.0, best)


def footprint_table(polygon_xy, cell: float, heading_bins: int = 64, pad_m: Optional[float] = None):
    """The Footprint of the robot outline `polygon_xy` [n >= 3, 2] (metres, robot frame, x ahead; the origin is the point whose
    poses are checked) for maps of `cell` metres a cell and H = `heading_bins` bins.  Bin b holds the cells whose centre, with the
    robot's centre on the centre of cell (0, 0), lies inside or within `pad_m` of the polygon turned by 2 pi b / H; a row of cells
    is cut into spans of at most 64.
    The default pad_m is cell * sqrt(2) + r_max * 2 pi / H, r_max the farthest vertex.  The robot stands anywhere in its cell, up to
    half a cell diagonal from the centre; a point it covers lies anywhere in the cell that is reported for it, up to half a diagonal
    from that centre; and the heading tested is that of the bin pb + tmpl_bin, two roundings of half a bin each, which move a point
    at radius r by at most r * 2 pi / H.  So the table covers the true footprint wherever the robot stands in its cell and whichever
    way the two roundings fall.  pad_m = 0 is the bare outline on the cell centres.
    A table that passes +-127 cells, or 256 spans in a bin, is a ValueError that names the limit."""
    poly = np.asarray(polygon_xy, dtype=np.float64)
    H, cell = int(heading_bins), float(cell)
    if poly.ndim != 2 or poly.shape[1] != 2 or len(poly) < 3 or not np.all(np.isfinite(poly)) or not cell > 0 or not 1 <= H <= 256:
        raise ValueError("polygon_xy must be [n >= 3, 2] and finite, cell > 0 and 1 <= heading_bins <= 256")
    r_max = float(np.hypot(poly[:, 0], poly[:, 1]).max())
    pad = cell * np.sqrt(2.0) + r_max * 2.0 * np.pi / H if pad_m is None else float(pad_m)
    if not pad >= 0:
        raise ValueError("pad_m >= 0 is required")
    m = int(np.ceil((r_max + pad) / cell)) + 1
    if (r_max + pad) / cell > 4 * FOOTPRINT_MAX_OFFSET:                      # before a raster of that size is built
        raise ValueError(f"the footprint reaches {(r_max + pad) / cell:.0f} cells: a span's offsets are limited to +-{FOOTPRINT_MAX_OFFSET} cells")
    k = np.arange(-m, m + 1)
    gx, gy = np.meshgrid(k * cell, k * cell, indexing="ij")
    spans, offsets = [], [0]
    for b in range(H):
        th = 2.0 * np.pi * b / H
        c, s = np.cos(th), np.sin(th)
        turned = np.stack([c * poly[:, 0] - s * poly[:, 1], s * poly[:, 0] + c * poly[:, 1]], axis=1)
        mask = _polygon_distance(turned, gx, gy) <= pad
        mask[m, m] = True                                                   # the cell the robot stands on, however small the outline
        for i in np.flatnonzero(mask.any(axis=1)):
            ys = np.flatnonzero(mask[i])
            for run in np.split(ys, np.flatnonzero(np.diff(ys) > 1) + 1):
                for y0 in range(int(run[0]), int(run[-1]) + 1, FOOTPRINT_MAX_WIDTH):
                    y1 = min(y0 + FOOTPRINT_MAX_WIDTH - 1, int(run[-1]))
                    spans.append((int(i) - m, y0 - m, y1 - m))
        offsets.append(len(spans))
    sp = np.asarray(spans, dtype=np.int32).reshape(-1, 3)
    if np.abs(sp).max() > FOOTPRINT_MAX_OFFSET:
        raise ValueError(f"the footprint reaches {int(np.abs(sp).max())} cells: a span's offsets are limited to +-{FOOTPRINT_MAX_OFFSET} cells")
    for b in range(H):
        if offsets[b + 1] - offsets[b] > FOOTPRINT_MAX_SPANS:
            raise ValueError(f"bin {b} needs {offsets[b + 1] - offsets[b]} spans: a bin is limited to {FOOTPRINT_MAX_SPANS} spans")
    return Footprint(sp, np.asarray(offsets, dtype=np.int32), H, cell)


def footprint_cells(fp: Footprint, b: int):
    """int64 [n, 2]: the cells (dx, dy) bin `b` of the table covers, relative to the cell the robot's centre stands on."""
    if not 0 <= int(b) < fp.H:
        raise ValueError("bin out of range")
    rows = fp.spans[int(fp.offsets[b]):int(fp.offsets[b + 1])]
    out = [np.stack([np.full(int(y1) - int(y0) + 1, int(dx), np.int64), np.arange(int(y0), int(y1) + 1, dtype=np.int64)], axis=1) for dx, y0, y1 in rows]
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)
