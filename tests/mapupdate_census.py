"""A census of one scan's map update (OracleHybridMap.update, oracle/rbpf_oracle.py:211-252; hybridmap.py:95-145): the
same loop, but instead of changing cell values it records every operation as (beam, kind) on the STORAGE cell it lands in
(tile centre + the `set_index` pair, which folds in the cells the index formula repeats on the negative side of a tile) and
the global source cells of every storage cell.  From that, for every flagged storage cell (one with an occupied or nearby
operation) what the map-update kernels' fixed-capacity tables see: the number of events, of occupied / nearby hits, whether
the cell is near the start cell, on its rim, on an axis or diagonal through it, and the window kernel's window, bucket rank,
bucket depth and bucket count.  CPU only; the GPU tier tests (test_gpu_mapray_tiers.py, test_gpu_mapwin_tiers.py) prove on it
which rung of the kernels' table ladder a scene reaches before the GPU sees the scene.

The constants restate kernels_mapray.hip, kernels_mapupdate.hip and rbpf_mapupdate.h."""
from collections import Counter

import numpy as np

from oracle import rbpf_oracle as orc

EMP, NEAR, OCC = 0, 1, 2            # kinds of operation: gridmap.py:97-101 / hybridmap.py:139-142 / hybridmap.py:137

# kernels_mapray.hip / rbpf_mapupdate.h
NEAR_R = 16                         # ray steps counted in the 16-bit block round the start cell
ECAP, PCAP, NPOOL = 16, 64, 48      # events of a per-pair list, of a pool list, pool lists
RSLOW, NNEAR, NSPC, RSPEC = 256, 128, 32, 512
HIT_BOUND = 63
# kernels_mapupdate.hip
WIN, EV_TOT, NB_MAX, REG_EVENTS = 128, 4096, 1536, 16


class Cell:
    """One storage cell: key = (tile cx, tile cy, a, b); ops in the order the reference applies them."""
    __slots__ = ("key", "ops", "sources", "events", "hits", "pairs", "near", "rim", "inside", "special", "window", "rank", "kwindow", "krank")

    def __init__(self, key):
        self.key, self.ops, self.sources = key, [], set()

    @property
    def flagged(self):
        return any(k != EMP for _, k in self.ops)


class Census:
    def __init__(self, pose, cell_size, map_len_m, n_beams):
        self.pose, self.cs, self.map_len_m, self.B = pose, cell_size, map_len_m, n_beams
        self.dim = round(map_len_m / cell_size)
        self.cells = {}             # key -> Cell, every cell a ray touches
        self.n_ops = 0              # all operations = the oracle's cells_visited of this update + n_near_ops
        self.n_near_ops = 0         # nearby hits (no ray point of their own)
        self.start = None
        self.ends = []              # per beam: (end cell, occupied?) or None for a ray without points
        self.flagged = []           # flagged cells in (tile, row-major) order
        self.fan = None             # global bounding box of the start cell and the rays' end cells: x0, x1, y0, y1


def _axis(g, cs, map_len_m, dim):
    """Tile centre and storage index of global index g along one axis (hybridmap.py:193-200, gridmap.py:93)."""
    c = orc.map_centre_1d(g * cs, map_len_m)
    return c, orc.set_index(g * cs - c, cs, dim)


def census(pose, ranges, angles, cell_size=0.05, map_len_m=40):
    """The operations of OracleHybridMap(cell_size).update(pose, *scan_xy(ranges, angles)) on a fresh map."""
    cs = cell_size
    sx, sy = orc.scan_xy(ranges, angles)
    gx, gy = orc.transform(sx, sy, pose)
    c = Census(tuple(float(v) for v in pose), cs, map_len_m, len(gx))
    dim, half = c.dim, map_len_m / 2
    tiles = [(0, 0)]

    def tile_with_pos(x, y):                                          # hybridmap.py:263-272, :44-45
        for t in tiles:
            if x >= t[0] - half and x < t[0] + half and y >= t[1] - half and y < t[1] + half:
                return t
        return None

    def op(t, rx, ry, src, beam, kind):
        key = (t[0], t[1], orc.set_index(rx, cs, dim), orc.set_index(ry, cs, dim))
        cell = c.cells.get(key)
        if cell is None:
            cell = c.cells[key] = Cell(key)
        cell.ops.append((beam, kind))
        cell.sources.add(src)
        c.n_ops += 1

    if tile_with_pos(pose[0], pose[1]) is None:                       # :98-100
        return c
    start = c.start = (int(pose[0] / cs), int(pose[1] / cs))          # :102
    fan = [start[0], start[0], start[1], start[1]]
    for i in range(len(gx)):
        end_is_occ = True
        dist = np.sqrt(sx[i] ** 2 + sy[i] ** 2)
        end = (int(gx[i] / cs), int(gy[i] / cs))
        if dist > orc.MAX_RAY_M:                                      # :107-113
            scale = 15.0 / dist
            end = (int(start[0] + scale * (end[0] - start[0])), int(start[1] + scale * (end[1] - start[1])))
            end_is_occ = False
        pts = orc.get_affected_points(start[0], start[1], end[0], end[1])
        c.ends.append((end, end_is_occ) if pts else None)
        if pts:
            fan = [min(fan[0], end[0]), max(fan[1], end[0]), min(fan[2], end[1]), max(fan[3], end[1])]
        for j, ind in enumerate(pts):
            px, py = ind[0] * cs, ind[1] * cs
            m = tile_with_pos(px, py)
            if m is None:                                             # :125-133
                m = (orc.map_centre_1d(px, map_len_m), orc.map_centre_1d(py, map_len_m))
                if m not in tiles:
                    tiles.append(m)
            if end_is_occ and ind[0] == end[0] and ind[1] == end[1]:  # :137
                op(m, px - m[0], py - m[1], ind, i, OCC)
                if j > 0:                                             # :139-142
                    nx, ny = pts[j - 1][0] * cs, pts[j - 1][1] * cs
                    if nx >= m[0] - half and nx < m[0] + half and ny >= m[1] - half and ny < m[1] + half:
                        op(m, nx - m[0], ny - m[1], pts[j - 1], i, NEAR)
                        c.n_near_ops += 1
            else:                                                     # :144
                op(m, px - m[0], py - m[1], ind, i, EMP)
    c.fan = tuple(fan)
    _classify(c)
    return c


def _classify(c):
    x0, y0 = c.start
    cs, L, dim = c.cs, c.map_len_m, c.dim
    first_g = {}

    def tile_first(centre):                                           # first global index of the tile with this centre along an axis
        if centre not in first_g:
            g = int(round((centre - L / 2) / cs)) - 3
            while orc.map_centre_1d(g * cs, L) != centre:
                g += 1
            first_g[centre] = g
        return first_g[centre]

    flagged = [cell for cell in c.cells.values() if cell.flagged]
    for cell in flagged:
        cell.events = len(cell.ops)
        cell.pairs = [(b, 0 if k == OCC else 1) for b, k in cell.ops if k != EMP]
        cell.hits = len(cell.pairs)
        d = [max(abs(gx - x0), abs(gy - y0)) for gx, gy in cell.sources]
        cell.near = min(d) < NEAR_R
        cell.rim = cell.near and max(d) >= NEAR_R
        cell.inside = cell.near and not cell.rim
        cell.special = any(gx == x0 or gy == y0 or abs(gx - x0) == abs(gy - y0) for gx, gy in cell.sources)
        cx, cy, a, b = cell.key
        cell.window = (cx, cy, a // WIN, b // WIN)
        # the window kernel lays its windows from the fan's first storage row of the tile and its first 32-cell group of columns
        a_lo = _axis(max(tile_first(cx), c.fan[0]), cs, L, dim)[1]
        b_lo = _axis(max(tile_first(cy), c.fan[2]), cs, L, dim)[1] & ~31
        cell.kwindow = (cx, cy, (a - a_lo) // WIN, (b - b_lo) // WIN)
    flagged.sort(key=lambda cell: cell.key)                           # per tile: row-major
    for attr, rk in (("window", "rank"), ("kwindow", "krank")):
        seen = Counter()
        for cell in flagged:
            w = getattr(cell, attr)
            setattr(cell, rk, seen[w])
            seen[w] += 1
    c.flagged = flagged


def replay(c, maps=None, cc=(orc.LOG_ODDS_OCC, orc.LOG_ODDS_NEARBY, orc.LOG_ODDS_EMP, orc.MAX_ODDS_OCC, orc.MIN_ODDS_EMP)):
    """The census' operations applied with the reference's clamped adds (gridmap.py:86-117), cell by cell in recorded order,
    onto maps = {tile centre: [dim][dim] array} (made where missing).  Returns maps."""
    occ, near, emp, vmax, vmin = cc
    maps = {} if maps is None else maps
    for (cx, cy, a, b), cell in c.cells.items():
        m = maps.get((cx, cy))
        if m is None:
            m = maps[(cx, cy)] = np.zeros((c.dim, c.dim))
        val = m[a][b]
        for _, kind in cell.ops:
            val = max(val + emp, vmin) if kind == EMP else min(val + (occ if kind == OCC else near), vmax)
        m[a][b] = val
    return maps


# ---- what the kernels' tables see ---------------------------------------------------------------------------------------

def window_tables(c, B=None, kernel_windows=True):
    """Per window of the 128x128-window kernel: nflag, cap (events per bucket), nbk (buckets), NB (bucket ids)
    (kernels_mapupdate.hip, "event slots are shared out evenly").  kernel_windows=False: 128-aligned storage windows."""
    B = c.B if B is None else B
    NB = min(2 * B, NB_MAX)
    out = {}
    for w, nflag in Counter(cell.kwindow if kernel_windows else cell.window for cell in c.flagged).items():
        cap = min(64, max(4, EV_TOT // nflag))
        out[w] = {"nflag": nflag, "cap": cap, "nbk": min(nflag, NB, EV_TOT // cap), "NB": NB}
    return out


def window_routing(c, B=None):
    """(slow, pool, register) cells of the window kernel: slow iff events > cap or rank >= nbk (nbk <= NB), pool iff
    16 < events <= cap in a bucket, else replayed in registers."""
    tabs = window_tables(c, B)
    slow = pool = reg = 0
    for cell in c.flagged:
        t = tabs[cell.kwindow]
        if cell.events > t["cap"] or cell.krank >= t["nbk"]:
            slow += 1
        elif cell.events > REG_EVENTS:
            pool += 1
        else:
            reg += 1
    return slow, pool, reg


def pairs_in_play(c):
    """The (beam, e) pairs the global-index kernel lists (kernels_mapray.hip pass 1): every pair of an occupied beam whose
    global cell is not that of a smaller pair of the same beam or of the two beams before it."""
    def gcell(b, e):
        if b < 0 or c.ends[b] is None or not c.ends[b][1]:
            return None
        end = c.ends[b][0]
        if e == 0:
            return end
        pts = orc.get_affected_points(c.start[0], c.start[1], end[0], end[1])
        return pts[-2] if len(pts) >= 2 and _same_tile(c, pts[-2], end) else None
    out = []
    for b in range(c.B):
        g0, g1 = gcell(b, 0), gcell(b, 1)
        if g0 is None:
            continue
        prev = (gcell(b - 1, 0), gcell(b - 1, 1), gcell(b - 2, 0))
        if g0 not in prev:
            out.append((b, 0, g0))
        if g1 is not None and g1 != g0 and g1 not in prev:
            out.append((b, 1, g1))
    return out


def _same_tile(c, g, h):
    return all(orc.map_centre_1d(g[k] * c.cs, c.map_len_m) == orc.map_centre_1d(h[k] * c.cs, c.map_len_m) for k in (0, 1))


def storage_key(c, g):
    (cx, a), (cy, b) = _axis(g[0], c.cs, c.map_len_m, c.dim), _axis(g[1], c.cs, c.map_len_m, c.dim)
    return (cx, cy, a, b)


def special_far_pairs(c):
    """Pairs in play whose storage cell is special and not near: each takes a slot of the special list (RSPEC)."""
    return sum(1 for b, e, g in pairs_in_play(c) if c.cells[storage_key(c, g)].special and not c.cells[storage_key(c, g)].near)


def near_inside_cells(c):
    """Flagged cells with every source inside the block's walk: the first NNEAR of them fold from the second walk."""
    return sum(1 for cell in c.flagged if cell.inside)


def summary(c):
    f = c.flagged
    return {"flagged": len(f), "near": sum(x.near for x in f), "rim": sum(x.rim for x in f), "inside": near_inside_cells(c),
            "special": sum(x.special for x in f), "gt16": sum(x.events > ECAP for x in f), "gt64": sum(x.events > PCAP for x in f),
            "max_events": max((x.events for x in f), default=0), "windows": len({x.kwindow for x in f})}
