"""Scalar oracle of rbpf_check_paths (include/rbpf_hip.h) on a rendered raster.  The walk is an incremental
Bresenham that carries an error term from cell to cell - not the closed form of the kernel and of plan.path_cells, so the two
pin each other - the clearance is travel_oracle.clearance, and the rules of a blocked step are written out once more.

The raster is the box grown by m = travel_oracle.margin(clear_max) cells on every side (ParticleEngine.render_map of the grown
box: 0 outside the tiles and outside the lattice); every waypoint's cell must lie in the box."""
import numpy as np

from tests import travel_oracle as T


def bresenham(cells):
    """[(X, Y)] of the walk through the waypoint cells `cells`: from A to B the major axis moves by one a step; the error term,
    in units of 1 / (2 n), starts at a half (n), grows by 2 * |minor change| a step and carries the minor axis at 2 n."""
    cells = [(int(x), int(y)) for x, y in cells]
    out = [cells[0]]
    for (xa, ya), (xb, yb) in zip(cells[:-1], cells[1:]):
        ax, ay = abs(xb - xa), abs(yb - ya)
        sx, sy = (1 if xb >= xa else -1), (1 if yb >= ya else -1)
        n, err = max(ax, ay), max(ax, ay)
        x, y = xa, ya
        for _ in range(n):
            if ax >= ay:
                x += sx
                err += 2 * ay
                if err >= 2 * n:
                    err -= 2 * n
                    y += sy
            else:
                y += sy
                err += 2 * ax
                if err >= 2 * n:
                    err -= 2 * n
                    x += sx
            out.append((x, y))
    return out


FREE, WALL = -30, 30


def fuzz_scene(seed=1):
    """int8 [200, 150]: free cells, walls every 20 rows with a 6-cell gap at alternating ends, 0.2 % clutter and a 40 x 50 patch
    of unknown cells across two of the walls."""
    c = np.full((200, 150), FREE, np.int8)
    clutter = np.random.default_rng(seed).random(c.shape) < 0.002
    for k in range(1, 10):
        c[20 * k] = WALL
    c[clutter] = WALL
    for k in range(1, 10):
        c[20 * k, (slice(3, 9) if k % 2 else slice(141, 147))] = FREE
    c[70:110, 60:110] = 0
    return c


def fuzz_paths(rng, n, shape, origin, inv, leg=8):
    """n three-waypoint paths (metres) with legs of at most `leg` cells inside a raster of `shape` whose cell (0, 0) is mosaic
    cell `origin`: a start anywhere, two moves drawn uniformly, clipped to the raster."""
    hi = np.array(shape) - 1
    a = rng.integers(0, hi + 1, size=(n, 2))
    b = np.clip(a + rng.integers(-leg, leg + 1, size=(n, 2)), 0, hi)
    c = np.clip(b + rng.integers(-leg, leg + 1, size=(n, 2)), 0, hi)
    cells = np.stack([a, b, c], axis=1) + np.asarray(origin)
    return (cells + rng.uniform(0.05, 0.95, size=cells.shape)) / float(inv)


class Field:
    """What a check needs of one map over one box: v, min(d, clear_max) and ok(c), computed once and shared by every path."""

    def __init__(self, grown, box, quantum, occupied_threshold, inflate, clear_max, through_unknown=False):
        assert 0 <= inflate < clear_max <= 320
        m = T.margin(clear_max)
        nx, ny = box[1] - box[0], box[3] - box[2]
        assert np.asarray(grown).shape == (nx + 2 * m, ny + 2 * m)
        self.box, self.inflate, self.clear_max = tuple(box), int(inflate), int(clear_max)
        self.v = np.asarray(grown)[m:m + nx, m:m + ny].astype(np.int64)
        self.clear = T.clearance(grown, clear_max, quantum, occupied_threshold).astype(np.int64)
        blocked = (self.v.astype(np.float64) * float(quantum) > float(occupied_threshold)) if through_unknown else self.v >= 0
        self.ok = ~blocked & (self.clear > int(inflate))

    def check(self, cells, start_exempt=False):
        """(first_blocked, first_unknown, min_clearance, n_unknown, steps) of the path through the waypoint cells (mosaic)."""
        walk = bresenham(cells)
        x0, y0 = self.box[0], self.box[2]
        first = walk[0]

        def ok(c):
            if start_exempt and c == first:
                return True
            return bool(self.ok[c[0] - x0, c[1] - y0])

        first_blocked = first_unknown = -1
        n_unknown, min_clear = 0, self.clear_max
        for s, c in enumerate(walk):
            i, j = c[0] - x0, c[1] - y0
            assert 0 <= i < self.v.shape[0] and 0 <= j < self.v.shape[1], "the path leaves the oracle's box"
            free = ok(c)
            if free and s > 0:
                q = walk[s - 1]
                if q[0] != c[0] and q[1] != c[1]:                          # diagonal: no corner is cut
                    free = ok((c[0], q[1])) and ok((q[0], c[1]))
            if not free and first_blocked < 0:
                first_blocked = s
            if self.v[i, j] == 0:
                n_unknown += 1
                if first_unknown < 0:
                    first_unknown = s
            min_clear = min(min_clear, int(self.clear[i, j]))
        return first_blocked, first_unknown, min_clear, n_unknown, len(walk)

    def check_xy(self, paths, inv, start_exempt=False):
        """int32 [K, 4] and steps int32 [K] of paths in metres (a list of [m, 2+] arrays)."""
        res = [self.check(T.cells_of(np.asarray(p, dtype=np.float64)[:, :2], inv), start_exempt) for p in paths]
        return np.array([r[:4] for r in res], dtype=np.int32).reshape(-1, 4), np.array([r[4] for r in res], dtype=np.int32)
