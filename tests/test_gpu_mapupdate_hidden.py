"""Written boxes and occupancy words after map updates, on the shapes the tier scenes (tests/helpers.py::run_map_case) do not
aim at: a. cells crossing the occupied threshold both ways, and cells at the clamps;  b. ray ends on the bit and word borders of
the occupancy words, on the first and last row of a tile and round the four-tile corner;  c. the partial last word of a tile row
(0.1 m cells) under a thin and a dense fan;  d. a thin fan whose 32-cell groups hold one to four touched words beside occupied
cells in the untouched ones, also on 0.025 m cells;  e. boxes that grow over what load_map, set_tile and a resample copy wrote.

Every case: small engines (P <= 6), at most three scans of a few dozen beams, under the default kernel chain, the event walk,
the global-index kernel and the window kernel.  Cells, boxes and occupancy words are exact against OracleHybridMap with its
visited planes (tests/mapupdate_hidden.py); cells_written and ray_cells_visited are exact against the oracle's counts.  Each
scene asserts on the oracle's numbers that it reaches what it was built for.

GPU only:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests import mapupdate_hidden as H
from tests import resample_oracle as R
from tests.resample_scenes import TILE, apply_sources, box_union, raster, same_tiles
from tests.test_gpu_wb_whole_groups import thin

pytestmark = pytest.mark.gpu

Q = 0.1
HOME = (0.0, 0.0)
KERNELS = ["default", "ev", "ray", "window"]


@pytest.fixture(params=KERNELS)
def eng(request, monkeypatch):
    """thesis_amd.engine with the map kernel chosen as tests/test_gpu_parity.py chooses it (rbpf_create reads RBPF_MAP_KERNEL)."""
    monkeypatch.delenv("RBPF_EV_GRID", raising=False)
    if request.param == "default":
        monkeypatch.delenv("RBPF_MAP_KERNEL", raising=False)
    else:
        monkeypatch.setenv("RBPF_MAP_KERNEL", request.param)
    from thesis_amd import engine
    return engine


class Case:
    """An engine and one oracle map per particle, with what the model of the hidden state needs beside the oracle's cells: the
    cells any scan visited, the boxes other writers left, and the two counters."""

    def __init__(self, engine, P, cs, max_beams, pool=32):
        self.e = engine.ParticleEngine(P, max_beams=max_beams, cell_size=cs, pool_tiles=pool)
        self.P, self.cs, self.dim = P, cs, self.e.dim
        self.maps = [orc.OracleHybridMap(cs) for _ in range(P)]
        self.visited = [{} for _ in range(P)]            # {centre: bool plane}: the union over the scans
        self.last = [{} for _ in range(P)]               # the same of the last scan alone
        self.written = [{} for _ in range(P)]            # {centre: box} of set_tile, load_map
        self.c0 = self.e.counters()
        self.cells_written = self.ray_cells = 0

    def tile(self, p, centre):
        for t in self.maps[p].tiles:
            if (float(t.cx), float(t.cy)) == centre:
                return t
        t = orc.OracleTile(int(centre[0]), int(centre[1]), 40, self.cs)
        self.maps[p].tiles.append(t)
        return t

    def set_tile(self, p, centre, cells):
        """rbpf_set_tile: the whole tile counts as written."""
        self.e.set_tile(p, centre, cells)
        self.tile(p, centre).map = cells.astype(np.float64) * Q
        self.written[p][centre] = (0, self.dim - 1, 0, self.dim - 1)

    def load(self, p, centre, x, y, vals):
        """rbpf_load_map of a raster inside one tile, at the tile's cell (x, y): its box is written, zeros included."""
        ox, oy = R.tile_origin(centre, self.dim, TILE)
        self.e.load_map(raster(self.e, ox + x, oy + y, vals), particle=p)
        h, w = vals.shape
        self.tile(p, centre).map[x:x + h, y:y + w] = vals.astype(np.float64) * Q
        self.written[p][centre] = box_union(self.written[p].get(centre), (x, x + h - 1, y, y + w - 1))

    def copy(self, idx):
        """A resample with the ancestors idx: a new particle has what its ancestor had, boxes included."""
        apply_sources(self.e, idx)
        self.maps = [self.maps[i].copy() for i in idx]
        self.visited = [{c: v.copy() for c, v in self.visited[i].items()} for i in idx]
        self.written = [dict(self.written[i]) for i in idx]

    def scan(self, r, ang, poses):
        self.e.set_scan(r, ang)
        self.e.map_update(np.asarray(poses, dtype=np.float64))
        sx, sy = orc.scan_xy(r, ang)
        for p, hm in enumerate(self.maps):
            before = hm.cells_visited
            hm.clear_visited()
            hm.update(tuple(float(v) for v in poses[p]), sx, sy)
            self.ray_cells += hm.cells_visited - before
            self.last[p] = {c: v.copy() for c, v in H.visited_planes(hm).items()}
            for c, v in self.last[p].items():
                self.cells_written += int(v.sum())
                self.visited[p][c] = self.visited[p].get(c, False) | v

    def cells(self, p):
        return H.oracle_planes(self.maps[p], Q)[0]

    def box(self, p, centre):
        """The model's box of a tile: the visited cells united with the other writers' boxes."""
        v = self.visited[p].get(centre)
        return box_union(None if v is None else H.bounding_box(v), self.written[p].get(centre))

    def check(self, what):
        e = self.e
        got = H.read_hidden_of(e, range(self.P))
        for p in range(self.P):
            cells = self.cells(p)
            same_tiles(e, p, cells, what)
            vis = {c: self.visited[p].get(c, np.zeros((self.dim, self.dim), bool)) for c in cells}
            H.check_map_hidden(e, p, self.maps[p], visited=vis, written=self.written[p], what=what, hidden=got[p])
        c = e.counters()
        have = (c["cells_written"] - self.c0["cells_written"], c["ray_cells_visited"] - self.c0["ray_cells_visited"])
        print(what, "cells_written, ray_cells_visited", have, "oracle", (self.cells_written, self.ray_cells))
        assert have == (self.cells_written, self.ray_cells), (what, have, (self.cells_written, self.ray_cells))
        return c

    def close(self):
        self.e.close()


def centred(cells, cs):
    """Metres of the middle of a global cell: half a cell from every border the index formulas round at."""
    return (np.asarray(cells, dtype=np.float64) + 0.5) * cs


# ---- a. the threshold, both ways ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamps", [False, True])
def test_cells_cross_the_threshold_both_ways(eng, clamps):
    """The home tile preloaded by set_tile.  Values thr - 1 .. thr + 3 under the fan: free cells go from thr + 1, thr + 2 and
    thr + 3 down to or below thr (bit 1 -> 0; thr + 3 lands on thr exactly), end cells go from thr - 1 and thr up across it
    (bit 0 -> 1; the cell before an end cell is first a free cell of the same ray, so it goes down by one), unvisited cells at
    thr keep 0.  At the clamps: stripes of vmin and vmax, where a visited cell may not change at all and its word must stay."""
    cs, B = 0.05, 48
    poses = [[0.2, -0.1, 0.4], [3.11, 2.22, 1.0], [1.26, 0.77, -2.0]]
    k = Case(eng, len(poses), cs, B)
    thr = H.geom(k.e)[2]
    x, y = np.meshgrid(np.arange(k.dim), np.arange(k.dim), indexing="ij")
    if clamps:
        pre = np.where(((y // 64) + (x // 16)) % 2 == 1, 30, -30).astype(np.int8)
    else:
        pre = (thr - 1 + (x + 2 * y) % 5).astype(np.int8)
    for p in range(k.P):
        k.set_tile(p, HOME, pre)
    ang = np.linspace(-0.7, 0.7, B)
    k.scan(2.5 + 0.5 * np.sin(5 * ang), ang, poses)
    for p in range(k.P):                                 # the scene reaches what it is for
        post, v = k.cells(p)[HOME], k.last[p][HOME]
        assert len(k.maps[p].tiles) == 1
        was, now = pre > thr, post > thr
        if clamps:
            assert (v & (pre == -30) & (post == -30)).any() and (v & (pre == 30) & (post == 30)).any()
            assert (v & (pre == 30) & (post == 27)).any() and (v & (pre == -30) & (post > -30)).any()
            rows, cols = np.nonzero(v & (pre == post))
            grp = {(int(a), int(b) // 32) for a, b in zip(rows, cols)} - {(int(a), int(b) // 32) for a, b in zip(*np.nonzero(v & (pre != post)))}
            assert len(grp) > 20                         # 32-cell groups whose visited cells all stay as they are
        else:
            assert (v & was & ~now).any() and (v & ~was & now).any()
            assert (v & (pre == thr + 3) & (post == thr)).any() and (~v & (post == thr)).any()
            assert (v & (pre <= thr) & (post >= thr + 5)).any()              # an end cell
    k.check("clamps" if clamps else "threshold")
    k.close()


# ---- b. bit and word positions -----------------------------------------------------------------------------------------------
def test_ray_ends_on_bit_word_and_group_borders(eng):
    """Six particles one cell apart in y, beams along +y, -y, +x and two diagonals: the rays' ends, which are their tiles' box
    rims, walk over the columns 32k - 1, 32k, 32k + 1 and the 16-column borders between them."""
    cs = 0.05
    poses = [[centred(3, cs), centred(j, cs), 0.0] for j in range(6)]
    ang = np.array([np.pi / 2, np.pi / 2 + 1e-3, -np.pi / 2, -np.pi / 2 + 1e-3, 0.0, 0.6, -2.2])
    r1 = np.array([45, 45, 50, 50, 30, 37, 41]) * cs
    r2 = np.array([61, 61, 66, 66, 30, 37, 41]) * cs
    k = Case(eng, 6, cs, len(ang))
    k.scan(r1, ang, poses)
    rims = {k.box(p, HOME)[3] % 32 for p in range(6)} | {k.box(p, HOME)[2] % 32 for p in range(6)}
    k.scan(r2, ang, poses)
    rims |= {k.box(p, HOME)[3] % 32 for p in range(6)} | {k.box(p, HOME)[2] % 32 for p in range(6)}
    assert {31, 0, 1, 15, 16, 17} <= rims, rims
    k.check("bit and word borders")
    k.close()


def test_first_and_last_rows_and_the_four_tile_corner(eng):
    """From two cells off the corner where four tiles meet, eight short beams: one scan grows four boxes, on the last row and
    column of one tile and the first of another.  The same at the corner on the negative side."""
    cs = 0.05
    poses = [[centred(397, cs), centred(397, cs), 0.0], [centred(398, cs), centred(396, cs), 0.3],
             [centred(-397, cs), centred(-397, cs), 0.0], [centred(397, cs), centred(-397, cs), 1.0]]
    ang = np.arange(8) * (np.pi / 4) + 0.05
    k = Case(eng, len(poses), cs, len(ang))
    k.scan(np.full(8, 9 * cs), ang, poses)
    d = k.dim - 1
    for p in (0, 1):
        boxes = {c: k.box(p, c) for c in k.cells(p)}
        assert set(boxes) == {HOME, (40.0, 0.0), (0.0, 40.0), (40.0, 40.0)}
        assert boxes[HOME][1] == d and boxes[HOME][3] == d and boxes[(40.0, 40.0)][0] == 0 and boxes[(40.0, 40.0)][2] == 0
        assert boxes[(40.0, 0.0)][0] == 0 and boxes[(0.0, 40.0)][2] == 0
    for p in (2, 3):
        assert len(k.cells(p)) >= 3 and all(k.box(p, c) is not None for c in k.cells(p))
    k.scan(np.full(8, 7 * cs) + 0.01, ang + 0.2, poses)
    k.check("tile rims and corners")
    k.close()


# ---- c. the partial last word ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [None, 1])
def test_partial_last_word_under_thin_and_dense_fans(eng, monkeypatch, grid):
    """0.1 m cells: dim 400, a tile row ends in half a word.  Thin fans (diagonal) and dense ones (along y) in turn run across
    their tile's last 16 columns and the seam behind them; with RBPF_EV_GRID=1 one resident workgroup takes them all, and so
    both instantiations of the write-back in one launch."""
    if grid is not None:
        monkeypatch.setenv("RBPF_EV_GRID", str(grid))
    cs, B = 0.1, 16
    ang = np.linspace(-0.15, 0.15, B)
    scans = [np.full(B, 6.0), 6.0 - 0.4 * np.cos(9 * ang) ** 2]
    poses = [[14.05, 16.05, np.pi / 4], [0.35, 16.05, np.pi / 2], [-14.05, -16.05, -3 * np.pi / 4], [0.35, -16.05, -np.pi / 2],
             [3.05, 16.25, 3 * np.pi / 4], [-7.75, 15.05, np.pi / 2]]
    for r in scans:
        ratio = [thin(p, r, ang, cs) for p in poses]
        assert all(q < 0.9 for q in ratio[0::2]) and all(q > 1.1 for q in ratio[1::2]), ratio
    k = Case(eng, len(poses), cs, B)
    assert k.dim == 400
    for r in scans:
        k.scan(r, ang, poses)
    for p in range(k.P):                                 # two tiles each; the last 16 columns of one, the first of the other
        boxes = [k.box(p, c) for c in k.cells(p)]
        assert len(boxes) == 2 and any(b[3] == 399 for b in boxes) and any(b[2] == 0 for b in boxes), (p, boxes)
        assert p in (2, 3) or any(b[3] == 399 and b[2] < 384 for b in boxes), (p, boxes)   # (2 and 3 look down the negative side)
    k.check("partial last word")
    k.close()


# ---- d. a thin fan's groups with one to four touched words -------------------------------------------------------------------
@pytest.mark.parametrize("cs", [0.05, 0.025])
def test_thin_fan_touches_one_to_four_words_of_a_group(eng, cs):
    """Five beams at slopes 1, 6, 10, 14 and 30 columns a row: in a row a beam covers that many columns, one to eight of a
    group's words.  The thin branch stores up to three words alone and falls through at four.  The cells under the fan were
    loaded with values round the threshold, so the untouched words of a touched group hold occupied cells whose bits must
    survive."""
    n = 120                                              # cells a beam runs
    slopes = np.array([1.0, 6.0, 10.0, 14.0, 30.0])
    ang = np.arctan(slopes)
    r = np.full(len(ang), n * cs)
    poses = [[centred(40, cs), centred(37, cs), 0.0], [centred(90, cs), centred(51, cs), 0.02]]
    assert all(thin(p, r, ang, cs) < 0.9 for p in poses)
    k = Case(eng, len(poses), cs, len(ang), pool=16)
    thr = H.geom(k.e)[2]
    side = 200
    x, y = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    pre = (thr - 1 + (3 * x + y) % 4).astype(np.int8)    # thr - 1 .. thr + 2
    at = k.dim // 2 + 10
    for p in range(k.P):
        k.load(p, HOME, at, at, pre)
    k.scan(r, ang, poses)
    for p in range(k.P):
        v = k.last[p][HOME]
        words = v.reshape(k.dim, k.dim // 32, 8, 4).any(axis=3)           # [row, group, word]
        counts = words.sum(axis=2)
        assert {1, 2, 3, 4} <= set(np.unique(counts).tolist()), np.unique(counts)
        full = np.zeros((k.dim, k.dim), np.int8)
        full[at:at + side, at:at + side] = pre
        occ_words = (full > thr).reshape(k.dim, k.dim // 32, 8, 4).any(axis=3)
        beside = (occ_words & ~words).any(axis=2)                         # an occupied cell in an untouched word of the group
        for c in (1, 2, 3, 4):
            assert (beside & (counts == c)).any(), c
    k.scan(r - 3 * cs, ang + 0.01, poses)
    k.check(f"thin fan, {cs} m")
    k.close()


# ---- e. boxes that grow over other writers -----------------------------------------------------------------------------------
def test_boxes_grow_over_load_map_set_tile_and_resample_copies(eng):
    """Particle 0: a loaded raster whose box is larger than its non-zero cells, the fan leaves it on one side.  1: a set_tile
    tile next to the home tile, the fan runs into it.  2 and 3: their own fans, then 3 is overwritten by a copy of 2 and both
    are updated from different poses - the box is the union of the ancestor's and the new cells, never less.  4: stands in a
    loaded tile and never looks into the home tile, which it holds with the empty box.  5: nothing but its fans."""
    cs, B = 0.1, 24
    k = Case(eng, 6, cs, B, pool=48)
    dim = k.dim
    rng = np.random.default_rng(12)
    ring = rng.integers(-30, 31, size=(30, 40)).astype(np.int8)
    ring[:3], ring[-3:], ring[:, :5], ring[:, -5:] = 0, 0, 0, 0
    ring[10, 20] = 30
    k.load(0, HOME, 215, 190, ring)
    east = rng.integers(-30, 31, size=(dim, dim)).astype(np.int8)
    k.set_tile(1, (40.0, 0.0), east)
    k.load(2, (0.0, 40.0), 198, 2, np.full((6, 4), 25, np.int8))
    k.load(3, HOME, 100, 100, np.full((9, 9), -7, np.int8))
    k.load(4, (40.0, 0.0), 200, 200, np.full((4, 4), 12, np.int8))
    assert R.written_box(k.cells(0)[HOME]) != k.written[0][HOME]
    ang = np.linspace(-0.5, 0.5, B)
    poses = np.array([[1.05, -1.05, 0.0], [17.05, 0.35, 0.1], [0.35, 17.05, 1.5], [-6.05, -6.05, -2.0], [40.35, 0.25, 0.0], [5.05, 5.05, 3.0]])
    k.scan(4.0 + 0.5 * np.sin(6 * ang), ang, poses)
    assert k.box(4, HOME) is None and k.box(1, (40.0, 0.0)) == (0, dim - 1, 0, dim - 1)
    assert k.box(0, HOME)[0] == 210 and k.box(0, HOME)[1] > 244          # the fan starts before the raster and ends behind it
    k.check("before the copy")
    before = [{c: k.box(p, c) for c in k.cells(p)} for p in range(6)]
    k.copy([0, 1, 2, 2, 4, 5])
    assert set(k.cells(3)) == set(k.cells(2)) == {HOME, (0.0, 40.0)}
    poses[3] = [1.35, 17.55, 1.2]
    poses[2] = poses[2] + [0.3, -0.2, 0.2]
    k.scan(3.5 + 0.5 * np.cos(5 * ang), ang, poses)
    for c, b in before[2].items():                       # never shrunk: the ancestor's box lies inside both
        for p in (2, 3):
            assert box_union(k.box(p, c), b) == k.box(p, c)
        assert k.box(3, c) != b
    assert k.box(2, HOME) != before[2][HOME]
    assert k.box(2, HOME) != k.box(3, HOME) and k.box(4, HOME) is None
    k.check("after the copy")
    k.close()
