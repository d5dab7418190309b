"""Engines, scenes and checks shared by the tests of what moves a particle: tests/test_gpu_resample.py (the local copies) and
tests/test_gpu_migrate.py (the packed particles between ranks).  Everything here needs the GPU except geometry_cases, the
constants and the pure helpers (bits, box_union, free_positions, steady)."""
import ctypes as C

import numpy as np

from tests import resample_oracle as R
from tests import travel_oracle as T

TILE = 40.0
CLEAR_MAX = 11                  # chamfer units: the clearance reads the occupancy words up to 3 cells round the box
MARGIN = 5                      # cells round a map's extent that render_map and the clearance also look at
_I32 = C.POINTER(C.c_int32)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def make_engine(P, cs=0.1, pool=None):
    from thesis_amd.engine import ParticleEngine
    return ParticleEngine(P, cell_size=cs, max_beams=8, pool_tiles=4 * P + 64 if pool is None else pool)


def raster(e, x0, y0, cells):
    from thesis_amd.mapio import MapRaster
    return MapRaster(x0=int(x0), y0=int(y0), cell_size=float(e.cfg.cell_size), quantum=float(e.cfg.quantum), dim=e.dim,
                     tile_len=float(e.cfg.tile_len_m), cells=np.ascontiguousarray(cells, dtype=np.int8))


def queue_sources(e, src):
    """rbpf_apply_resample_local without arrivals; it returns without waiting and without reading the device's error word."""
    s = np.ascontiguousarray(src, dtype=np.int32)
    g = np.arange(e.P, dtype=np.int32)
    assert s.shape == (e.P,)
    e._check(e._lib.rbpf_apply_resample_local(e._h, s.ctypes.data_as(_I32), g.ctypes.data_as(_I32)))


def apply_sources(e, src):
    queue_sources(e, src)
    e.synchronize()                                      # a checked call: a device-side error of the resample surfaces here


def tile_count(e, p):
    n = C.c_int32()
    e._check(e._lib.rbpf_get_tile_count(e._h, int(p), C.byref(n)))
    return n.value


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def lattice_clip(e, box):
    lo = -int(e.cfg.lattice_radius) * e.dim - e.dim // 2
    hi = lo + (2 * int(e.cfg.lattice_radius) + 1) * e.dim
    return (max(box[0], lo), min(box[1], hi), max(box[2], lo), min(box[3], hi))


def box_union(a, b):
    if a is None or b is None:
        return a if b is None else b
    return (min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]))


def same_tiles(e, j, want, what):
    got = dict(e.tiles(j))
    assert set(got) == set(want), (what, j, sorted(got), sorted(want))
    for c in want:
        if not np.array_equal(got[c], want[c]):
            bad = np.argwhere(got[c] != want[c])
            raise AssertionError(f"{what}: particle {j} tile {c}: {len(bad)} cells differ, first {tuple(bad[0])}: "
                                 f"got {got[c][tuple(bad[0])]}, model {want[c][tuple(bad[0])]}")


def check_hidden(e, j, tiles, ext, what, also=None, need_occupied=True):
    """The structures tiles() does not read, for particle j with the modelled tiles and extent: the written boxes through
    map_extent and render_map (which skips what lies outside them), the occupancy words through the clearance of travel_cost
    (which reads nothing else).  `also`: a box to look at as well, e.g. where the previous owner of the map slot had written.
    `need_occupied`: the scenes of the resample and migration suites are built to hold an occupied cell; a map that a test did
    not build for this check may hold none, and every occupancy word it looks at must then be 0."""
    assert e.map_extent(j) == ext, (what, j, e.map_extent(j), ext)
    look = box_union(ext, also)
    if look is None:
        return
    dim, inv = e.dim, e.dim / TILE
    box = lattice_clip(e, (look[0] - MARGIN, look[1] + MARGIN, look[2] - MARGIN, look[3] + MARGIN))
    got = e.render_map(particle=j, box=box).cells
    want = R.mosaic(tiles, box, dim, TILE)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: render of particle {j} over {box}: {len(bad)} cells differ, first {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]}, model {want[tuple(bad[0])]}")
    clear = T.clearance(R.mosaic(tiles, T.grown_box(box, CLEAR_MAX), dim, TILE), CLEAR_MAX, float(e.cfg.quantum),
                        float(e.cfg.occupied_threshold))
    if ext is not None and need_occupied:
        assert (clear < CLEAR_MAX).any(), (what, j, "no occupied cell: the clearance would say nothing")
    outside = [[(box[1] + 2) / inv, (box[3] + 2) / inv]]                   # no start in the box: no path is searched
    tr = e.travel_cost(outside, particle=j, box=box, clear_max=CLEAR_MAX, through_unknown=True)
    assert tr.clear_max == CLEAR_MAX and tr.clearance.shape == clear.shape
    if not np.array_equal(tr.clearance, clear):
        bad = np.argwhere(tr.clearance != clear)
        raise AssertionError(f"{what}: clearance of particle {j} over {box}: {len(bad)} cells differ, first {tuple(bad[0])}: "
                             f"got {tr.clearance[tuple(bad[0])]}, model {clear[tuple(bad[0])]}")


STEADY = ("ms_", "stamps")                               # counters that are times


def steady(c):
    return {k: v for k, v in c.items() if not k.startswith(STEADY)}


# ---- maps built by map updates -----------------------------------------------------------------------------------------------
FAR = (-120.0, 80.0)                                     # the tile of the extra rasters: on the lattice's rim, negative side
NEAR = (-250, 250, -250, 250)                            # every pose of the scene and every ray's end, in cells of 0.1 m


def extras(P):
    """Particles with one more tile than their poses give them."""
    return [5, 37, 200, P - 3]


def scene_poses(P, rng):
    """One tile (k < 4), two (an edge of the home tile, k = 4 and 7) or four (its corners at +20 and -20 m, k = 5 and 6)."""
    k = np.arange(P) % 8
    xy = rng.uniform(-8.0, 8.0, size=(P, 2))
    jit = rng.uniform(-0.15, 0.15, size=(P, 2))
    xy[k == 4, 0] = 19.5 + jit[k == 4, 0]
    xy[k == 7, 0] = -19.5 + jit[k == 7, 0]
    xy[k == 5] = 19.6 + jit[k == 5]
    xy[k == 6] = -19.6 + jit[k == 6]
    return np.column_stack([xy, rng.uniform(-np.pi, np.pi, P)])


class Scene:
    """An engine whose particles hold different maps with tight written boxes, and its state read back: what the model gets.
    `seed`, `extra` and `lowest` are for scenes smaller than 201 particles, or for two scenes that differ: the generator's seed
    (100 + P), the particles that get a far raster (extras(P)) and the smallest value in those rasters (-30; with 1 a raster
    holds no zero and its written box is the box of its non-zero cells)."""

    def __init__(self, P, weights=None, seed=None, extra=None, lowest=-30):
        self.e = e = make_engine(P)
        self.extra = extras(P) if extra is None else list(extra)
        rng = np.random.default_rng(100 + P if seed is None else seed)
        e.load_map(raster(e, -31, 12, np.full((7, 5), 25, dtype=np.int8)))             # occupied cells in every map
        self.update_poses = scene_poses(P, rng)
        e.set_scan(np.array([2.1, 3.3, 2.7, 3.9, 1.6, 3.1, 2.4, 3.6]), np.arange(8) * (np.pi / 4) + 0.1)
        e.map_update(self.update_poses)
        e.map_update(self.update_poses + np.array([0.25, -0.15, 0.2]))
        ox, oy = R.tile_origin(FAR, e.dim, TILE)
        for n, p in enumerate(self.extra):
            e.load_map(raster(e, ox + 50 + 90 * n, oy + 300 - 70 * n, rng.integers(lowest, 31, size=(20 + n, 30 - n))), particle=p)
        e.set_state(poses=rng.normal(size=(P, 3)), covs=rng.normal(size=(P, 3, 3)),
                    weights=rng.uniform(0.0, 150.0, size=P) if weights is None else weights)
        self.read()

    def read(self):
        e = self.e
        self.poses, self.covs, self.weights = e.poses(), e.covs(), e.weights()
        self.maps = [dict(e.tiles(p)) for p in range(e.P)]
        self.extent = [R.extent(m, e.dim, TILE) for m in self.maps]
        for p in range(e.P):                             # the written boxes are those of the non-zero cells: map_extent can be modelled
            assert e.map_extent(p) == self.extent[p], (p, e.map_extent(p), self.extent[p])
        return self

    def check_is_varied(self):
        counts = {len(m) for m in self.maps}
        assert {1, 2, 4} <= counts, counts
        assert any(c[0] < 0 and c[1] < 0 for m in self.maps for c in m)                 # the negative side
        x = extras(self.e.P)
        assert all(FAR in self.maps[p] for p in x) and sum(FAR in m for m in self.maps) == len(x)
        boxes = {R.written_box(m[(0.0, 0.0)]) for m in self.maps[:64]}
        assert len(boxes) > 32                           # the written boxes differ between particles


# ---- directed box and occupancy-word geometry --------------------------------------------------------------------------------
ANC, DEAD = 3, 7                                         # the ancestor that is copied and the particle whose map slot takes the copy
HOME, POS = (0.0, 0.0), (-40.0, 40.0)


class Loaded:
    """P = 16 particles whose tiles are loaded rasters: the written box of every tile is the raster's box, zeros included."""

    def __init__(self, cs, spec, pool=160):
        self.e = e = make_engine(16, cs=cs, pool=pool)
        self.dim = dim = e.dim
        rng = np.random.default_rng(int(1 / cs))
        self.maps, self.boxes = [], []
        for p in range(16):
            want = spec.get(p, {HOME: (10 + p, 12 + p, 20, 23 + p)})
            tiles, boxes = {HOME: np.zeros((dim, dim), np.int8)}, {HOME: None}
            for c, b in want.items():
                if b is None:
                    assert c == HOME                     # the only tile a particle holds unwritten
                    continue
                vals = rng.integers(-30, 31, size=(b[1] - b[0] + 1, b[3] - b[2] + 1)).astype(np.int8)
                vals[0, 0] = 30                          # occupied
                ox, oy = R.tile_origin(c, dim, TILE)
                e.load_map(raster(e, ox + b[0], oy + b[2], vals), particle=p)
                tiles.setdefault(c, np.zeros((dim, dim), np.int8))[b[0]:b[1] + 1, b[2]:b[3] + 1] = vals
                boxes[c] = b
            self.maps.append(tiles)
            self.boxes.append(boxes)
        rng2 = np.random.default_rng(5)
        e.set_state(poses=rng2.normal(size=(16, 3)), covs=rng2.normal(size=(16, 3, 3)), weights=rng2.uniform(2.0, 9.0, size=16))
        self.poses, self.covs, self.weights = e.poses(), e.covs(), e.weights()
        self.extent = [R.extent(self.maps[p], dim, TILE, self.boxes[p]) for p in range(16)]
        for p in range(16):                              # the engine holds what was meant to be loaded
            same_tiles(e, p, self.maps[p], "as loaded")
            assert e.map_extent(p) == self.extent[p], (p, e.map_extent(p), self.extent[p])

    def copy_anc_over_dead(self, what):
        """Particle ANC twice, particle DEAD not at all: one job.  Everything compared for every particle."""
        e = self.e
        idx = np.array(sorted([p for p in range(16) if p != DEAD] + [ANC]))
        dest = ANC + 1
        assert R.copy_destinations(idx) == [dest]
        c0 = e.counters()
        apply_sources(e, idx)
        c1 = e.counters()
        m = R.move(self.poses, self.covs, self.weights, self.maps, idx, True)
        assert np.array_equal(bits(e.poses()), bits(m.poses)) and np.array_equal(bits(e.covs()), bits(m.covs)), what
        assert np.array_equal(bits(e.weights()), bits(m.weights)), what
        assert c1["tiles_in_use"] == m.tiles_in_use, (what, c1["tiles_in_use"], m.tiles_in_use)
        assert c1["resample_copies"] - c0["resample_copies"] == m.copies == len(self.maps[ANC]), what
        want_bytes = R.copy_bytes(self.boxes[ANC], self.boxes[DEAD], self.dim)
        assert c1["bytes_copied"] - c0["bytes_copied"] == want_bytes, (what, c1["bytes_copied"] - c0["bytes_copied"], want_bytes)
        for j in range(16):
            same_tiles(e, j, m.maps[j], what)
            check_hidden(e, j, m.maps[j], self.extent[idx[j]], what, also=self.extent[DEAD] if j == dest else None)
        self.maps, self.boxes = m.maps, [self.boxes[i] for i in idx]
        self.extent = [self.extent[i] for i in idx]
        self.poses, self.covs, self.weights = m.poses, m.covs, m.weights
        return m, want_bytes


def geometry_cases(dim):
    """name -> (tiles of the ancestor, tiles of the dead particle), written boxes (x0, x1, y0, y1) inclusive in tile cells."""
    d = {POS: (100, 120, 37, 90)}
    s = (60, 70, 100, 110)
    return {
        "cell_at_y0": ({POS: (5, 5, 0, 0)}, d),
        "cell_at_ylast": ({POS: (5, 5, dim - 1, dim - 1)}, d),
        "cell_at_x0": ({POS: (0, 0, 77, 77)}, d),
        "cell_at_xlast": ({POS: (dim - 1, dim - 1, 77, 77)}, d),
        "across_15_16": ({POS: (50, 52, 15, 16)}, {POS: (51, 51, 40, 40)}),
        "across_31_32": ({POS: (50, 52, 31, 32)}, {POS: (51, 51, 40, 40)}),
        "across_383_384": ({POS: (50, 52, 383, 384)}, {POS: (51, 51, 300, 300)}),
        "old_box_contains_new": ({POS: s}, {POS: (40, 90, 70, 150)}),
        "old_box_apart_from_new": ({POS: s}, {POS: (200, 230, 300, 390)}),
        "nothing_written_over_something": ({HOME: None}, {HOME: (30, 60, 33, 95)}),
        "two_allocated_two_released": ({(40.0, -40.0): (3, 9, 380, 399), (40.0, 0.0): (390, 399, 0, 17)},
                                       {(-40.0, 0.0): (0, 40, 31, 32), (-40.0, 40.0): (7, 7, 64, 95), HOME: (1, 2, 3, 4)}),
        "corner_of_the_tile": ({POS: (dim - 10, dim - 1, dim - 15, dim - 1)}, {POS: (0, 3, 0, 40)}),
    }


# ---- the free stack ----------------------------------------------------------------------------------------------------------
def free_positions(tiles):
    return [(40.0 * a, 40.0 * b) for a in range(-3, 4) for b in range(-3, 4) if (40.0 * a, 40.0 * b) not in tiles]


def load_one_cell(ld, p, centre, x, y):
    """A raster of one occupied cell into a lattice position the particle does not hold: takes one tile from the pool."""
    ox, oy = R.tile_origin(centre, ld.dim, TILE)
    ld.e.load_map(raster(ld.e, ox + x, oy + y, np.full((1, 1), 30, np.int8)), particle=p)
    cells = np.zeros((ld.dim, ld.dim), np.int8)
    cells[x, y] = 30
    ld.maps[p], ld.boxes[p] = dict(ld.maps[p]), dict(ld.boxes[p])   # (a copy shares its ancestor's dicts in the model)
    ld.maps[p][centre], ld.boxes[p][centre] = cells, (x, x, y, y)
    ld.extent[p] = R.extent(ld.maps[p], ld.dim, TILE, ld.boxes[p])


def fill_the_pool(ld, n, first=0):
    """n one-cell loads spread over the particles; returns [(particle, centre, x, y)]."""
    made = []
    for k in range(first, first + n):
        p = (5 * k) % 16
        c = free_positions(ld.maps[p])[k % 7]
        load_one_cell(ld, p, c, 7 + k, 390 - 3 * k)
        made.append((p, c, 7 + k, 390 - 3 * k))
    return made
