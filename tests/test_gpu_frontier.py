"""Frontier regions on the GPU (rbpf_frontier_regions, kernels_frontier.hip) against the scalar oracle of
tests/frontier_oracle.py run on the rendered maps: labels, table and counts by equality.  Then labels that travel through every
block, connectivity at block corners, the clearance, the box edge, the selection, every particle at once, what the call leaves
alone, its device outputs and its argument checks, and a view chosen from the regions."""
import ctypes as C

import numpy as np
import pytest

from tests import frontier_oracle as F
from tests.cast_oracle import lattice_bounds
from tests.test_gpu_cast import built_engine, engine, load_room16, raster, rng_state

pytestmark = pytest.mark.gpu

FREE, WALL = -30, 30


def oracle(e, p, box, clear, min_size=1, max_regions=64):
    """(label, regions [max_regions, 10], counts) of the oracle on render_map(p) over the box grown by the margin."""
    grown = e.render_map(p, box=F.grown_box(box, clear)).cells
    return F.regions(grown, tuple(box), clear, min_size, max_regions, float(e.cfg.quantum), float(e.cfg.occupied_threshold))


def table_of(regions):
    """The structured regions as int64 [..., 10]."""
    r = np.ascontiguousarray(regions)
    return r.view(np.int64).reshape(r.shape + (10,))


def same(got, want, what=""):
    """(label, table, counts) equal the oracle's; entries of `got` that are None are skipped."""
    for name, g, ref in zip(("label", "regions", "counts"), got, want):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.shape == ref.shape and g.dtype == ref.dtype, (what, name, g.shape, g.dtype, ref.shape)
        bad = g != ref
        if bad.any():
            k = tuple(int(q) for q in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {name} differs in {int(bad.sum())} of {bad.size} places; first {k}: got {g[k]}, oracle {ref[k]}")


def check(e, p, box, clear, min_size=1, max_regions=64, what=""):
    fr = e.frontier_regions(p, box=box, clearance_cells=clear, min_size=min_size, max_regions=max_regions)
    want = oracle(e, p, box, clear, min_size, max_regions)
    same((fr.label, table_of(fr.regions), fr.counts), want, what or f"box {box} clear {clear}")
    assert fr.box == tuple(box) and fr.regions.dtype.names[0] == "label" and fr.regions.dtype.names[9] == "rep_Y"
    return fr, want


def raw(e, particle, box, clear=0, min_size=1, max_regions=8, flags=0, want=("label", "regions", "counts"), fill=-77):
    """rbpf_frontier_regions itself: (return code, label, regions, counts); outputs not in `want` are passed as NULL, the others
    are prefilled with `fill`."""
    nx, ny = (4, 4) if box is None else (max(int(box[1]) - int(box[0]), 0), max(int(box[3]) - int(box[2]), 0))
    lead = (e.P,) if particle < 0 else ()
    K = max(int(max_regions), 1)
    label = np.full((min(nx, 4096), min(ny, 4096)), fill, np.int32) if "label" in want else None
    regions = np.full(lead + (min(K, 2048), 10), fill, np.int64) if "regions" in want else None
    counts = np.full(lead + (3,), fill, np.int32) if "counts" in want else None
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    b = None if box is None else np.array(box, np.int32)
    rc = e._lib.rbpf_frontier_regions(e._h, particle, None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)), clear, min_size,
                                      max_regions, flags, vp(label), vp(regions), vp(counts))
    return rc, label, regions, counts


def load_cells(e, box, cells, particle=None):
    e.load_map(raster(e, box, np.ascontiguousarray(cells, np.int8)), particle=particle)


# ---- 1. nothing, then a ring ----------------------------------------------------------------------------------------------------
def test_an_unknown_room_has_no_frontier_and_a_disc_has_a_ring():
    e = engine(2)
    load_room16(e)                                       # walls 30 round an interior of 0
    box = e.map_extent(1)
    assert box == (-200, 200, -200, 200)
    fr, _ = check(e, 1, box, 4, what="room16")
    assert fr.counts.tolist() == [0, 0, 0] and np.all(fr.label == -1) and np.all(table_of(fr.regions) == -1)
    ii, jj = np.mgrid[-45:46, -45:46]
    load_cells(e, (-45, 46, -45, 46), np.where(ii * ii + jj * jj <= 40 * 40, FREE, 0), particle=1)
    fr, want = check(e, 1, box, 4, what="disc")
    r = fr.regions[0]
    assert fr.counts[1] == fr.counts[2] == 1 and fr.counts[0] == r["size"] > 200 and r["x_min"] == r["y_min"] == -40 and r["x_max"] == 40
    cx, cy = (2 * r["sum_dx"] + r["size"]) // (2 * r["size"]), (2 * r["sum_dy"] + r["size"]) // (2 * r["size"])
    assert (cx, cy) == (200, 200) and fr.label[cx, cy] == -1                # the centre of the disc: free, but no frontier cell
    ij = np.argwhere(fr.label >= 0)
    d2 = ((ij - [cx, cy]) ** 2).sum(axis=1)
    nearest = ij[d2 == d2.min()]
    assert len(nearest) >= 4 and [r["rep_X"] - box[0], r["rep_Y"] - box[2]] == nearest[0].tolist()     # of the ties, the smallest L
    assert e.frontier_regions(0, box=box).counts.tolist() == [0, 0, 0]    # particle 0 still holds the bare room
    e.close()


# ---- 1b. the rounds: what the host queues, reads and counts ---------------------------------------------
def test_rounds_of_one_block_with_work():
    e = engine(1)
    box = (-30, 30, 5, 65)                                # 60 x 60: one block
    ii, jj = np.mgrid[-25:26, -25:26]
    load_cells(e, (-25, 26, 10, 61), np.where(ii * ii + jj * jj <= 20 * 20, FREE, 0))
    fr, _ = check(e, 0, box, 0, what="disc in one block")
    assert fr.counts[0] > 100 and fr.counts[1:].tolist() == [1, 1]        # a ring: its labels fall to one
    # round 0 changes the block, round 1 runs it and changes nothing, rounds 2 .. 7 of the first read find no dirty block
    assert e.frontier_stats() == {"rounds": 8, "block_runs": 2, "blocks": 1}
    e.close()


def test_rounds_with_nothing_to_do():
    e = engine(1)                                         # no map: not one known cell
    fr = e.frontier_regions(0, box=(0, 100, 0, 100), clearance_cells=0)   # 2 x 2 blocks
    assert fr.counts.tolist() == [0, 0, 0] and np.all(fr.label == -1)
    assert e.frontier_stats() == {"rounds": 8, "block_runs": 0, "blocks": 4}
    e.close()


# ---- 2. a label that has to travel through every block, against the sweeps ---------------------------------------------------------
def serpentine_cells():
    """200 x 150: one-cell-wide free rows at every second x, joined at alternating ends; everything else unknown."""
    c = np.zeros((200, 150), np.int8)
    c[0::2] = FREE
    for k in range(99):
        c[2 * k + 1, 149 if k % 2 == 0 else 0] = FREE
    return c


def test_a_serpentine_across_blocks_and_a_tile_seam():
    e = engine(1)
    h = e.dim // 2
    x0, y0 = -h - 77, -31                                 # negative, no multiple of 64, across the seam X = -h
    cells = serpentine_cells()
    box = (x0, x0 + 200, y0, y0 + 150)
    load_cells(e, box, cells)
    fr, _ = check(e, 0, box, 0, what="serpentine")
    n = int((cells < 0).sum())
    assert fr.counts.tolist() == [n, 1, 1] and np.all(fr.label[cells < 0] == 0)    # every cell of the path is a frontier cell
    stats = e.frontier_stats()
    print(f"serpentine: {stats['rounds']} rounds for {stats['blocks']} blocks, {stats['block_runs']} block runs, {n} cells")
    assert stats["blocks"] == 12 and stats["rounds"] > 12  # no single pass over the box does this
    again = e.frontier_regions(0, box=box, clearance_cells=0)
    assert again.label.tobytes() == fr.label.tobytes() and again.regions.tobytes() == fr.regions.tobytes()
    cut = (x0, x0 + 193, y0, y0 + 150)                    # the last blocks along x are one cell wide
    fr, _ = check(e, 0, cut, 0, what="serpentine, cut box")
    assert fr.counts[1] == 1 and e.frontier_stats()["rounds"] > 12
    cut = (x0, x0 + 193, y0, y0 + 149)                    # the joints at y = 149 are outside: the box clips the path into pieces
    fr, _ = check(e, 0, cut, 0, what="serpentine, clipped")
    assert fr.counts[1] == 49
    for one in ((x0, x0 + 1, y0, y0 + 1), (x0 + 1, x0 + 2, y0, y0 + 1)):   # a single cell: on the path, beside it
        fr, _ = check(e, 0, one, 0, what="1 x 1")
        assert fr.counts.tolist() == ([1, 1, 1] if one[0] == x0 else [0, 0, 0])
    e.close()


# ---- 3. connectivity at block corners ------------------------------------------------------------------------------------------
def test_diagonal_neighbours_across_block_corners():
    e = engine(1)
    h = e.dim // 2
    for x0, y0 in ((5, 7), (-h - 64, h - 128)):           # inside the home tile; the corner of four tiles at block corner (64, 128)
        c = np.zeros((130, 200), np.int8)
        pairs = [((63, 63), (64, 64)), ((63, 128), (64, 127)), ((127, 127), (128, 128)), ((127, 64), (128, 63))]
        for a, b in pairs:
            c[a] = c[b] = FREE
        c[10, 10] = c[10, 12] = FREE                      # two apart: not neighbours
        box = (x0, x0 + 130, y0, y0 + 200)
        load_cells(e, box, c)
        fr, _ = check(e, 0, box, 0, what=f"corners at {(x0, y0)}")
        assert fr.counts.tolist() == [10, 6, 6]
        for a, b in pairs:
            assert fr.label[a] == fr.label[b] == a[0] * 200 + a[1], (a, b)
        assert fr.label[10, 10] == 2010 and fr.label[10, 12] == 2012
        assert fr.regions["size"][:6].tolist() == [2, 2, 2, 2, 1, 1]
    e.close()


# ---- 4. clearance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clear", [0, 4, 16])
def test_clearance_is_a_chebyshev_distance_in_the_real_map(clear):
    e = engine(1, pool_tiles=24, lattice_radius=1)
    h = e.dim // 2
    lo, hi = lattice_bounds(e.dim, 1)
    thr = int(round(float(e.cfg.occupied_threshold) / float(e.cfg.quantum)))
    # (the frontier cell, the side the occupied cell lies on, the box): the occupied cell outside the box within the margin;
    # across the seam X = -h; at the lattice's last cell, where the margin leaves the lattice
    for cell, side, box in (((2, 20), (-1, 1), (0, 40, 0, 40)), ((-h + 1, 30), (-1, -1), (-h - 30, -h + 30, 0, 64)),
                            ((hi - 1, hi - 1), (-1, -1), (hi - 40, hi, hi - 40, hi))):
        area = (cell[0] - 20, cell[0] + 21, cell[1] - 20, cell[1] + 21)
        area = tuple(int(np.clip(v, lo, hi)) for v in area)
        for d, value in ((clear, thr + 1), (clear + 1, thr + 1), (clear, thr)):
            c = np.zeros((area[1] - area[0], area[3] - area[2]), np.int8)
            c[cell[0] - area[0], cell[1] - area[2]] = FREE
            o = (cell[0] + side[0] * d, cell[1] + side[1] * d)
            if d > 0:
                c[o[0] - area[0], o[1] - area[2]] = value
            load_cells(e, area, c)
            fr, _ = check(e, 0, box, clear, what=f"cell {cell} clear {clear} distance {d} value {value}")
            removed = d == clear and value > thr and d > 0
            assert (fr.label[cell[0] - box[0], cell[1] - box[2]] == -1) == removed, (cell, d, value)
            assert fr.counts[0] == (0 if removed else 1)
    e.close()


# ---- 5. the real map decides at the box edge ---------------------------------------------------------------------------------------
def test_a_neighbour_outside_the_box_is_read_from_the_map():
    e = engine(1)
    load_cells(e, (5, 25, 5, 25), np.full((20, 20), FREE, np.int8))
    assert e.map_extent(0) == (5, 25, 5, 25)
    box = (5, 15, 5, 25)                                  # smaller than the extent: row 14 is the box's edge, row 15 is known free
    fr, _ = check(e, 0, box, 0, what="box edge")
    assert np.all(fr.label[0] == 0) and np.all(fr.label[9, 1:19] == -1) and fr.label[9, 0] == 0 and fr.label[9, 19] == 0
    assert fr.counts.tolist() == [20 + 9 + 9, 1, 1]
    e.close()


# ---- 6. selection --------------------------------------------------------------------------------------------------------------
def scattered(nx, ny, step, sizes, seed):
    c = np.zeros((nx, ny), np.int8)
    rng = np.random.default_rng(seed)
    n = 0
    for i in range(0, nx - step + 1, step):
        for j in range(0, ny - step + 1, step):
            c[i, j:j + int(rng.choice(sizes))] = FREE
            n += 1
    return c, n


def test_selection_order_ties_and_null_patterns():
    e = engine(1)
    c, n = scattered(75, 100, 5, (1, 2, 3), 4)
    assert n == 300
    box = (-20, 55, 40, 140)
    load_cells(e, box, c)
    for max_regions in (7, 64, 1024):
        for min_size in (1, 2, 4):
            fr, want = check(e, 0, box, 0, min_size, max_regions, what=f"selection {max_regions} {min_size}")
            kept = int(fr.counts[2])
            sizes, labels = fr.regions["size"][:kept], fr.regions["label"][:kept]
            assert fr.counts[1] == 300 and kept == (0 if min_size == 4 else min(max_regions, int((want[1][:, 1] >= min_size).sum())))
            assert np.all(np.diff(sizes) <= 0) and np.all((np.diff(sizes) < 0) | (np.diff(labels) > 0))
            assert np.all(table_of(fr.regions)[kept:] == -1)
            if max_regions == 7 and min_size == 1:
                assert np.all(sizes == 3) and (want[1][:, 1] == 3).sum() == 7 and (c[:, 2::5] < 0).sum() > 7   # cut inside a tie group
    want = oracle(e, 0, box, 0, 2, 64)
    for pattern in (("label",), ("regions",), ("counts",), ("label", "counts"), ("regions", "counts"), ("label", "regions")):
        rc, label, regions, counts = raw(e, 0, box, 0, 2, 64, want=pattern)
        assert rc == 0, pattern
        same((label, regions, counts), want, f"pattern {pattern}")
    e.close()


def test_more_regions_than_the_selection_holds_at_once():
    e = engine(1)
    c, n = scattered(198, 150, 3, (1, 2, 2), 6)
    assert n == 3300
    box = (-100, 98, -75, 75)
    load_cells(e, box, c)
    for max_regions, min_size in ((1024, 1), (100, 1), (1024, 2), (3, 2)):
        fr, _ = check(e, 0, box, 0, min_size, max_regions, what=f"3300 regions {max_regions} {min_size}")
        assert fr.counts[1] == 3300 and fr.counts[2] == max_regions
    e.close()


# ---- 7. maps the engine built: every particle -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    e = built_engine()
    yield e
    e.close()


def every_particle(e, monkeypatch, oracle_for):
    P, box = e.P, e.map_extent(None)
    allp = e.frontier_regions(None, min_size=3, max_regions=32)
    assert allp.label is None and allp.regions.shape == (P, 32) and allp.counts.shape == (P, 3) and allp.box == box
    one = [e.frontier_regions(p, box=box, min_size=3, max_regions=32) for p in range(P)]
    assert np.array_equal(table_of(allp.regions), np.stack([table_of(f.regions) for f in one]))
    assert np.array_equal(allp.counts, np.stack([f.counts for f in one]))
    for p in oracle_for:
        same((one[p].label, table_of(one[p].regions), one[p].counts), oracle(e, p, box, 4, 3, 32), f"built map, particle {p}")
    monkeypatch.setenv("RBPF_FRONTIER_BATCH", "5")        # 16 particles in four batches
    batched = e.frontier_regions(None, min_size=3, max_regions=32)
    monkeypatch.delenv("RBPF_FRONTIER_BATCH")
    assert batched.regions.tobytes() == allp.regions.tobytes() and np.array_equal(batched.counts, allp.counts)
    return allp


def test_every_particle(built, monkeypatch):
    e = built
    allp = every_particle(e, monkeypatch, range(e.P))
    assert np.all(allp.counts[:, 2] > 0) and len(np.unique(table_of(allp.regions), axis=0)) > 1     # the particles hold different maps
    k = int(np.argmax(e.weights()))
    assert e.frontier_regions("best", box=allp.box, min_size=3, max_regions=32).regions.tobytes() == allp.regions[k].tobytes()


def test_every_particle_after_a_resample_with_duplicates(built, monkeypatch):
    e = built
    w = e.weights()
    w[2] += 400.0
    e.set_state(weights=w)
    did, idx = e.resample()
    assert did and (np.bincount(idx, minlength=e.P) > 1).any()
    allp = every_particle(e, monkeypatch, range(e.P))
    dup = np.nonzero(idx == np.argmax(np.bincount(idx)))[0]
    assert len(dup) > 1 and all(allp.regions[q].tobytes() == allp.regions[dup[0]].tobytes() for q in dup)


def test_a_finer_grid():
    e = engine(2, cs=0.025)
    assert e.dim == 1600
    rng = np.random.default_rng(12)
    c = rng.choice(np.array([0, FREE, FREE, 11, 10], np.int8), size=(150, 170), p=[.3, .4, .27, .01, .02])
    box = (-800 - 70, -800 + 80, 800 - 90, 800 + 80)      # the corner of four tiles
    load_cells(e, box, c, particle=1)
    for clear in (0, 2):
        fr, _ = check(e, 1, box, clear, 2, 128, what=f"0.025 m, clear {clear}")
        assert fr.counts[0] > 100 and fr.counts[2] >= 1
    e.close()


# ---- 8. side effects, device outputs, arguments ---------------------------------------------------------------------------------
def test_a_call_changes_nothing_and_device_outputs_equal_host_outputs(built):
    torch = pytest.importorskip("torch")
    e = built

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.map_extent()) + tuple(e.render_map(p, box=e.map_extent()).cells for p in range(e.P))

    s0 = state()
    a = e.frontier_regions(2, min_size=2)
    b = e.frontier_regions(2, min_size=2)
    allp = e.frontier_regions(None, min_size=2)
    assert a.label.tobytes() == b.label.tobytes() and a.regions.tobytes() == b.regions.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    for x, y in zip(state(), s0):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
    d = e.frontier_regions(2, min_size=2, device=True)
    assert isinstance(d.label, torch.Tensor) and d.label.device.type == "cuda" and d.label.dtype == torch.int32 and d.regions.dtype == torch.int64
    assert np.array_equal(d.label.cpu().numpy(), a.label) and np.array_equal(d.regions.cpu().numpy(), table_of(a.regions))
    assert np.array_equal(d.counts.cpu().numpy(), a.counts)
    dall = e.frontier_regions(None, min_size=2, device=True)
    assert dall.label is None and np.array_equal(dall.regions.cpu().numpy(), table_of(allp.regions)) and np.array_equal(dall.counts.cpu().numpy(), allp.counts)
    s = torch.cuda.Stream()                               # on a borrowed stream that is torch's current one
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = e.frontier_regions(2, min_size=2, device=True)
        ok = torch.equal(d2.label, d.label) and torch.equal(d2.regions, d.regions) and torch.equal(d2.counts, d.counts)
        e.release_stream()
    assert ok


def test_bad_arguments_and_call_order_write_nothing():
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P = 3
    e = engine(P)
    load_room16(e)
    box = (-40, 30, -20, 50)
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))

    def untouched(out, fill=-77):
        return all(a is None or np.all(a == fill) for a in out[1:])

    cases = dict(
        no_box=dict(box=None), no_outputs=dict(want=()), all_with_label=dict(particle=-1, want=("label", "regions", "counts")),
        all_without_outputs=dict(particle=-1, want=()), particle_high=dict(particle=P), particle_low=dict(particle=-2),
        box_reversed=dict(box=(30, -40, -20, 50)), box_empty=dict(box=(0, 0, 0, 10)), box_outside=dict(box=(hi - 5, hi + 1, 0, 10)),
        box_outside_low=dict(box=(0, 10, lo - 1, lo + 5)), clear_negative=dict(clear=-1), clear_large=dict(clear=17),
        min_size_zero=dict(min_size=0), max_regions_zero=dict(max_regions=0), max_regions_large=dict(max_regions=1025), flags=dict(flags=2))
    for name, kw in cases.items():
        args = dict(particle=1, box=box, clear=4, min_size=1, max_regions=8)
        args.update(kw)
        out = raw(e, args.pop("particle"), args.pop("box"), **args)
        assert out[0] == _lib.RBPF_EINVAL, (name, out[0])
        assert untouched(out), name
    assert e._lib.rbpf_frontier_regions(None, 1, None, 4, 1, 8, 0, None, None, None) == _lib.RBPF_EINVAL
    # between the halves of a scan update
    ang, ranges, odo, truth = synthetic.make_log(2, 181)
    e.set_scan(ranges[0], ang)
    e.scan_update_begin(adj=False)
    out = raw(e, 1, box)
    assert out[0] == _lib.RBPF_ESTATE and untouched(out)
    e.scan_update_end()
    out = raw(e, 1, box)                                  # the engine is still usable
    assert out[0] == 0 and not untouched(out)
    out = raw(e, -1, box, want=("regions",))              # with particle -1 either of regions and counts may be NULL
    assert out[0] == 0 and out[2].shape == (P, 8, 10) and not untouched(out)
    with pytest.raises(ValueError):
        e.frontier_regions("worst")
    with pytest.raises(ValueError):
        e.frontier_regions(0, box=(0, 1, 2))
    e.close()


def test_the_cell_limit_in_a_lattice_wide_enough_for_the_box():
    """nx * ny <= 2^27 where nothing else is at fault.  The limit of 32768 cells on a side cannot be met alone: tiles have at most
    4096 cells and the lattice at most 7 tiles on a side, so a longer box leaves every lattice (box_outside above)."""
    from thesis_amd import _lib
    e = engine(1, tile_len_m=200, pool_tiles=2)           # 4000-cell tiles: the lattice is 28000 cells wide
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    assert e.dim == 4000 and hi - lo == 28000
    for box in ((lo, lo + 16385, lo, lo + 8192), (lo, lo + 8192, lo, lo + 16385), (lo, hi, lo, lo + 4794)):    # more than 2^27 cells
        assert (box[1] - box[0]) * (box[3] - box[2]) > 1 << 27
        out = raw(e, 0, box, want=("regions", "counts"))
        assert out[0] == _lib.RBPF_EINVAL and all(np.all(a == -77) for a in out[2:]), box
    for box in ((lo, hi, 0, 1), (0, 1, lo, hi)):          # the longest boxes there are: all unknown
        out = raw(e, 0, box, want=("regions", "counts"))
        assert out[0] == 0 and out[3].tolist() == [0, 0, 0] and np.all(out[2] == -1), box
    e.close()


# ---- 9. a view chosen from the regions ------------------------------------------------------------------------------------------
def test_next_frontier_view_end_to_end(built):
    from thesis_amd import explore
    from thesis_amd.datasets import synthetic
    e = built
    ang = synthetic.beam_angles(91)
    k = int(np.argmax(e.weights()))
    fr = e.frontier_regions(k, min_size=4, labels=False)
    nv = explore.next_frontier_view(e, ang, particle="best", k=6, n_headings=4)
    reps = {(int(r["rep_X"]), int(r["rep_Y"])) for r in fr.regions[:int(fr.counts[2])]}
    inv = e.dim / float(e.cfg.tile_len_m)
    assert 0 < len(nv.poses) <= 6 and all((int(np.floor(x * inv)), int(np.floor(y * inv))) in reps for x, y, _ in nv.poses)
    assert np.array_equal(np.asarray(e.view_gain(nv.poses, ang, particle=k).gain), nv.gain[nv.order])
    assert np.all(np.diff(nv.scores) <= 0) and np.all(nv.size >= 4) and np.all(nv.support == 1.0)
    allv = explore.next_frontier_view(e, ang, particle=None, weights=e.weights() - e.weights().min() + 1.0, k=6, n_headings=4)
    assert allv.gain.shape == (e.P, len(allv.candidates)) and np.all((allv.support > 0) & (allv.support <= 1.0))
    assert np.array_equal(np.asarray(e.view_gain(allv.poses, ang, particle=None).gain), allv.gain[:, allv.order])
    every = e.frontier_regions(None, min_size=4, labels=False)
    reps = {(int(r["rep_X"]), int(r["rep_Y"])) for p in range(e.P) for r in every.regions[p, :int(every.counts[p, 2])]}
    assert all((int(np.floor(x * inv)), int(np.floor(y * inv))) in reps for x, y, _ in allv.poses)
