"""Map scores on the GPU (rbpf_score_maps, kernels_score.hip) against the scalar oracle of tests/score_oracle.py
run on the rendered maps: all 13 fields by equality.  Ragged boxes across tile seams, the halo at every kind of edge, full
counters, a grid whose tile rows end in a partial occupancy word, maps the engine built, many particles, device inputs and
outputs, what the call leaves alone, its argument checks, and thesis_amd.mapeval end to end."""
import ctypes as C

import numpy as np
import pytest

from tests import score_oracle as S
from tests.cast_oracle import lattice_bounds
from tests.test_gpu_cast import built_engine, engine, load_room16, raster, rng_state

pytestmark = pytest.mark.gpu

FREE, WALL = -30, 30
VALUES = np.array([FREE, -4, 0, 0, 3, 10, 11, WALL], np.int8)     # every class, and both sides of the threshold


def table(seed=3):
    return np.random.default_rng(seed).integers(0, (1 << 20) + 1, 61).astype(np.int32)


def oracle(e, p, box, ref, tol, tab):
    """The oracle on render_map(p) over the box grown by tol."""
    grown = e.render_map(p, box=S.grown_box(box, tol)).cells
    return S.scores(grown, tuple(box), ref, tol, tab, float(e.cfg.quantum), float(e.cfg.occupied_threshold),
                    int(round(float(e.cfg.min_odds_emp) / float(e.cfg.quantum))))


def fields(s):
    """A MapScores as the [..., 13] rows of the library."""
    return np.concatenate([s.n.reshape(s.n.shape[:-2] + (9,)), np.stack([s.hit_m, s.hit_r, s.l1, s.tab], axis=-1)], axis=-1)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.int64, (what, got.shape, got.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: fields differ at {bad.tolist()[:8]} ({S.FIELDS}): got {got.tolist()}, oracle {want.tolist()}")


def check(e, p, box, ref, tol, tab, what=""):
    """score_maps equals the oracle; tab None: no table at all, which only the library itself takes (a NULL value_tab)."""
    if tab is None:
        from thesis_amd.mapeval import MapScores
        rc, row = raw(e, p, box, np.ascontiguousarray(ref, np.int8), tol)
        assert rc == 0
        s = MapScores.from_fields(row, box, tol, float(e.cfg.quantum))
    else:
        s = e.score_maps(ref, particle=p, box=box, tol_cells=tol, table=tab)
    want = oracle(e, p, box, ref, tol, tab)
    same(fields(s), want, what or f"particle {p} box {box} tol {tol}")
    assert s.box == tuple(box) and s.tol == tol and s.n.sum() == s.cells()
    return s


def raw(e, particle, box, ref, tol=1, tab=None, flags=0, fill=-77, out=True):
    """rbpf_score_maps itself: (return code, scores prefilled with `fill`)."""
    scores = np.full(((e.P,) if particle < 0 else ()) + (13,), fill, np.int64) if out else None
    b = None if box is None else np.array(box, np.int32)
    rc = e._lib.rbpf_score_maps(e._h, particle, None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)),
                                None if ref is None else C.c_void_p(ref.ctypes.data), tol,
                                None if tab is None else tab.ctypes.data_as(C.POINTER(C.c_int32)), flags,
                                None if scores is None else C.c_void_p(scores.ctypes.data))
    return rc, scores


def load_cells(e, box, cells, particle=None):
    e.load_map(raster(e, box, np.ascontiguousarray(cells, np.int8)), particle=particle)


# ---- 1. a ragged box across a tile seam, partly over cells without a tile -----------------------------------------------------
def test_a_ragged_box_across_tile_seams():
    e = engine(2)
    load_room16(e, particle=1)                            # the tile round the origin
    h = e.dim // 2
    rng = np.random.default_rng(1)
    load_cells(e, (-h - 30, -h + 25, -220, -180), rng.choice(VALUES, size=(55, 40)), particle=1)   # across the seam X = -h
    box = (-h - 70, -h + 247, -h - 50, -h + 250)          # 317 x 300: the tiles with Y < -h do not exist
    assert (box[1] - box[0]) % 64 and (box[3] - box[2]) % 64 and box[0] < -h < box[1] and box[2] < -h < box[3]
    ref = rng.choice(VALUES, size=(box[1] - box[0], box[3] - box[2]), p=[.3, .1, .2, .2, .05, .05, .05, .05])
    tab = table()
    prev = None
    for tol in (0, 1, 5, 16):
        s = check(e, 1, box, ref, tol, tab)
        s0 = check(e, 1, box, ref, tol, None)
        assert s0.tab == 0 and np.array_equal(fields(s0)[:12], fields(s)[:12])
        assert s.n[S.O].sum() > 100 and s.n[S.F].sum() > 100 and s.hit_m > 0
        if tol == 0:
            assert s.hit_m == s.hit_r == s.n[S.O, S.O]
        else:
            assert s.hit_m >= prev.hit_m and s.hit_r >= prev.hit_r
        prev = s
        # particle 0 has no map: the sums of the reference alone
        z = check(e, 0, box, ref, tol, tab)
        cr = S.classes(ref, 0.1, 1.0)
        want_n = np.zeros((3, 3), np.int64)
        want_n[S.U] = [(cr == c).sum() for c in (S.F, S.U, S.O)]
        assert np.array_equal(z.n, want_n) and z.hit_m == z.hit_r == 0 and z.l1 == np.abs(ref.astype(np.int64)).sum()
        assert z.tab == int(tab[30]) * ref.size
    e.close()


# ---- 2. the halo -----------------------------------------------------------------------------------------------------------------
def test_occupied_cells_at_every_kind_of_edge():
    e = engine(1)
    h = e.dim // 2
    box = (-h - 70, -h + 75, 37, 177)                     # 145 x 140; rows 63 | 64 are X = -h - 7 | -h - 6, columns 63 | 64 are Y = 100 | 101
    x0, x1, y0, y1 = box
    walls = [(x0 - 1, 60), (x1, 90), (-h - 40, y0 - 1), (-h + 50, y1), (x0 - 1, y0 - 1), (x0 - 1, y1), (x1, y0 - 1), (x1, y1),   # outside the box
             (x0 + 63, 120), (x0 + 64, 150), (-h - 50, y0 + 63), (-h - 30, y0 + 64),                                             # a block edge
             (-h + 20, 47), (-h + 40, 48),                                                                                       # an occupancy word: (Y + h) % 32 = 31 | 0
             (-h - 1, 70), (-h, 140)]                                                                                            # the tile seam
    assert (47 + h) % 32 == 31 and x0 + 63 == -h - 7
    g = S.grown_box(box, 2)
    cells = np.zeros((g[1] - g[0], g[3] - g[2]), np.int8)
    cells[::7, ::5] = FREE
    for X, Y in walls:
        cells[X - g[0], Y - g[2]] = WALL
    load_cells(e, g, cells)
    for tol in (0, 1, 3, 16):
        ref = np.zeros((x1 - x0, y1 - y0), np.int8)
        for X, Y in walls:                                # reference walls at distance exactly tol and tol + 1, where the box has room
            for RX, RY in ((X + tol, Y), (X - tol - 1, Y), (X, Y - tol), (X, Y + tol + 1), (X - tol, Y + tol), (X + tol + 1, Y - tol - 1)):
                if x0 <= RX < x1 and y0 <= RY < y1:
                    ref[RX - x0, RY - y0] = WALL
        s = check(e, 0, box, ref, tol, None)
        found = int(s.hit_r)
        assert 0 < found < int(s.n[:, S.O].sum())         # some at distance tol are found, some at tol + 1 are not
    # every wall alone, with the reference wall that only a halo read finds: two cells inside the box from a wall outside it
    for X, Y in walls[:8]:
        RX, RY = min(max(X, x0), x1 - 1), min(max(Y, y0), y1 - 1)           # the box cell nearest to the wall
        ref = np.zeros((x1 - x0, y1 - y0), np.int8)
        ref[RX - x0, RY - y0] = WALL
        assert check(e, 0, box, ref, 1, None).hit_r == 1 and check(e, 0, box, ref, 0, None).hit_r == 0
    e.close()


# ---- 3. full counters ----------------------------------------------------------------------------------------------------------
def test_every_cell_in_one_class():
    e = engine(1)
    box = (-100, 30, 200, 270)                            # 130 x 70
    load_cells(e, box, np.full((130, 70), FREE))
    ref = np.full((130, 70), WALL, np.int8)
    tab = table()
    s = check(e, 0, box, ref, 2, tab)
    want = np.zeros((3, 3), np.int64)
    want[S.F, S.O] = 130 * 70
    assert np.array_equal(s.n, want) and s.l1 == 60 * 130 * 70 and s.hit_m == 0 and s.hit_r == 0 and s.tab == int(tab[0]) * 130 * 70
    load_cells(e, box, np.full((130, 70), WALL))
    s = check(e, 0, box, ref, 0, np.full(61, 1 << 20, np.int32))               # the largest table entry in every cell
    assert s.n[S.O, S.O] == s.hit_m == s.hit_r == 130 * 70 and s.l1 == 0 and s.tab == 130 * 70 << 20
    e.close()


# ---- 4. 0.1 m cells: tile rows end in a partial occupancy word ------------------------------------------------------------------
def test_the_coarse_grid():
    e = engine(1, cs=0.1)
    assert e.dim == 400 and e.dim % 32
    rng = np.random.default_rng(4)
    box = (-30, 45, 150, 260)                             # Y = 184 .. 199 is the last, half-used word of a tile row; 200 the next tile
    g = S.grown_box(box, 3)
    load_cells(e, g, rng.choice(VALUES, size=(g[1] - g[0], g[3] - g[2])))
    ref = rng.choice(VALUES, size=(75, 110))
    for tol in (0, 1, 3):
        s = check(e, 0, box, ref, tol, table())
        assert s.hit_m > 0 and s.hit_r > 0
    e.close()


# ---- 5. maps the engine built -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    e = built_engine()
    yield e
    e.close()


def shifted_reference(e):
    """The best particle's map moved by one cell along x and two along y: a reference that is near every map and equals none."""
    box = e.map_extent(None)
    return box, np.ascontiguousarray(np.roll(e.render_map("best", box=box).cells, (1, 2), axis=(0, 1)))


def test_built_maps(built):
    e = built
    assert e.counters()["resample_copies"] > 0
    box, ref = shifted_reference(e)
    tab = table()
    allp = e.score_maps(ref, box=box, tol_cells=1, table=tab)
    rows = fields(allp)
    assert rows.shape == (e.P, 13) and allp.box == box
    for p in range(e.P):
        same(rows[p], oracle(e, p, box, ref, 1, tab), f"built map, particle {p}")
        same(fields(e.score_maps(ref, particle=p, box=box, tol_cells=1, table=tab)), rows[p], f"particle {p} alone")
    assert len(np.unique(rows, axis=0)) > 1               # the particles hold different maps
    again = e.score_maps(ref, box=box, tol_cells=1, table=tab)
    assert fields(again).tobytes() == rows.tobytes()
    k = int(np.argmax(e.weights()))
    same(fields(e.score_maps(raster(e, box, ref), particle="best", tol_cells=1, table=tab)), rows[k], "a MapRaster, the best particle")


def test_exact_duplicates_after_a_resample():
    e = built_engine(P=8, steps=8)
    w = e.weights()
    w[2] += 400.0
    e.set_state(weights=w)
    did, idx = e.resample()
    assert did and (np.bincount(idx, minlength=e.P) > 1).any()
    box, ref = shifted_reference(e)
    rows = fields(e.score_maps(ref, box=box, tol_cells=2))                    # the entropy table
    dup = np.nonzero(idx == np.argmax(np.bincount(idx)))[0]
    assert len(dup) > 1 and all(np.array_equal(rows[q], rows[dup[0]]) for q in dup)
    from thesis_amd.explore import entropy_table
    for p in (int(dup[0]), int(dup[-1])):                 # computed again for every copy, not shared
        same(rows[p], oracle(e, p, box, ref, 2, entropy_table(e.cfg)), f"duplicate {p}")
    e.close()


# ---- 6. many particles --------------------------------------------------------------------------------------------------------------
def test_three_hundred_particles():
    P = 300
    e = engine(P, cs=0.1, pool_tiles=P + 8)
    rng = np.random.default_rng(6)
    box = (-35, 35, -35, 35)                              # 70 x 70: four blocks
    g = S.grown_box(box, 2)
    load_cells(e, g, rng.choice(VALUES, size=(g[1] - g[0], g[3] - g[2])))
    for p in (7, P - 1):
        load_cells(e, (-10, 20, -5, 30), rng.choice(VALUES, size=(30, 35)), particle=p)
    ref = rng.choice(VALUES, size=(70, 70))
    tab = table()
    rows = fields(e.score_maps(ref, box=box, tol_cells=2, table=tab))
    assert rows.shape == (P, 13)
    for p in (0, 7, P - 1):
        same(rows[p], oracle(e, p, box, ref, 2, tab), f"particle {p} of {P}")
    others = np.delete(rows, (7, P - 1), axis=0)
    assert np.all(others == rows[0]) and not np.array_equal(rows[7], rows[0]) and not np.array_equal(rows[7], rows[P - 1])
    e.close()


# ---- 7. device in and out ---------------------------------------------------------------------------------------------------------
def test_device_reference_and_device_scores(built):
    torch = pytest.importorskip("torch")
    from thesis_amd import mapeval
    e = built
    box, ref = shifted_reference(e)
    tab = table()
    host = fields(e.score_maps(ref, box=box, tol_cells=2, table=tab))
    dref = torch.from_numpy(ref).to("cuda")
    assert fields(e.score_maps(dref, box=box, tol_cells=2, table=tab)).tobytes() == host.tobytes()
    d = e.score_maps(dref, box=box, tol_cells=2, table=tab, device=True)
    assert isinstance(d, torch.Tensor) and d.device.type == "cuda" and d.dtype == torch.int64 and tuple(d.shape) == (e.P, 13)
    assert d.cpu().numpy().tobytes() == host.tobytes()
    d1 = e.score_maps(ref, particle=3, box=box, tol_cells=2, table=tab, device=True)
    assert tuple(d1.shape) == (13,) and np.array_equal(d1.cpu().numpy(), host[3])
    s = torch.cuda.Stream()                               # on a borrowed stream that is torch's current one
    with torch.cuda.stream(s):
        e.set_stream(s.cuda_stream)
        d2 = e.score_maps(torch.from_numpy(ref).to("cuda"), box=box, tol_cells=2, table=tab, device=True)
        ok = torch.equal(d2, d)
        e.release_stream()
    assert ok
    k = int(np.argmax(e.weights()))
    ap = mapeval.against_particle(e, "best", tol_cells=1)
    assert ap.n.shape == (e.P, 3, 3) and ap.box == e.map_extent(None)
    assert np.array_equal(ap.n[k], np.diag(np.diag(ap.n[k]))) and ap.l1[k] == 0 and ap.hit_m[k] == ap.hit_r[k] == ap.n[k, S.O, S.O] > 0
    assert (ap.l1 > 0).any()


# ---- 8. what the call leaves alone ------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing(built):
    e = built

    def state():
        return (e.poses(), e.covs(), e.weights(), e.counters(), rng_state(e), e.map_extent()) + tuple(e.render_map(p, box=e.map_extent()).cells for p in range(e.P))

    box, ref = shifted_reference(e)
    s0 = state()
    assert s0[3]["tiles_in_use"] > 0                      # the free-tile count is pool_tiles minus this counter
    e.score_maps(ref, box=box, tol_cells=3)
    e.score_maps(ref, particle=5, box=box, tol_cells=0, table=table())
    for x, y in zip(state(), s0):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)


# ---- 9. arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_call_order_write_nothing():
    torch = pytest.importorskip("torch")
    from thesis_amd import _lib
    from thesis_amd.datasets import synthetic
    P = 3
    e = engine(P)
    load_room16(e)
    box = (-40, 30, -20, 50)
    ref = np.zeros((70, 70), np.int8)
    lo, hi = lattice_bounds(e.dim, int(e.cfg.lattice_radius))
    high, low, tab_neg, tab_big = ref.copy(), ref.copy(), table(), table()
    high[69, 69], low[0, 0], tab_neg[5], tab_big[60] = 31, -31, -1, (1 << 20) + 1
    cases = dict(
        no_box=dict(box=None), no_ref=dict(ref=None), no_scores=dict(out=False), particle_high=dict(particle=P), particle_low=dict(particle=-2),
        box_reversed=dict(box=(30, -40, -20, 50)), box_empty=dict(box=(0, 0, 0, 10)), box_outside=dict(box=(hi - 5, hi + 1, 0, 10)),
        box_outside_low=dict(box=(0, 10, lo - 1, lo + 5)), tol_negative=dict(tol=-1), tol_large=dict(tol=17), flags=dict(flags=4),
        table_negative=dict(tab=tab_neg), table_large=dict(tab=tab_big), ref_high=dict(ref=high), ref_low=dict(ref=low),
        ref_high_all=dict(ref=high, particle=-1))
    for name, kw in cases.items():
        args = dict(particle=1, box=box, ref=ref, tol=1, tab=table())
        args.update(kw)
        rc, out = raw(e, args.pop("particle"), args.pop("box"), args.pop("ref"), **args)
        assert rc == _lib.RBPF_EINVAL, (name, rc)
        assert out is None or np.all(out == -77), name
    assert e._lib.rbpf_score_maps(None, 1, None, None, 1, None, 0, None) == _lib.RBPF_EINVAL
    # a device reference with one value out of range: found on the device, before anything is written
    dev = torch.device("cuda", int(e.cfg.device))
    for particle in (1, -1):
        for bad in (high, low):
            d = torch.from_numpy(bad).to(dev)
            out = torch.full(((P,) if particle < 0 else ()) + (13,), -77, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            b = np.array(box, np.int32)
            for flags in (_lib.RBPF_SCORE_DEVICE_IN, _lib.RBPF_SCORE_DEVICE_IN | _lib.RBPF_SCORE_DEVICE_OUT):
                host_out = np.full(tuple(out.shape), -77, np.int64)
                optr = out.data_ptr() if flags & _lib.RBPF_SCORE_DEVICE_OUT else host_out.ctypes.data
                rc = e._lib.rbpf_score_maps(e._h, particle, b.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(d.data_ptr()), 1, None, flags, C.c_void_p(optr))
                e.synchronize()
                assert rc == _lib.RBPF_EINVAL and np.all(host_out == -77) and bool((out == -77).all())
    with pytest.raises(ValueError):
        e.score_maps(torch.from_numpy(ref).to(dev)[:, :60], box=box)          # a shape that is not the box's
    # between the halves of a scan update
    ang, ranges, odo, truth = synthetic.make_log(2, 181)
    e.set_scan(ranges[0], ang)
    e.scan_update_begin(adj=False)
    rc, out = raw(e, 1, box, ref)
    assert rc == _lib.RBPF_ESTATE and np.all(out == -77)
    e.scan_update_end()
    rc, out = raw(e, 1, box, ref)                         # the engine is still usable; a NULL table is allowed
    assert rc == 0 and out[:9].sum() == 4900 and out[12] == 0
    rc, out = raw(e, -1, box, ref, tol=16, tab=table())
    assert rc == 0 and out.shape == (P, 13) and np.all(out[:, :9].sum(axis=1) == 4900) and np.all(out[:, 12] > 0)
    for bad in (dict(particle="worst"), dict(box=(0, 1, 2)), dict(box=None), dict(table=np.zeros(60, np.int32))):
        kw = dict(box=box)
        kw.update(bad)
        with pytest.raises(ValueError):
            e.score_maps(ref, **kw)
    e.close()


# ---- 10. end to end -------------------------------------------------------------------------------------------------------------------
def test_truth_consensus_and_spread(built):
    from thesis_amd import mapeval
    from thesis_amd.mapio import source_from_raster
    e = engine(4)
    cells, x0, y0 = load_room16(e)
    src = source_from_raster(raster(e, (x0, x0 + cells.shape[0], y0, y0 + cells.shape[1]), cells))
    s = mapeval.against_truth(e, src, tol_cells=0)
    assert s.n.shape == (4, 3, 3) and np.all(s.precision() == 1.0) and np.all(s.recall() == 1.0) and np.all(s.accuracy() == 1.0) and np.all(s.l1 == 0)
    assert mapeval.against_truth(e, src, tol_cells=0, particle=2).precision() == 1.0
    cs = float(e.cfg.cell_size)
    moved = src.moved((cs, cs, 0.0))                      # the same truth, one cell off along both axes
    m0, m1 = mapeval.against_truth(e, moved, tol_cells=0), mapeval.against_truth(e, moved, tol_cells=1)
    assert np.all(m0.precision() < 1.0) and np.all(m0.recall() < 1.0) and np.all(m0.f1() < 1.0) and np.all(m0.l1 > 0)
    assert np.all(m1.precision() == 1.0) and np.all(m1.recall() == 1.0) and np.all(m1.f1() == 1.0)
    con = mapeval.consensus(e)
    one = e.render_map(0, box=e.map_extent(None))
    assert con.cells.dtype == np.int8 and (con.x0, con.y0) == (one.x0, one.y0) and np.array_equal(con.cells, one.cells)
    assert np.array_equal(con.cells[x0 - con.x0:x0 - con.x0 + cells.shape[0], y0 - con.y0:y0 - con.y0 + cells.shape[1]], cells)
    ac = mapeval.against_consensus(e)
    assert mapeval.spread(ac) == (0.0, 0.0) and mapeval.rank(ac).tolist() == [0, 1, 2, 3]
    e.close()
    b = built                                             # maps that differ
    ac = mapeval.against_consensus(b, weights="resample")
    sp = mapeval.spread(ac)
    assert sp.disagreement > 0.0 and sp.mean_abs_logodds > 0.0
    order = mapeval.rank(ac, "f1")
    assert sorted(order.tolist()) == list(range(b.P))
    print(f"built maps against their consensus: spread {sp}; f1 best {ac.f1()[order[0]]:.4f} (particle {order[0]}) worst {ac.f1()[order[-1]]:.4f}; "
          f"precision {np.nanmin(ac.precision()):.4f} .. {np.nanmax(ac.precision()):.4f}, recall {np.nanmin(ac.recall()):.4f} .. {np.nanmax(ac.recall()):.4f}, "
          f"accuracy {np.nanmin(ac.accuracy()):.4f} .. {np.nanmax(ac.accuracy()):.4f}, coverage {np.nanmin(ac.coverage()):.4f} .. {np.nanmax(ac.coverage()):.4f}, "
          f"entropy {ac.entropy_bits().min():.0f} .. {ac.entropy_bits().max():.0f} bits, mean |dl| {ac.mean_abs_logodds().min():.4f} .. {ac.mean_abs_logodds().max():.4f}")
