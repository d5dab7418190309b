"""What moves a particle between ranks (gather_meta_kernel, pack_kernel, unpack_kernel with its release launch,
export_weights_kernel; layout_packed and the entry points round it in rbpf_api.hip) against the NumPy model of
tests/migrate_oracle.py, everything by equality.

One process, two engines on one device - a sender A and a receiver B - both behind thesis_amd.sharding.EngineShard, in the order
of ShardedResampler._apply: gather_pack_meta on the sender, the records read back, meta_from_raw, pack_raw, apply_local on the
receiver, unpack, one checked call.

a. the records, the meta rows and the payload bytes;  b. what arrives, for every geometry case, through tiles(), map_extent,
render_map and the clearance;  c. an unwritten tile under the next map update;  d. several arrivals beside duplicates, two rounds,
a map update after them, and a rank that sends to itself;  e. a particle that holds the whole lattice;  f. the free stack and its
exhaustion;  g. the weight export;  h. calls that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import migrate_oracle as M
from tests import resample_oracle as R
from tests import travel_oracle as T
from tests.resample_scenes import (ANC, CLEAR_MAX, DEAD, FAR, HOME, NEAR, TILE, Loaded, Scene, bits, check_hidden,
                                   fill_the_pool, free_positions, geometry_cases, load_one_cell, make_engine, raster, same_tiles,
                                   scene_poses, steady, tile_count)

pytestmark = pytest.mark.gpu

_I32 = C.POINTER(C.c_int32)
P = 16


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
def shard(e):
    from thesis_amd.sharding import EngineShard
    return EngineShard(e, 0)


def geom(e):
    """(dim, occupancy words a row, occupied threshold in lattice units, L, R) of an engine."""
    rr = int(e.cfg.lattice_radius)
    return e.dim, (e.dim + 31) // 32, M.threshold(e.cfg.quantum, e.cfg.occupied_threshold), 2 * rr + 1, rr


def model_of(x):
    """The model's state of a Loaded or a Scene (whose written boxes are those of the non-zero cells)."""
    return M.State(x.poses, x.covs, x.weights, list(x.maps), list(getattr(x, "boxes", [None] * P)))


def restate(x, seed):
    """Another pose, covariance and weight for every particle: two engines built alike then differ in them."""
    rng = np.random.default_rng(seed)
    x.e.set_state(poses=rng.normal(size=(P, 3)), covs=rng.normal(size=(P, 3, 3)), weights=rng.uniform(2.0, 9.0, size=P))
    x.poses, x.covs, x.weights = x.e.poses(), x.e.covs(), x.e.weights()
    return x


def send(sa, leaving):
    """Steps 1 to 4 on the sender: (records [n, L*L, 5] as read back, meta rows, payload bytes, payload on the device)."""
    leaving = np.asarray(leaving, dtype=np.int32)
    raw = sa.gather_pack_meta(leaving).cpu().numpy()                                   # the wait
    meta = sa.meta_from_raw(raw, len(leaving))
    nbytes = int(meta[:, 1].astype(np.int64).sum()) * 16
    pay = sa.pack_raw(leaving, raw, nbytes)
    return raw.reshape(len(leaving), -1, 5), meta, nbytes, pay


def queue_receive(sb, new_src, raw, pay):
    """Steps 3, 5 and 6 on the receiver: its own meta rows from the records, apply_local, unpack.  Nothing is waited for."""
    new_src = np.asarray(new_src, dtype=np.int32)
    arrivals = np.nonzero(new_src < 0)[0].astype(np.int32)
    meta = sb.meta_from_raw(raw.reshape(-1), len(arrivals))
    sb.apply_local(new_src, np.arange(P, dtype=np.int32))
    sb.unpack(arrivals, meta, pay)
    return arrivals


def receive(sb, new_src, raw, pay):
    arrivals = queue_receive(sb, new_src, raw, pay)
    sb.e.synchronize()                                   # step 7, a checked call: a device-side error surfaces here
    return arrivals


def compare(e, st, what, also=None):
    """Every particle of the engine against the modelled state; also: {particle: box to look at as well}."""
    also = also or {}
    dim = e.dim
    assert np.array_equal(bits(e.poses()), bits(st.poses)), what
    assert np.array_equal(bits(e.covs()), bits(st.covs)), what
    assert np.array_equal(bits(e.weights()), bits(st.weights)), (what, e.weights(), st.weights)
    assert e.counters()["tiles_in_use"] == st.tiles_in_use, (what, e.counters()["tiles_in_use"], st.tiles_in_use)
    ext = M.extents(st, dim)
    for j in range(P):
        assert tile_count(e, j) == len(st.maps[j]), (what, j)
        same_tiles(e, j, st.maps[j], what)
        check_hidden(e, j, st.maps[j], ext[j], what, also=also.get(j))


def sender_snapshot(e, st, what):
    """What packing must leave alone."""
    compare(e, st, what)
    return bits(e.poses()).copy(), bits(e.covs()).copy(), bits(e.weights()).copy(), steady(e.counters())


def shut(*shards):
    for s in shards:
        e = s.e
        s.close()
        e.close()


# ---- a. records, meta rows and payload ---------------------------------------------------------------------------------------
def check_wire(sa, st, leaving, what):
    """One send of `leaving` against the model; returns (raw, meta, nbytes, payload as numpy)."""
    dim, ow, thr, L, rr = geom(sa.e)
    raw, meta, nbytes, pay = send(sa, leaving)
    want_raw = M.raw_records(st.maps, st.boxes, leaving, L, rr)
    assert np.array_equal(raw[..., 0] >= 0, want_raw[..., 0] == 1), what
    assert np.array_equal(raw[..., 1:], want_raw[..., 1:]), (what, np.argwhere(raw[..., 1:] != want_raw[..., 1:])[:4])
    held = raw[..., 0][raw[..., 0] >= 0]
    assert held.max() < int(sa.e.cfg.pool_tiles)         # pool indices, none twice unless a particle leaves twice
    assert len(set(held.tolist())) == len(held) or len(set(leaving)) < len(leaving)
    want_meta, want_bytes = M.meta_rows(want_raw, dim, ow)
    assert meta.shape == want_meta.shape == (len(leaving), sa.meta_width)
    assert np.array_equal(meta, want_meta), (what, np.argwhere(meta != want_meta)[:6])
    assert nbytes == want_bytes == M.closed_form_bytes(want_raw, dim, ow), (what, nbytes, want_bytes)
    buf, known, _ = M.payload(st, leaving, dim, ow, thr, L, rr)
    got = pay.cpu().numpy()
    assert got.shape == buf.shape
    if not np.array_equal(got[known], buf[known]):
        bad = np.nonzero(known & (got != buf))[0]
        raise AssertionError(f"{what}: {len(bad)} payload bytes differ, first at {bad[0]}: got {got[bad[0]]}, model {buf[bad[0]]}")
    return raw, meta, nbytes, got


@pytest.mark.parametrize("cs", [0.1, 0.05])
def test_records_meta_rows_and_payload_bytes(cs):
    import torch
    from thesis_amd._lib import RBPF_ENOMEM, RBPF_OK
    dim = int(round(TILE / cs))
    cases = geometry_cases(dim)
    names = list(cases)
    assert len(names) == 12
    spec = {k: cases[name][0] for k, name in enumerate(names)}                         # particle k: the ancestor's tiles of case k
    spec[12] = cases["two_allocated_two_released"][1]                                  # three tiles, HOME written
    spec[13] = cases["old_box_contains_new"][1]
    ld = Loaded(cs, spec, pool=40)
    sa, e, st = shard(ld.e), ld.e, model_of(ld)
    before = sender_snapshot(e, st, "before packing")
    for k, name in enumerate(names):
        check_wire(sa, st, [k], f"{name} at {cs}")
    # three particles in one payload, not in index order: the running offsets, and the particle each job reads
    three = [names.index("two_allocated_two_released"), 12, names.index("across_383_384")]
    raw, meta, nbytes, got = check_wire(sa, st, three, f"three particles at {cs}")
    assert list(meta[:, 0]) == [3, 3, 2] and nbytes > 3 * 128
    check_wire(sa, st, [names.index("nothing_written_over_something")] * 2 + [15], f"a particle twice at {cs}")
    # rbpf_pack_particles_raw itself: nothing behind bytes_out is written, and a buffer too small is refused before any launch
    idx = np.asarray(three, dtype=np.int32)
    flat = np.ascontiguousarray(raw.reshape(-1), dtype=np.int32)
    known = M.payload(st, three, *geom(e))[1]            # the padding between tiles is nobody's: it keeps the fill
    for cap, rc_want in ((nbytes + 256, RBPF_OK), (nbytes - 16, RBPF_ENOMEM)):
        dbuf = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
        out = C.c_int64(-1)
        rc = e._lib.rbpf_pack_particles_raw(e._h, idx.ctypes.data_as(_I32), len(idx), flat.ctypes.data_as(_I32),
                                            C.c_void_p(dbuf.data_ptr()), cap, C.byref(out))
        e.synchronize()
        h = dbuf.cpu().numpy()
        assert rc == rc_want, (cap, rc)
        if rc_want == RBPF_OK:
            assert out.value == nbytes and np.all(h[nbytes:] == 0xA5) and np.array_equal(h[:nbytes][known], got[known])
        else:
            assert out.value == 0 and np.all(h == 0xA5)
    after = sender_snapshot(e, st, "after packing")
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3], (before[3], after[3])
    shut(sa)


# ---- b. what arrives ---------------------------------------------------------------------------------------------------------
SOMETHING_OVER_NOTHING = ({HOME: (30, 60, 33, 95)}, {HOME: None})                      # beside geometry_cases: a written tile into an unwritten one


def migrate_cases(dim):
    return dict(geometry_cases(dim), something_written_over_nothing=SOMETHING_OVER_NOTHING)


def branches(src, dst):
    """The branches of unpack_kernel that the 49 lattice positions of one case take (every particle holds HOME)."""
    s, d, out = {HOME: None, **src}, {HOME: None, **dst}, set()
    for c in [(TILE * a, TILE * b) for a in range(-3, 4) for b in range(-3, 4)]:
        if c in s and c in d:
            sb, db = s[c], d[c]
            if sb is None:
                out.add("unwritten over written" if db else "unwritten over unwritten")
            elif db is None:
                out.add("over a tile, old box absent")
            elif db[0] <= sb[0] and sb[1] <= db[1] and db[2] <= sb[2] and sb[3] <= db[3]:
                out.add("over a tile, old box contains the new")
            elif db[0] > sb[1] or sb[0] > db[1] or db[2] > sb[3] or sb[2] > db[3]:
                out.add("over a tile, old box apart from the new")
            else:
                out.add("over a tile, boxes overlap")
        elif c in s:
            out.add("into a newly allocated tile")
        elif c in d:
            out.add("released")
        else:
            out.add("neither side")
    return out


GEOMETRY = ([(cs, name) for cs in (0.1, 0.05) for name in geometry_cases(400)] + [(0.025, "corner_of_the_tile")]
            + [(0.1, "something_written_over_nothing")])
_reached = set().union(*(branches(*migrate_cases(int(round(TILE / cs)))[name]) for cs, name in GEOMETRY))
assert {"over a tile, old box absent", "over a tile, old box contains the new", "over a tile, old box apart from the new",
        "into a newly allocated tile", "released", "neither side", "unwritten over written"} <= _reached, _reached
assert "unwritten over written" in branches(*geometry_cases(400)["nothing_written_over_something"])


def arrival_scene(cs, src, dst, pool_b=48, seed_a=11):
    """A whose particle ANC holds `src`, B whose particle DEAD holds `dst`; the two differ in every particle's state."""
    a = restate(Loaded(cs, {ANC: src}, pool=max(48, 16 + len(src))), seed_a)
    b = Loaded(cs, {DEAD: dst}, pool=pool_b)
    return a, b, shard(a.e), shard(b.e)


ONE_ARRIVAL = np.array([p for p in range(P) if p != DEAD] + [-1])                      # DEAD dies, its slot takes the arrival


def anc_arrives(a, b, sa, sb, what):
    """ANC leaves A, arrives as B's last particle; B compared with the model.  Returns (model of B, bytes sent)."""
    stA, stB = model_of(a), model_of(b)
    raw, meta, nbytes, pay = send(sa, [ANC])
    arrivals = receive(sb, ONE_ARRIVAL, raw, pay)
    assert list(arrivals) == [P - 1]
    m = M.arrive(stB, ONE_ARRIVAL, arrivals, stA, [ANC])
    assert M.extents(m, b.dim)[P - 1] == a.extent[ANC]                                 # the sender's extent, exactly
    compare(b.e, m, what, also={P - 1: b.extent[DEAD]})
    return m, nbytes


@pytest.mark.parametrize("cs,name", GEOMETRY)
def test_what_arrives_is_the_senders_particle(cs, name):
    dim = int(round(TILE / cs))
    src, dst = migrate_cases(dim)[name]
    a, b, sa, sb = arrival_scene(cs, src, dst)
    assert a.dim == b.dim == dim
    m, nbytes = anc_arrives(a, b, sa, sb, f"{name} at {cs}")
    print(f"{name} at {cs}: {len(m.maps[P - 1])} tiles, {nbytes} bytes")
    if name == "two_allocated_two_released":
        assert set(m.maps[P - 1]) == {HOME, (40.0, -40.0), (40.0, 0.0)} and m.tiles_in_use == 15 + 3
    shut(sa, sb)


# ---- c. an unwritten tile stays unwritten ------------------------------------------------------------------------------------
def engine_of(st, cs, pool=64):
    """A fresh engine given the modelled tiles with their written boxes, as loaded rasters."""
    e = make_engine(P, cs=cs, pool=pool)
    for p in range(P):
        for c, b in st.boxes[p].items():
            if b is not None:
                ox, oy = R.tile_origin(c, e.dim, TILE)
                e.load_map(raster(e, ox + b[0], oy + b[2], st.maps[p][c][b[0]:b[1] + 1, b[2]:b[3] + 1]), particle=p)
    return e


def test_an_unwritten_tile_that_arrived_is_unwritten_for_the_next_map_update():
    src, dst = geometry_cases(400)["nothing_written_over_something"]
    a, b, sa, sb = arrival_scene(0.1, src, dst)
    m, _ = anc_arrives(a, b, sa, sb, "unwritten arrival")
    assert m.boxes[P - 1] == {HOME: None} and M.extents(m, 400)[P - 1] is None
    fresh = engine_of(m, 0.1)
    # a short scan round poses a few metres up and right of the tile's middle: the patch lies near cell (240, 250) of HOME
    poses = np.column_stack([np.linspace(3.0, 5.0, P), np.linspace(6.0, 4.0, P), np.linspace(-1.0, 1.0, P)])
    ranges, angles = np.array([1.2, 0.9, 1.5, 1.1, 0.8, 1.4, 1.0, 1.3]), np.arange(8) * (np.pi / 4) + 0.2
    for eng in (b.e, fresh):
        eng.set_scan(ranges, angles)
        eng.map_update(poses)
        eng.map_update(poses)                            # twice: the cells hit twice are occupied, the clearance has something to say
    ext = fresh.map_extent(P - 1)
    assert ext is not None and -150 < ext[0] < ext[1] < 150 and -150 < ext[2] < ext[3] < 150, ext   # a patch, far from cell (0, 0) at -200
    for j in range(P):
        want = dict(fresh.tiles(j))
        assert b.e.map_extent(j) == fresh.map_extent(j), (j, b.e.map_extent(j), fresh.map_extent(j))
        same_tiles(b.e, j, want, "map update after an unwritten arrival")
        check_hidden(b.e, j, want, fresh.map_extent(j), "map update after an unwritten arrival")
    assert not np.array_equal(dict(fresh.tiles(P - 1))[HOME], m.maps[P - 1][HOME])      # the update wrote something
    fresh.close()
    shut(sa, sb)


# ---- d. several arrivals beside duplicates, two rounds, a map update ---------------------------------------------------------
EXTRA = (5, 11)                                          # far-rim rasters: a four-tile and a one-tile particle


def small_scene(seed):
    """Scene at P = 16: extras() names particles up to 200, so the far rasters go to EXTRA, and they hold no zero."""
    sc = Scene(P, seed=seed, extra=EXTRA, lowest=1)
    counts = [len(m) for m in sc.maps]
    assert {1, 2, 4} <= set(counts) and [FAR in m for m in sc.maps] == [p in EXTRA for p in range(P)], counts
    return sc


def one_round(s_from, st_from, leaving, src_from, s_to, st_to, src_to, what):
    """`leaving` go from one engine to the other; the sender fills their places with copies (src_from, no arrivals), the
    receiver takes them beside its own copies (src_to).  The pack is queued before the sender's apply_local.  Both engines
    compared with the model; returns both models."""
    src_from, src_to = np.asarray(src_from), np.asarray(src_to)
    assert not set(leaving) & set(src_from.tolist()) and (src_from >= 0).all() and (src_to < 0).sum() == len(leaving)
    raw, meta, nbytes, pay = send(s_from, leaving)
    s_from.apply_local(src_from, np.arange(P, dtype=np.int32))
    arrivals = receive(s_to, src_to, raw, pay)
    s_from.e.synchronize()
    m_from = M.arrive(st_from, src_from, [], None, [])
    m_to = M.arrive(st_to, src_to, arrivals, st_from, leaving)
    # a copy's or an arrival's slot was some dead particle's: look where those wrote
    compare(s_from.e, m_from, what + ", sender", also={j: NEAR for j in R.copy_destinations(src_from)})
    keep = src_to[src_to >= 0]
    compare(s_to.e, m_to, what + ", receiver", also={j: NEAR for j in R.copy_destinations(keep) + [int(j) for j in arrivals]})
    return m_from, m_to


def test_five_arrivals_beside_duplicates_two_rounds_and_a_map_update():
    a, b = small_scene(1), small_scene(2)
    sa, sb = shard(a.e), shard(b.e)
    stA, stB = model_of(a), model_of(b)
    # round 1, A to B: both far-tile particles, a four-tile, a two-tile and a one-tile particle leave A; on B seven die, two of
    # their slots take copies (of a one-tile and a four-tile particle), five take the arrivals
    leave1 = [5, 2, 11, 6, 12]
    assert sorted(len(stA.maps[p]) for p in leave1) == [1, 2, 2, 4, 5]
    srcA1 = [0, 0, 1, 3, 3, 4, 7, 7, 7, 8, 9, 10, 13, 13, 14, 15]
    srcB1 = [0, 2, 3, 3, 7, 9, 10, 12, 13, 13, 15, -1, -1, -1, -1, -1]
    stA, stB = one_round(sa, stA, leave1, srcA1, sb, stB, srcB1, "round 1")
    assert FAR in stB.maps[11] and FAR in stB.maps[13] and len(stB.maps[14]) == 4
    # round 2, B to A, on top of the permuted slots: an arrival of round 1, a copy of round 1 and its ancestor among the leaving
    leave2 = [11, 3, 2, 15, 0]
    srcB2 = [1, 1, 4, 5, 6, 6, 7, 8, 9, 9, 10, 12, 12, 12, 13, 14]
    srcA2 = [0, 1, 1, 2, 4, 5, 8, 9, 9, 12, 14, -1, -1, -1, -1, -1]
    stB, stA = one_round(sb, stB, leave2, srcB2, sa, stA, srcA2, "round 2")
    # a map update lands in the map the model says each particle has: against fresh engines that were given the modelled tiles
    rng = np.random.default_rng(3)
    ranges, angles = np.array([3.0, 2.2, 3.7, 1.9, 2.8, 3.4, 2.0, 3.1]), np.arange(8) * (np.pi / 4) - 0.3
    for eng, st, what in ((a.e, stA, "A"), (b.e, stB, "B")):
        poses = scene_poses(P, rng)
        fresh = make_engine(P, pool=P * 10)
        for j in range(P):
            for c, cells in st.maps[j].items():
                fresh.set_tile(j, c, cells)
        for x in (eng, fresh):
            x.set_scan(ranges, angles)
            x.map_update(poses)
        changed = 0
        for j in range(P):
            want = dict(fresh.tiles(j))
            same_tiles(eng, j, want, f"map update after two rounds, engine {what}")
            changed += any(c not in st.maps[j] or not np.array_equal(want[c], st.maps[j][c]) for c in want)
        assert changed == P
        fresh.close()
    shut(sa, sb)


def test_a_rank_that_sends_to_itself():
    """Particles 2 and 9 leave and arrive on the same engine, in the slots of others; the pack is queued before apply_local."""
    sc = small_scene(3)
    s, st = shard(sc.e), model_of(sc)
    leaving = [2, 9]
    new_src = np.array([0, 1, 3, 5, 6, 6, 7, 8, 10, 11, 13, 13, 14, 15, -1, -1])       # 4 and 12 die as well
    raw, meta, nbytes, pay = send(s, leaving)
    arrivals = receive(s, new_src, raw, pay)
    m = M.arrive(st, new_src, arrivals, st, leaving)
    compare(sc.e, m, "self-migration", also={j: NEAR for j in (5, 11, 14, 15)})
    assert np.array_equal(bits(m.poses[14]), bits(st.poses[2])) and m.maps[15] is st.maps[9]
    shut(s)


# ---- e. the whole lattice ----------------------------------------------------------------------------------------------------
def test_a_particle_that_holds_the_whole_lattice_arrives():
    src = M.whole_lattice()
    dst = {HOME: (300, 320, 0, 50), (80.0, 80.0): (0, 10, 0, 10)}
    a, b, sa, sb = arrival_scene(0.1, src, dst, pool_b=16 + 1 + 47)                     # B's pool: exactly what the arrival allocates
    assert len(a.maps[ANC]) == 49 and b.e.counters()["tiles_in_use"] == 17
    raw, meta, nbytes, got = check_wire(sa, model_of(a), [ANC], "whole lattice")       # the byte total among the rest
    assert meta[0, 0] == 49 and nbytes > 128 + 49 * 16
    m, nbytes2 = anc_arrives(a, b, sa, sb, "whole lattice")
    assert nbytes2 == nbytes and tile_count(b.e, P - 1) == 49 and m.tiles_in_use == 15 + 49 == b.e.counters()["tiles_in_use"]
    shut(sa, sb)


# ---- f. the free stack and its exhaustion ------------------------------------------------------------------------------------
def adopt(ld, m):
    """The Loaded's own book-keeping after a migration, as the model has it (fill_the_pool reads and extends it)."""
    ld.maps, ld.boxes, ld.extent = list(m.maps), list(m.boxes), M.extents(m, ld.dim)
    ld.poses, ld.covs, ld.weights = m.poses, m.covs, m.weights


def test_the_free_stack_after_an_arrival_allocated_and_released_tiles():
    from thesis_amd.engine import RbpfError
    from thesis_amd._lib import RBPF_ENOMEM
    pool = 40
    src = {(40.0, -40.0): (3, 9, 380, 399), (40.0, 0.0): (390, 399, 0, 17)}
    dst = {(-40.0, 0.0): (0, 40, 31, 32), (-40.0, 40.0): (7, 7, 64, 95), (0.0, 40.0): (100, 140, 100, 140), HOME: (1, 2, 3, 4)}
    a, b, sa, sb = arrival_scene(0.1, src, dst, pool_b=pool)
    e = b.e
    assert e.counters()["tiles_in_use"] == 19
    m, _ = anc_arrives(a, b, sa, sb, "before the pool is filled")                      # two tiles allocated, three released
    assert m.tiles_in_use == 18
    adopt(b, m)
    made = fill_the_pool(b, pool - 18)
    assert e.counters()["tiles_in_use"] == pool
    with pytest.raises(RbpfError) as err:                                              # exactly the free tiles can be had, no more
        load_one_cell(b, 0, free_positions(b.maps[0])[-1], 1, 1)
    assert err.value.code == RBPF_ENOMEM                 # (refused before anything was written: the model did not change)
    # every tile handed out is zero but for its cell - the released ones were wiped in cells and occupancy words - and no tile
    # was handed out twice: every earlier map still reads as before
    inv = b.dim / TILE
    for p in range(P):
        same_tiles(e, p, b.maps[p], "after the pool was filled")
    for p, c, x, y in made:
        ox, oy = R.tile_origin(c, b.dim, TILE)
        box = (ox, ox + b.dim, oy, oy + b.dim)
        clear = T.clearance(R.mosaic(b.maps[p], T.grown_box(box, CLEAR_MAX), b.dim, TILE), CLEAR_MAX,
                            float(e.cfg.quantum), float(e.cfg.occupied_threshold))
        assert (clear == 0).sum() == 1 and clear[x, y] == 0
        tr = e.travel_cost([[(box[1] + 2) / inv, (box[3] + 2) / inv]], particle=p, box=box, clear_max=CLEAR_MAX, through_unknown=True)
        assert np.array_equal(tr.clearance, clear), (p, c, np.argwhere(tr.clearance != clear)[:4])
    assert e.counters()["tiles_in_use"] == pool
    shut(sa, sb)


def full_pool_scene(free, release):
    """A receiver with `free` free tiles in which the arrival of A's ANC allocates one tile; with `release` DEAD also holds a
    tile that the arrival does not, which the unpack gives up."""
    src, dst = {(40.0, 0.0): (5, 9, 5, 9)}, ({(-40.0, 0.0): (7, 8, 7, 8)} if release else {})
    used = 16 + len(dst)
    a, b, sa, sb = arrival_scene(0.1, src, dst, pool_b=used + 3 + free)
    fill_the_pool(b, 3)
    assert b.e.counters()["tiles_in_use"] == used + 3 == int(b.e.cfg.pool_tiles) - free
    return a, b, sa, sb


@pytest.mark.parametrize("release", [False, True])
def test_an_arrival_needs_as_many_free_tiles_as_it_allocates(release):
    """Exhaustion is an error code at the next checked call, never silent - also when the same unpack releases a tile: released
    tiles return to the stack only after the kernel, so the net number of tiles does not count."""
    from thesis_amd.engine import RbpfError
    from thesis_amd._lib import RBPF_ENOMEM
    a, b, sa, sb = full_pool_scene(0, release)
    raw, meta, nbytes, pay = send(sa, [ANC])
    queue_receive(sb, ONE_ARRIVAL, raw, pay)
    with pytest.raises(RbpfError) as err:
        b.e.synchronize()
    assert err.value.code == RBPF_ENOMEM
    shut(sa, sb)                                         # the maps are incomplete: nothing more is asked of this engine
    a, b, sa, sb = full_pool_scene(1, release)           # one free tile is enough, and then everything is as modelled
    anc_arrives(a, b, sa, sb, f"one free tile, release {release}")
    assert b.e.counters()["tiles_in_use"] == int(b.e.cfg.pool_tiles) - (1 if release else 0)
    shut(sa, sb)


# ---- g. the weight export ----------------------------------------------------------------------------------------------------
def test_the_weight_export_scatters_to_the_global_ids():
    """The owned entries are the weights, bit for bit.  Every other entry of the n_global is +0.0: the call zeroes the vector
    (include/rbpf_hip.h) so that the ranks' vectors can be summed.  What lies behind the n_global entries keeps the sentinel."""
    import torch
    n_global, sentinel = 40, -12345.678
    e = make_engine(P)
    s = shard(e)
    rng = np.random.default_rng(40)
    ids = rng.permutation(n_global)[:P].astype(np.int32)
    w = rng.uniform(-700.0, 50.0, size=P)
    assert len(set(ids.tolist())) == P and len(set(w.tolist())) == P and not np.array_equal(ids, np.sort(ids))
    e.set_state(weights=w)
    s.set_global_ids(ids)
    t = torch.full((n_global + 8,), sentinel, dtype=torch.float64, device="cuda:0")
    e._check(e._lib.rbpf_export_weights(e._h, C.c_void_p(t.data_ptr()), n_global))
    e.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(bits(got[ids]), bits(w))
    others = np.setdiff1d(np.arange(n_global), ids)
    assert len(others) == 24 and np.all(bits(got[others]) == 0), got[others]
    assert np.array_equal(bits(got[n_global:]), bits(np.full(8, sentinel)))
    assert np.array_equal(bits(e.weights()), bits(w))
    shut(s)


# ---- h. calls that launch nothing --------------------------------------------------------------------------------------------
def test_no_particle_and_indices_out_of_range_launch_nothing():
    import torch
    from thesis_amd._lib import RBPF_EINVAL, RBPF_OK
    ld = Loaded(0.1, {ANC: {(40.0, 0.0): (5, 9, 5, 9)}}, pool=24)
    e, s, st = ld.e, shard(ld.e), model_of(ld)
    lib, h = e._lib, e._h
    raw, meta, nbytes, pay = send(s, [ANC])              # a valid record, row and payload for the calls below
    e.synchronize()
    before = sender_snapshot(e, st, "before the refused calls")
    nb, out = C.c_int64(-1), C.c_int64(-1)
    assert lib.rbpf_gather_pack_meta(h, None, 0, None) == RBPF_OK
    assert lib.rbpf_meta_from_raw(h, None, 0, None, C.byref(nb)) == RBPF_OK and nb.value == 0
    assert lib.rbpf_pack_particles_raw(h, None, 0, None, None, 0, C.byref(out)) == RBPF_OK and out.value == 0
    assert lib.rbpf_unpack_particles(h, None, 0, None, None) == RBPF_OK
    flat = np.ascontiguousarray(raw.reshape(-1), dtype=np.int32)
    row = np.ascontiguousarray(meta, dtype=np.int32)
    d_raw = torch.full((s.raw_width,), -7, dtype=torch.int32, device="cuda:0")
    d_buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    for bad in (-1, P):
        idx = np.array([bad], dtype=np.int32)
        ip = idx.ctypes.data_as(_I32)
        assert lib.rbpf_gather_pack_meta(h, ip, 1, C.c_void_p(d_raw.data_ptr())) == RBPF_EINVAL
        out = C.c_int64(-1)
        assert lib.rbpf_pack_particles_raw(h, ip, 1, flat.ctypes.data_as(_I32), C.c_void_p(d_buf.data_ptr()), nbytes,
                                           C.byref(out)) == RBPF_EINVAL and out.value == 0
        assert lib.rbpf_unpack_particles(h, ip, 1, C.c_void_p(pay.data_ptr()), row.ctypes.data_as(_I32)) == RBPF_EINVAL
    e.synchronize()
    assert torch.all(d_raw == -7).item() and torch.all(d_buf == 0xA5).item()
    after = sender_snapshot(e, st, "after the refused calls")
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3], (before[3], after[3])
    shut(s)
