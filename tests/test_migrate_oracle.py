"""tests/migrate_oracle.py against itself and against tests/resample_oracle.py: what the model packs it unpacks to the sender's
tiles, boxes and occupancy words; the bytes follow the closed form; without arrivals arrive() is a local resample."""
import numpy as np
import pytest

from tests import migrate_oracle as M
from tests import resample_oracle as R
from tests.resample_scenes import HOME, geometry_cases

DIM, OW, L, RR, THR = 400, 13, 7, 3, 10


def particle(spec, rng, dim=DIM):
    """(tiles, boxes) as tests/resample_scenes.Loaded models them: random cells over each written box, HOME always held."""
    tiles, boxes = {HOME: np.zeros((dim, dim), np.int8)}, {HOME: None}
    for c, b in spec.items():
        if b is None:
            continue
        vals = rng.integers(-30, 31, size=(b[1] - b[0] + 1, b[3] - b[2] + 1)).astype(np.int8)
        vals[0, 0] = 30
        tiles.setdefault(c, np.zeros((dim, dim), np.int8))[b[0]:b[1] + 1, b[2]:b[3] + 1] = vals
        boxes[c] = b
    return tiles, boxes


def state_of(specs, seed=0):
    rng = np.random.default_rng(seed)
    parts = [particle(s, rng) for s in specs]
    n = len(parts)
    return M.State(rng.normal(size=(n, 3)), rng.normal(size=(n, 3, 3)), rng.uniform(2.0, 9.0, size=n),
                   [p[0] for p in parts], [p[1] for p in parts])


def all_specs():
    cases = geometry_cases(DIM)
    return [s for name in cases for s in cases[name]] + [M.whole_lattice()]


def test_the_threshold_is_the_engines():
    assert M.threshold(0.1, 1.0) == THR


def test_positions_and_centres():
    for pos in range(L * L):
        assert M.position(M.centre_of(pos, L, RR), L, RR) == pos
    assert M.position(HOME, L, RR) == 24 and M.position((-120.0, 80.0), L, RR) == 5


def test_unpacking_the_models_payload_gives_the_senders_particles():
    st = state_of(all_specs())
    leaving = list(range(len(st.maps)))
    buf, known, meta = M.payload(st, leaving, DIM, OW, THR, L, RR)
    raw = M.raw_records(st.maps, st.boxes, leaving, L, RR)
    rows, total = M.meta_rows(raw, DIM, OW)
    assert np.array_equal(rows, meta) and total == len(buf) == M.closed_form_bytes(raw, DIM, OW) and total % 16 == 0
    assert known.sum() < total                           # some padding exists: the mask matters
    noise = np.random.default_rng(1).integers(0, 256, size=total).astype(np.uint8)
    got = M.unpack(np.where(known, buf, noise), meta, DIM, OW, L, RR)              # undefined bytes are not read
    for p, (state, tiles, boxes, words) in enumerate(got):
        want = np.concatenate([st.poses[p], st.covs[p].reshape(9), [st.weights[p]]])
        assert np.array_equal(state.view(np.uint64), want.view(np.uint64))
        assert set(tiles) == set(st.maps[p]) and boxes == st.boxes[p], p
        assert meta[p, 0] == len(tiles)
        for c in tiles:
            assert np.array_equal(tiles[c], st.maps[p][c]), (p, c)
            assert np.array_equal(words[c], M.occupancy_words(st.maps[p][c], OW, THR)), (p, c)
    assert len(got[-1][1]) == 49


def test_occupancy_words_bit_by_bit():
    cells = np.zeros((DIM, DIM), np.int8)
    cells[3, 0], cells[3, 31], cells[3, 32], cells[3, 399], cells[4, 5], cells[5, 6] = 11, 30, 12, 11, 10, -30
    w = M.occupancy_words(cells, OW, THR)
    assert w.shape == (DIM, OW) and w[3, 0] == 1 | 1 << 31 and w[3, 1] == 1 and w[3, 12] == 1 << 15
    assert w.sum() == int(w[3, 0]) + 1 + (1 << 15)       # a value of 10 is not above the threshold


def test_bytes_of_one_tile_by_hand():
    st = state_of([{(-40.0, 40.0): (50, 52, 15, 16)}])
    raw = M.raw_records(st.maps, st.boxes, [0], L, RR)
    rows, total = M.meta_rows(raw, DIM, OW)
    assert total == 128 + 3 * 32 + 3 * 13 * 4 + 4        # three rows of columns [0, 32), their words, padded from 252 to 256
    pos = M.position((-40.0, 40.0), L, RR)
    assert list(rows[0, 2 + 6 * pos:8 + 6 * pos]) == [1, 50, 52, 15, 16, 8] and list(rows[0, :2]) == [2, total // 16]
    assert list(rows[0, 2 + 6 * 24:8 + 6 * 24]) == [1, 0, -1, 0, -1, 24]               # HOME, a later position: held, unwritten, no bytes
    assert list(raw[0, 24]) == [1, M.INT_MAX, -1, M.INT_MAX, -1] and list(raw[0, 0]) == [0] * 5


@pytest.mark.parametrize("did_copy", [False, True])
def test_without_arrivals_arrive_is_a_local_resample(did_copy):
    st = state_of(all_specs()[:8], seed=3)
    idx = np.array([0, 1, 1, 3, 4, 4, 4, 7]) if did_copy else np.arange(8)
    got = M.arrive(st, idx, [], None, [])
    m = R.move(st.poses, st.covs, st.weights, st.maps, idx, True)
    assert np.array_equal(got.poses, m.poses) and np.array_equal(got.covs, m.covs) and np.array_equal(got.weights, m.weights)
    assert all(a is b for a, b in zip(got.maps, m.maps)) and got.tiles_in_use == m.tiles_in_use
    assert got.boxes == [st.boxes[i] for i in idx]


def test_arrivals_are_the_senders_particles():
    a, b = state_of(all_specs()[:8], seed=3), state_of(all_specs()[8:16], seed=4)
    got = M.arrive(b, [0, 2, 2, 5, 6, -1, -1, -1], [5, 6, 7], a, [4, 1, 1])
    assert [got.maps[j] is a.maps[p] for j, p in ((5, 4), (6, 1), (7, 1))] == [True] * 3
    assert np.array_equal(got.poses[5:], a.poses[[4, 1, 1]]) and np.array_equal(got.covs[6], a.covs[1])
    assert np.array_equal(got.poses[:5], b.poses[[0, 2, 2, 5, 6]]) and np.all(got.weights == 1.0)
    assert got.boxes[7] is a.boxes[1] and got.tiles_in_use == sum(len(m) for m in got.maps)
    assert M.extents(got, DIM)[5] == M.extents(a, DIM)[4]
