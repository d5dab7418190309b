"""The reader and the model of tests/mapupdate_hidden.py against each other, without a GPU: a modelled map goes through
migrate_oracle's own payload() - the wire format the reader decodes on the GPU - and comes back as the model says; a wrong bit,
a short box and a word outside the box's columns are seen.  Also: the two oracles' visited planes are equal."""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import rbpf_oracle as orc
from tests import migrate_oracle as M
from tests import mapupdate_hidden as H

DIM, OW, L, RR = 400, 13, 7, 3
Q, THR = 0.1, M.threshold(0.1, 1.0)
HOME, EAST = (0.0, 0.0), (40.0, 0.0)


def modelled_map():
    """dim 400.  The home tile: a fan's cells in rows 100..140, columns 380..399 (the partial last word), values round the
    threshold; the rim row 100 and the rim column 380 were visited and are 0 again.  The tile east of it: held, never visited."""
    rng = np.random.default_rng(3)
    hm = orc.OracleHybridMap(0.1)
    t = hm.tiles[0]
    assert t.dim == DIM
    t.map[101:141, 381:400] = rng.integers(THR - 2, THR + 3, size=(40, 19)) * Q
    t.map[120, 399], t.map[121, 399], t.map[122, 384] = 3.0, -3.0, (THR + 1) * Q
    t.visited[100:141, 380:400] = True
    assert not t.map[100].any() and not t.map[:, 380].any()
    hm.tiles.append(orc.OracleTile(40, 0, 40, 0.1))
    return hm


def through_the_wire(cells, boxes):
    st = M.State(np.zeros((1, 3)), np.zeros((1, 3, 3)), np.ones(1), [cells], [boxes])
    buf, known, meta = M.payload(st, [0], DIM, OW, THR, L, RR)
    buf = buf.copy()
    buf[~known] = 0xA5                                   # padding and the state block's tail are undefined
    return buf, meta


def test_reader_and_model_agree_on_a_modelled_map():
    hm = modelled_map()
    cells, vis = H.oracle_planes(hm, Q)
    want = H.model_hidden(cells, vis, OW, THR)
    assert want[HOME][0] == (100, 140, 380, 399) and want[EAST][0] is None
    assert want[HOME][1].shape == (41, OW) and want[EAST][1].shape == (0, OW)
    assert want[HOME][1][:, :11].max() == 0 and want[HOME][1][:, 12].max() > 0         # columns outside the box; the half word
    assert not (want[HOME][1][:, 12] >> 16).any()                                      # bits past dim
    assert want[HOME][1][20, 12] >> 15 & 1 == 1 and want[HOME][1][21, 12] >> 15 & 1 == 0
    assert not want[HOME][1][0].any()                                                  # the rim row: visited, all 0
    buf, meta = through_the_wire(cells, {c: b for c, (b, _r) in want.items()})
    got = H.decode(buf, meta, DIM, OW, L, RR)[0]
    H.compare_hidden(got, want, DIM, "modelled map")

    # the box of the non-zero cells is not the model's box: the rim that returned to 0 is missing from it
    from tests import resample_oracle as R
    assert R.written_box(cells[HOME]) == (101, 140, 381, 399)

    flipped = {c: (b, r.copy()) for c, (b, r) in got.items()}
    flipped[HOME][1][7, 12] ^= 1 << 3
    with pytest.raises(AssertionError, match="occupancy words differ, first row 107 word 12"):
        H.compare_hidden(flipped, want, DIM, "one bit")
    stale = {c: (b, r.copy()) for c, (b, r) in got.items()}
    stale[HOME][1][0, 2] = 1                                                           # a word outside y0..y1
    with pytest.raises(AssertionError, match="first row 100 word 2"):
        H.compare_hidden(stale, want, DIM, "outside the columns")
    short = dict(got)
    short[HOME] = ((100, 140, 380, 398), got[HOME][1])
    with pytest.raises(AssertionError, match="written box"):
        H.compare_hidden(short, want, DIM, "a column short")
    past = {c: (b, r.copy()) for c, (b, r) in got.items()}
    past[HOME][1][3, 12] |= 1 << 16                                                    # a bit past dim
    with pytest.raises(AssertionError, match="occupancy words differ"):
        H.compare_hidden(past, want, DIM, "past dim")


def test_other_writers_boxes_are_united_with_the_visited_cells():
    hm = modelled_map()
    cells, vis = H.oracle_planes(hm, Q)
    want = H.model_hidden(cells, vis, OW, THR, written={HOME: (130, 150, 390, 395), EAST: (0, DIM - 1, 0, DIM - 1)})
    assert want[HOME][0] == (100, 150, 380, 399) and want[EAST][0] == (0, DIM - 1, 0, DIM - 1)
    assert want[EAST][1].shape == (DIM, OW) and not want[EAST][1].any()


def test_visited_planes_of_the_two_oracles_are_equal(golden):
    """Scene b of G3 (tests/test_oracle_c.py): per scan and as the union, and the count of Bresenham points."""
    g = golden("G3_map_update")
    cs = float(g["b_cs"])
    py, cm = orc.OracleHybridMap(cs), c_oracle.CMap(c_oracle.load(), cs)
    union, seen = {}, 0
    for p, r in zip(g["b_poses"], g["b_ranges"]):
        sx, sy = orc.scan_xy(r, g["b_angles"])
        py.clear_visited()
        cm.clear_visited()
        py.update(p, sx, sy)
        cm.update(p, sx, sy, ld=False)
        a = {(float(t.cx), float(t.cy)): t.visited for t in py.tiles}
        b = cm.visited()
        assert set(a) == set(b) == set(cm.tiles())
        for c in a:
            assert b[c].dtype == np.uint8 and b[c].max() <= 1
            assert np.array_equal(a[c], b[c] != 0), c
            union[c] = union.get(c, False) | a[c]
        seen += sum(int(v.sum()) for v in a.values())
        assert py.cells_visited == cm.cells_visited > 0
    assert seen > 0
    for t in py.tiles:                                   # every non-zero cell was visited; a visited cell may be 0
        assert not t.map[~union[(float(t.cx), float(t.cy))]].any()
    py.clear_visited()
    cm.clear_visited()
    assert not any(t.visited.any() for t in py.tiles) and not any(v.any() for v in cm.visited().values())
    assert all(np.array_equal(cm.tiles()[(float(t.cx), float(t.cy))], t.map) for t in py.tiles)
