"""The census of a scan's flagged cells (tests/mapupdate_census.py) against the oracle it restates, and the precondition of every
scene of the GPU tier tests (tests/mapupdate_scenes.py): which rung of the map-update kernels' table ladder a scene reaches is
settled here, on the CPU."""
import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests import mapupdate_census as mc, mapupdate_scenes as ms


def _fan(B, seed, lo, hi):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(lo, hi, B), np.linspace(-2.2, 2.2, B)


@pytest.mark.parametrize("pose,B,lo,hi", [((0.02, 0.03, 0.0), 61, 0.3, 4.0), ((3.111, -2.222, 1.0), 47, 0.2, 0.9),
                                          (ms.NEG, 61, 0.3, 6.0), ((18.7, 19.2, 0.7), 33, 2.0, 16.5)],
                         ids=["home", "short", "negative-side", "tile-border-long-rays"])
def test_replayed_census_is_the_oracle(pose, B, lo, hi):
    """Two scans: the census' operations, applied with the clamped adds, give OracleHybridMap.update cell for cell (the
    second scan on the first one's values), and as many ray-point operations as the oracle's cells_visited."""
    hm = orc.OracleHybridMap(0.05)
    maps, ops = None, 0
    for k in range(2):
        r, a = _fan(B, 40 + k, lo, hi)
        hm.update(pose, *orc.scan_xy(r, a))
        c = mc.census(pose, r, a)
        maps = mc.replay(c, maps)
        ops += c.n_ops - c.n_near_ops
        assert c.n_near_ops == sum(k == mc.NEAR for cell in c.cells.values() for _, k in cell.ops) > 0
        assert sum(x.events for x in c.flagged) + sum(len(x.ops) for x in c.cells.values() if not x.flagged) == c.n_ops
    assert ops == hm.cells_visited
    assert set(maps) == {(t.cx, t.cy) for t in hm.tiles}
    for t in hm.tiles:
        assert np.array_equal(maps[(t.cx, t.cy)], t.map)


def test_negative_side_repeats_cells():
    c = mc.census(ms.NEG, *_fan(61, 40, 0.3, 6.0))
    assert any(len(x.sources) > 1 for x in c.cells.values()) and not ms.regular(c)
    assert ms.regular(mc.census((0.02, 0.03, 0.0), *_fan(61, 40, 0.3, 4.0)))


def test_cell_classes_by_hand():
    """One beam along +x from a cell centre, 20 cells long: end cell and the cell before it on the axis (special), not near;
    8 cells long: near, inside.  Rank and window of the two cells."""
    c = mc.census((0.025, 0.025, 0.0), np.array([1.0]), np.array([0.0]))
    assert c.start == (0, 0) and [x.key for x in c.flagged] == [(0, 0, 419, 400), (0, 0, 420, 400)]
    assert [(x.events, x.hits, x.near, x.special, x.rank) for x in c.flagged] == [(2, 1, False, True, 0), (1, 1, False, True, 1)]
    assert {x.window for x in c.flagged} == {(0, 0, 3, 3)} and c.n_ops == 22 and c.n_near_ops == 1
    c = mc.census((0.025, 0.025, 0.0), np.array([0.4]), np.array([0.0]))
    assert [(x.near, x.inside, x.rim) for x in c.flagged] == [(True, True, False)] * 2
    assert mc.window_tables(c)[c.flagged[0].kwindow] == {"nflag": 2, "cap": 64, "nbk": 2, "NB": 2}


def test_rim_beams_are_what_the_search_finds():
    assert ms.find_rim_beams() == list(ms.RIM_BEAMS)


@pytest.mark.parametrize("case", sorted(ms.RAY_CASES))
def test_ray_scene_reaches_its_rung(case):
    make, pre = ms.RAY_CASES[case]
    scene = make()
    print(case, pre(scene), [mc.summary(c) for c in ms.censuses(scene)[0]])


@pytest.mark.parametrize("case", sorted(ms.WIN_CASES))
def test_window_scene_reaches_its_rung(case):
    make, pre = ms.WIN_CASES[case]
    for side in ms.split_sides(make()):
        pre(side)
        print(case, len(side.poses), "particles: slow, pool =", ms.window_prediction(side))
