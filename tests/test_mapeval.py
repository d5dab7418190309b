"""thesis_amd.mapeval on the host: the metric formulas on hand-made scores, the order of rank, spread, and the round trip of
consensus from lattice values through float32 probabilities and back.  No GPU."""
import math
from types import SimpleNamespace

import numpy as np

from thesis_amd import mapeval
from thesis_amd.mapeval import F, O, U, MapScores
from thesis_amd.mapio import MapRaster

CFG = SimpleNamespace(quantum=0.1, min_odds_emp=-3.0, max_odds_occ=3.0)


def made(n, hit_m, hit_r, l1, tab, box=(0, 10, 0, 10), tol=1):
    return MapScores(n=np.array(n, np.int64), hit_m=np.array(hit_m, np.int64), hit_r=np.array(hit_r, np.int64), l1=np.array(l1, np.int64),
                     tab=np.array(tab, np.int64), box=box, tol=tol, quantum=0.1)


def test_metrics_of_one_particle():
    #            reference F   U   O
    s = made([[40, 5, 2],      # map F
              [10, 20, 3],     # map U
              [1, 4, 15]],     # map O
             hit_m=18, hit_r=16, l1=250, tab=3 * 65536 + 32768)
    assert s.n.sum() == s.cells() == 100
    assert s.precision() == 18 / 20 and s.recall() == 16 / 20                # 20 occupied cells on either side
    assert math.isclose(float(s.f1()), 2 * 0.9 * 0.8 / 1.7, rel_tol=1e-15)
    assert s.accuracy() == 55 / 58                                           # known on both sides: 40 + 2 + 1 + 15
    assert s.coverage() == 58 / 71                                           # the reference knows 51 + 20 cells
    assert s.entropy_bits() == 3.5 and s.mean_abs_logodds() == 250 * 0.1 / 100
    assert all(np.asarray(getattr(s, m)()).dtype == np.float64 for m in ("precision", "recall", "f1", "accuracy", "coverage", "entropy_bits", "mean_abs_logodds"))


def test_empty_denominators_are_nan():
    z = np.zeros((3, 3), int)
    unknown = z.copy(); unknown[U, U] = 100
    s = made(unknown, 0, 0, 0, 0)
    for m in ("precision", "recall", "f1", "accuracy", "coverage"):
        assert np.isnan(getattr(s, m)()), m
    assert s.mean_abs_logodds() == 0.0 and s.entropy_bits() == 0.0
    miss = z.copy(); miss[O, U] = 4; miss[U, O] = 6; miss[U, U] = 90           # walls on both sides, none confirmed
    s = made(miss, 0, 0, 0, 0)
    assert s.precision() == 0.0 and s.recall() == 0.0 and np.isnan(s.f1()) and np.isnan(s.accuracy()) and s.coverage() == 0.0
    assert np.isnan(made(z, 0, 0, 0, 0, box=(0, 0, 0, 0)).mean_abs_logodds())


def test_leading_axis_and_from_fields():
    rows = np.arange(3 * 13, dtype=np.int64).reshape(3, 13)
    s = MapScores.from_fields(rows, (-5, 5, 0, 20), 2, 0.1)
    assert s.n.shape == (3, 3, 3) and s.n[1, O, F] == 13 + 6 and s.n[2, F, U] == 27
    assert s.hit_m.tolist() == [9, 22, 35] and s.hit_r.tolist() == [10, 23, 36] and s.l1.tolist() == [11, 24, 37] and s.tab.tolist() == [12, 25, 38]
    assert s.box == (-5, 5, 0, 20) and s.tol == 2 and s.cells() == 200
    assert s.precision().shape == (3,) and s.precision()[0] == 9 / (6 + 7 + 8)
    one = MapScores.from_fields(rows[1], (-5, 5, 0, 20), 2, 0.1)
    assert one.n.shape == (3, 3) and one.recall() == 23 / (15 + 18 + 21)


def test_rank_orders_ties_and_nan():
    n = np.zeros((5, 3, 3), int)
    n[:, O, O] = 10
    s = made(n, hit_m=[5, 10, 5, 0, 10], hit_r=[5, 10, 5, 0, 10], l1=[3, 0, 3, 9, 1], tab=[0] * 5)
    assert mapeval.rank(s).tolist() == [1, 4, 0, 2, 3]                        # f1 1, 1, .5, .5, NaN (0 / 0): ties to the lower index
    assert mapeval.rank(s, "precision").tolist() == [1, 4, 0, 2, 3]           # 0 is a value, not NaN: it still comes last here
    assert mapeval.rank(s, "mean_abs_logodds").tolist() == [1, 4, 0, 2, 3]    # lower is better
    s.hit_m[:] = s.hit_r[:] = [0, 10, 0, 10, 7]                               # f1 NaN, 1, NaN, 1, .7: NaN last wherever it stands
    assert mapeval.rank(s, "f1").tolist() == [1, 3, 4, 0, 2]
    assert mapeval.rank(s).dtype == np.int64


def test_spread():
    n = np.zeros((3, 3, 3), int)
    n[:, F, F] = 50; n[:, O, O] = 10
    same = made(n, [10] * 3, [10] * 3, [0] * 3, [0] * 3)
    assert mapeval.spread(same) == (0.0, 0.0)
    n2 = n.copy(); n2[1, F, O] = 20                                          # particle 1 disagrees on 20 of its 80 known cells
    diff = made(n2, [10] * 3, [10] * 3, [0, 300, 0], [0] * 3)
    sp = mapeval.spread(diff)
    assert math.isclose(sp.disagreement, 0.25 / 3) and math.isclose(sp.mean_abs_logodds, 0.3 / 3)
    sp = mapeval.spread(diff, weights=[0.0, 2.0, 0.0])
    assert math.isclose(sp.disagreement, 0.25) and math.isclose(sp.mean_abs_logodds, 0.3)
    n3 = n.copy(); n3[2] = 0; n3[2, U, U] = 60                                # particle 2 knows nothing: no accuracy, left out of that mean
    sp = mapeval.spread(made(n3, [10, 10, 0], [10, 10, 0], [0, 0, 0], [0] * 3))
    assert sp == (0.0, 0.0)


def test_consensus_round_trip_of_every_lattice_value():
    v = np.arange(-30, 31, dtype=np.int8).reshape(1, 61)
    e = np.exp(v.astype(np.float64) * 0.1)
    prob = (e / (1.0 + e)).astype(np.float32)                                 # what a whole-filter render of one shared map gives
    ras = MapRaster(x0=-3, y0=7, cell_size=0.05, quantum=0.1, dim=800, tile_len=40.0, prob=prob)
    out = mapeval.consensus_from_probability(ras, CFG)
    assert out.cells.dtype == np.int8 and np.array_equal(out.cells, v) and (out.x0, out.y0, out.dim) == (-3, 7, 800)
    assert out.prob is None and out.cells[0, 30] == 0 and prob[0, 30] == 0.5
    # a weighted mean of equal values may be off by a few units in the last place of the float64 sum: still the same value
    wobble = np.nextafter(prob, np.float32(1)), np.nextafter(prob, np.float32(0))
    for p in wobble:
        got = mapeval.consensus_from_probability(MapRaster(x0=0, y0=0, cell_size=0.05, quantum=0.1, dim=800, tile_len=40.0, prob=p), CFG).cells
        assert np.array_equal(got, v)
    # certainty clips to the ends of the lattice
    ends = mapeval.consensus_from_probability(MapRaster(x0=0, y0=0, cell_size=0.05, quantum=0.1, dim=800, tile_len=40.0,
                                                        prob=np.array([[0.0, 1.0]], np.float32)), CFG).cells
    assert ends.tolist() == [[-30, 30]]
