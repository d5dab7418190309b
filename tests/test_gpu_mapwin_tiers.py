"""The 128x128-window map kernel's buckets (kernels_mapupdate.hip) rung by rung: cap = min(64, max(4, 4096 / nflag)) events
per flagged cell of a window, nbk = min(nflag, NB, 4096 / cap) buckets, NB = min(2 B, 1536) bucket ids; cells of up to 16
events replay in registers, of 17 .. cap are folded by a wave (map_pool_cells), all others - more than cap events, no
bucket, no bucket id - take the exact scan (slow_cells).

Every case forces RBPF_MAP_KERNEL=window and asserts its census precondition first (tests/mapupdate_scenes.py).  The
particles whose index map is a pure offset (the positive side of the home tile) run in one engine: there the census models
the kernel's windows exactly - they start at the fan's first storage row and first 32-cell group of columns - and slow_cells
and map_pool_cells must EQUAL its prediction.  The negative-side particles run in a second engine: where the index formula
repeats cells the fan's first storage row, from which the windows are laid, is less surely the census' one, so there the
prediction is asserted as a lower bound on each counter: slow_cells >= the census' slow cells (more than cap events, no
bucket, no bucket id), map_pool_cells >= its pool cells.  Maps and read-out are compared in both.

Counters seen on an MI355X (slow_cells, map_pool_cells), positive side (4 or 3 particles x 2 scans) / negative side (2 x 2):
  bundle-4, -8: (0, 0) / (0, 0) and (0, 4)     bundle-9: (0, 8) / (0, 4)     bundle-32: (0, 16) / (4, 4)     bundle-33: (8, 8) / (4, 4)
  shallow: (214, 0) / (232, 0)     very-shallow: (5089, 0) / (3300, 0)     more-cells-than-ids: (9936, 0) / (5902, 0)
(the negative side's figures are the census' predictions there too).

GPU only:  python -m pytest tests -m gpu"""
import pytest

from tests import mapupdate_scenes as ms
from tests.helpers import run_map_case

pytestmark = pytest.mark.gpu


@pytest.fixture()
def win_engine(monkeypatch):
    """thesis_amd.engine with the 128x128-window kernel forced (rbpf_create reads RBPF_MAP_KERNEL)."""
    monkeypatch.setenv("RBPF_MAP_KERNEL", "window")
    from thesis_amd import engine
    return engine


def run(engine, case):
    make, pre = ms.WIN_CASES[case]
    pos, neg = ms.split_sides(make())
    pre(pos), pre(neg)
    slow, pool = ms.window_prediction(pos)
    print(case, "positive side: predicted slow, pool =", slow, pool)
    c = run_map_case(engine, pos.poses, pos.scans, pos.angles, cell_size=pos.cs, pool_tiles=pos.pool_tiles)
    assert (c["slow_cells"], c["map_pool_cells"]) == (slow, pool)
    assert c["window_fallbacks"] == 0 and c["map_near_cells"] == 0
    nslow, npool = ms.window_prediction(neg)
    print(case, "negative side: predicted slow, pool =", nslow, npool)
    n = run_map_case(engine, neg.poses, neg.scans, neg.angles, cell_size=neg.cs, pool_tiles=neg.pool_tiles)
    assert n["slow_cells"] >= nslow and n["map_pool_cells"] >= npool
    assert n["window_fallbacks"] == 0 and n["map_near_cells"] == 0
    return slow, pool, len(pos.poses) * len(pos.scans)


@pytest.mark.parametrize("n", [4, 8, 9, 32, 33])
def test_register_and_wave_replay_edges(win_engine, n):
    """One bundle: n and 2 n events: 8 and 16 (the two sorting networks), 18 (a wave), 64 and 66 against cap = 64."""
    slow, pool, PS = run(win_engine, "bundle-%d" % n)                # PS = positive-side particles x scans
    assert (slow, pool) == {4: (0, 0), 8: (0, 0), 9: (0, PS), 32: (0, 2 * PS), 33: (PS, PS)}[n]


def test_shallow_buckets(win_engine):
    """About 300 flagged cells in a window: 12 or 13 events per bucket, dozens of cells above that."""
    slow, pool, PS = run(win_engine, "shallow")
    assert slow >= 5 * PS and pool == 0


def test_very_shallow_buckets(win_engine):
    """More than 1024 flagged cells: cap = 4, and the cells past the 1024th have no bucket."""
    slow, pool, PS = run(win_engine, "very-shallow")
    assert slow > 0


def test_more_flagged_cells_than_bucket_ids(win_engine):
    """1081 beams, more than 1536 flagged cells in one window: the cells past the last bucket id are found by bisection over
    the flag words' prefix counts.  (The engine raises if the kernel reports an error.)"""
    slow, pool, PS = run(win_engine, "more-cells-than-ids")
    assert slow > 0
