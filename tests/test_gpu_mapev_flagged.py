"""The event-walk kernel's flagged cells (kernels_mapev.hip: flags, hash table, pass counts, fold) against the oracle.

Every case forces RBPF_MAP_KERNEL=ev, applies two consecutive scans to a few particles (the second scan meets non-zero
old values) and compares every tile byte with OracleHybridMap.update and the read-out (get_odds_at) at the scans' end
points and the cells before them - the flagged cells.  The shapes are the smallest that reach each branch of the fold:

  a cell's (beam, end cell / cell before it) pairs are folded from a 64-bit set in registers when they lie within
  FOLD_SPAN = 64 pair ids of each other, i.e. up to 32 consecutive beams per cell; pairs further apart take the
  lists laid out in LDS.

GPU only:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

from tests.helpers import run_map_case

pytestmark = pytest.mark.gpu

FOLD_BEAMS = 32          # consecutive beams per cell that the register fold holds (FOLD_SPAN / 2 in kernels_mapev.hip)


@pytest.fixture()
def ev_engine(monkeypatch):
    """thesis_amd.engine with the event-walk kernel forced (rbpf_create reads RBPF_MAP_KERNEL)."""
    monkeypatch.setenv("RBPF_MAP_KERNEL", "ev")
    from thesis_amd import engine
    return engine


def run_case(engine, poses, scans, angles, cell_size=0.05, pool_tiles=32):
    """tests.helpers.run_map_case with the Python oracle at every size.  Returns the counters."""
    return run_map_case(engine, poses, scans, angles, cell_size=cell_size, pool_tiles=pool_tiles, c_oracle_above=10 ** 9)


def bundle(n, centre, width=2e-4):
    """n beam angles within `width` rad of `centre`: at a few metres their end points share one cell."""
    return centre + np.linspace(-width / 2, width / 2, n)


POSES_4 = [[0.02, 0.03, 0.0], [0.02, 0.03, 0.0], [3.111, -2.222, 1.0], [-1.26, 0.77, -2.0]]


@pytest.mark.parametrize("B,rng_m", [(64, 0.5), (60, 3.0)])
def test_long_lists_take_the_lds_path(ev_engine, B, rng_m):
    """All end points in one cell: one list of B pairs (and one of the cells before it), longer than the register fold
    holds.  64 beams of one direction fit the 8-bit fields' bound (62 per class) only inside the 16-bit block round the
    start cell (0.5 m = 10 cells); 60 beams do at 3 m."""
    ang = bundle(B, 0.3)
    c = run_case(ev_engine, POSES_4, [np.full(B, rng_m), np.full(B, rng_m - 0.004)], ang)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
    assert c["map_event_overflows"] == 0


@pytest.mark.parametrize("per_cell", [FOLD_BEAMS, FOLD_BEAMS + 1])
def test_register_fold_capacity_boundary(ev_engine, per_cell):
    """Two bundles of exactly capacity / capacity + 1 consecutive beams per cell (pair ids 62 / 64 apart)."""
    ang = np.concatenate([bundle(per_cell, 0.3), bundle(per_cell, 1.9)])
    r1 = np.concatenate([np.full(per_cell, 0.5), np.full(per_cell, 2.4)])
    c = run_case(ev_engine, POSES_4, [r1, r1 + 0.003], ang)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]


def test_passes_between_events(ev_engine):
    """A wall seen obliquely from both sides: grazing beams run along the wall's row of cells through the end cells of
    earlier beams (the far half of the fan) and of later ones (the near half) before they end themselves."""
    B = 181
    ang = np.linspace(np.radians(4.0), np.radians(176.0), B)
    wall = 0.52 / np.sin(ang)                                     # the line y = 0.52 m in the sensor frame
    poses = [[0.01, 0.01, 0.0], [0.01, 0.01, 0.0], [5.03, -3.02, 0.7], [-2.51, 4.26, -1.2], [0.03, 0.02, 0.02], [1.0, 1.0, 3.0]]
    c = run_case(ev_engine, poses, [wall, wall + 0.02 * np.cos(7 * ang)], ang)
    assert c["map_events"] > 0
    assert c["window_fallbacks"] == 0 and c["map_event_overflows"] == 0


def test_near_block(ev_engine):
    """Every range below 16 cells: flags and events live in the 16-bit block round the start cell."""
    rng = np.random.Generator(np.random.PCG64(5))
    B = 181
    ang = np.linspace(-2.0, 2.0, B)
    c = run_case(ev_engine, POSES_4, [rng.uniform(0.3, 0.7, B), rng.uniform(0.3, 0.7, B)], ang)
    assert c["map_events"] > 0 and c["window_fallbacks"] == 0


def test_glitched_index_map(ev_engine):
    """The negative side of a tile, where the reference's index formula repeats cells: storage cells with two or four
    source cells."""
    rng = np.random.Generator(np.random.PCG64(6))
    B = 181
    ang = np.linspace(-2.3, 2.3, B)
    poses = [[-12.3, -15.1, 0.3], [-12.3, -15.1, 0.3], [-19.7, -3.3, 2.0], [-9.7, -9.9, -1.0], [-15.0, -19.5, 0.9]]
    c = run_case(ev_engine, poses, [4.5 + 3.0 * np.sin(3 * ang), 3.0 + 2.0 * np.cos(5 * ang) + rng.normal(0, 0.01, B)], ang, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]


def test_strips(ev_engine):
    """0.025 m cells, ranges to 14 m: the fan does not fit one LDS window and is written back in strips of rows."""
    B = 181
    ang = np.linspace(-2.3, 2.3, B)
    poses = [[0.2, -0.1, 0.4], [0.2, -0.1, 0.4], [0.2, -0.1, 0.4], [-6.33, 2.21, -2.0]]
    scans = [9.0 + 5.0 * np.sin(3 * ang), 9.0 + 5.0 * np.cos(2 * ang)]
    c = run_case(ev_engine, poses, scans, ang, cell_size=0.025, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
    assert c["map_windows"] > len(poses) * len(scans)                # more than one window per particle-update


def test_pass_list_overflow_replays_every_flagged_cell(ev_engine):
    """Short random ranges: every beam crosses the end cells of many others, more than the 3072 passes the list keeps.
    The exact replay of every flagged cell takes over."""
    rng = np.random.Generator(np.random.PCG64(7))
    B = 1081
    ang = np.linspace(-2.356, 2.356, B)
    c = run_case(ev_engine, POSES_4, [rng.uniform(0.3, 1.5, B), rng.uniform(0.3, 1.5, B)], ang)
    assert c["map_event_overflows"] > 0
    assert c["slow_cells"] > 0 and c["window_fallbacks"] == 0


def test_partial_groups(ev_engine):
    """0.1 m cells: dim 400, the last 32-cell group of a tile row holds 16 cells."""
    rng = np.random.Generator(np.random.PCG64(8))
    B = 181
    ang = np.linspace(-2.3, 2.3, B)
    poses = [[0.2, -0.1, 0.4], [0.2, -0.1, 0.4], [19.2, 18.7, 0.7], [-19.5, 3.3, 2.5]]
    c = run_case(ev_engine, poses, [6.0 + 4.0 * np.sin(3 * ang), 5.0 + 3.0 * np.cos(4 * ang) + rng.normal(0, 0.02, B)], ang, cell_size=0.1, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
