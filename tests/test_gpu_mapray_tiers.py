"""The global-index map kernel's table ladder (kernels_mapray.hip) rung by rung: per-pair lists of ECAP = 16 events, the pool
of NPOOL = 48 lists of PCAP = 64, the slow list of RSLOW = 256 cells, the NNEAR = 128 cells of the block round the start
cell with NSPC = 32 hits each, the rim of that block, the RSPEC = 512 special pairs, the two tiers of the 8-bit counter
bound HIT_BOUND = 63, and the give-backs when a table is full.

Every case forces RBPF_MAP_KERNEL=ray, first asserts on the CPU census (tests/mapupdate_census.py, the cases of
tests/mapupdate_scenes.py) that its scene reaches the rung, then applies two scans to 4 - 5 particles and compares every
tile byte and the read-out at the flagged cells with the oracle (tests/helpers.run_map_case), then the counters that show
which rung ran.  PS = particles x scans below.

Counters seen on an MI355X (the tests print them), 5 particles x 2 scans unless noted, slow / pool / near = slow_cells /
map_pool_cells / map_near_cells:
  ecap-7, -8: pool 2 (the negative-side particle: 21 / 24 events)     ecap-9, -15: pool 10     ecap-16, -17: pool 20
  pcap-31, -32: slow 2, pool 18     pcap-33: slow 10, pool 10         pool-56: slow 80, pool 480     pool-40: pool 400
  near-60: near 1030                near-hits-32: near 20             near-hits-33: slow 20
  near-300: slow 2326, near 1280    slow-full-720: fallback_tables 10 = window_fallbacks     rim: slow 12, near 70
  special-8x8 (4 particles): all 0  special-8x44 (4 particles): fallback_tables 8 = window_fallbacks
  bound-63: slow 10, pool 10        bound-64: fallback_bound 10 = window_fallbacks            bound-two-tier: slow 30, pool 10
  strips-pool (4 particles): map_windows 64, slow 91, pool 384

GPU only:  python -m pytest tests -m gpu"""
import pytest

from tests import mapupdate_census as mc, mapupdate_scenes as ms
from tests.helpers import run_map_case

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ray_engine(monkeypatch):
    """thesis_amd.engine with the global-index kernel forced (rbpf_create reads RBPF_MAP_KERNEL)."""
    monkeypatch.setenv("RBPF_MAP_KERNEL", "ray")
    from thesis_amd import engine
    return engine


def run(engine, case):
    make, pre = ms.RAY_CASES[case]
    scene = make()
    fig = pre(scene)                                                  # the rung is reached: proven on the census
    c = run_map_case(engine, scene.poses, scene.scans, scene.angles, cell_size=scene.cs, pool_tiles=scene.pool_tiles)
    return c, fig, len(scene.poses) * len(scene.scans)


@pytest.mark.parametrize("n", [7, 8, 9, 15, 16, 17])
def test_pair_list_capacity(ray_engine, n):
    """One bundle of n far beams: lists of n and 2 n events, 14 / 16 / 18 and 15 / 16 / 17 against ECAP; the longer ones
    move to a pool list (on the negative side the repeated cells make 3 n of 2 n)."""
    c, fig, PS = run(ray_engine, "ecap-%d" % n)
    assert c["window_fallbacks"] == 0
    if n >= 9:
        assert fig["gt16"] >= PS and c["map_pool_cells"] + c["slow_cells"] >= fig["gt16"]
    if n in (9, 17):
        assert c["map_pool_cells"] >= PS


@pytest.mark.parametrize("n", [31, 32, 33])
def test_pool_list_capacity(ray_engine, n):
    """62 / 64 / 66 events against PCAP: 66 go to the scan over all beams; the end cell's n events fold from the pool."""
    c, fig, PS = run(ray_engine, "pcap-%d" % n)
    assert c["window_fallbacks"] == 0 and c["map_pool_cells"] >= PS
    if n == 33:
        assert c["slow_cells"] >= PS


def test_pool_exhausted(ray_engine):
    """56 cells of 18 events, 48 pool lists: at least 8 per particle and scan take the scan over all beams."""
    c, fig, PS = run(ray_engine, "pool-56")
    assert fig["beyond_pool"] == PS * (56 - mc.NPOOL)
    assert c["slow_cells"] >= fig["beyond_pool"] and c["map_pool_cells"] >= 1 and c["window_fallbacks"] == 0


def test_pool_nearly_exhausted(ray_engine):
    """40 such cells: pairs that turn out not to own their cell can draw pool lists too, so some owners may go without."""
    c, fig, PS = run(ray_engine, "pool-40")
    assert fig["gt16"] == 40 * PS and c["map_pool_cells"] + c["slow_cells"] >= fig["gt16"] and c["window_fallbacks"] == 0


def test_near_block_fold(ray_engine):
    """60 short beams: at most NNEAR flagged cells, all inside the block: folded from the block's second walk."""
    c, fig, PS = run(ray_engine, "near-60")
    assert c["map_near_cells"] > 0 and c["slow_cells"] == 0 and c["window_fallbacks"] == 0


def test_near_cell_hits_at_capacity(ray_engine):
    """32 beams end in one cell 10 cells out: 32 occupied hits there, 32 nearby ones before it: NSPC holds them."""
    c, fig, PS = run(ray_engine, "near-hits-32")
    assert c["map_near_cells"] >= PS and c["window_fallbacks"] == 0


def test_near_cell_hits_beyond_capacity(ray_engine):
    """33 of them: the scan over all beams."""
    c, fig, PS = run(ray_engine, "near-hits-33")
    assert c["slow_cells"] >= PS and c["window_fallbacks"] == 0


def test_near_cells_beyond_the_block_list(ray_engine):
    """More than NNEAR cells inside the block (300 short beams): the rest goes to the slow list, which holds them."""
    c, fig, PS = run(ray_engine, "near-300")
    assert fig["beyond_near"] >= PS and c["slow_cells"] >= fig["beyond_near"] and c["map_near_cells"] > 0 and c["window_fallbacks"] == 0


def test_slow_list_full_hands_back_untouched(ray_engine):
    """720 short beams: more cells than block list and slow list hold together.  Every particle is handed to the window
    kernel; a byte written before that would be applied twice."""
    c, fig, PS = run(ray_engine, "slow-full-720")
    assert c["fallback_tables"] == PS and c["window_fallbacks"] == PS


def test_rim_cells(ray_engine):
    """A storage cell with one source inside the block's walk and one on its rim: straight to the scan over all beams, every
    one of them (kernels_mapray.hip: a near cell that is not `inside` takes no place in the block's list).  Only the particle
    at RIM_POSE has such cells; the counters are sums over all particles, so that it is THAT particle's rim cells which went
    there rests on the census precondition and on the maps being exact."""
    c, fig, PS = run(ray_engine, "rim")
    assert fig["with_rim"] >= 2 and c["slow_cells"] >= fig["rim_cells"] >= fig["with_rim"] and c["window_fallbacks"] == 0


def test_special_cells(ray_engine):
    """Cells on the axes and diagonals through the start cell, which rays of other direction classes reach: the dense
    second pass; 8 directions x 8 beams fit the special list, and no such cell has more than ECAP events.  No counter
    tells that the second pass ran (all of them stay 0 here): that these cells take it rests on the census precondition -
    every far flagged cell is special, none has a long list - and its result is checked by the maps and the read-out."""
    c, fig, PS = run(ray_engine, "special-8x8")
    assert c["window_fallbacks"] == 0


def test_special_list_full(ray_engine):
    """More than RSPEC special pairs: handed back, maps exact."""
    c, fig, PS = run(ray_engine, "special-8x44")
    assert c["fallback_tables"] == PS and c["window_fallbacks"] == PS


def test_counter_bound_first_tier_holds(ray_engine):
    c, fig, PS = run(ray_engine, "bound-63")
    assert c["fallback_bound"] == 0 and c["window_fallbacks"] == 0 and c["slow_cells"] >= PS      # 126 events


def test_counter_bound_fails(ray_engine):
    c, fig, PS = run(ray_engine, "bound-64")
    assert c["fallback_bound"] == PS and c["window_fallbacks"] == PS


def test_counter_bound_second_tier_holds(ray_engine):
    """240 rays in the slope buckets of one cell, 40 of them long enough to reach an 8-bit field."""
    c, fig, PS = run(ray_engine, "bound-two-tier")
    assert c["fallback_bound"] == 0 and c["window_fallbacks"] == 0


def test_tiers_under_strips(ray_engine):
    """0.025 m cells, bundles at 9 - 14 m: the fan is written back in strips, the pool runs out as above."""
    c, fig, PS = run(ray_engine, "strips-pool")
    assert c["map_windows"] > PS
    assert fig["beyond_pool"] >= PS * (56 - mc.NPOOL)
    assert c["slow_cells"] >= fig["beyond_pool"] and c["map_pool_cells"] >= 1 and c["window_fallbacks"] == 0
