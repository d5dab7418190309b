"""The event-walk kernel's resident workgroups (kernels_mapev.hip): a workgroup runs one particle after the other, taking the
next one from a queue word, so the static LDS words, the window and the queue are reused from particle to particle and from
launch to launch.

Every case forces RBPF_MAP_KERNEL=ev and goes through tests/test_gpu_mapev_flagged.py::run_case: two scans (two launches on one
engine: the queue re-arms itself in between), every tile byte and the read-out at the flagged cells against
OracleHybridMap.update.  RBPF_EV_GRID = 1 or 2 caps the resident workgroups, so one workgroup runs several particles in a
row - with one workgroup in the order of their numbers - and each case puts a particle that leaves the kernel early or takes
another path right in front of one that does not.  The same case with RBPF_EV_RESIDENT=0 (one workgroup per particle) runs once
per case; its tiles equal the oracle's byte for byte as well, so the two launch shapes' tiles are equal, and their counters
(fallbacks and their reasons included) are compared here.

GPU only:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests.test_gpu_mapev_flagged import bundle, run_case

pytestmark = pytest.mark.gpu

GRIDS = [1, 2]
_one_per_particle = {}       # case name -> counters of the RBPF_EV_RESIDENT=0 run


def counts(c):
    """Every counter that is not a time (the phase stamps are zero in a product build)."""
    return {k: v for k, v in c.items() if not k.startswith("ms_") and k != "stamps"}


def both_shapes(monkeypatch, name, grid, **case):
    """run_case with resident workgroups (capped at `grid`; None: as many as particles or CUs) and, once per case, with one
    workgroup per particle; the counters must agree, and the event walk must have been launched with the workgroups the
    setting asks for (every case has at most 8 particles, fewer than any device has CUs).  Returns the resident run's counters."""
    from thesis_amd import engine
    launched = []
    close = engine.ParticleEngine.close

    def close_and_note(self):
        launched.append(self.map_update_workgroups())       # of the engine's last map update
        close(self)

    monkeypatch.setattr(engine.ParticleEngine, "close", close_and_note)
    monkeypatch.setenv("RBPF_MAP_KERNEL", "ev")
    P = len(case["poses"])
    if name not in _one_per_particle:
        monkeypatch.setenv("RBPF_EV_RESIDENT", "0")
        monkeypatch.delenv("RBPF_EV_GRID", raising=False)
        _one_per_particle[name] = counts(run_case(engine, **case))
        assert launched == [P]
        del launched[:]
    monkeypatch.setenv("RBPF_EV_RESIDENT", "1")
    if grid is None:
        monkeypatch.delenv("RBPF_EV_GRID", raising=False)
    else:
        monkeypatch.setenv("RBPF_EV_GRID", str(grid))
    c = counts(run_case(engine, **case))
    assert launched == [min(P, grid) if grid else P]        # the cap took effect: a workgroup ran several particles in a row
    assert c == _one_per_particle[name]
    return c


def fan(B, lo=-2.0, hi=2.0):
    return np.linspace(lo, hi, B)


def room_scans(B, seed):
    """Two scans of a few metres: the second meets the first one's values."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ang = fan(B)
    return [3.0 + 1.5 * np.sin(3 * ang), 2.5 + 1.2 * np.cos(4 * ang) + rng.normal(0, 0.01, B)], ang


@pytest.mark.parametrize("grid", GRIDS)
def test_off_home_tile_then_normal(monkeypatch, grid):
    """Particles 0, 2 and 5 stand where they hold no tile (hybridmap.py:98-100: the update does nothing and the workgroup
    returns before the particle's first barrier); the one behind each of them is a normal one."""
    scans, ang = room_scans(97, 11)
    poses = [[27.0, 3.0, 0.5], [0.31, -0.22, 0.4], [-3.0, 31.5, -1.0], [2.13, 1.07, 2.0], [-1.4, 0.6, -2.5], [25.5, -26.0, 0.1],
             [0.31, -0.22, 0.4]]
    c = both_shapes(monkeypatch, "off_home", grid, poses=poses, scans=scans, angles=ang)
    assert c["window_fallbacks"] == 0 and c["map_windows"] == 4 * len(scans)      # only the four particles on their tiles walk


@pytest.mark.parametrize("grid", GRIDS)
def test_give_back_then_normal(monkeypatch, grid):
    """70 beams on one line, 1 m long.  Along an axis they are 20 cells long and reach the 8-bit fields, where 62 rays of one
    direction is the bound: the particle is given back to the window kernel (reason 2) after its first barriers.  On the diagonal
    they are 14 cells long and stay inside the 16-bit block round the start cell: a normal particle."""
    B = 70
    ang = bundle(B, 0.3)
    axis, diag = -0.3 + 0.05, np.pi / 4 - 0.3        # (0.05 rad off the axis: from these poses all 70 end points lie well inside one row of cells, so one direction class holds them all)
    poses = [[0.02, 0.03, axis], [0.02, 0.03, diag], [3.11, -2.22, axis], [3.11, -2.22, diag], [0.02, 0.03, diag], [-1.26, 0.77, axis],
             [-1.26, 0.77, diag], [0.02, 0.03, axis]]
    scans = [np.full(B, 1.0), np.full(B, 0.996)]
    c = both_shapes(monkeypatch, "give_back", grid, poses=poses, scans=scans, angles=ang)
    assert c["fallback_bound"] == 4 * len(scans) and c["window_fallbacks"] == 4 * len(scans)
    assert c["fallback_geometry"] == 0 and c["fallback_tables"] == 0


@pytest.mark.parametrize("grid", GRIDS)
def test_strips_then_single_window(monkeypatch, grid):
    """0.025 m cells, a fan of 0.5 rad and 470 cells: along an axis its box is 470 x 241 cells and fits one LDS window (some 135 000
    cells); on the diagonal the box is 404 x 404 and takes strips of rows."""
    B = 121
    ang = fan(B, -0.25, 0.25)
    poses = [[0.2, -0.1, np.pi / 4], [0.2, -0.1, 0.0], [0.2, -0.1, np.pi / 4], [-6.33, 2.21, 0.0], [-6.33, 2.21, -3 * np.pi / 4], [0.2, -0.1, 0.0]]
    scans = [np.full(B, 11.75), 11.75 - 0.6 * np.cos(9 * ang) ** 2]
    c = both_shapes(monkeypatch, "strips", grid, poses=poses, scans=scans, angles=ang, cell_size=0.025, pool_tiles=64)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
    n = len(poses) * len(scans)
    assert n < c["map_windows"] < 2 * n                                # three particles take one window, three take more


@pytest.mark.parametrize("grid", GRIDS)
def test_lds_fold_then_register_fold(monkeypatch, grid):
    """40 beams whose end points lie 0.04 m apart across the beams' direction, 2.4 m away along +x.  From y = 0.025 m they all end in
    one cell: 40 beams' pairs are more than 64 pair ids apart, the lists laid out in LDS fold them.  From y = 0.05 m they end in two
    cells, 20 each: folded from the 64-bit set in registers."""
    B = 64
    ang = np.concatenate([bundle(40, 0.3, width=0.04 / 2.4), fan(B - 40, 1.0, 2.2)])
    th = -0.3
    poses = [[0.02, 0.025, th], [0.02, 0.05, th], [0.02, 0.025, th], [4.02, -2.975, th], [4.02, -2.95, th]]
    scans = [np.concatenate([np.full(40, 2.4), np.full(B - 40, 1.7)]), np.concatenate([np.full(40, 2.397), np.full(B - 40, 1.9)])]
    sx, sy = orc.scan_xy(scans[0], ang)
    most = []
    for pose in poses:                                                  # the construction itself: beams per end cell
        gx, gy = orc.transform(sx[:40], sy[:40], tuple(pose))
        cells = np.stack([np.trunc(gx / 0.05), np.trunc(gy / 0.05)], axis=1)
        most.append(int(np.unique(cells, axis=0, return_counts=True)[1].max()))
    assert most[0] > 32 and most[2] > 32 and most[3] > 32 and most[1] <= 32 and most[4] <= 32, most
    c = both_shapes(monkeypatch, "folds", grid, poses=poses, scans=scans, angles=ang)
    assert c["window_fallbacks"] == 0 and c["map_event_overflows"] == 0


@pytest.mark.parametrize("grid", GRIDS)
def test_dim_400_then_dim_800(monkeypatch, grid):
    """Two engines one after the other: 0.1 m cells (dim 400, the last 32-cell group of a tile row is partial), then 0.05 m cells."""
    scans, ang = room_scans(181, 12)
    poses = [[0.2, -0.1, 0.4], [19.2, 18.7, 0.7], [0.2, -0.1, 0.4], [-19.5, 3.3, 2.5], [19.2, 18.7, 0.7]]
    for name, cs in (("dim400", 0.1), ("dim800", 0.05)):
        c = both_shapes(monkeypatch, name, grid, poses=poses, scans=scans, angles=ang, cell_size=cs, pool_tiles=64)
        assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]


@pytest.mark.parametrize("P,grid", [(1, None), (1, 2), (3, 8), (6, None)])
def test_few_particles(monkeypatch, P, grid):
    """One particle; fewer particles than the cap on the workgroups (no workgroup is launched without a first particle); the
    product's own grid."""
    scans, ang = room_scans(64, 13)
    poses = [[0.31 + 0.7 * p, -0.22 - 0.4 * p, 0.4 * p] for p in range(P)]
    c = both_shapes(monkeypatch, "few%d" % P, grid, poses=poses, scans=scans, angles=ang)
    assert c["window_fallbacks"] == 0 and c["map_windows"] == P * len(scans)


def test_queue_rearms_between_launches(monkeypatch):
    """Four launches on one engine, seven particles on two workgroups: every launch starts from a queue at zero (a queue left where
    the launch before ended would hand out no particle beyond the workgroups' first ones)."""
    rng = np.random.Generator(np.random.PCG64(14))
    ang = fan(90)
    scans = [rng.uniform(1.5, 4.0, 90) for _ in range(4)]
    poses = [[0.31 + 0.5 * p, -0.22 + 0.3 * p, 0.9 * p] for p in range(7)]
    c = both_shapes(monkeypatch, "rearm", 2, poses=poses, scans=scans, angles=ang)
    assert c["window_fallbacks"] == 0 and c["map_windows"] == 7 * len(scans)
