"""thesis_amd/rebuild.py on the host: counts to rasters against plain NumPy, the scan log's alignment with the trajectory log's
records, and rebuild()'s choice of poses, box and chunks on a stand-in engine whose build_map is the oracle."""
import numpy as np
import pytest

from tests.build_oracle import build_map as oracle_build
from thesis_amd import rebuild
from thesis_amd.engine import BuiltMap, ParticleEngine


def built(hits, seen, x0=-3, y0=7, cs=0.025):
    return BuiltMap(np.asarray(hits, np.int32), np.asarray(seen, np.int32), x0, y0, cs, 1.0 / cs)


class Cfg:
    quantum, log_odds_occ, log_odds_emp, min_odds_emp, max_odds_occ = 0.1, 0.8, -0.3, -3.0, 3.0
    tile_len_m, cell_size, max_ray_m = 40, 0.05, 15.0


class Eng:
    cfg, dim = Cfg, 800


# ---- counts to rasters ---------------------------------------------------------------------------------------------------------
def test_to_cells_adds_clamps_and_leaves_the_unseen_at_zero():
    hits = np.array([[0, 0, 1, 5, 0, 2], [0, 1, 1, 0, 0, 3]])
    seen = np.array([[0, 1, 1, 5, 40, 4], [0, 3, 9, 2, 10, 3]])
    b = built(hits, seen)
    got = rebuild.to_cells(b, occ=8, emp=-3, vmin=-30, vmax=30)
    want = np.clip(hits * 8 + (seen - hits) * -3, -30, 30)
    want[seen == 0] = 0
    assert got.dtype == np.int8 and np.array_equal(got, want)
    assert got[0, 0] == 0 and got[0, 3] == 30 and got[0, 4] == -30 and got[0, 5] == 10 and got[1, 1] == 2
    # a seen cell whose sum is 0 stays 0 like an unseen one; hit_ratio tells them apart
    assert rebuild.to_cells(built([[3]], [[11]]), occ=8, emp=-3, vmin=-30, vmax=30)[0, 0] == 0
    assert np.array_equal(rebuild.to_cells(b, engine=Eng), got)                     # the engine's sensor model is the same
    assert np.array_equal(rebuild.to_cells(b, engine=Eng, occ=1, emp=0, vmax=2), np.minimum(hits, 2))
    with pytest.raises(ValueError):
        rebuild.to_cells(b, occ=8, emp=-3)               # no clamps and no engine
    with pytest.raises(ValueError):
        rebuild.to_cells(b, occ=8, emp=-3, vmin=-200, vmax=30, quantum=0.1)


def test_hit_ratio_is_nan_where_nothing_was_seen():
    r = rebuild.hit_ratio(built([[0, 1, 3]], [[0, 4, 3]]))
    assert r.dtype == np.float32 and np.isnan(r[0, 0]) and r[0, 1] == np.float32(0.25) and r[0, 2] == 1.0


def test_as_source_and_as_raster_carry_the_geometry(tmp_path):
    b = built([[0, 1], [2, 0], [0, 0]], [[1, 1], [2, 5], [0, 9]])
    cells = rebuild.to_cells(b, engine=Eng)
    s = rebuild.as_source(b, engine=Eng)
    assert np.array_equal(s.cells, cells) and s.cell_size == 0.025 and s.quantum == 0.1
    assert s.origin == (-3 * 0.025, 7 * 0.025, 0.0)
    r = rebuild.as_raster(b, engine=Eng)
    assert (r.x0, r.y0, r.cell_size, r.dim, r.tile_len, r.quantum) == (-3, 7, 0.025, 1600, 40.0, 0.1)
    assert np.array_equal(r.cells, cells) and r.prob is None
    from thesis_amd import mapio
    pgm, yml = mapio.write_occupancy_map(str(tmp_path / "final"), r)               # the exporter takes it as it is
    back = mapio.read_occupancy_map(yml, 0.1, -3.0, 3.0, cell_size=0.025)
    assert (back.x0, back.y0) == (-3, 7) and np.array_equal(back.cells, cells)
    own = BuiltMap(b.hits, b.seen, 4, 5, 0.05, 800 / 40.0)                         # the engine's own cells: loadable
    assert rebuild.as_raster(own, engine=Eng).dim == 800
    with pytest.raises(ValueError):
        rebuild.as_raster(built([[0]], [[1]], cs=0.07), engine=Eng)               # 40 m is no whole number of 0.07 m cells
    assert rebuild.as_source(built([[0]], [[1]], cs=0.07), engine=Eng).cell_size == 0.07


# ---- the scan log ------------------------------------------------------------------------------------------------------------------
def test_scan_log_keeps_scans_under_their_records():
    log = rebuild.ScanLog()
    rec, rg = log.ranges_for(0, 10)
    assert len(log) == 0 and rec.shape == (0,) and rg.shape == (0, 0)
    scans = np.arange(5 * 4, dtype=np.float64).reshape(5, 4)
    scans[2, 1] = np.nan
    for r, s in zip((1, 3, 4, 8, 9), scans):
        log.append(r, s)
    scans[0, 0] = -1.0                                   # the log holds copies
    rec, rg = log.ranges_for()
    assert rec.tolist() == [1, 3, 4, 8, 9] and rg.shape == (5, 4) and rg[0, 0] == 0.0 and np.isnan(rg[2, 1])
    rec, rg = log.ranges_for(3, 9)
    assert rec.tolist() == [3, 4, 8] and np.array_equal(rg[2], scans[3])
    assert log.ranges_for(5, 8)[1].shape == (0, 4)
    with pytest.raises(ValueError):
        log.append(9, scans[0])                          # records only grow
    with pytest.raises(ValueError):
        log.append(12, np.zeros(5))                      # another beam count


# ---- rebuild() -------------------------------------------------------------------------------------------------------------------
class LoggedEngine(Eng):
    """What rebuild() asks of an engine, with the oracle for build_map: T records, three particles' lineages."""

    def __init__(self, T):
        rng = np.random.Generator(np.random.PCG64(2))
        self.paths = rng.uniform(-1.0, 1.0, (3, T, 3))
        self.mean = self.paths.mean(axis=0)
        self.T, self.calls = T, []

    build_box = staticmethod(ParticleEngine.build_box)

    def track_info(self):
        return {"n_records": self.T, "capacity": self.T, "dropped": 2}

    def trajectory(self, particle="best"):
        if particle != "best":
            raise ValueError(particle)
        return self.paths[1]

    def lineage(self, particles):
        return None, self.paths[particles[0]][:, None, :]

    def trajectory_summary(self):
        return type("S", (), {"pose": self.mean})

    def build_map(self, poses, ranges, angles, cell_size=None, box=None, min_range=0.0, max_range=None, device=False, into=None):
        inv = self.dim / float(self.cfg.tile_len_m) if cell_size is None else 1.0 / cell_size
        mr = self.cfg.max_ray_m if max_range is None else max_range
        self.calls.append((len(poses), tuple(box), into is not None))
        h, s, _ = oracle_build(poses, ranges, angles, inv, box, min_range, mr)
        if into is not None:
            into.hits[...] += h
            into.seen[...] += s
            return into
        return BuiltMap(h, s, box[0], box[2], self.cfg.cell_size if cell_size is None else cell_size, inv)


def test_rebuild_takes_the_records_with_a_scan_in_chunks(monkeypatch):
    T, B = 12, 9
    e = LoggedEngine(T)
    angles = np.linspace(-2.0, 2.0, B)
    rng = np.random.Generator(np.random.PCG64(3))
    log = rebuild.ScanLog()
    records = [2, 3, 5, 8, 9, 10, 11]
    scans = rng.uniform(0.2, 1.5, (len(records), B))
    scans[1, 4], scans[3, 0] = np.nan, np.inf
    for r, s in zip(records, scans):
        log.append(r, s)
    log.append(T + 3, scans[0])                          # a record this engine's log does not hold: left out
    monkeypatch.setattr(rebuild, "CHUNK", 3)
    for particle, path in (("best", e.paths[1]), (2, e.paths[2]), ("mean", e.mean)):
        e.calls.clear()
        got = rebuild.rebuild(e, log, angles, particle=particle, cell_size=0.1, max_range=1.0)
        poses = path[records]
        box = ParticleEngine.build_box(poses, 10.0, 1.0)
        assert e.calls == [(3, box, False), (3, box, True), (1, box, True)]
        h, s, _ = oracle_build(poses, scans, angles, 10.0, box, 0.0, 1.0)
        assert (got.x0, got.y0, got.cell_size, got.cells_per_m) == (box[0], box[2], 0.1, 10.0)
        assert np.array_equal(got.hits, h) and np.array_equal(got.seen, s) and s.max() > 1
    fx = np.floor(e.mean[records][:, 0] * 10.0)         # the box of the last of them
    assert box[0] == fx.min() - 12 and box[1] == fx.max() + 13        # floor(x inv) -+ (ceil(max_range inv) + 2), half-open
    with pytest.raises(ValueError):
        rebuild.rebuild(e, log, angles, particle="worst")
    with pytest.raises(ValueError):
        rebuild.rebuild(e, rebuild.ScanLog(), angles)
