"""Shared test helpers: oracle-side map construction from golden dumps, and the map-update case runner of the kernel tier tests."""
import numpy as np

from oracle import rbpf_oracle as orc


def oracle_map_from_dump(g, prefix, cs):
    """Rebuild an OracleHybridMap from a `dump_map` record in a golden file."""
    hm = orc.OracleHybridMap(cs)
    hm.tiles = []
    centres, offs = g[prefix + "centres"], g[prefix + "offs"]
    for t in range(len(centres)):
        cx, cy = centres[t]
        cx = int(cx) if float(cx).is_integer() else float(cx)
        cy = int(cy) if float(cy).is_integer() else float(cy)
        tile = orc.OracleTile(cx, cy, 40, cs)
        s, e = offs[t], offs[t + 1]
        tile.map[g[prefix + "xs"][s:e], g[prefix + "ys"][s:e]] = g[prefix + "vals"][s:e]
        hm.tiles.append(tile)
    return hm


def dump_oracle_map(hm):
    out = {}
    for t in hm.tiles:
        xs, ys = np.nonzero(t.map)
        out[(float(t.cx), float(t.cy))] = (xs, ys, t.map[xs, ys])
    return out


def golden_dump_as_dict(g, prefix):
    out = {}
    centres, offs = g[prefix + "centres"], g[prefix + "offs"]
    for t in range(len(centres)):
        s, e = offs[t], offs[t + 1]
        out[(float(centres[t][0]), float(centres[t][1]))] = (
            g[prefix + "xs"][s:e], g[prefix + "ys"][s:e], g[prefix + "vals"][s:e])
    return out


MAP_COUNTERS = ("map_windows", "window_fallbacks", "fallback_geometry", "fallback_bound", "fallback_tables", "slow_cells",
                "map_pool_cells", "map_near_cells", "map_events", "map_event_overflows")


def run_map_case(engine, poses, scans, angles, cell_size=0.05, pool_tiles=32, c_oracle_above=400):
    """Scans into an engine (whose map kernel the caller has forced) and into one oracle map per DISTINCT pose; every tile
    byte and the read-out (get_odds_at) at the flagged cells - the last scan's end points and the points one cell short of
    them - compared.  Scans of more than c_oracle_above beams go through the oracle's C restatement.  Then what the update
    maintains beside the cells, for every particle and every held tile (tests/mapupdate_hidden.py): the written boxes against
    the box of the cells the oracle visited, the occupancy words against the oracle's cells; and the two counters the bench's
    roofline is computed from: cells_written = the distinct storage cells a scan visited, summed over scans and particles,
    ray_cells_visited = the oracle's Bresenham points summed the same way.  Prints and returns the engine's counters."""
    from tests import mapupdate_hidden as hidden
    Q = 0.1
    poses = np.asarray(poses, dtype=np.float64)
    P = len(poses)
    angs = angles if isinstance(angles, list) else [angles] * len(scans)
    B = max(len(r) for r in scans)
    e = engine.ParticleEngine(P, max_beams=B, cell_size=cell_size, pool_tiles=pool_tiles)
    keys = [tuple(float(v) for v in poses[p]) for p in range(P)]
    if B > c_oracle_above:
        from oracle import c_oracle
        lib = c_oracle.load()
        maps = {k: c_oracle.CMap(lib, cell_size) for k in keys}
    else:
        maps = {k: orc.OracleHybridMap(cell_size) for k in keys}
    union = {k: {} for k in keys}                                            # per pose {centre: cells visited by any scan}
    written = {k: 0 for k in keys}                                           # per pose: distinct cells visited, summed over scans
    c0 = e.counters()
    for r, a in zip(scans, angs):
        e.set_scan(r, a)
        e.map_update(poses)
        sx, sy = orc.scan_xy(r, a)
        for pose, hm in maps.items():
            hm.clear_visited()
            hm.update(pose, sx, sy)
            for cxy, plane in hidden.visited_planes(hm).items():
                written[pose] += int(plane.sum())
                union[pose][cxy] = union[pose].get(cxy, False) | plane
    c = e.counters()
    print({k: c[k] for k in MAP_COUNTERS})
    want_written = sum(written[k] for k in keys)
    want_visited = sum(maps[k].cells_visited for k in keys)
    print({"cells_written": c["cells_written"] - c0["cells_written"], "oracle": want_written,
           "ray_cells_visited": c["ray_cells_visited"] - c0["ray_cells_visited"], "oracle_visited": want_visited})
    for k, hm in list(maps.items()):
        if not isinstance(hm, orc.OracleHybridMap):                      # the C map's tiles in the Python oracle's clothes
            py = orc.OracleHybridMap(cell_size)
            py.tiles = []
            for (cx, cy), cells in hm.tiles().items():
                t = orc.OracleTile(cx, cy, 40, cell_size)
                t.map = cells
                py.tiles.append(t)
            maps[k] = py
    dim = e.dim
    for p in range(P):
        hm = maps[keys[p]]
        got = {cxy: cells for cxy, cells in e.tiles(p)}
        assert set(got.keys()) == {(float(t.cx), float(t.cy)) for t in hm.tiles}
        for t in hm.tiles:
            q = np.rint(t.map / Q)
            assert np.max(np.abs(t.map - q * Q)) < 1e-9
            have = got[(float(t.cx), float(t.cy))]
            assert have.shape == (dim, dim)
            if not np.array_equal(have, q.astype(np.int8)):
                bad = np.argwhere(have != q.astype(np.int8))
                raise AssertionError(f"particle {p} tile ({t.cx}, {t.cy}): {len(bad)} cells differ, first {bad[:5].tolist()} "
                                     f"got {have[tuple(bad[0])]} want {q[tuple(bad[0])]}")
        sx, sy = orc.scan_xy(scans[-1], angs[-1])
        rr = np.hypot(sx, sy)
        keep = rr > 1e-9
        short = np.where(keep, np.maximum(rr - cell_size, 0.0) / np.where(keep, rr, 1.0), 0.0)
        gx, gy = orc.transform(np.concatenate([sx, sx * short]), np.concatenate([sy, sy * short]), keys[p])
        pts = np.stack([gx, gy], axis=1)
        vals, none = e.get_odds_at(p, pts)
        want = [hm.get_odds_at(float(x), float(y)) for x, y in pts]
        assert np.array_equal(none, np.array([w is None for w in want]))
        np.testing.assert_allclose(vals[~none], np.array([w for w in want if w is not None], dtype=np.float64), rtol=0, atol=1e-9)
    got_hidden = hidden.read_hidden_of(e, range(P))
    for p in range(P):
        hidden.check_map_hidden(e, p, maps[keys[p]], visited=union[keys[p]], what="run_map_case", hidden=got_hidden[p])
    assert c["cells_written"] - c0["cells_written"] == want_written, (c["cells_written"] - c0["cells_written"], want_written)
    assert c["ray_cells_visited"] - c0["ray_cells_visited"] == want_visited, (c["ray_cells_visited"] - c0["ray_cells_visited"], want_visited)
    e.close()
    return c
