"""The host side of map placement (thesis_amd/mapio.py): maps of any resolution, origin and yaw read from PGM + YAML files
written by hand, the box a source lands in, and rigid transforms of a source."""
import math

import numpy as np
import pytest

from thesis_amd import mapio


def write_map(tmp_path, name, pix, yaml_lines):
    pix = np.asarray(pix, dtype=np.uint8)
    with open(tmp_path / (name + ".pgm"), "wb") as f:
        f.write(b"P5\n# made by hand\n%d %d\n255\n" % (pix.shape[1], pix.shape[0]))
        f.write(pix.tobytes())
    with open(tmp_path / (name + ".yaml"), "w") as f:
        f.write(f"image: {name}.pgm\n" + "\n".join(yaml_lines) + "\n")
    return str(tmp_path / (name + ".yaml"))


PIX = [[0, 254, 205],          # image row 0: the largest y
       [254, 254, 0]]


def test_foreign_resolution_origin_and_yaw(tmp_path):
    y = write_map(tmp_path, "foreign", PIX, ["resolution: 0.025", "origin: [-51.224998, -51.224998, 0.3]", "negate: 0",
                                             "occupied_thresh: 0.65", "free_thresh: 0.196"])
    s = mapio.read_map_image(y, 0.1, -3.0, 3.0)
    assert isinstance(s, mapio.SourceMap)
    assert s.cell_size == 0.025 and s.origin == (-51.224998, -51.224998, 0.3) and s.quantum == 0.1
    # cells[i][j]: image column i, row rows - 1 - j; 0 -> occupied (+30), 254 -> free (-30), 205 -> unknown (0)
    assert s.cells.dtype == np.int8 and s.cells.tolist() == [[-30, 30], [-30, -30], [30, 0]]
    # the reader for the engine's own maps still refuses it, for each of the three reasons
    with pytest.raises(ValueError, match="not resampled"):
        mapio.read_occupancy_map(y, 0.1, -3.0, 3.0, mode="trinary")
    with pytest.raises(ValueError, match="yaw"):
        mapio.read_occupancy_map(y, 0.1, -3.0, 3.0, mode="trinary", cell_size=0.025)
    y2 = write_map(tmp_path, "offgrid", PIX, ["resolution: 0.05", "origin: [-51.224998, 0.0, 0.0]"])
    with pytest.raises(ValueError, match="whole number"):
        mapio.read_occupancy_map(y2, 0.1, -3.0, 3.0)
    assert mapio.read_map_image(y2, 0.1, -3.0, 3.0).origin == (-51.224998, 0.0, 0.0)


def test_scale_mode_and_negate(tmp_path):
    y = write_map(tmp_path, "scaled", PIX, ["resolution: 0.1", "origin: [0.5, -0.25, -1.0]"])
    s = mapio.read_map_image(y, 0.1, -3.0, 3.0, mode="scale")
    p = (255.0 - np.array(PIX, dtype=np.float64)) / 255.0
    assert np.array_equal(s.cells, mapio.cells_from_probability(p[::-1, :].T, 0.1, -3.0, 3.0))
    yn = write_map(tmp_path, "negated", PIX, ["resolution: 0.1", "origin: [0, 0, 0]", "negate: 1"])
    assert mapio.read_map_image(yn, 0.1, -3.0, 3.0).cells.tolist() == [[30, -30], [30, 30], [-30, 30]]


def test_what_the_reader_refuses(tmp_path):
    for name, lines, match in (("zero", ["resolution: 0", "origin: [0, 0, 0]"], "positive"),
                               ("neg", ["resolution: -0.05", "origin: [0, 0, 0]"], "positive"),
                               ("short", ["resolution: 0.05", "origin: [0, 0]"], "origin"),
                               ("none", ["resolution: 0.05"], "origin")):
        with pytest.raises(ValueError, match=match):
            mapio.read_map_image(write_map(tmp_path, name, PIX, lines), 0.1, -3.0, 3.0)
    with pytest.raises(ValueError, match="mode"):
        mapio.read_map_image(write_map(tmp_path, "m", PIX, ["resolution: 0.05", "origin: [0, 0, 0]"]), 0.1, -3.0, 3.0, mode="nearest")


def test_source_from_raster():
    r = mapio.MapRaster(x0=-7, y0=12, cell_size=0.1, quantum=0.1, dim=400, tile_len=40.0, cells=np.zeros((3, 4), np.int8))
    s = mapio.source_from_raster(r)
    assert s.cells is r.cells and s.cell_size == 0.1 and s.origin == (-7 * 0.1, 12 * 0.1, 0.0) and s.quantum == 0.1
    with pytest.raises(ValueError):
        mapio.source_from_raster(mapio.MapRaster(x0=0, y0=0, cell_size=0.1, quantum=0.1, dim=400, tile_len=40.0, prob=np.zeros((2, 2))))


def src(shape, cell, origin):
    return mapio.SourceMap(cells=np.zeros(shape, np.int8), cell_size=cell, origin=origin)


def test_placed_box_by_hand():
    # unrotated, 10 x 20 cells of 0.1 m at (0.26, -1.0): x in [0.26, 1.26], y in [-1.0, 1.0]; 0.05 m cells
    assert mapio.placed_box(src((10, 20), 0.1, (0.26, -1.0, 0.0)), 0.05, 800, 3) == (5, 26, -20, 21)
    # a quarter turn: the source's x axis runs along +y, its y axis along -x: x in [-2.0, 0.0] + 1.0, y in [0, 1.0] + 0.5
    b = mapio.placed_box(src((10, 20), 0.1, (1.0, 0.5, math.pi / 2)), 0.05, 800, 3)
    assert b == (-20, 21, 10, 31)
    # yaw 0.3, 100 x 40 cells of 0.03 m at (-1, 2): corners (0,0), (3,0), (0,1.2), (3,1.2) rotated and shifted
    c, s = math.cos(0.3), math.sin(0.3)
    xs = [-1.0, -1.0 + 3 * c, -1.0 - 1.2 * s, -1.0 + 3 * c - 1.2 * s]
    ys = [2.0, 2.0 + 3 * s, 2.0 + 1.2 * c, 2.0 + 3 * s + 1.2 * c]
    assert min(xs) == xs[2] and max(xs) == xs[1] and min(ys) == ys[0] and max(ys) == ys[3]
    # by hand: x in [-1.3546, 1.8660], y in [2.0, 4.0330]
    assert [round(v, 4) for v in (xs[2], xs[1], ys[3])] == [-1.3546, 1.866, 4.033]
    assert mapio.placed_box(src((100, 40), 0.03, (-1.0, 2.0, 0.3)), 0.05, 800, 3) == (-28, 38, 40, 81)
    # clipped to the lattice: radius 0, dim 400 at 0.1 m holds the cells [-200, 200)
    assert mapio.placed_box(src((1000, 10), 0.1, (-30.0, 19.5, 0.0)), 0.1, 400, 0) == (-200, 200, 195, 200)
    assert mapio.placed_box(src((10, 10), 0.1, (50.0, 50.0, 0.0)), 0.1, 400, 0) == (200, 200, 200, 200)      # wholly outside: empty


def test_moved_and_its_inverse():
    s = src((4, 4), 0.03, (1.25, -0.5, 0.4))
    # a quarter turn about the world origin, then a shift: (x, y) -> (-y, x) + (2, 3)
    m = s.moved((2.0, 3.0, math.pi / 2))
    assert m.cells is s.cells and m.cell_size == s.cell_size
    np.testing.assert_allclose(m.origin, (2.0 + 0.5, 3.0 + 1.25, 0.4 + math.pi / 2), atol=1e-15)
    rng = np.random.Generator(np.random.PCG64(4))
    for pose in rng.uniform(-3, 3, size=(8, 3)):
        back = s.moved(pose).moved(mapio.inverse_pose(pose))
        np.testing.assert_allclose(back.origin, s.origin, atol=1e-12)
        fwd = s.moved(mapio.inverse_pose(pose)).moved(pose)
        np.testing.assert_allclose(fwd.origin, s.origin, atol=1e-12)
    # two moves compose like the poses
    a, b = (0.3, -1.1, 0.7), (-2.0, 0.4, -1.9)
    ca, sa = math.cos(b[2]), math.sin(b[2])
    ab = (b[0] + ca * a[0] - sa * a[1], b[1] + sa * a[0] + ca * a[1], a[2] + b[2])
    np.testing.assert_allclose(s.moved(a).moved(b).origin, s.moved(ab).origin, atol=1e-12)
