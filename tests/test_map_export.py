"""Occupancy-map export (thesis_amd/mapio.py): PGM + YAML of a rendered raster, and the resample weight distribution.
CPU only: the rasters here are built by hand."""
import numpy as np
import pytest

from thesis_amd.mapio import MapRaster, resample_weights, write_occupancy_map


def read_pgm(path):
    data = open(path, "rb").read()
    parts, pos = [], 0
    while len(parts) < 4:                                   # magic, width, height, maxval; then one whitespace byte
        while data[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        parts.append(data[pos:end])
        pos = end
    pos += 1
    assert parts[0] == b"P5" and parts[3] == b"255"
    w, h = int(parts[1]), int(parts[2])
    img = np.frombuffer(data[pos:], dtype=np.uint8)
    assert img.size == w * h
    return img.reshape(h, w)


def read_yaml(path):
    out = {}
    for line in open(path):
        k, v = line.split(":", 1)
        out[k.strip()] = v.strip()
    return out


def raster(nx, ny, x0, y0, **arrays):
    return MapRaster(x0=x0, y0=y0, cell_size=0.05, quantum=0.1, dim=800, tile_len=40.0, **arrays)


@pytest.mark.parametrize("x0,y0", [(-7, -3), (12, 5), (-405, 390)])
def test_orientation_and_origin(tmp_path, x0, y0):
    nx, ny = 9, 6
    prob = np.full((nx, ny), 0.5, dtype=np.float32)
    X, Y = x0 + 6, y0 + 1                                    # one occupied cell at a known mosaic cell
    prob[X - x0, Y - y0] = 1.0
    pgm, yml = write_occupancy_map(str(tmp_path / "m"), raster(nx, ny, x0, y0, prob=prob))
    img = read_pgm(pgm)
    assert img.shape == (ny, nx)                             # width = X extent, height = Y extent
    row, col = ny - 1 - (Y - y0), X - x0                     # row 0 is the largest Y
    assert img[row, col] == 0
    mask = np.ones_like(img, dtype=bool)
    mask[row, col] = False
    assert np.all(img[mask] == 128)                          # round(255 * 0.5) = 127.5 -> 128 (half to even)
    y = read_yaml(yml)
    assert y["image"] == "m.pgm" and y["negate"] == "0"
    assert float(y["resolution"]) == 0.05
    org = [float(t) for t in y["origin"].strip("[]").split(",")]
    assert org == [x0 * 0.05, y0 * 0.05, 0.0]
    assert float(y["occupied_thresh"]) == 0.65 and float(y["free_thresh"]) == 0.196


def test_value_mapping(tmp_path):
    p = np.array([[0.0, 0.25, 0.75, 1.0, 0.2, 0.9]], dtype=np.float32)
    pgm, _ = write_occupancy_map(str(tmp_path / "v"), raster(1, 6, 0, 0, prob=p), occupied_thresh=0.7, free_thresh=0.3)
    img = read_pgm(pgm)
    want = np.rint(255.0 * (1.0 - p.astype(np.float64)))[0, ::-1]
    assert np.array_equal(img[:, 0], want.astype(np.uint8))
    assert list(img[:, 0]) == [26, 204, 0, 64, 191, 255]
    y = read_yaml(str(tmp_path / "v.yaml"))
    assert float(y["occupied_thresh"]) == 0.7 and float(y["free_thresh"]) == 0.3


def test_single_particle_cells_use_sigma(tmp_path):
    cells = np.array([[-30, -3, 0, 8, 30]], dtype=np.int8)
    pgm, _ = write_occupancy_map(str(tmp_path / "c"), raster(1, 5, -1, -2, cells=cells))
    e = np.exp(cells.astype(np.float64) * 0.1)
    want = np.rint(255.0 * (1.0 - e / (1.0 + e)))[0, ::-1].astype(np.uint8)
    assert np.array_equal(read_pgm(pgm)[:, 0], want)


def test_refuses_a_mosaic_that_is_not_a_world_grid(tmp_path):
    r = MapRaster(x0=0, y0=0, cell_size=0.03, quantum=0.1, dim=1333, tile_len=40.0, prob=np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="tile length"):
        write_occupancy_map(str(tmp_path / "bad"), r)
    assert not (tmp_path / "bad.pgm").exists()
    with pytest.raises(ValueError):
        write_occupancy_map(str(tmp_path / "none"), raster(2, 2, 0, 0, occ_frac=np.zeros((2, 2), np.float32)))


def test_resample_weights_match_the_reference_rule():
    w = [10, -250, -100, 300, 5, -np.inf, 0, 42]
    got = resample_weights(w)
    assert got.dtype == np.float64
    assert list(got) == [260.0, 0.0, 150.0, 550.0, 255.0, 0.0, 0.0, 292.0]
    assert list(resample_weights([1.0, 2.0, -np.inf])) == [1.0, 2.0, 0.0]   # no negative weight: only -inf changes
    src = np.array([3.0, -1.0])
    resample_weights(src)
    assert list(src) == [3.0, -1.0]                                         # the caller's array is left alone
