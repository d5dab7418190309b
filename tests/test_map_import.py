"""Occupancy-map import (thesis_amd/mapio.py): read_occupancy_map and cells_from_probability, the inverse of
write_occupancy_map.  CPU only: the maps here are written by hand or by write_occupancy_map."""
import numpy as np
import pytest

from thesis_amd.mapio import MapRaster, cells_from_probability, read_occupancy_map, write_occupancy_map

Q, VMIN, VMAX = 0.1, -3.0, 3.0


def raster(cells, x0=0, y0=0, cs=0.05):
    return MapRaster(x0=x0, y0=y0, cell_size=cs, quantum=Q, dim=int(round(40.0 / cs)), tile_len=40.0, cells=cells)


def read(yml, **kw):
    return read_occupancy_map(str(yml), Q, VMIN, VMAX, **kw)


def write_files(tmp_path, img, header=None, **meta):
    """A PGM (rows as given) and its YAML; `header` replaces the PGM header bytes."""
    img = np.asarray(img, dtype=np.uint8)
    pgm = tmp_path / "m.pgm"
    pgm.write_bytes((header if header is not None else b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0])) + img.tobytes())
    y = {"image": "m.pgm", "resolution": "0.05", "origin": "[0.0, 0.0, 0.0]", "negate": "0",
         "occupied_thresh": "0.65", "free_thresh": "0.196"}
    y.update({k: str(v) for k, v in meta.items()})
    yml = tmp_path / "m.yaml"
    yml.write_text("".join(f"{k}: {v}\n" for k, v in y.items()))
    return yml


def test_every_lattice_value_round_trips(tmp_path):
    v = np.arange(-30, 31, dtype=np.int8)
    cells = np.stack([v, v[::-1], np.roll(v, 7)])
    stem = str(tmp_path / "all")
    _, yml = write_occupancy_map(stem, raster(cells, -3, 11))
    back = read_occupancy_map(yml, Q, VMIN, VMAX, mode="scale")
    assert back.cells.dtype == np.int8
    np.testing.assert_array_equal(back.cells, cells)
    pix = np.frombuffer(open(stem + ".pgm", "rb").read()[-cells.size:], dtype=np.uint8)
    assert len(set(pix.tolist())) == 61                           # 61 values on 61 distinct pixels


@pytest.mark.parametrize("x0,y0", [(-7, -3), (12, 5), (-405, 390), (0, 0)])
def test_origin_and_orientation_round_trip(tmp_path, x0, y0):
    rng = np.random.Generator(np.random.PCG64(abs(x0) + abs(y0)))
    cells = rng.integers(-30, 31, size=(13, 9)).astype(np.int8)   # not square: a transposition would show
    _, yml = write_occupancy_map(str(tmp_path / "o"), raster(cells, x0, y0))
    back = read(yml)
    assert (back.x0, back.y0) == (x0, y0)
    assert (back.cell_size, back.quantum, back.dim, back.tile_len) == (0.05, Q, 800, 40.0)
    np.testing.assert_array_equal(back.cells, cells)


def test_image_orientation_by_hand(tmp_path):
    # row 0 of the image is the largest Y, column 0 the smallest X
    img = np.full((2, 3), 254, dtype=np.uint8)                    # free
    img[0, 2] = 0                                                 # X = x0 + 2, Y = y0 + 1: occupied
    yml = write_files(tmp_path, img, origin="[-0.1, 0.25, 0.0]")
    r = read(yml, mode="trinary")
    assert (r.x0, r.y0) == (-2, 5) and r.cells.shape == (3, 2)
    want = np.full((3, 2), -30, dtype=np.int8)
    want[2, 1] = 30
    np.testing.assert_array_equal(r.cells, want)


def test_negate_and_header_comments(tmp_path):
    img = np.array([[0, 128, 255]], dtype=np.uint8)
    hdr = b"P5\n# written by another tool\n3 # width\n 1\n# maxval next\n255\n"
    plain = read(write_files(tmp_path, img, header=hdr))
    neg = read(write_files(tmp_path, img, header=hdr, negate=1))
    # negate 0: p = (255 - pixel) / 255; negate 1: p = pixel / 255
    np.testing.assert_array_equal(plain.cells[:, 0], cells_from_probability((255.0 - img[0]) / 255.0, Q, VMIN, VMAX))
    np.testing.assert_array_equal(neg.cells[:, 0], cells_from_probability(img[0] / 255.0, Q, VMIN, VMAX))
    np.testing.assert_array_equal(plain.cells[:, 0], [30, 0, -30])
    np.testing.assert_array_equal(neg.cells[:, 0], [-30, 0, 30])


def test_trinary_thresholds(tmp_path):
    # p = (255 - pixel) / 255 against occupied_thresh 0.65 and free_thresh 0.196
    img = np.array([[0, 89, 90, 128, 204, 205, 206, 255]], dtype=np.uint8)
    r = read(write_files(tmp_path, img), mode="trinary")
    p = (255.0 - img[0]) / 255.0
    want = np.where(p > 0.65, 30, np.where(p < 0.196, -30, 0))
    np.testing.assert_array_equal(r.cells[:, 0], want)
    assert want.tolist() == [30, 30, 0, 0, 0, 0, -30, -30]      # 205: p = 0.19608, not below 0.196


def test_cells_from_probability():
    p = np.array([0.0, 1e-9, 0.5, 0.5 + 1e-9, 1.0 - 1e-9, 1.0])
    np.testing.assert_array_equal(cells_from_probability(p, Q, VMIN, VMAX), [-30, -30, 0, 0, 30, 30])
    v = np.arange(-30, 31)
    s = 1.0 / (1.0 + np.exp(-v * Q))
    np.testing.assert_array_equal(cells_from_probability(s, Q, VMIN, VMAX), v)
    with pytest.raises(ValueError):
        cells_from_probability(np.array([1.5]), Q, VMIN, VMAX)


@pytest.mark.parametrize("meta,match", [({"resolution": "0.1"}, "resolution"),
                                        ({"origin": "[0.01, 0.0, 0.0]"}, "whole number"),
                                        ({"origin": "[0.0, 0.0, 0.3]"}, "yaw")])
def test_refusals_of_the_yaml(tmp_path, meta, match):
    yml = write_files(tmp_path, np.zeros((2, 2), np.uint8), **meta)
    with pytest.raises(ValueError, match=match):
        read(yml)


def test_refuses_other_images(tmp_path):
    with pytest.raises(ValueError, match="P5"):
        read(write_files(tmp_path, np.zeros((2, 2), np.uint8), header=b"P2\n2 2\n255\n"))
    with pytest.raises(ValueError, match="maxval"):
        read(write_files(tmp_path, np.zeros((2, 2), np.uint8), header=b"P5\n2 2\n65535\n"))
    with pytest.raises(ValueError, match="mode"):
        read(write_files(tmp_path, np.zeros((2, 2), np.uint8)), mode="raw")
