"""The event-walk kernel's write-back has two instantiations (kernels_mapev.hip): tile rows of whole 32-cell groups under a fan that
is not thin take the one without the partial group's word tests and the thin fan's branch, everything else the general one.  The
choice is made per particle, so one resident workgroup (RBPF_EV_GRID=1) that runs a thin fan, a dense one, a thin one ... in a row
takes both in one launch.  55 beams over 0.5 rad and 11 m on 0.05 m cells: along an axis the fan's box is 220 x 110 cells and the
rays' cells are more than two fifths of it, on the diagonal the box is 190 x 190 and they are fewer (the kernel's test, restated
below with a margin).  Tiles and read-outs against OracleHybridMap.update through tests/test_gpu_mapev_flagged.py::run_case.

GPU only:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

from oracle import rbpf_oracle as orc
from tests.test_gpu_mapev_flagged import run_case

pytestmark = pytest.mark.gpu


def thin(pose, r, ang, cs):
    """The kernel's test on the reference's numbers: five times the rays' cells against twice the fan's box."""
    sx, sy = orc.scan_xy(r, ang)
    gx, gy = orc.transform(sx, sy, tuple(pose))
    x0, y0 = int(pose[0] / cs), int(pose[1] / cs)
    ex, ey = np.trunc(gx / cs).astype(int), np.trunc(gy / cs).astype(int)
    cells = int(np.sum(np.maximum(np.abs(ex - x0), np.abs(ey - y0)) + 1))
    box = (max(ex.max(), x0) - min(ex.min(), x0) + 1) * (max(ey.max(), y0) - min(ey.min(), y0) + 1)
    return 5 * cells / (2 * box)


@pytest.mark.parametrize("grid", [1, None])
def test_thin_and_dense_fans_in_one_launch(monkeypatch, grid):
    monkeypatch.setenv("RBPF_MAP_KERNEL", "ev")
    if grid is None:
        monkeypatch.delenv("RBPF_EV_GRID", raising=False)
    else:
        monkeypatch.setenv("RBPF_EV_GRID", str(grid))
    from thesis_amd import engine
    B = 55
    ang = np.linspace(-0.25, 0.25, B)
    scans = [np.full(B, 11.0), 11.0 - 0.6 * np.cos(9 * ang) ** 2]
    diag, axis = np.pi / 4, 0.0
    poses = [[0.2, -0.1, diag], [0.2, -0.1, axis], [3.11, -2.22, diag], [3.11, -2.22, axis + np.pi / 2], [-1.26, 0.77, -3 * np.pi / 4], [0.2, -0.1, axis]]
    for r in scans:
        ratio = [thin(p, r, ang, 0.05) for p in poses]
        assert all(q < 0.9 for q in ratio[0::2]) and all(q > 1.1 for q in ratio[1::2]), ratio
    c = run_case(engine, poses, scans, ang)
    assert c["window_fallbacks"] == 0, "fallback reasons %x" % c["fallback_reasons"]
    assert c["map_windows"] == len(poses) * len(scans)
