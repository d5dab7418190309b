"""Adjacent-scan (mode 1) problems of the NDT-stage tests.  In mode 1 the matcher's field is rasterised from the previous
scan's points, so the whole problem -- field, grid stage, NDT stage -- is computable without a GPU:
tests/test_oracle_ndt.py checks on the CPU that every case enters the stage, is decisive and is stable in the reference;
tests/test_gpu_matcher_ndt.py runs the same cases on the device.

World: a closed three-lobed curve round the origin, sized to the configuration's match_max_range so that every point
lies inside the range filter.  Scans see every world point (no occlusion) with seeded noise."""
from functools import lru_cache
from types import SimpleNamespace
from typing import NamedTuple, Tuple

import numpy as np

from oracle import matcher_oracle as mo
from oracle import rbpf_oracle as orc
from tests.test_gpu_matcher_grid import oracle_particle, rot

NC2_POSE_TOL = 1e-6       # metres / radians, tests/test_gpu_matcher.py test_ndt_stage_equals_oracle
NC2_SCORE_RTOL = 1e-6
GENERAL_MARGIN = 64.0     # nc != 2: times the reference's own summation-order sensitivity
GENERAL_FLOOR = 1e-12


class AdjCase(NamedTuple):
    name: str
    cell_size: float
    max_range: float
    N: int                 # what match_geometry must give (a later change of the geometry must not turn nc into 2 unseen)
    ds: int
    nc: int
    true0: Tuple[float, float, float]      # where the previous scan was taken
    true1: Tuple[float, float, float]      # where the current scan is taken
    poses: Tuple[Tuple[float, float, float], ...]
    covs: Tuple[Tuple[float, float, float], ...]     # diagonals
    mode: int = 1          # ndt_refine
    thin: int = 1          # every thin-th point of the previous scan makes the field
    thick: int = 1         # wall layers of the world, one matcher cell apart (2 x 2 NDT cells need walls two cells thick)
    expect: Tuple[str, ...] = ("accept",)  # per particle (one entry: all): "accept" / "score" (rejected by 2 * ndtScore >
                                           # gridScore) / "window" (rejected by the validity gate)


_WIDE = (4e-4, 4e-4, 1e-5)            # 0.7 m window
_POSES4 = ((0.32, 0.21, 0.13), (-0.23, 0.18, 0.06), (-0.17, -0.3, 0.12), (0.23, -0.13, 0.04))     # origins: four residue pairs mod every nc below
_TRUE0, _TRUE1 = (0.0, 0.0, 0.0), (0.04, -0.03, 0.1)

CASES = {c.name: c for c in [
    # case 3: the shipped geometry, cell_off 0, three windows (the smallest 0.1 m)
    AdjCase("adjacent", 0.05, 11.0, 512, 1, 2, (0.5, -0.3, 0.2), (0.8, -0.1, 0.3),
            ((0.83, -0.07, 0.32), (0.77, -0.14, 0.28), (0.9, 0.0, 0.35)), ((1e-4, 4e-5, 1e-5), (1e-7, 1e-7, 1e-6), _WIDE), thick=2,
            expect=("accept", "accept", "score")),
    # case 4: the general form
    AdjCase("nc4", 0.025, 5.0, 512, 1, 4, _TRUE0, _TRUE1, _POSES4, (_WIDE,) * 4),
    AdjCase("nc3", 0.03125, 9.0, 672, 1, 3, _TRUE0, _TRUE1, _POSES4, (_WIDE,) * 4),
    AdjCase("nc5", 40.0 / 2048, 5.0, 640, 1, 5, _TRUE0, _TRUE1, _POSES4, (_WIDE,) * 4),
    AdjCase("nc8", 0.0125, 2.5, 608, 1, 8, _TRUE0, _TRUE1, _POSES4, (_WIDE,) * 4),     # stands in for nc5 if rbpf_create refuses it
    # case 5: rejections
    AdjCase("thin", 0.05, 11.0, 512, 1, 2, (0.5, -0.3, 0.2), (0.8, -0.1, 0.3),
            ((0.83, -0.07, 0.32), (0.75, -0.2, 0.25), (0.9, 0.0, 0.35)), (_WIDE,) * 3, thin=7, thick=2, expect=("score",)),
    AdjCase("window", 0.05, 11.0, 512, 1, 2, (0.5, -0.3, 0.2), (0.8, -0.1, 0.3),
            ((0.93, -0.1, 0.3), (0.8, -0.23, 0.3), (0.67, 0.03, 0.3)), ((1e-7, 1e-7, 1e-6),) * 3, thick=2, expect=("window",)),
]}
GENERAL = ("nc4", "nc3", "nc5", "nc8")


def world(max_range: float, thick: int = 1, step: float = 0.0, n: int = 1081) -> np.ndarray:
    phi = np.linspace(-np.pi, np.pi, n, endpoint=False)
    r = 0.5 * max_range * (1.0 + 0.3 * np.sin(3 * phi + 0.4)) + step * (np.arange(n) % thick)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)


@lru_cache(maxsize=None)
def scans(name: str):
    """(x0, y0): the previous scan in its sensor frame; last: the same points in the world frame, as the host hands
    them over; (x, y): the current scan."""
    c = CASES[name]
    rng = np.random.Generator(np.random.PCG64(int(1e4 * c.cell_size) + c.nc))
    w = world(c.max_range, c.thick, c.cell_size * c.ds)
    s0 = (w - np.asarray(c.true0[:2])) @ rot(c.true0[2]) + rng.normal(0, 0.004, w.shape)
    s1 = (w - np.asarray(c.true1[:2])) @ rot(c.true1[2]) + rng.normal(0, 0.004, w.shape)
    gx, gy = orc.transform(s0[:, 0], s0[:, 1], tuple(c.true0))
    last = np.stack([gx, gy], axis=1)[::c.thin]
    return (s0[:, 0].copy(), s0[:, 1].copy()), last, (s1[:, 0].copy(), s1[:, 1].copy())


def expected(c: AdjCase, p: int) -> str:
    return c.expect[p if len(c.expect) > 1 else 0]


def covariances(c: AdjCase) -> np.ndarray:
    return np.array([np.diag(d) for d in c.covs])


def stage(r: dict, nc: int, mode: int, cell_off: float = 0.0, reverse: bool = False) -> dict:
    """ndt_stage on the problem oracle_particle left in r; reverse: the beams in reverse order (another summation order,
    the same problem)."""
    pts = np.stack([r["bx"], r["by"]], axis=1).astype(np.float64)
    return mo.ndt_stage(r["occ"], r["ox"], r["oy"], pts[::-1] if reverse else pts, r, r["pose"], r["window"], r["mcs"],
                        cell_off, nc, mode)


def beam_cells(r: dict, st: dict):
    """Region cells (u, w) of the beams at the stage's start pose."""
    tx, ty, th = st["start"]
    bx, by = r["bx"].astype(np.float64), r["by"].astype(np.float64)
    ex, ey = np.cos(th) * bx - np.sin(th) * by + tx, np.sin(th) * bx + np.cos(th) * by + ty
    return np.floor(ex).astype(np.int64), np.floor(ey).astype(np.int64)


def negative_and_positive_cells(r: dict, st: dict, nc: int) -> bool:
    """Whether the left operands of ndt_point's two % (global cell index less the grid's shift) take both signs on either
    axis, over the beams inside the region at the start pose."""
    u, w = beam_cells(r, st)
    N = r["occ"].shape[0]
    live = (u >= 0) & (u < N) & (w >= 0) & (w < N)
    h = nc >> 1
    gu, gw = u[live] + r["ox"], w[live] + r["oy"]
    return bool((gu - h < 0).any() and (gu >= 0).any() and (gw - h < 0).any() and (gw >= 0).any())


def cpu_engine(c: AdjCase):
    """What oracle_particle reads of an engine, for the CPU."""
    return SimpleNamespace(cfg=SimpleNamespace(cell_size=c.cell_size, match_min_range=1e-3, match_max_range=c.max_range))


@lru_cache(maxsize=None)
def cpu_solution(name: str):
    """Per particle: (grid dict, stage, stage with the beams reversed), sines and cosines from NumPy."""
    c = CASES[name]
    _, last, (x, y) = scans(name)
    e, covs = cpu_engine(c), covariances(c)
    out = []
    for p, pose in enumerate(c.poses):
        r = oracle_particle(e, p, x, y, np.array(pose), covs[p], True, last, sincos=mo.np_sincos)
        out.append((r, stage(r, c.nc, c.mode), stage(r, c.nc, c.mode, reverse=True)))
    return out


def order_sensitivity(names) -> Tuple[float, float]:
    """Worst pose (m / rad) and relative score difference of the reference with itself under reversed beam order."""
    dp, ds = 0.0, 0.0
    for n in names:
        for r, a, b in cpu_solution(n):
            mcs = r["mcs"]
            d = np.abs(a["pose"] - b["pose"]) * [mcs, mcs, 1.0]
            dp = max(dp, float(d.max()))
            ds = max(ds, abs(a["score"] - b["score"]) / max(abs(a["score"]), 1e-300))
    return dp, ds


def general_bounds(names=("nc4", "nc3", "nc5")) -> Tuple[float, float]:
    """nc != 2 tolerances (pose absolute, score relative): 64 times the reference's summation-order sensitivity, at
    least 1e-12 -- and never above the nc == 2 bound, or the cases are badly conditioned."""
    dp, ds = order_sensitivity(names)
    bp, bs = max(GENERAL_MARGIN * dp, GENERAL_FLOOR), max(GENERAL_MARGIN * ds, GENERAL_FLOOR)
    assert bp <= NC2_POSE_TOL and bs <= NC2_SCORE_RTOL, (dp, ds)
    return bp, bs
