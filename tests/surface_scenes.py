"""Two small analytic scenes for the score-surface tests: a corridor, where a match is sharp across and flat
along, and a square room, where a quarter turn fits almost as well as the truth when the robot stands at the centre.  Ranges
are exact ray-wall intersections in float64; nothing is random.  Each scene is (poses [6, 3], ranges [6, B], angles [B], pair,
search): five reference scans and the query, scan 5, matched against the run 0 .. 4."""
import math

import numpy as np

B = 90                                                   # beams, all round
ANGLES = -math.pi + (np.arange(B) + 0.5) * (2.0 * math.pi / B)
CELL = 0.1
RANGES = dict(min_range=0.2, max_range=8.0)
PAIR = np.array([[5, 0, 5]], dtype=np.int32)


def corridor_ranges(pose):
    """Walls at y = +-1 m, endless along x."""
    x, y, th = pose
    out = []
    for a in ANGLES:
        s = math.sin(th + a)
        out.append(((1.0 - y) / s if s > 0 else (-1.0 - y) / s) if abs(s) > 1e-9 else 1e9)
    return np.array(out)


def room_ranges(pose, half=2.0):
    """A square room of 2 * half metres a side round the origin."""
    x, y, th = pose
    out = []
    for a in ANGLES:
        c, s = math.cos(th + a), math.sin(th + a)
        tx = ((half - x) / c if c > 0 else (-half - x) / c) if abs(c) > 1e-12 else math.inf
        ty = ((half - y) / s if s > 0 else (-half - y) / s) if abs(s) > 1e-12 else math.inf
        out.append(min(tx, ty))
    return np.array(out)


def _scene(cast, poses, window, rotations, rot_step):
    poses = np.array(poses, dtype=np.float64)
    ranges = np.stack([cast(p) for p in poses])
    search = dict(cell_size=CELL, substeps=1, window=window, rotations=rotations, rot_step=rot_step, **RANGES)
    return poses, ranges, ANGLES.copy(), PAIR.copy(), search


def corridor():
    """W = 6, R = 4 steps of 0.5 degrees: 1521 candidates.  The run walks 0.4 m along the corridor; the query stands in it."""
    poses = [(0.1 * n, 0.02, 0.0) for n in range(5)] + [(0.23, -0.04, 0.01)]
    return _scene(corridor_ranges, poses, 6, 4, math.radians(0.5))


def room(centre=(0.0, 0.0)):
    """W = 3, R = 19 steps of 5 degrees: 1911 candidates, a quarter turn (18 steps) inside the window.  The run and the query
    stand within 4 cm of `centre`."""
    cx, cy = centre
    poses = [(cx + 0.01 * n, cy - 0.005 * n, 0.0) for n in range(5)] + [(cx + 0.03, cy + 0.02, 0.0)]
    return _scene(room_ranges, poses, 3, 19, math.radians(5.0))


def oracle_volume(scene):
    """(pose [3], m8 [8], scores [nk, nw, nw]) of the scene's pair from tests.pairs_oracle.match_one."""
    from tests import pairs_oracle
    poses, ranges, angles, pair, s = scene
    return pairs_oracle.match_one(poses, ranges, angles, pair[0], None, 1.0 / s["cell_size"], s["min_range"], s["max_range"], s["substeps"],
                                  s["window"], s["rotations"], s["rot_step"])
