"""Scalar oracle of rbpf_check_footprints (include/rbpf_hip.h) on a rendered raster.  The walk is the
incremental one of tests/paths_oracle.py, a segment at a time - not the closed form of the kernel - the clearance is
travel_oracle.clearance, and the rule of the bins a step tests and the rule of a blocked step are written out once more, cell by
cell: the table is turned into lists of cells first (plan.footprint_cells), no span is looked at here.

The raster is the box of the centre cells grown by g = grow(clear_max, reach) cells on every side (ParticleEngine.render_map of
the grown box: 0 outside the tiles and outside the lattice), so that it holds the clearance margin and every covered cell."""
import numpy as np

from tests import paths_oracle as PO
from tests import travel_oracle as T
from thesis_amd import plan


def table_reach(fp):
    return int(np.abs(np.asarray(fp.spans)).max())


def grow(clear_max, reach):
    return max(T.margin(clear_max), int(reach))


def grown_box(box, clear_max, reach):
    g = grow(clear_max, reach)
    return (box[0] - g, box[1] + g, box[2] - g, box[3] + g)


def walk_bins(cells, bins):
    """[(cell, [bins])] of the walk through the waypoint cells: step 0 stands on waypoint 0; a segment of n steps from waypoint
    j - 1 to j adds its steps t = 1 .. n, of which t = n stands on waypoint j and t < n tests the bin of j - 1 if 2 t < n, else
    that of j; a segment of no step adds the bin of j to the step the walk stands on."""
    cells = [(int(x), int(y)) for x, y in cells]
    out = [(cells[0], [int(bins[0])])]
    for j in range(1, len(cells)):
        seg = PO.bresenham([cells[j - 1], cells[j]])[1:]
        n = len(seg)
        if n == 0:
            out[-1][1].append(int(bins[j]))
        for t, c in enumerate(seg, start=1):
            out.append((c, [int(bins[j] if t == n or 2 * t >= n else bins[j - 1])]))
    return out


class Field:
    """What a check needs of one map over one box of centre cells, computed once and shared by every rollout."""

    def __init__(self, wide, box, quantum, occupied_threshold, inflate, clear_max, fp, through_unknown=False):
        assert 0 <= inflate < clear_max <= 320
        self.g, m = grow(clear_max, table_reach(fp)), T.margin(clear_max)
        nx, ny = box[1] - box[0], box[3] - box[2]
        wide = np.asarray(wide)
        assert wide.shape == (nx + 2 * self.g, ny + 2 * self.g)
        self.box, self.inflate, self.clear_max = tuple(box), int(inflate), int(clear_max)
        self.v = wide.astype(np.int64)                                       # cell (X, Y) is v[X - x0 + g, Y - y0 + g]
        k = self.g - m
        self.clear = T.clearance(wide[k:wide.shape[0] - k, k:wide.shape[1] - k], clear_max, quantum, occupied_threshold).astype(np.int64)   # the box alone
        self.blocked = (self.v.astype(np.float64) * float(quantum) > float(occupied_threshold)) if through_unknown else self.v >= 0
        self.cells = [plan.footprint_cells(fp, b) for b in range(fp.H)]

    def check(self, cells, bins, exempt=-1):
        """(first_blocked, first_unknown, min_clearance, n_unknown, steps) of one rollout: waypoint cells (mosaic) and their bins."""
        walk = walk_bins(cells, bins)
        x0, y0, g = self.box[0], self.box[2], self.g
        fx, fy = walk[0][0]
        first_blocked = first_unknown = -1
        n_unknown, min_clear = 0, self.clear_max
        for s, ((x, y), tested) in enumerate(walk):
            i, j = x - x0, y - y0
            assert 0 <= i < self.clear.shape[0] and 0 <= j < self.clear.shape[1], "the rollout leaves the oracle's box"
            d = int(self.clear[i, j])
            ex = exempt >= 0 and max(abs(x - fx), abs(y - fy)) <= exempt
            bad = (not ex) and (bool(self.blocked[i + g, j + g]) or d <= self.inflate)
            unknown = self.v[i + g, j + g] == 0
            for b in tested:
                cx, cy = self.cells[b][:, 0] + x, self.cells[b][:, 1] + y
                vals, stop = self.v[cx - x0 + g, cy - y0 + g], self.blocked[cx - x0 + g, cy - y0 + g]
                if exempt >= 0:
                    stop = stop & ~(np.maximum(np.abs(cx - fx), np.abs(cy - fy)) <= exempt)
                bad = bad or bool(stop.any())
                unknown = unknown or bool((vals == 0).any())
            if bad and first_blocked < 0:
                first_blocked = s
            if unknown:
                n_unknown += 1
                if first_unknown < 0:
                    first_unknown = s
            min_clear = min(min_clear, d)
        return first_blocked, first_unknown, min_clear, n_unknown, len(walk)


def rollout_cells(poses, templates, headings, H, inv):
    """[N][K] (waypoint cells, bins): the templates placed by plan.place_templates, the bins (pose bin + waypoint bin) mod H."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    pb = plan.heading_bins(poses[:, 2], H)
    out = []
    for n in range(len(poses)):
        row = []
        for t, hd in zip(templates, headings):
            xy = plan.place_templates(poses[n], np.asarray(t, dtype=np.float64)[None, :, :2])[0]
            row.append((T.cells_of(xy, inv), (int(pb[n]) + plan.heading_bins(hd, H).astype(np.int64)) % H))
        out.append(row)
    return out


def box_of(rollouts):
    c = np.concatenate([cells for row in rollouts for cells, _ in row])
    return (int(c[:, 0].min()), int(c[:, 0].max()) + 1, int(c[:, 1].min()), int(c[:, 1].max()) + 1)


def check_all(field, rollouts, exempt=-1):
    """(int32 [N, K, 4], steps int32 [N, K]) of rollout_cells' result in one map."""
    res = [[field.check(cells, bins, exempt) for cells, bins in row] for row in rollouts]
    a = np.array(res, dtype=np.int32)
    return a[..., :4].copy(), a[..., 4].copy()
