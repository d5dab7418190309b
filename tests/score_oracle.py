"""Scalar oracle of rbpf_score_maps (include/rbpf_hip.h), written from the definitions with whole-array
comparisons and shifts: classes by comparison, "within Chebyshev distance tol" by or-ing the (2 tol + 1)^2 shifted copies of the
occupancy mask, every field a count or a sum over the box.  It shares nothing with the kernels' method (bit planes in LDS, packed
counters, atomics) and nothing with thesis_amd.mapeval.

The particle's raster is the box grown by `tol` cells on every side (ParticleEngine.render_map of the grown box: 0 outside the
tiles and outside the lattice), so that the real map decides near the box edge.  The reference exists inside the box only."""
import numpy as np

FIELDS = ("n_FF", "n_FU", "n_FO", "n_UF", "n_UU", "n_UO", "n_OF", "n_OU", "n_OO", "hit_m", "hit_r", "l1", "tab")
F, U, O = 0, 1, 2


def grown_box(box, tol):
    t = int(tol)
    return (box[0] - t, box[1] + t, box[2] - t, box[3] + t)


def occupied(x, quantum, threshold):
    return np.asarray(x).astype(np.float64) * float(quantum) > float(threshold)


def classes(x, quantum, threshold):
    """0 (F) where x < 0, 2 (O) where occupied, 1 (U) elsewhere."""
    x = np.asarray(x).astype(np.int64)
    return np.where(x < 0, F, np.where(occupied(x, quantum, threshold), O, U))


def near(occ_grown, tol):
    """For a mask over a box grown by tol: bool over the box, "some True cell within Chebyshev distance tol"."""
    t = int(tol)
    nx, ny = occ_grown.shape[0] - 2 * t, occ_grown.shape[1] - 2 * t
    out = np.zeros((nx, ny), bool)
    for di in range(2 * t + 1):
        for dj in range(2 * t + 1):
            out |= occ_grown[di:di + nx, dj:dj + ny]
    return out


def scores(grown_cells, box, ref, tol, table, quantum, threshold, vmin=-30):
    """The 13 fields (int64) for one particle: `grown_cells` [nx + 2 tol, ny + 2 tol] its raster over grown_box(box, tol),
    `ref` [nx, ny] the reference over `box`, `table` one int per lattice value from `vmin` up, or None."""
    t = int(tol)
    g = np.asarray(grown_cells).astype(np.int64)
    r = np.asarray(ref).astype(np.int64)
    nx, ny = box[1] - box[0], box[3] - box[2]
    assert g.shape == (nx + 2 * t, ny + 2 * t) and r.shape == (nx, ny)
    v = g[t:t + nx, t:t + ny]
    cv, cr = classes(v, quantum, threshold), classes(r, quantum, threshold)
    out = [int(((cv == a) & (cr == b)).sum()) for a in (F, U, O) for b in (F, U, O)]
    occ_r_grown = np.zeros_like(g, dtype=bool)            # no reference outside the box
    occ_r_grown[t:t + nx, t:t + ny] = cr == O
    near_m, near_r = near(occupied(g, quantum, threshold), t), near(occ_r_grown, t)
    out.append(int(((cv == O) & near_r).sum()))
    out.append(int(((cr == O) & near_m).sum()))
    out.append(int(np.abs(v - r).sum()))
    out.append(0 if table is None else int(np.asarray(table).astype(np.int64)[v - int(vmin)].sum()))
    return np.array(out, dtype=np.int64)
