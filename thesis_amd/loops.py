"""Loops closed after the run (ParticleEngine.match_pairs; include/rbpf_hip.h, rbpf_match_pairs).

A path that comes back to a place with accumulated drift draws that place twice, and refine_trajectory cannot mend it: each copy
of a wall holds its own scans where they are.  Here a scan is matched against earlier scans only, over a window wide enough for
the drift (candidates, match), the matches become constraints between poses, and a 2-D pose graph spreads them along the path
(relax).  close_loops runs the three on a filter's trajectory log and draws the map again; refine_trajectory then polishes it:

    closed = loops.close_loops(pf.engine, pf.scans, angles, min_gap=200, radius=3.0)
    polished = refine.refine_trajectory(pf.engine, pf.scans, angles, poses=closed.poses)
    raster = rebuild.as_raster(polished.built, engine=pf.engine)

By default candidates come from the poses, not from appearance: a loop whose drift exceeds `radius` plus the search window is
not found that way.  candidates="appearance" asks the scans instead (candidates_by_appearance; ParticleEngine.describe_scans and
match_places): every scan becomes a polar occupancy image, the earlier scan that looks most like the query,
and the turn at which it does, give the pair and its guess, whatever the drift:

    closed = loops.close_loops(pf.engine, pf.scans, angles, min_gap=200, candidates="appearance")

A match says more than its best candidate.  In a corridor it is sharp across and arbitrary along; in a nearly symmetric room a
second place fits almost as well.  information="surface" reads both off the score volume on the GPU (match_informed;
ParticleEngine.score_surface): every loop edge gets an information matrix of its own, weak where its match was
flat, and max_ambiguity refuses a match whose runner-up comes too close:

    closed = loops.close_loops(pf.engine, pf.scans, angles, min_gap=200, information="surface", max_ambiguity=0.8)

Everything here is host NumPy and SciPy; the searches run on the GPU.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional

import numpy as np

from . import rebuild as _rebuild
from . import refine as _refine

SCRATCH_BYTES = 1 << 30    # what match() lets one match_pairs call take of the library's 4 GiB


class LoopEdges(NamedTuple):
    q: np.ndarray              # [M] int32: the query scan of each pair
    r: np.ndarray              # [M] int32: the middle scan of its run, whose frame z is in
    z: np.ndarray              # [M, 3]: the matched pose of scan q seen from poses[r]: (R_r^T (t_q - t_r), theta_q - theta_r)
    fraction: np.ndarray       # [M] score / (2 n_used) of the match, 0 where no beam was used
    fraction_guess: np.ndarray # [M] the same of the guess
    accepted: np.ndarray       # [M] bool


class InformedEdges(NamedTuple):
    edges: LoopEdges           # match()'s edges; `accepted` also refuses ambiguity > max_ambiguity where that is given
    information: np.ndarray    # [M, 3, 3] of z in the frame of poses[r] (edge_information)
    ambiguity: np.ndarray      # [M] score of the second peak / score of the best, 0 where there is no second peak
    surface: object            # ScoreSurface of all pairs, host arrays


class LoopRound(NamedTuple):
    pairs: int                 # candidate pairs
    accepted: int              # loop edges that went into the graph
    moved: float               # the largest translation of a pose in the relaxation, metres


class ClosedTrajectory(NamedTuple):
    poses: np.ndarray          # [n, 3] the poses of the scans after the last round
    records: np.ndarray        # [n] int64: the trajectory record of each
    edges: LoopEdges           # the last round's pairs
    built: object              # BuiltMap: the map the poses draw
    rounds: List[LoopRound]


def _wrap(a):
    return (np.asarray(a) + math.pi) % (2.0 * math.pi) - math.pi


def candidates(poses, min_gap: int, radius: float, half_run: int = 5, stride: int = 1, per_query: int = 1) -> np.ndarray:
    """Pairs {q, r0, r1} int32 [M, 3] for match_pairs.  For every `stride`-th scan q: the earlier scans r with r + half_run <
    q - min_gap (the whole run lies more than min_gap scans back) within `radius` metres of q's position, nearest first, ties
    to the smaller r, `per_query` of them; each gives the run max(r - half_run, 0) .. r + half_run.  Empty [0, 3] if none."""
    t = np.asarray(poses, dtype=np.float64).reshape(-1, 3)[:, :2]
    if min_gap < 0 or half_run < 0 or stride < 1 or per_query < 1 or not radius >= 0.0:
        raise ValueError("min_gap >= 0, radius >= 0, half_run >= 0, stride >= 1 and per_query >= 1 are required")
    out = []
    for q in range(0, len(t), int(stride)):
        last = q - int(min_gap) - int(half_run)          # r < last
        if last <= 0:
            continue
        d = np.hypot(t[:last, 0] - t[q, 0], t[:last, 1] - t[q, 1])
        near = np.flatnonzero(d <= radius)
        for r in near[np.argsort(d[near], kind="stable")][:int(per_query)]:
            out.append((q, max(int(r) - int(half_run), 0), int(r) + int(half_run) + 1))
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def candidates_by_appearance(engine, poses, ranges, angles, min_gap: int, half_run: int = 5, stride: int = 1, ref_stride: int = 1,
                             per_query: int = 1, rings: int = 24, min_similarity: float = 0.0, min_range: Optional[float] = None,
                             max_range: Optional[float] = None):
    """Pairs for match_pairs from what the scans look like, wherever their poses are: (pairs {q, r0, r1} int32 [M, 3], guesses
    [M, 3], similarity [M]).  engine.describe_scans describes every scan (`rings`, `min_range`, `max_range`), engine.match_places
    compares every `stride`-th scan q with every `ref_stride`-th scan r, r + half_run < q - min_gap as in candidates().  Of its
    min(16, 4 per_query) best references a query keeps up to `per_query`, in rank order: one is kept if its similarity reaches
    `min_similarity` and it lies more than half_run scans from every one kept before.  Each gives the run max(r - half_run, 0)
    .. r + half_run and the guess (x_r, y_r, wrap(theta_r - shift * 2 pi / 64)): the query on the reference, turned as the
    descriptors say.  min_similarity is a prefilter that saves search work; match()'s acceptance rule is the verifier."""
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    if min_gap < 0 or half_run < 0 or stride < 1 or ref_stride < 1 or per_query < 1:
        raise ValueError("min_gap >= 0, half_run >= 0, stride >= 1, ref_stride >= 1 and per_query >= 1 are required")
    none = np.zeros((0, 3), np.int32), np.zeros((0, 3)), np.zeros(0)
    n = len(p)
    qs = np.arange(0, n, int(stride))
    rs = np.arange(0, n, int(ref_stride))
    # references r < q - min_gap - half_run: the first of rs that is not, per query
    limit = np.searchsorted(rs, qs - int(min_gap) - int(half_run), side="left").astype(np.int32)
    some = limit > 0
    if not some.any():
        return none
    qs, limit = qs[some], limit[some]
    desc = engine.describe_scans(ranges, angles, rings=rings, min_range=min_range, max_range=max_range).desc
    found = engine.match_places(desc[qs], desc[rs[:int(limit.max())]], ref_limit=limit, k=min(16, 4 * int(per_query)))
    sim = found.similarity()
    pairs, guesses, sims = [], [], []
    for m, q in enumerate(qs):
        kept = []
        for j in range(int(found.count[m])):
            r = int(rs[found.ref[m, j]])
            if len(kept) == int(per_query):
                break
            if sim[m, j] < min_similarity or any(abs(r - o) <= int(half_run) for o in kept):
                continue
            kept.append(r)
            pairs.append((int(q), max(r - int(half_run), 0), r + int(half_run) + 1))
            guesses.append((p[r, 0], p[r, 1], float(_wrap(p[r, 2] - int(found.shift[m, j]) * (2.0 * math.pi / 64.0)))))
            sims.append(float(sim[m, j]))
    if not pairs:
        return none
    return np.array(pairs, dtype=np.int32).reshape(-1, 3), np.array(guesses, dtype=np.float64).reshape(-1, 3), np.array(sims)


def pairs_per_call(engine, n_scans: int, n_beams: int, cell_size=None, substeps: int = 1, window: int = 16, rotations: int = 20,
                   max_range=None, limit: Optional[int] = None, scores: bool = False, **_) -> int:
    """How many pairs one match_pairs call takes within `limit` bytes of scratch (default SCRATCH_BYTES; include/rbpf_hip.h
    has the terms): per pair 112 bytes with the host outputs, 32 per rotation and the field of its window; per scan 32 bytes
    and 8 per beam.  scores=True counts the score volume as well, 4 bytes per candidate."""
    inv = engine.dim / float(engine.cfg.tile_len_m) if cell_size is None else 1.0 / float(cell_size)
    hi = float(engine.cfg.match_max_range if max_range is None else max_range)
    mw = int(math.ceil(hi * inv)) + -(-int(window) // int(substeps)) + 2
    ww = (((2 * mw + 32) >> 5) + 2) | 1
    per_pair = 112 + 32 * (2 * int(rotations) + 1) + (2 * mw + 1) * ww * 8
    if scores:
        per_pair += 4 * (2 * int(rotations) + 1) * (2 * int(window) + 1) ** 2
    fixed = n_scans * (32 + 8 * n_beams) + 16 * n_beams + 4096
    return max(1, (int(SCRATCH_BYTES if limit is None else limit) - fixed) // per_pair)


def match(engine, poses, ranges, angles, pairs, accept: float = 0.55, gain: float = 0.1, min_used: int = 30, guesses=None,
          **search) -> LoopEdges:
    """match_pairs on `pairs` (from candidates) with the scans' current poses as guesses, or with `guesses` [M, 3] (from
    candidates_by_appearance; fraction_guess is then the appearance guess's), in as many calls as the scratch limit asks for.
    Edge m says where scan q sits in the frame of poses[r], r = (r0 + r1) // 2 the middle of the run.  It is accepted if its
    fraction score / (2 n_used) reaches `accept` with at least `min_used` beams, and the search either raised the guess's
    fraction by `gain` or kept the guess: a match that moved the pose for nothing is noise.  `search` goes to
    ParticleEngine.match_pairs (cell_size, substeps, window, rotations, rot_step, min_range, max_range)."""
    for bad in ("return_scores", "device"):
        if bad in search:
            raise ValueError(f"match() reads every result on the host: {bad} is not for it")
    found, _ = _search(engine, poses, ranges, angles, pairs, guesses, search)
    return _edges(*found, accept, gain, min_used)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def _search(engine, poses, ranges, angles, pairs, guesses, search, reduce=None):
    """match_pairs on `pairs` in as many calls as the scratch limit asks for, gathered on the host: ((poses, q, r, matched
    poses, index, score, score of the guess, n_used), parts).  With `reduce`, every call keeps its results and its score
    volume on the GPU (the volume counted against the limit) and `parts` holds reduce(result) of each call."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.ascontiguousarray(ranges, dtype=np.float64).reshape(len(poses), -1)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 3)
    M = len(pairs)
    if guesses is not None:
        guesses = np.ascontiguousarray(guesses, dtype=np.float64).reshape(-1, 3)
        if len(guesses) != M:
            raise ValueError(f"{len(guesses)} guesses for {M} pairs")
    q, r = pairs[:, 0].copy(), ((pairs[:, 1] + pairs[:, 2]) // 2).astype(np.int32)
    out, index, score, guess, used = np.empty((M, 3)), np.empty((M, 3), np.int32), np.empty(M, np.int64), np.empty(M, np.int64), np.empty(M, np.int64)
    on_gpu = {} if reduce is None else dict(return_scores=True, device=True)
    step = pairs_per_call(engine, len(poses), ranges.shape[1], scores=reduce is not None, **search)
    parts = []
    for k in range(0, M, step):
        res = engine.match_pairs(poses, ranges, angles, pairs[k:k + step], None if guesses is None else guesses[k:k + step], **on_gpu, **search)
        if reduce is not None:
            parts.append(reduce(res))
        out[k:k + step], index[k:k + step] = _host(res.poses), _host(res.index)
        score[k:k + step], guess[k:k + step], used[k:k + step] = _host(res.score), _host(res.score_guess), _host(res.n_used)
        del res                                          # a volume goes back to the allocator before the next call
    return (poses, q, r, out, index, score, guess, used), parts


def _edges(poses, q, r, out, index, score, guess, used, accept, gain, min_used) -> LoopEdges:
    """The edges and the acceptance rule of match() from the gathered results of match_pairs."""
    M = len(q)
    some = used > 0
    frac, frac_guess = np.zeros(M), np.zeros(M)
    frac[some], frac_guess[some] = score[some] / (2.0 * used[some]), guess[some] / (2.0 * used[some])
    c, s = np.cos(poses[r, 2]), np.sin(poses[r, 2])
    dx, dy = out[:, 0] - poses[r, 0], out[:, 1] - poses[r, 1]
    z = np.stack([c * dx + s * dy, -s * dx + c * dy, _wrap(out[:, 2] - poses[r, 2])], axis=1).reshape(M, 3)
    stayed = ~np.any(index != 0, axis=1)
    accepted = (frac >= accept) & (used >= min_used) & ((frac - frac_guess >= gain) | stayed)
    return LoopEdges(q, r, z, frac, frac_guess, accepted)


def edge_information(surface, theta_r, loop_sigma=(0.05, 0.01)) -> np.ndarray:
    """[M, 3, 3]: the information of each match as a measurement in the frame of a pose of heading `theta_r` [M].  The
    second moment C of the best peak's plateau (ScoreSurface.second_moment(0), along world x, world y and heading) is what
    the search itself could not tell apart; its translation block and translation-heading terms are turned into that frame,
    C' = T C T^T with T = diag(R(theta_r)^T, 1), and added to the fixed covariance: information = (diag(st^2, st^2, sh^2) +
    C')^-1 with (st, sh) = `loop_sigma`.  It never exceeds the fixed information, and equals it where the plateau is the
    peak alone."""
    C = np.asarray(surface.second_moment(0), dtype=np.float64)
    th = np.broadcast_to(np.asarray(theta_r, dtype=np.float64), (len(C),))
    T = np.zeros((len(C), 3, 3))
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th), 1.0
    fixed = np.array([float(loop_sigma[0]) ** 2, float(loop_sigma[0]) ** 2, float(loop_sigma[1]) ** 2])
    info = np.empty_like(C)
    flat = ~np.any(C != 0.0, axis=(1, 2))
    info[flat] = np.diag(1.0 / fixed)                    # no plateau beyond the peak: the fixed information, exactly
    rest = ~flat
    if rest.any():
        Cr = T[rest] @ C[rest] @ np.transpose(T[rest], (0, 2, 1))
        Cr = 0.5 * (Cr + np.transpose(Cr, (0, 2, 1)))
        info[rest] = np.linalg.inv(Cr + np.diag(fixed))
        info[rest] = 0.5 * (info[rest] + np.transpose(info[rest], (0, 2, 1)))
    return info


def match_informed(engine, poses, ranges, angles, pairs, accept: float = 0.55, gain: float = 0.1, min_used: int = 30, guesses=None,
                   loop_sigma=(0.05, 0.01), drop_fraction: float = 0.05, exclude=None, max_ambiguity: Optional[float] = None,
                   **search) -> InformedEdges:
    """match() that also reads the score volume of every pair, on the GPU: match_pairs runs with device=True and
    return_scores=True in match()'s batches (the volume counted against the scratch limit), engine.score_surface reduces each
    batch to two peaks and the best one's plateau (`drop_fraction`, `exclude`: its arguments), and only those records come to
    the host.  The edges and the acceptance rule are match()'s; an edge whose ambiguity (ScoreSurface.ambiguity) exceeds
    `max_ambiguity` is refused as well when that is given.  `information` is edge_information of every pair with `loop_sigma`."""
    for bad in ("return_scores", "device"):
        if bad in search:
            raise ValueError(f"match_informed() sets {bad} itself")
    from .engine import ScoreSurface
    found, parts = _search(engine, poses, ranges, angles, pairs, guesses, search,
                           reduce=lambda res: engine.score_surface(res, drop_fraction=drop_fraction, exclude=exclude, peaks=2))
    if parts:
        surface = ScoreSurface(*(np.concatenate([np.asarray(p[f]) for p in parts]) for f in range(6)), *parts[0][6:])
    else:
        z = np.zeros
        surface = ScoreSurface(z((0, 2, 3), np.int64), z((0, 2), np.int64), z(0, np.int32), z((0, 2), np.int64), z((0, 2, 10), np.int64),
                               z(0, np.int32), int(search.get("substeps", 1)), 0.0, 1.0)
    poses, r = found[0], found[2]
    edges = _edges(*found, accept, gain, min_used)
    ambiguity = surface.ambiguity()
    if max_ambiguity is not None:
        edges = edges._replace(accepted=edges.accepted & ~(ambiguity > float(max_ambiguity)))
    return InformedEdges(edges, edge_information(surface, poses[r, 2], loop_sigma), ambiguity, surface)


def relative(poses, i, j) -> np.ndarray:
    """[E, 3]: pose j seen from pose i, (R_i^T (t_j - t_i), wrap(theta_j - theta_i)): the measurement an edge (i, j) holds when
    the poses agree with it."""
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    c, s = np.cos(p[i, 2]), np.sin(p[i, 2])
    dx, dy = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1]
    return np.stack([c * dx + s * dy, -s * dx + c * dy, _wrap(p[j, 2] - p[i, 2])], axis=-1)


def relax(poses, edges_ij, z, sigma_t=None, sigma_th=None, iterations: int = 20, tol: float = 1e-9, information=None) -> np.ndarray:
    """The poses [n, 3] that fit the edges best: Gauss-Newton on the sum over the edges (i, j) of |e_t|^2 / sigma_t^2 +
    e_th^2 / sigma_th^2 with e = [R_i^T (t_j - t_i) - z_t; wrap(theta_j - theta_i - z_th)], analytic Jacobians, sparse normal
    equations, pose 0 held where it is.  sigma_t, sigma_th: a number, or one per edge.  Stops when no component of a step
    exceeds `tol`.  Poses no edge reaches from pose 0 make the system singular: the caller joins consecutive scans.
    `information` [E, 3, 3], a symmetric positive-definite matrix per edge in the frame of pose i, replaces the sigmas: the
    sum is then over e^T information e, each edge's rows whitened by the Cholesky factor of its matrix."""
    from scipy import sparse
    from scipy.sparse.linalg import spsolve
    x = np.array(poses, dtype=np.float64).reshape(-1, 3)
    ij = np.asarray(edges_ij, dtype=np.int64).reshape(-1, 2)
    z = np.asarray(z, dtype=np.float64).reshape(-1, 3)
    n, E = len(x), len(ij)
    if E == 0 or n < 2:
        return x
    if len(z) != E or ij.min() < 0 or ij.max() >= n or np.any(ij[:, 0] == ij[:, 1]):
        raise ValueError("edges must join two different poses and come with one measurement each")
    if information is not None:
        return _relax_information(x, ij, z, information, iterations, tol)
    if sigma_t is None or sigma_th is None:
        raise ValueError("relax needs sigma_t and sigma_th, or information")
    wt = 1.0 / np.broadcast_to(np.asarray(sigma_t, dtype=np.float64), (E,))
    wh = 1.0 / np.broadcast_to(np.asarray(sigma_th, dtype=np.float64), (E,))
    i, j = ij[:, 0], ij[:, 1]
    e3 = 3 * np.arange(E)
    for _ in range(int(iterations)):
        c, s = np.cos(x[i, 2]), np.sin(x[i, 2])
        dx, dy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
        ex, ey = (c * dx + s * dy - z[:, 0]) * wt, (-s * dx + c * dy - z[:, 1]) * wt
        eh = _wrap(x[j, 2] - x[i, 2] - z[:, 2]) * wh
        # rows 3e, 3e + 1, 3e + 2; columns 3i .. 3i + 2 and 3j .. 3j + 2
        rows = np.concatenate([e3, e3, e3, e3, e3, e3 + 1, e3 + 1, e3 + 1, e3 + 1, e3 + 1, e3 + 2, e3 + 2])
        cols = np.concatenate([3 * i, 3 * i + 1, 3 * i + 2, 3 * j, 3 * j + 1, 3 * i, 3 * i + 1, 3 * i + 2, 3 * j, 3 * j + 1, 3 * i + 2, 3 * j + 2])
        vals = np.concatenate([-c * wt, -s * wt, (-s * dx + c * dy) * wt, c * wt, s * wt,
                               s * wt, -c * wt, (-c * dx - s * dy) * wt, -s * wt, c * wt, -wh, wh])
        J = sparse.csc_matrix((vals, (rows, cols)), shape=(3 * E, 3 * n))[:, 3:]       # pose 0 is fixed
        e = np.stack([ex, ey, eh], axis=1).reshape(-1)
        step = spsolve((J.T @ J).tocsc(), -(J.T @ e))
        x[1:] += np.asarray(step).reshape(-1, 3)
        if np.max(np.abs(step)) < tol:
            break
    return x


def _relax_information(x, ij, z, information, iterations, tol) -> np.ndarray:
    """relax() with a full information matrix per edge: with information = L L^T the rows of an edge are L^T e and L^T J."""
    from scipy import sparse
    from scipy.sparse.linalg import spsolve
    n, E = len(x), len(ij)
    info = np.asarray(information, dtype=np.float64)
    if info.shape != (E, 3, 3) or not np.allclose(info, np.transpose(info, (0, 2, 1)), rtol=1e-9, atol=0.0):
        raise ValueError("information must be [E, 3, 3] and symmetric")
    try:
        Lt = np.transpose(np.linalg.cholesky(info), (0, 2, 1))
    except np.linalg.LinAlgError:
        raise ValueError("information must be positive definite") from None
    i, j = ij[:, 0], ij[:, 1]
    e3 = 3 * np.arange(E)
    # rows 3e + a, a = 0 .. 2; columns 3i + b and 3j + b, b = 0 .. 2
    rows = np.concatenate([np.repeat(e3[:, None] + np.arange(3), 3, axis=1).reshape(-1)] * 2)
    cols = np.concatenate([np.tile(3 * i[:, None] + np.arange(3), (1, 3)).reshape(-1), np.tile(3 * j[:, None] + np.arange(3), (1, 3)).reshape(-1)])
    zero, one = np.zeros(E), np.ones(E)
    for _ in range(int(iterations)):
        c, s = np.cos(x[i, 2]), np.sin(x[i, 2])
        dx, dy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
        e = np.stack([c * dx + s * dy - z[:, 0], -s * dx + c * dy - z[:, 1], _wrap(x[j, 2] - x[i, 2] - z[:, 2])], axis=1)
        Ji = np.stack([np.stack([-c, -s, -s * dx + c * dy], axis=1), np.stack([s, -c, -c * dx - s * dy], axis=1),
                       np.stack([zero, zero, -one], axis=1)], axis=1)
        Jj = np.stack([np.stack([c, s, zero], axis=1), np.stack([-s, c, zero], axis=1), np.stack([zero, zero, one], axis=1)], axis=1)
        vals = np.concatenate([(Lt @ Ji).reshape(-1), (Lt @ Jj).reshape(-1)])
        J = sparse.csc_matrix((vals, (rows, cols)), shape=(3 * E, 3 * n))[:, 3:]       # pose 0 is fixed
        we = (Lt @ e[:, :, None]).reshape(-1)
        step = spsolve((J.T @ J).tocsc(), -(J.T @ we))
        x[1:] += np.asarray(step).reshape(-1, 3)
        if np.max(np.abs(step)) < tol:
            break
    return x


def close_loops(engine, log, angles, particle="best", rounds: int = 1, odo_sigma=(0.02, 0.005), loop_sigma=(0.05, 0.01),
                cell_size: Optional[float] = None, build_args: Optional[dict] = None, poses=None, candidates: str = "pose",
                information: str = "fixed", max_ambiguity: Optional[float] = None, **search) -> ClosedTrajectory:
    """Closes the loops of a logged run.  refine.scan_poses picks the scans and the poses of `particle`'s trajectory (`poses`
    [n, 3] replaces them).  Each round: odometry edges between consecutive scans hold the current poses' own relative poses
    (sigmas `odo_sigma` = (metres, radians) per edge), candidates() proposes pairs, match() turns the accepted ones into loop
    edges (`loop_sigma`), relax() spreads them.  Then rebuild.rebuild_at draws the map at the new poses (`build_args`:
    min_range, max_range, box, device).  `search` holds candidates' min_gap (default 50), radius (2 m), half_run, stride and
    per_query, match's accept, gain and min_used, and match_pairs' search arguments.  With no accepted edge the poses come
    back as they went in, bit for bit.  `candidates`: "pose" proposes pairs from the poses as above; "appearance" from what the
    scans look like (candidates_by_appearance, which also takes ref_stride, rings and min_similarity from `search`, the ranges
    of the search, and ignores radius), each pair with its own guess; "both" the pose pairs and then the appearance pairs
    whose (q, middle r) no pose pair has.  `information`: "fixed" gives every loop edge `loop_sigma`; "surface" matches with
    match_informed (which also takes drop_fraction and exclude from `search`), gives every loop edge its own information
    matrix (edge_information: weak where the match was flat, never more than `loop_sigma` gives) and refuses the edges whose
    ambiguity exceeds `max_ambiguity` where that is given; odometry edges keep `odo_sigma` as diagonal matrices.
    max_ambiguity needs "surface"."""
    if information not in ("fixed", "surface"):
        raise ValueError(f"unknown information {information!r}: fixed or surface")
    if max_ambiguity is not None and information != "surface":
        raise ValueError('max_ambiguity needs information="surface"')
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    if candidates not in ("pose", "appearance", "both"):
        raise ValueError(f"unknown candidates {candidates!r}: pose, appearance or both")
    propose = globals()["candidates"]                    # the argument hides the function of that name
    records, start, ranges = _refine.scan_poses(engine, log, particle)
    if poses is not None:
        start = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        if len(start) != len(records):
            raise ValueError(f"{len(start)} poses for {len(records)} logged scans")
    search = dict(search)
    cand = {k: search.pop(k) for k in ("half_run", "stride", "per_query") if k in search}
    min_gap, radius = search.pop("min_gap", 50), search.pop("radius", 2.0)
    look = {}
    if candidates != "pose":
        look = {k: search.pop(k) for k in ("ref_stride", "rings", "min_similarity") if k in search}
        look.update({k: search[k] for k in ("min_range", "max_range") if k in search})
    if cell_size is not None:
        search["cell_size"] = cell_size
    informed = {k: search.pop(k) for k in ("drop_fraction", "exclude") if k in search} if information == "surface" else None
    cur = np.array(start, dtype=np.float64)
    n = len(cur)
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    out: List[LoopRound] = []
    edges = None
    for _ in range(rounds):
        pairs, guesses = None, None
        if candidates != "appearance":
            pairs = propose(cur, min_gap, radius, **cand)
        if candidates != "pose":
            seen, guesses, _ = candidates_by_appearance(engine, cur, ranges, angles, min_gap, **cand, **look)
            if pairs is None:
                pairs = seen
            else:                                        # pose pairs first, at their own poses; then what only appearance found
                have = {(int(q), (int(a) + int(b)) // 2) for q, a, b in pairs}
                fresh = np.array([(int(q), (int(a) + int(b)) // 2) not in have for q, a, b in seen], dtype=bool)
                guesses = np.concatenate([cur[pairs[:, 0]], guesses[fresh]])
                pairs = np.concatenate([pairs, seen[fresh]])
        if informed is None:
            edges = match(engine, cur, ranges, angles, pairs, guesses=guesses, **search)
        else:
            found = match_informed(engine, cur, ranges, angles, pairs, guesses=guesses, loop_sigma=loop_sigma, max_ambiguity=max_ambiguity,
                                   **informed, **search)
            edges = found.edges
        ok = edges.accepted
        if not ok.any():
            out.append(LoopRound(len(pairs), 0, 0.0))
            break
        n_ok = int(ok.sum())
        ij = np.concatenate([chain, np.stack([edges.r[ok], edges.q[ok]], axis=1)])
        z = np.concatenate([relative(cur, chain[:, 0], chain[:, 1]), edges.z[ok]])
        st = np.concatenate([np.full(n - 1, float(odo_sigma[0])), np.full(n_ok, float(loop_sigma[0]))])
        sh = np.concatenate([np.full(n - 1, float(odo_sigma[1])), np.full(n_ok, float(loop_sigma[1]))])
        if informed is None:
            new = relax(cur, ij, z, st, sh)
        else:
            odo = np.diag([float(odo_sigma[0]) ** -2, float(odo_sigma[0]) ** -2, float(odo_sigma[1]) ** -2])
            new = relax(cur, ij, z, information=np.concatenate([np.broadcast_to(odo, (n - 1, 3, 3)), found.information[ok]]))
        out.append(LoopRound(len(pairs), n_ok, float(np.hypot(new[:, 0] - cur[:, 0], new[:, 1] - cur[:, 1]).max())))
        cur = new
    built = _rebuild.rebuild_at(engine, cur, ranges, angles, cell_size=cell_size, **dict(build_args or {}))
    return ClosedTrajectory(cur, records, edges, built, out)
