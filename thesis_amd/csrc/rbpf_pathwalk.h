// rbpf_pathwalk.h -- the walk of a path check, once, for every kernel that walks one (kernels_paths.hip: check_paths_kernel reads
// waypoint cells the host formed, check_rollouts_kernel places them itself; include/rbpf_hip.h, rbpf_check_paths, has the rule;
// DESIGN 3.22 and 3.24).  A wave holds one path: its waypoint cells and the step at which the walk stands on each.
//   clearance   the row trick of travel_mask_kernel without its rasters: in the row at offset dx only the occupied cell nearest in
//               y counts, found with count-trailing / leading-zeros on the row's occupancy bits; rows in the order 0, +-1, +-2, ...
//               until 5 |dx| >= min(best, cap), which is exact because 5 max(|dx|, |dy|) + 2 min(|dx|, |dy|) >= 5 |dx|.
//   reduction   two mins and a sum by wave shuffles; lane 0 stores the four results.  No atomics, no scratch rasters.
#pragma once
#include "rbpf_device.h"

namespace rbpf {

static const int PATH_WAVES = 4;       // paths of a workgroup, a wave each
static const int PATH_STAGE = 128;     // waypoints of a path staged in LDS

// Occupancy bits of n <= 64 cells of lattice row u from column w0 on: bit k = cell (u, w0 + k) is occupied.  0 outside the lattice,
// without a tile and outside a tile's written box (as occ_word32), but read a tile's word at a time.
__device__ __forceinline__ uint64_t occ_run64(const DevView& v, const int32_t* __restrict__ tab, int u, int w0, int n) {
    const int dim = v.dim, edge = v.L * dim;
    if (u < 0 || u >= edge) return 0ull;
    const int a = u / dim, i = u - a * dim, hi = min(w0 + n, edge);
    uint64_t bits = 0ull;
    for (int w = max(w0, 0); w < hi; ) {
        const int b = w / dim, j = w - b * dim;
        const int end = min(b * dim + min((j | 31) + 1, dim), hi);        // the end of this word of this tile, or of the run
        const int tile = tab[a * v.L + b];
        if (tile >= 0) {
            uint32_t word = v.occ[(size_t)tile * dim * v.ow + (size_t)i * v.ow + (j >> 5)] >> (j & 31);
            if (end - w < 32) word &= (1u << (end - w)) - 1u;
            bits |= (uint64_t)word << (w - w0);
        }
        w = end;
    }
    return bits;
}

// min(d, cap) at lattice cell (u, w), d the chamfer distance to the nearest occupied cell of the map; 1 <= cap <= 320
__device__ inline int path_clearance(const DevView& v, const int32_t* __restrict__ tab, int u, int w, int cap) {
    int best = cap;
    for (int ax = 0; 5 * ax < best; ++ax) {
        const int r = (best - 1) / 5;                                      // a cell farther off in y cannot improve best; r <= 63
        for (int side = 0; side < (ax ? 2 : 1); ++side) {
            const int row = side ? u - ax : u + ax;
            const uint64_t right = occ_run64(v, tab, row, w, r + 1), left = occ_run64(v, tab, row, w - r, r + 1);   // bit r of left is column w
            const int dr = right ? __builtin_ctzll(right) : 64, dl = left ? r - 63 + __builtin_clzll(left) : 64;
            const int g = min(dr, dl);
            if (g < 64) best = min(best, 5 * max(ax, g) + 2 * min(ax, g));
        }
    }
    return best;
}

// The cell of step t = 0 .. n of the segment from A to B (rbpf_pathbatch.h, path_segment_cell: the same expression).  t <= n < 2^20
// and the minor axis' change is <= n, so 2 t a + n < 2^42 in 64 bits: no overflow whatever the lattice.
__device__ __forceinline__ void path_cell(int xa, int ya, int xb, int yb, int t, int& x, int& y) {
    const int dx = xb - xa, dy = yb - ya, ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, n = max(ax, ay);
    const int minor = (int)((2ull * (uint64_t)t * (uint64_t)min(ax, ay) + (uint64_t)n) / (2ull * (uint64_t)n));
    const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    if (ax >= ay) { x = xa + sx * t; y = ya + sy * minor; }
    else { y = ya + sy * t; x = xa + sx * minor; }
}

// what the rule of a blocked step takes from the call
struct PathRule {
    int inflate, clear_max;            // a cell carries the robot if d > inflate; min_clearance is capped at clear_max
    int through_unknown, start_exempt; // 1: blocked = occupied, else v >= 0; 1: the cell of step 0 always carries the robot
};

// A wave walks the path of nw >= 1 waypoints through the map whose tile table is `tab`: lane l takes the steps l, l + 64, ... of
// the 1 + step_of(nw - 1) there are, and lane 0 stores the four results at o.  step_of(j): the step at which the walk stands on
// waypoint j; cell_of(j, x, y): its cell, counted from the lattice's first.  Every waypoint's cell lies in the lattice (the host
// sees to it), so every walked cell and its side cells do.
template <class StepOf, class CellOf>
__device__ __forceinline__ void path_walk(const DevView& v, const int32_t* __restrict__ tab, const PathRule& a, int nw, int lane,
                                          StepOf step_of, CellOf cell_of, int32_t* __restrict__ o) {
    const int dim = v.dim;
    auto value = [&](int x, int y) -> int {
        const int ta = x / dim, tb = y / dim, tile = tab[ta * v.L + tb];
        return tile >= 0 ? (int)v.pool[(size_t)tile * dim * dim + (size_t)(x - ta * dim) * dim + (y - tb * dim)] : 0;
    };
    int x0, y0;
    cell_of(0, x0, y0);
    auto ok = [&](int x, int y) -> bool {                 // a side cell of a diagonal step
        if (a.start_exempt && x == x0 && y == y0) return true;
        if (!a.through_unknown && value(x, y) >= 0) return false;
        return path_clearance(v, tab, x, y, a.inflate + 1) > a.inflate;
    };
    const int S = step_of(nw - 1) + 1;
    int blocked = INT32_MAX, unknown = INT32_MAX, clear = a.clear_max, n_unknown = 0;
    for (int s = lane; s < S; s += 64) {
        int x = x0, y = y0, xp = x0, yp = y0;
        if (s > 0) {
            int lo = 1, hi = nw - 1;                      // the first waypoint j with step_of(j) >= s: the step lies on segment j - 1 -> j
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (step_of(mid) < s) lo = mid + 1; else hi = mid; }
            int xa, ya, xb, yb;
            cell_of(lo - 1, xa, ya); cell_of(lo, xb, yb);
            const int t = s - step_of(lo - 1);            // 1 .. n
            path_cell(xa, ya, xb, yb, t, x, y);
            path_cell(xa, ya, xb, yb, t - 1, xp, yp);      // t - 1 = 0 is A, where the step before stands
        }
        const int val = value(x, y), d = path_clearance(v, tab, x, y, a.clear_max);
        bool free_ = (a.start_exempt && x == x0 && y == y0) || ((a.through_unknown || val < 0) && d > a.inflate);
        if (free_ && x != xp && y != yp) free_ = ok(x, yp) && ok(xp, y);
        if (!free_) blocked = min(blocked, s);
        if (val == 0) { unknown = min(unknown, s); ++n_unknown; }
        clear = min(clear, d);
    }
    for (int off = 32; off > 0; off >>= 1) {
        blocked = min(blocked, __shfl_down(blocked, off, 64));
        unknown = min(unknown, __shfl_down(unknown, off, 64));
        clear = min(clear, __shfl_down(clear, off, 64));
        n_unknown += __shfl_down(n_unknown, off, 64);
    }
    if (lane == 0) { o[0] = blocked == INT32_MAX ? -1 : blocked; o[1] = unknown == INT32_MAX ? -1 : unknown; o[2] = clear; o[3] = n_unknown; }
}

}  // namespace rbpf
