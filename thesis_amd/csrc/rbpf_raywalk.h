// rbpf_raywalk.h -- the supercover (4-connected) ray walk of DESIGN 3.7 against the occupancy bit planes: one copy of the
// arithmetic for every kernel that walks it (kernels_cast.hip, kernels_gain.hip; kernels_scancheck.hip walks walk_ray_to).
//
// The walk is float64: the crossing parameters are (n + f) * td, functions of the step counts alone, so every lane reproduces
// the specification's values whatever its neighbours do.  A ray tests occ[tile][row][col >> 5], bit col & 31 (cell > threshold,
// zero outside a tile's written box like the cells themselves), 32 cells per 4-byte load.  The current word stays in a register
// and is loaded again only when (tile, row, col >> 5) changes.  The position is kept as (lattice tile, tile-local cell) per axis
// and stepped by +-1 with a wrap at the seam, so the loop has no division and the tile table is read only at a seam (and once
// at the start).  Every step moves one cell away from the origin along one axis, so a ray ends after at most 2 * L * dim steps
// (it has left the lattice by then).
#pragma once
#include "rbpf_internal.h"

namespace rbpf {

// ps = x, y, cos(theta), sin(theta); bm = cos(angle), sin(angle); tab = the particle's row of the tile table.  Returns the
// status of rbpf_cast_scans (1 hit, 0 nothing occupied within tlim, 2 the ray or its origin left the lattice); t is the
// parameter (cells) at which the last tested cell was entered.  visit(kx, ky) is called for every cell the loop tests while
// inside the lattice, the hit cell included: (kx, ky) = its offset from the origin cell, in cells.
template <class Visit>
__device__ __forceinline__ int walk_ray(const DevView& v, const int32_t* __restrict__ tab, const double4 ps, const double2 bm,
                                        const double inv, const double tlim, double& t, Visit&& visit) {
    const int L = v.L, dim = v.dim, ow = v.ow;
    const double ox = ps.x * inv, oy = ps.y * inv;                        // origin in mosaic-cell units
    const double dx = ps.z * bm.x - ps.w * bm.y, dy = ps.w * bm.x + ps.z * bm.y;
    const double fX = __builtin_floor(ox), fY = __builtin_floor(oy);
    const int off = v.R * dim + dim / 2;                                  // mosaic X + off = tile * dim + cell
    const double lo = -(double)off, hi = (double)(L * dim - off);
    t = 0.0;
    if (!(fX >= lo && fX < hi && fY >= lo && fY < hi)) return 2;          // (a NaN as well)
    const int u = (int)fX + off, w = (int)fY + off;
    int ta = u / dim, i = u - ta * dim, tb = w / dim, j = w - tb * dim;
    const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
    const double inf = __builtin_inf();
    // a ray along an axis never crosses the other one: (n + 1) * inf = inf stands for the specification's "inf"
    const double tdx = dx != 0 ? 1.0 / __builtin_fabs(dx) : inf, tdy = dy != 0 ? 1.0 / __builtin_fabs(dy) : inf;
    const double fx = dx != 0 ? (dx > 0 ? (fX + 1.0) - ox : ox - fX) : 1.0;
    const double fy = dy != 0 ? (dy > 0 ? (fY + 1.0) - oy : oy - fY) : 1.0;
    double nx = 0.0, ny = 0.0;                                            // step counts (exact in float64)
    int kx = 0, ky = 0;
    int cur_pos = -1, cur_w = -1, tile = -1;
    uint32_t word = 0u;
    for (;;) {
        if ((unsigned)ta >= (unsigned)L || (unsigned)tb >= (unsigned)L) return 2;           // left the lattice
        visit(kx, ky);
        const int pos = ta * L + tb, wi = i * ow + (j >> 5);
        if (pos != cur_pos) { tile = tab[pos]; cur_pos = pos; cur_w = -1; }
        if (wi != cur_w) {
            word = tile >= 0 ? v.occ[(size_t)tile * dim * ow + (size_t)wi] : 0u;              // no tile: free
            cur_w = wi;
        }
        if ((word >> (j & 31)) & 1u) return 1;
        const double tmx = (nx + fx) * tdx, tmy = (ny + fy) * tdy;
        const bool step_x = tmx < tmy;                                    // a tie steps in y
        t = step_x ? tmx : tmy;
        nx += step_x ? 1.0 : 0.0; ny += step_x ? 0.0 : 1.0;
        i += step_x ? sx : 0; j += step_x ? 0 : sy;
        kx += step_x ? sx : 0; ky += step_x ? 0 : sy;
        if (i == dim) { i = 0; ++ta; } else if (i < 0) { i = dim - 1; --ta; }
        if (j == dim) { j = 0; ++tb; } else if (j < 0) { j = dim - 1; --tb; }
        if (t > tlim) return 0;
    }
}

// The same ray with no map to test (kernels_build.hip).  ray_start is walk_ray's set-up, statement for statement;
// walk_ray keeps its own copy because taking it from here changed the register allocation of cast_scans_kernel, and that
// kernel is to compile as it did.  The origin cell (fX, fY) stays a double: it may lie outside any lattice.
struct RayStart { double fX, fY, tdx, tdy, fx, fy; int sx, sy; };
__device__ __forceinline__ RayStart ray_start(const double4 ps, const double2 bm, const double inv) {
    RayStart r;
    const double ox = ps.x * inv, oy = ps.y * inv;                        // origin in cells
    const double dx = ps.z * bm.x - ps.w * bm.y, dy = ps.w * bm.x + ps.z * bm.y;
    r.fX = __builtin_floor(ox); r.fY = __builtin_floor(oy);
    r.sx = dx > 0 ? 1 : -1; r.sy = dy > 0 ? 1 : -1;
    const double inf = __builtin_inf();
    r.tdx = dx != 0 ? 1.0 / __builtin_fabs(dx) : inf; r.tdy = dy != 0 ? 1.0 / __builtin_fabs(dy) : inf;
    r.fx = dx != 0 ? (dx > 0 ? (r.fX + 1.0) - ox : ox - r.fX) : 1.0;
    r.fy = dy != 0 ? (dy > 0 ? (r.fY + 1.0) - oy : oy - r.fY) : 1.0;
    return r;
}

// visit(kx, ky) for the origin cell and for every cell entered at a parameter t <= tend, in the order of the walk; (kx, ky) is
// the cell's offset from the origin cell and, on return, the cell the ray ends in.  tend is finite and >= 0 and at least one of
// tdx, tdy is finite, so the walk ends after at most 2 * (tend + 2) steps.
template <class Visit>
__device__ __forceinline__ void walk_free(const RayStart& r, const double tend, int& kx, int& ky, Visit&& visit) {
    double nx = 0.0, ny = 0.0;                                            // step counts (exact in float64)
    kx = ky = 0;
    for (;;) {
        visit(kx, ky);
        const double tmx = (nx + r.fx) * r.tdx, tmy = (ny + r.fy) * r.tdy;
        const bool step_x = tmx < tmy;                                    // a tie steps in y
        if (!((step_x ? tmx : tmy) <= tend)) return;                      // (a NaN ends the walk as well)
        nx += step_x ? 1.0 : 0.0; ny += step_x ? 0.0 : 1.0;
        kx += step_x ? r.sx : 0; ky += step_x ? 0 : r.sy;
    }
}

// walk_ray with the limit per ray and what a scan check needs beside the status (kernels_scancheck.hip): on a hit t
// is the parameter at which the hit cell was entered, as there, and E is tracked while walking - the last cell the loop tested
// whose entry parameter is <= tz (the origin cell is entered at 0), as its pool tile (-1: no tile there) and its tile-local cell
// e_i, e_j - so that v(E) is one int8 load afterwards (scan_end_value).  A second copy of the walk and not a parameter of the
// first: cast_scans_kernel is to compile as it did (see ray_start above).  The same bounds hold: the tile table is read at
// positions inside the lattice only, occ only where there is a tile, and the loop ends after at most 2 * L * dim steps.  With
// an origin outside the lattice (status 2) E is not set.
__device__ __forceinline__ int walk_ray_to(const DevView& v, const int32_t* __restrict__ tab, const double4 ps, const double2 bm,
                                           const double inv, const double tlim, const double tz, double& t, int& e_tile, int& e_i,
                                           int& e_j) {
    const int L = v.L, dim = v.dim, ow = v.ow;
    const double ox = ps.x * inv, oy = ps.y * inv;                        // origin in mosaic-cell units
    const double dx = ps.z * bm.x - ps.w * bm.y, dy = ps.w * bm.x + ps.z * bm.y;
    const double fX = __builtin_floor(ox), fY = __builtin_floor(oy);
    const int off = v.R * dim + dim / 2;                                  // mosaic X + off = tile * dim + cell
    const double lo = -(double)off, hi = (double)(L * dim - off);
    t = 0.0;
    e_tile = -1; e_i = e_j = 0;
    if (!(fX >= lo && fX < hi && fY >= lo && fY < hi)) return 2;          // (a NaN as well)
    const int u = (int)fX + off, w = (int)fY + off;
    int ta = u / dim, i = u - ta * dim, tb = w / dim, j = w - tb * dim;
    const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
    const double inf = __builtin_inf();
    const double tdx = dx != 0 ? 1.0 / __builtin_fabs(dx) : inf, tdy = dy != 0 ? 1.0 / __builtin_fabs(dy) : inf;
    const double fx = dx != 0 ? (dx > 0 ? (fX + 1.0) - ox : ox - fX) : 1.0;
    const double fy = dy != 0 ? (dy > 0 ? (fY + 1.0) - oy : oy - fY) : 1.0;
    double nx = 0.0, ny = 0.0;                                            // step counts (exact in float64)
    int cur_pos = -1, cur_w = -1, tile = -1;
    uint32_t word = 0u;
    for (;;) {
        if ((unsigned)ta >= (unsigned)L || (unsigned)tb >= (unsigned)L) return 2;           // left the lattice
        const int pos = ta * L + tb, wi = i * ow + (j >> 5);
        if (pos != cur_pos) { tile = tab[pos]; cur_pos = pos; cur_w = -1; }
        if (t <= tz) { e_tile = tile; e_i = i; e_j = j; }                 // t never decreases: E is the last cell of a prefix
        if (wi != cur_w) {
            word = tile >= 0 ? v.occ[(size_t)tile * dim * ow + (size_t)wi] : 0u;              // no tile: free
            cur_w = wi;
        }
        if ((word >> (j & 31)) & 1u) return 1;
        const double tmx = (nx + fx) * tdx, tmy = (ny + fy) * tdy;
        const bool step_x = tmx < tmy;                                    // a tie steps in y
        t = step_x ? tmx : tmy;
        nx += step_x ? 1.0 : 0.0; ny += step_x ? 0.0 : 1.0;
        i += step_x ? sx : 0; j += step_x ? 0 : sy;
        if (i == dim) { i = 0; ++ta; } else if (i < 0) { i = dim - 1; --ta; }
        if (j == dim) { j = 0; ++tb; } else if (j < 0) { j = dim - 1; --tb; }
        if (t > tlim) return 0;
    }
}

// v of the cell walk_ray_to left in (e_tile, e_i, e_j): the lattice value rbpf_render_map gives, 0 without a tile and outside
// the tile's written box
__device__ __forceinline__ int scan_end_value(const DevView& v, int e_tile, int e_i, int e_j) {
    if (e_tile < 0) return 0;
    const int* bb = v.tile_bbox + 4 * (size_t)e_tile;
    if (e_i < bb[0] || e_i > bb[1] || e_j < bb[2] || e_j > bb[3]) return 0;
    return (int)v.pool[(size_t)e_tile * v.dim * v.dim + (size_t)e_i * v.dim + e_j];
}

}  // namespace rbpf
