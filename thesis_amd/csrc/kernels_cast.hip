// kernels_cast.hip -- lidar scans cast from the particles' occupancy maps (include/rbpf_hip.h, rbpf_cast_scans).
//
// One lane per ray; ray r = pose * B + beam, so the beams of a pose lie in consecutive lanes: neighbouring beams walk
// neighbouring cells and share the occupancy words they load.  The walk is the supercover (4-connected) grid traversal of
// DESIGN 3.7 in float64: the crossing parameters are (n + f) * td, functions of the step counts alone, so every lane
// reproduces the specification's values whatever its neighbours do.
//
// A ray tests the occupancy bit planes (occ[tile][row][col >> 5], bit col & 31: cell > threshold, zero outside a tile's
// written box like the cells themselves), 32 cells per 4-byte load.  The current word stays in a register and is loaded
// again only when (tile, row, col >> 5) changes.  The position is kept as (lattice tile, tile-local cell) per axis and
// stepped by +-1 with a wrap at the seam, so the loop has no division and the tile table is read only at a seam (and
// once at the start): it is not staged in LDS.  Every step moves one cell away from the origin along one axis, so a ray
// ends after at most 2 * L * dim steps (it has left the lattice by then).
#include "rbpf_internal.h"

namespace rbpf {

static const int CB = 256;

__global__ __launch_bounds__(CB) void cast_scans_kernel(DevView v, CastArgs a) {
    const long long r = (long long)blockIdx.x * CB + threadIdx.x;
    if (r >= (long long)a.n_poses * a.B) return;
    const int n = (int)(r / a.B), b = (int)(r - (long long)n * a.B);
    const int p = a.particle >= 0 ? a.particle : n;
    const int L = v.L, dim = v.dim, ow = v.ow;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * L * L;
    const double4 ps = reinterpret_cast<const double4*>(a.pose4)[n];     // x, y, cos(theta), sin(theta)
    const double2 bm = reinterpret_cast<const double2*>(a.beam2)[b];     // cos(angle), sin(angle)
    const double ox = ps.x * a.inv, oy = ps.y * a.inv;                    // origin in mosaic-cell units
    const double dx = ps.z * bm.x - ps.w * bm.y, dy = ps.w * bm.x + ps.z * bm.y;
    const double fX = __builtin_floor(ox), fY = __builtin_floor(oy);
    const int off = v.R * dim + dim / 2;                                  // mosaic X + off = tile * dim + cell
    const double lo = -(double)off, hi = (double)(L * dim - off);
    double range = a.max_range;
    int st = 2;
    if (fX >= lo && fX < hi && fY >= lo && fY < hi) {                     // (false for a NaN as well)
        const int u = (int)fX + off, w = (int)fY + off;
        int ta = u / dim, i = u - ta * dim, tb = w / dim, j = w - tb * dim;
        const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
        const double inf = __builtin_inf();
        // a ray along an axis never crosses the other one: (n + 1) * inf = inf stands for the specification's "inf"
        const double tdx = dx != 0 ? 1.0 / __builtin_fabs(dx) : inf, tdy = dy != 0 ? 1.0 / __builtin_fabs(dy) : inf;
        const double fx = dx != 0 ? (dx > 0 ? (fX + 1.0) - ox : ox - fX) : 1.0;
        const double fy = dy != 0 ? (dy > 0 ? (fY + 1.0) - oy : oy - fY) : 1.0;
        double nx = 0.0, ny = 0.0, t = 0.0;                               // step counts (exact in float64)
        int cur_pos = -1, cur_w = -1, tile = -1;
        uint32_t word = 0u;
        for (;;) {
            if ((unsigned)ta >= (unsigned)L || (unsigned)tb >= (unsigned)L) break;          // left the lattice: status 2
            const int pos = ta * L + tb, wi = i * ow + (j >> 5);
            if (pos != cur_pos) { tile = tab[pos]; cur_pos = pos; cur_w = -1; }
            if (wi != cur_w) {
                word = tile >= 0 ? v.occ[(size_t)tile * dim * ow + (size_t)wi] : 0u;          // no tile: free
                cur_w = wi;
            }
            if ((word >> (j & 31)) & 1u) { st = 1; range = t / a.inv; break; }
            const double tmx = (nx + fx) * tdx, tmy = (ny + fy) * tdy;
            const bool step_x = tmx < tmy;                                // a tie steps in y
            t = step_x ? tmx : tmy;
            nx += step_x ? 1.0 : 0.0; ny += step_x ? 0.0 : 1.0;
            i += step_x ? sx : 0; j += step_x ? 0 : sy;
            if (i == dim) { i = 0; ++ta; } else if (i < 0) { i = dim - 1; --ta; }
            if (j == dim) { j = 0; ++tb; } else if (j < 0) { j = dim - 1; --tb; }
            if (t > a.tlim) { st = 0; break; }
        }
    }
    a.ranges[r] = range;
    if (a.status) a.status[r] = (uint8_t)st;
}

void launch_cast_scans(const DevView& v, const CastArgs& a, hipStream_t s) {
    const long long rays = (long long)a.n_poses * a.B;
    cast_scans_kernel<<<(unsigned)((rays + CB - 1) / CB), CB, 0, s>>>(v, a);
}

}  // namespace rbpf
