// kernels_travel.hip -- travel cost: clearance, traversable set and shortest-path cost from a set of start cells to every cell
// of a box of a particle's map (include/rbpf_hip.h, rbpf_travel_cost; the specification is DESIGN 3.12).
//
// The box is cut into 64 x 64 blocks; one 256-lane workgroup works on one (particle, block).
//   travel_mask_kernel    the block's occupancy bits with a margin of m = ceil(clear_max / 5) rows above and below (and 64
//                         columns either side) from the tiles' occupancy words into LDS.  The chamfer distance to the nearest
//                         occupied cell, d = min 5 max(|dx|, |dy|) + 2 min(|dx|, |dy|), grows with |dx| and with |dy|, so in
//                         the row at offset dx only the occupied cell nearest in y counts: g(row, y) = that |dy|, found with
//                         count-leading / trailing-zeros on the row's bits, and d = min over dx of 5 max(|dx|, g) + 2 min(|dx|, g).
//                         A lane owns 16 neighbouring cells of one row and reads 16 g bytes per dx with one LDS load.  Writes
//                         min(d, clear_max) if asked for and the block's traversable bits; the int8 cells are read only when
//                         "known free" (v < 0) has to be known.
//   travel_start_kernel   start cells: into T, cost 0, their block dirty.
//   travel_relax_kernel   one round of rbpf_blockrelax.h over the cost field with the rule of TravelRule: a cell of T takes the
//                         least of its 4 neighbours + 5 and its diagonal neighbours + 7.  A cell outside T holds TRAVEL_INF for
//                         ever, so "finite" stands for "in T" where a diagonal step asks for its two side cells: a side cell in
//                         T next to a reached cell is reached at the fixed point, and before that the test only withholds a step,
//                         it never admits a wrong one.  Every value is at all times the length of a real path.
//   travel_cost_kernel, travel_goal_kernel   TRAVEL_INF -> -1 into the cost raster; the cost at every goal's cell.
#include "rbpf_device.h"

namespace rbpf {

static const int TROWS = 192;         // rows of the mask window at the largest margin (64 + 2 * 64)

__global__ __launch_bounds__(BR_LANES) void travel_mask_kernel(DevView v, TravelArgs a) {
    __shared__ uint32_t s_occ[TROWS * 6];                 // row r = X0 - m + r; bit 32 w + k of a row = column Y0 - 64 + 32 w + k
    __shared__ __attribute__((aligned(16))) uint8_t s_g[TROWS * BR_EDGE];   // |dy| to the nearest occupied cell of the row, 64 = none within 63
    const int tid = threadIdx.x, pi = blockIdx.y, p = a.particle + pi;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int X0 = a.x0 + BR_EDGE * bx, Y0 = a.y0 + BR_EDGE * by, m = a.m, rows = BR_EDGE + 2 * m;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    const int dim = v.dim, off = v.R * dim + dim / 2;
    for (int k = tid; k < rows * 6; k += BR_LANES) {
        const int r = k / 6, w = k - 6 * r;
        s_occ[k] = occ_word32(v, tab, X0 - m + r + off, Y0 - BR_EDGE + 32 * w + off);
    }
    __syncthreads();
    for (int k = tid; k < rows * BR_EDGE; k += BR_LANES) {
        const int r = k >> 6, pos = BR_EDGE + (k & 63);        // the cell's bit in its row
        const uint64_t right = occ_bits64(s_occ + 6 * r, pos), left = occ_bits64(s_occ + 6 * r, pos - 63);
        const int dr = right ? __builtin_ctzll(right) : 64, dl = left ? __builtin_clzll(left) : 64;
        s_g[k] = (uint8_t)min(dr, dl);
    }
    __syncthreads();
    const int i = tid >> 2, seg = tid & 3, j0 = 16 * seg;
    int best[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) best[k] = a.clear_max;
    for (int dx = -(m - 1); dx <= m - 1; ++dx) {          // |dx| >= m is 5 m >= clear_max at the least
        union { uint4 u; uint8_t c[16]; } q;
        q.u = *reinterpret_cast<const uint4*>(s_g + (i + m + dx) * BR_EDGE + j0);
        const int ax = dx < 0 ? -dx : dx;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int g = q.c[k];
            best[k] = min(best[k], 5 * max(ax, g) + 2 * min(ax, g));
        }
    }
    const int ri = BR_EDGE * bx + i;                            // box-relative row
    uint32_t bits = 0u;
    if (ri < a.nx) {
        const int u = X0 + i + off, ta = u / dim, ti = u - ta * dim;   // inside the lattice: the host checked the box
        int cur_b = -1, tile = -1;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int rj = BR_EDGE * by + j0 + k;
            if (rj >= a.ny) break;
            bool ok = best[k] > a.inflate;
            if (ok && !a.through_unknown) {
                const int w = Y0 + j0 + k + off, b = w / dim, tj = w - b * dim;
                if (b != cur_b) { tile = tab[ta * v.L + b]; cur_b = b; }
                ok = tile >= 0 && v.pool[(size_t)tile * dim * dim + (size_t)ti * dim + tj] < 0;
            }
            if (ok) bits |= 1u << k;
            if (a.clearance) a.clearance[(size_t)ri * a.ny + rj] = (uint16_t)best[k];
        }
    }
    a.tbits[(size_t)pi * a.t_stride + (size_t)(BR_EDGE * bx + i) * (4 * a.nby) + 4 * by + seg] = (uint16_t)bits;
}

__global__ __launch_bounds__(BR_LANES) void travel_start_kernel(TravelArgs a) {
    const int each = a.start_each ? 1 : a.n_start;
    const long long t = (long long)blockIdx.x * BR_LANES + threadIdx.x;
    if (t >= (long long)a.n_part * each) return;
    const int pi = (int)(t / each), s = a.start_each ? a.particle + pi : (int)(t - (long long)pi * each);
    const int i = a.starts[2 * s], j = a.starts[2 * s + 1];
    if (i < 0) return;                                    // outside the box
    const size_t h = (size_t)pi * a.t_stride + (size_t)i * (4 * a.nby) + (j >> 4);   // halfword of tbits; t_stride and the row length are even
    atomicOr(reinterpret_cast<uint32_t*>(a.tbits) + (h >> 1), 1u << (16 * (int)(h & 1) + (j & 15)));
    a.ras[(size_t)pi * a.ras_stride + (size_t)(i + 1) * a.cw + (j + 1)] = 0;
    a.dirty[(size_t)pi * a.nbx * a.nby + (size_t)(i >> 6) * a.nby + (j >> 6)] = 1;
}

struct TravelRule {
    const uint16_t* tbits; long long t_stride;
    static const bool MASK_FROM_WINDOW = false;
    __device__ __forceinline__ uint32_t mask(int pi, int bx, int by, int i, int seg, const BlockRelaxArgs& g) const {
        return tbits[(size_t)pi * t_stride + (size_t)(BR_EDGE * bx + i) * (4 * g.nby) + 4 * by + seg];
    }
    static __device__ __forceinline__ void cell(int k, uint32_t m, const int (&u)[18], int (&c)[18], const int (&d)[18], int& changed) {
        if ((m >> k) & 1u) {
            const int l_ = c[k], r_ = c[k + 2], up_ = u[k + 1], dn_ = d[k + 1];
            int b_ = min(min(l_, r_), min(up_, dn_)) + 5;
            if (l_ < TRAVEL_INF && up_ < TRAVEL_INF) b_ = min(b_, u[k] + 7);
            if (r_ < TRAVEL_INF && up_ < TRAVEL_INF) b_ = min(b_, u[k + 2] + 7);
            if (l_ < TRAVEL_INF && dn_ < TRAVEL_INF) b_ = min(b_, d[k] + 7);
            if (r_ < TRAVEL_INF && dn_ < TRAVEL_INF) b_ = min(b_, d[k + 2] + 7);
            if (b_ < c[k + 1]) { c[k + 1] = b_; changed = 1; }
        }
    }
};

__global__ __launch_bounds__(BR_LANES) void travel_relax_kernel(TravelArgs a, int parity, int32_t* count) {
    block_relax_round(a, TravelRule{a.tbits, a.t_stride}, parity, count);
}

__global__ __launch_bounds__(BR_LANES) void travel_cost_kernel(TravelArgs a) {
    const long long t = (long long)blockIdx.x * BR_LANES + threadIdx.x;
    if (t >= (long long)a.nx * a.ny) return;
    const int i = (int)(t / a.ny), j = (int)(t - (long long)i * a.ny);
    const int32_t cv = a.ras[(size_t)(i + 1) * a.cw + (j + 1)];
    a.cost_out[t] = cv >= TRAVEL_INF ? -1 : cv;
}

__global__ __launch_bounds__(BR_LANES) void travel_goal_kernel(TravelArgs a) {
    const long long t = (long long)blockIdx.x * BR_LANES + threadIdx.x;
    if (t >= (long long)a.n_part * a.n_goals) return;
    const int pi = (int)(t / a.n_goals), g = (int)(t - (long long)pi * a.n_goals);
    const int i = a.goals[2 * g], j = a.goals[2 * g + 1];
    int32_t cv = TRAVEL_INF;
    if (i >= 0) cv = a.ras[(size_t)pi * a.ras_stride + (size_t)(i + 1) * a.cw + (j + 1)];
    a.goal_out[t] = cv >= TRAVEL_INF ? -1 : cv;
}

void launch_travel_mask(const DevView& v, const TravelArgs& a, hipStream_t s) {
    travel_mask_kernel<<<block_relax_grid(a), BR_LANES, 0, s>>>(v, a);
    travel_start_kernel<<<br_blocks((long long)a.n_part * (a.start_each ? 1 : a.n_start)), BR_LANES, 0, s>>>(a);
}

void launch_travel_round(const TravelArgs& a, int parity, int32_t* d_count, hipStream_t s) {
    travel_relax_kernel<<<block_relax_grid(a), BR_LANES, 0, s>>>(a, parity, d_count);
}

void launch_travel_output(const TravelArgs& a, hipStream_t s) {
    if (a.cost_out) travel_cost_kernel<<<br_blocks((long long)a.nx * a.ny), BR_LANES, 0, s>>>(a);
    if (a.goal_out) travel_goal_kernel<<<br_blocks((long long)a.n_part * a.n_goals), BR_LANES, 0, s>>>(a);
}

}  // namespace rbpf
