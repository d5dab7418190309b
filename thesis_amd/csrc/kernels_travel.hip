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
//   travel_relax_kernel   one round.  A block runs if it or one of its 8 neighbours changed in the previous round: it loads its
//                         costs with a one-cell halo (66 x 66) into LDS and sweeps to its local fixed point.  In a sweep a lane
//                         relaxes its 16 cells of one row from the three rows round them, left to right and back (so a value
//                         crosses the lane's cells in one sweep), and the workgroup votes on "anything changed" with
//                         __syncthreads_or.  A cell outside T holds TRAVEL_INF for ever, so "finite" stands for "in T" where a
//                         diagonal step asks for its two side cells: a side cell in T next to a reached cell is reached at the
//                         fixed point, and before that the test only withholds a step, it never admits a wrong one.  Values only
//                         fall and never pass below the true cost; a block that reads a neighbour's edge while that neighbour
//                         writes it gets the old or the new value, both are upper bounds, and the neighbour is dirty, so the
//                         block runs again.  There is no wait on another workgroup anywhere: a round is a kernel.
//   travel_cost_kernel, travel_goal_kernel   TRAVEL_INF -> -1 into the cost raster; the cost at every goal's cell.
#include "rbpf_device.h"

namespace rbpf {

static const int TB = 256;
static const int TS = 64;             // block edge
static const int TW = 66;             // block with its halo
static const int TSTRIDE = 67;        // LDS row stride of the cost window: odd, so the rows of a wave's lanes fall into different banks
static const int TROWS = 192;         // rows of the mask window at the largest margin (64 + 2 * 64)
static const int SWEEP_CAP = 4096;    // sweeps of one block run; a block that hits it is dirty and goes on in the next round

__global__ __launch_bounds__(TB) void travel_mask_kernel(DevView v, TravelArgs a) {
    __shared__ uint32_t s_occ[TROWS * 6];                 // row r = X0 - m + r; bit 32 w + k of a row = column Y0 - 64 + 32 w + k
    __shared__ __attribute__((aligned(16))) uint8_t s_g[TROWS * TS];   // |dy| to the nearest occupied cell of the row, 64 = none within 63
    const int tid = threadIdx.x, pi = blockIdx.y, p = a.particle + pi;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int X0 = a.x0 + TS * bx, Y0 = a.y0 + TS * by, m = a.m, rows = TS + 2 * m;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    const int dim = v.dim, off = v.R * dim + dim / 2;
    for (int k = tid; k < rows * 6; k += TB) {
        const int r = k / 6, w = k - 6 * r;
        s_occ[k] = occ_word32(v, tab, X0 - m + r + off, Y0 - TS + 32 * w + off);
    }
    __syncthreads();
    for (int k = tid; k < rows * TS; k += TB) {
        const int r = k >> 6, pos = TS + (k & 63);        // the cell's bit in its row
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
        q.u = *reinterpret_cast<const uint4*>(s_g + (i + m + dx) * TS + j0);
        const int ax = dx < 0 ? -dx : dx;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int g = q.c[k];
            best[k] = min(best[k], 5 * max(ax, g) + 2 * min(ax, g));
        }
    }
    const int ri = TS * bx + i;                            // box-relative row
    uint32_t bits = 0u;
    if (ri < a.nx) {
        const int u = X0 + i + off, ta = u / dim, ti = u - ta * dim;   // inside the lattice: the host checked the box
        int cur_b = -1, tile = -1;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int rj = TS * by + j0 + k;
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
    a.tbits[(size_t)pi * a.t_stride + (size_t)(TS * bx + i) * (4 * a.nby) + 4 * by + seg] = (uint16_t)bits;
}

__global__ __launch_bounds__(TB) void travel_start_kernel(TravelArgs a) {
    const int each = a.start_each ? 1 : a.n_start;
    const long long t = (long long)blockIdx.x * TB + threadIdx.x;
    if (t >= (long long)a.n_part * each) return;
    const int pi = (int)(t / each), s = a.start_each ? a.particle + pi : (int)(t - (long long)pi * each);
    const int i = a.starts[2 * s], j = a.starts[2 * s + 1];
    if (i < 0) return;                                    // outside the box
    const size_t h = (size_t)pi * a.t_stride + (size_t)i * (4 * a.nby) + (j >> 4);   // halfword of tbits; t_stride and the row length are even
    atomicOr(reinterpret_cast<uint32_t*>(a.tbits) + (h >> 1), 1u << (16 * (int)(h & 1) + (j & 15)));
    a.cost[(size_t)pi * a.cost_stride + (size_t)(i + 1) * a.cw + (j + 1)] = 0;
    a.dirty[(size_t)pi * a.nbx * a.nby + (size_t)(i >> 6) * a.nby + (j >> 6)] = 1;
}

// cell k of the lane's row from the rows above (u), of (c) and below (d) it; index k + 1 is the cell, k and k + 2 its row neighbours
#define TRAVEL_RELAX(k)                                                                                   \
    if ((tb >> (k)) & 1u) {                                                                               \
        const int l_ = c[k], r_ = c[(k) + 2], up_ = u[(k) + 1], dn_ = d[(k) + 1];                         \
        int b_ = min(min(l_, r_), min(up_, dn_)) + 5;                                                     \
        if (l_ < TRAVEL_INF && up_ < TRAVEL_INF) b_ = min(b_, u[k] + 7);                                   \
        if (r_ < TRAVEL_INF && up_ < TRAVEL_INF) b_ = min(b_, u[(k) + 2] + 7);                             \
        if (l_ < TRAVEL_INF && dn_ < TRAVEL_INF) b_ = min(b_, d[k] + 7);                                   \
        if (r_ < TRAVEL_INF && dn_ < TRAVEL_INF) b_ = min(b_, d[(k) + 2] + 7);                             \
        if (b_ < c[(k) + 1]) { c[(k) + 1] = b_; changed = 1; }                                            \
    }

__global__ __launch_bounds__(TB) void travel_relax_kernel(TravelArgs a, int parity, int32_t* count) {
    __shared__ int32_t s_c[TW * TSTRIDE];
    const int tid = threadIdx.x, pi = blockIdx.y, nblk = a.nbx * a.nby;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const uint8_t* __restrict__ din = a.dirty + ((size_t)parity * a.n_part + pi) * nblk;
    uint8_t* __restrict__ dout = a.dirty + ((size_t)(parity ^ 1) * a.n_part + pi) * nblk;
    int run = 0;
    for (int ex = max(bx - 1, 0); ex <= min(bx + 1, a.nbx - 1); ++ex)
        for (int ey = max(by - 1, 0); ey <= min(by + 1, a.nby - 1); ++ey) run |= din[ex * a.nby + ey];
    if (!run) {                                            // (uniform over the workgroup)
        if (tid == 0) dout[blockIdx.x] = 0;
        return;
    }
    int32_t* __restrict__ base = a.cost + (size_t)pi * a.cost_stride + (size_t)(TS * bx) * a.cw + TS * by;   // window cell [0][0]: the halo's corner
    for (int k = tid; k < TW * TW; k += TB) {
        const int r = k / TW, q = k - TW * r;
        s_c[r * TSTRIDE + q] = base[(size_t)r * a.cw + q];
    }
    const int i = tid >> 2, seg = tid & 3;
    const uint32_t tb = a.tbits[(size_t)pi * a.t_stride + (size_t)(TS * bx + i) * (4 * a.nby) + 4 * by + seg];
    const int32_t* su = s_c + i * TSTRIDE + 16 * seg;      // the row above the lane's, from the column left of its first cell
    int32_t* sc = s_c + (i + 1) * TSTRIDE + 16 * seg;
    const int32_t* sd = s_c + (i + 2) * TSTRIDE + 16 * seg;
    __syncthreads();
    int c[18], any = 0;
    for (int sweep = 0; sweep < SWEEP_CAP; ++sweep) {
        int changed = 0;
        if (tb) {
            int u[18], d[18];
#pragma unroll
            for (int k = 0; k < 18; ++k) { u[k] = su[k]; c[k] = sc[k]; d[k] = sd[k]; }
#pragma unroll
            for (int k = 0; k < 16; ++k) TRAVEL_RELAX(k)
#pragma unroll
            for (int k = 14; k >= 0; --k) TRAVEL_RELAX(k)
            if (changed) {
#pragma unroll
                for (int k = 0; k < 16; ++k) sc[k + 1] = c[k + 1];   // the lane's own cells: nobody else writes them
            }
        }
        if (!__syncthreads_or(changed)) break;
        any = 1;
    }
    if (any && tb) {                                       // c holds the last state of the lane's cells
        int32_t* out = base + (size_t)(i + 1) * a.cw + 16 * seg + 1;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((tb >> k) & 1u) out[k] = c[k + 1];
    }
    if (tid == 0) {
        dout[blockIdx.x] = (uint8_t)any;
        atomicAdd(count + 32, 1);                          // block runs of this round (rbpf_travel_stats)
        if (any) atomicAdd(count, 1);
    }
}
#undef TRAVEL_RELAX

__global__ __launch_bounds__(TB) void travel_cost_kernel(TravelArgs a) {
    const long long t = (long long)blockIdx.x * TB + threadIdx.x;
    if (t >= (long long)a.nx * a.ny) return;
    const int i = (int)(t / a.ny), j = (int)(t - (long long)i * a.ny);
    const int32_t cv = a.cost[(size_t)(i + 1) * a.cw + (j + 1)];
    a.cost_out[t] = cv >= TRAVEL_INF ? -1 : cv;
}

__global__ __launch_bounds__(TB) void travel_goal_kernel(TravelArgs a) {
    const long long t = (long long)blockIdx.x * TB + threadIdx.x;
    if (t >= (long long)a.n_part * a.n_goals) return;
    const int pi = (int)(t / a.n_goals), g = (int)(t - (long long)pi * a.n_goals);
    const int i = a.goals[2 * g], j = a.goals[2 * g + 1];
    int32_t cv = TRAVEL_INF;
    if (i >= 0) cv = a.cost[(size_t)pi * a.cost_stride + (size_t)(i + 1) * a.cw + (j + 1)];
    a.goal_out[t] = cv >= TRAVEL_INF ? -1 : cv;
}

static unsigned blocks_for(long long n) { return (unsigned)((n + TB - 1) / TB); }

void launch_travel_mask(const DevView& v, const TravelArgs& a, hipStream_t s) {
    travel_mask_kernel<<<dim3((unsigned)(a.nbx * a.nby), (unsigned)a.n_part), TB, 0, s>>>(v, a);
    travel_start_kernel<<<blocks_for((long long)a.n_part * (a.start_each ? 1 : a.n_start)), TB, 0, s>>>(a);
}

void launch_travel_round(const TravelArgs& a, int parity, int32_t* d_count, hipStream_t s) {
    travel_relax_kernel<<<dim3((unsigned)(a.nbx * a.nby), (unsigned)a.n_part), TB, 0, s>>>(a, parity, d_count);
}

void launch_travel_output(const TravelArgs& a, hipStream_t s) {
    if (a.cost_out) travel_cost_kernel<<<blocks_for((long long)a.nx * a.ny), TB, 0, s>>>(a);
    if (a.goal_out) travel_goal_kernel<<<blocks_for((long long)a.n_part * a.n_goals), TB, 0, s>>>(a);
}

}  // namespace rbpf
