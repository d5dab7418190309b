// kernels_frontier.hip -- frontier regions: the frontier cells of a box of a particle's map, their connected components under
// 8-connectivity, and a table of the largest with a cell of each to send the robot to (include/rbpf_hip.h, rbpf_frontier_regions;
// the specification is DESIGN 3.13).
//
// The box is cut into 64 x 64 blocks (rbpf_blockrelax.h); one 256-lane workgroup works on one (particle, block), and a lane
// owns 16 neighbouring cells of one row.
//   frontier_mask_kernel    the block's occupancy bits with `clear` rows above and below (and 64 columns either side) from the tiles'
//                           occupancy words, its int8 cells with a one-cell halo.  A row's bits are widened by `clear` columns, the
//                           widened rows of the 2 clear + 1 rows round a cell are or-ed: a bit of the result says "an occupied cell
//                           within Chebyshev distance clear".  A frontier cell gets its own L = i ny + j as its label; the others
//                           keep FRONTIER_NONE.  Counts |F| with one atomic per wave, marks the block dirty if it holds a cell of F.
//   frontier_label_kernel   one round of rbpf_blockrelax.h over the labels with the rule of FrontierRule: a frontier cell takes the
//                           least of its own and its 8 neighbours' labels.  A cell outside F holds FRONTIER_NONE for ever, which
//                           no minimum takes, so the window itself says which cells are active.  Labels only fall and are at all
//                           times the L of a member of the cell's own region.
//   frontier_reduce_kernel  the fixed point: label = the smallest L of the region, and the root is the cell with label == L.  Every
//                           frontier cell adds 1 to the size kept at its root's position; the roots are counted.
//   frontier_select_kernel  one workgroup per particle: the max_regions largest roots with size >= min_size by the key (size
//                           descending, label ascending), streamed through a 2048-key LDS buffer that a bitonic sort cuts back to
//                           max_regions whenever it fills.  Writes label and size of the table's rows and, at a kept root's
//                           position, -(row + 1).
//   frontier_moment_kernel  every cell of a kept region adds into its row: sum_dx, sum_dy, the four bounds (box-relative).
//   frontier_rep_kernel     every cell of a kept region offers dist2 2^27 + L to its row's 64-bit minimum.
//   frontier_finish_kernel  bounds to absolute cells, the minimum to rep_X, rep_Y.
// The three passes over the cells use integer atomics only, so their order is free.  Along a frontier line most cells of a wave
// share one label: a wave whose cells all do reduces across its lanes and issues one atomic per quantity; in any other wave a
// lane joins its runs of equal labels before it issues one.
#include "rbpf_device.h"

#include <limits.h>

namespace rbpf {

static const int FVS = 68;            // LDS row stride of the int8 window
static const int FROWS = 96;          // rows of the occupancy window at the largest clearance (64 + 2 * 16)
static const int SEL_N = 2048;        // keys of the selection buffer: 1024 kept at the most, 1024 (four per lane) added between two tests

typedef unsigned long long u64;

// v(X, Y): u, w count from the lattice's first cell.  0 outside the lattice and without a tile; outside its written box a tile holds 0.
__device__ __forceinline__ int frontier_cell(const DevView& v, const int32_t* __restrict__ tab, int u, int w) {
    const int dim = v.dim, edge = v.L * dim;
    if (u < 0 || u >= edge || w < 0 || w >= edge) return 0;
    const int a = u / dim, b = w / dim, tile = tab[a * v.L + b];
    return tile < 0 ? 0 : v.pool[(size_t)tile * dim * dim + (size_t)(u - a * dim) * dim + (w - b * dim)];
}

__global__ __launch_bounds__(BR_LANES) void frontier_mask_kernel(DevView v, FrontierArgs a) {
    __shared__ uint32_t s_occ[FROWS * 6];                 // row r = X0 - clear + r; bit 32 w + k of a row = column Y0 - 64 + 32 w + k
    __shared__ uint64_t s_wide[FROWS];                    // bit j: an occupied cell of the row within `clear` columns of Y0 + j
    __shared__ uint64_t s_near[BR_EDGE];                       // bit j of row i: an occupied cell within Chebyshev distance `clear` of (X0 + i, Y0 + j)
    __shared__ int8_t s_v[BR_WIN * FVS];                      // cell (X0 - 1 + r, Y0 - 1 + q) at [r][q]
    const int tid = threadIdx.x, pi = blockIdx.y, p = a.particle + pi;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int X0 = a.x0 + BR_EDGE * bx, Y0 = a.y0 + BR_EDGE * by, m = a.clear, rows = BR_EDGE + 2 * m;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    const int off = v.R * v.dim + v.dim / 2;
    for (int k = tid; k < rows * 6; k += BR_LANES) {
        const int r = k / 6, w = k - 6 * r;
        s_occ[k] = occ_word32(v, tab, X0 - m + r + off, Y0 - BR_EDGE + 32 * w + off);
    }
    for (int k = tid; k < BR_WIN * BR_WIN; k += BR_LANES) {
        const int r = k / BR_WIN, q = k - BR_WIN * r;
        s_v[r * FVS + q] = (int8_t)frontier_cell(v, tab, X0 - 1 + r + off, Y0 - 1 + q + off);
    }
    __syncthreads();
    if (tid < rows) {
        uint64_t d = 0;
        for (int k = -m; k <= m; ++k) d |= occ_bits64(s_occ + 6 * tid, BR_EDGE + k);
        s_wide[tid] = d;
    }
    __syncthreads();
    if (tid < BR_EDGE) {
        uint64_t d = 0;
        for (int dx = 0; dx <= 2 * m; ++dx) d |= s_wide[tid + dx];
        s_near[tid] = d;
    }
    __syncthreads();
    const int i = tid >> 2, j0 = 16 * (tid & 3), ri = BR_EDGE * bx + i;   // box-relative row
    int n = 0;
    if (ri < a.nx) {
        const uint32_t near = (uint32_t)(s_near[i] >> j0);
        const int8_t* c = s_v + (i + 1) * FVS + j0 + 1;
        int32_t* out = a.ras + (size_t)pi * a.ras_stride + (size_t)(ri + 1) * a.cw + BR_EDGE * by + j0 + 1;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int rj = BR_EDGE * by + j0 + k;
            if (rj >= a.ny) break;
            if (c[k] < 0 && !((near >> k) & 1u) && (c[k - FVS] == 0 || c[k + FVS] == 0 || c[k - 1] == 0 || c[k + 1] == 0)) {
                out[k] = ri * a.ny + rj;
                ++n;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((tid & 63) == 0 && n) atomicAdd(a.counts + 3 * (size_t)pi, n);
    if (__syncthreads_or(n) && tid == 0) a.dirty[(size_t)pi * a.nbx * a.nby + blockIdx.x] = 1;   // parity 0: the first round reads it
}

struct FrontierRule {
    static const bool MASK_FROM_WINDOW = true;
    __device__ __forceinline__ uint32_t mask(const int32_t* sc) const {   // the lane's frontier cells: they alone ever hold a label
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) m |= (uint32_t)(sc[k + 1] != FRONTIER_NONE) << k;
        return m;
    }
    static __device__ __forceinline__ void cell(int k, uint32_t m, const int (&u)[18], int (&c)[18], const int (&d)[18], int& changed) {
        if ((m >> k) & 1u) {
            const int b_ = min(min(min(u[k], u[k + 1]), min(u[k + 2], c[k])), min(min(c[k + 2], d[k]), min(d[k + 1], d[k + 2])));
            if (b_ < c[k + 1]) { c[k + 1] = b_; changed = 1; }
        }
    }
};

__global__ __launch_bounds__(BR_LANES) void frontier_label_kernel(FrontierArgs a, int parity, int32_t* count) {
    block_relax_round(a, FrontierRule{}, parity, count);
}

// position in the label raster of the cell whose L is given
__device__ __forceinline__ size_t frontier_at(const FrontierArgs& a, int L) {
    const int i = L / a.ny;
    return (size_t)(i + 1) * a.cw + (L - i * a.ny) + 1;
}

// The lane's 16 labels of the finished raster (FRONTIER_NONE beyond the box: nothing was ever written there) and the label all
// frontier cells of the wave share: FRONTIER_NONE if the wave has none, -1 if they differ.  Every lane of the wave calls it.
__device__ __forceinline__ int frontier_lane_labels(const FrontierArgs& a, int pi, int bx, int by, int i, int j0, int (&l)[16]) {
    const int32_t* row = a.ras + (size_t)pi * a.ras_stride + (size_t)(BR_EDGE * bx + i + 1) * a.cw + BR_EDGE * by + j0 + 1;
    int first = FRONTIER_NONE;
    bool same = true;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        l[k] = row[k];
        if (l[k] != FRONTIER_NONE) {
            if (first == FRONTIER_NONE) first = l[k];
            else same = same && l[k] == first;
        }
    }
    const u64 has = __ballot(first != FRONTIER_NONE);
    if (!has) return FRONTIER_NONE;
    const int lab = __shfl(first, __builtin_ctzll(has), 64);
    return __ballot(first != FRONTIER_NONE && !(same && first == lab)) ? -1 : lab;
}

__device__ __forceinline__ int wave_add(int x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64); return x; }
__device__ __forceinline__ int wave_min(int x) { for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64)); return x; }
__device__ __forceinline__ int wave_max(int x) { for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64)); return x; }
__device__ __forceinline__ u64 wave_min64(u64 x) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 y = ((u64)(uint32_t)__shfl_xor((int)(x >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)x, o, 64);
        x = min(x, y);
    }
    return x;
}

__global__ __launch_bounds__(BR_LANES) void frontier_reduce_kernel(FrontierArgs a) {
    const int tid = threadIdx.x, pi = blockIdx.y;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int i = tid >> 2, j0 = 16 * (tid & 3);
    int l[16];
    const int wl = frontier_lane_labels(a, pi, bx, by, i, j0, l);
    if (wl == FRONTIER_NONE) return;                       // (uniform over the wave)
    int32_t* aux = a.aux + (size_t)pi * a.ras_stride;
    const int own = (BR_EDGE * bx + i) * a.ny + BR_EDGE * by + j0;   // L of the lane's first cell
    int n = 0, roots = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { n += l[k] != FRONTIER_NONE; roots += l[k] == own + k; }
    if (wl >= 0) {
        n = wave_add(n);
        if ((tid & 63) == 0) atomicAdd(aux + frontier_at(a, wl), n);
    } else {
        int cur = FRONTIER_NONE, cnt = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (l[k] != cur) {
                if (cur != FRONTIER_NONE) atomicAdd(aux + frontier_at(a, cur), cnt);
                cur = l[k]; cnt = 0;
            }
            ++cnt;
        }
        if (cur != FRONTIER_NONE) atomicAdd(aux + frontier_at(a, cur), cnt);
    }
    if (roots) atomicAdd(a.counts + 3 * (size_t)pi + 1, roots);
}

// s[0 .. SEL_N) into descending order; ends with a barrier
__device__ __forceinline__ void frontier_sort(u64* s, int tid) {
    for (int k = 2; k <= SEL_N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < SEL_N; t += BR_LANES) {
                const int x = t ^ j;
                if (x > t) {
                    const u64 p = s[t], q = s[x];
                    if ((t & k) == 0 ? p < q : p > q) { s[t] = q; s[x] = p; }
                }
            }
            __syncthreads();
        }
}

static const u64 ROW_UNSET = ~0ull;   // a minimum nothing was offered to yet

__global__ __launch_bounds__(BR_LANES) void frontier_select_kernel(FrontierArgs a) {
    __shared__ u64 s_key[SEL_N];                           // size << 32 | ~label of a candidate root: larger is better; 0 = free
    __shared__ int s_n;                                    // keys in s_key
    __shared__ u64 s_floor;                                // once max_regions keys are held: the smallest of them
    const int tid = threadIdx.x, pi = blockIdx.x, K = a.max_regions;
    int32_t* aux = a.aux + (size_t)pi * a.ras_stride;
    for (int k = tid; k < SEL_N; k += BR_LANES) s_key[k] = 0;
    if (tid == 0) { s_n = 0; s_floor = 0; }
    __syncthreads();
    const long long ncell = (long long)a.nx * a.ny;
    for (long long base = 0; base < ncell; base += 4 * BR_LANES) {
        const u64 floor_key = s_floor;
        for (int q = 0; q < 4; ++q) {
            const long long t = base + q * BR_LANES + tid;
            if (t >= ncell) break;
            const int sz = aux[frontier_at(a, (int)t)];    // 0 wherever no root is
            if (sz < a.min_size) continue;
            const u64 key = ((u64)sz << 32) | (0xffffffffu - (uint32_t)t);
            if (key > floor_key) s_key[atomicAdd(&s_n, 1)] = key;
        }
        __syncthreads();
        const int held = s_n;                              // read between two barriers: the same in every lane, whatever the waves' pace
        __syncthreads();                                   // nobody appends for the next pass before everybody has read it
        if (held > SEL_N - 4 * BR_LANES) {                       // the next pass could overflow: keep the K best
            frontier_sort(s_key, tid);
            for (int k = K + tid; k < SEL_N; k += BR_LANES) s_key[k] = 0;
            if (tid == 0 && held >= K) { s_n = K; s_floor = s_key[K - 1]; }
            __syncthreads();
        }
    }
    frontier_sort(s_key, tid);
    const int kept = min(s_n, K);
    if (tid == 0) a.counts[3 * (size_t)pi + 2] = kept;
    for (int k = tid; k < K; k += BR_LANES) {
        u64* row = a.table + ((size_t)pi * K + k) * 10;
        if (k < kept) {
            const u64 key = s_key[k];
            const int label = (int)(0xffffffffu - (uint32_t)key);
            row[0] = (u64)label; row[1] = key >> 32; row[2] = 0; row[3] = 0;
            row[4] = ROW_UNSET; row[5] = 0; row[6] = ROW_UNSET; row[7] = 0; row[8] = ROW_UNSET; row[9] = 0;
            aux[frontier_at(a, label)] = -(k + 1);
        } else {
#pragma unroll
            for (int c = 0; c < 10; ++c) row[c] = ~0ull;   // -1
        }
    }
}

// the table row of the region with this label, or null if the table does not keep it
__device__ __forceinline__ u64* frontier_row(const FrontierArgs& a, int pi, int label) {
    const int r = a.aux[(size_t)pi * a.ras_stride + frontier_at(a, label)];
    return r < 0 ? a.table + ((size_t)pi * a.max_regions + (-r - 1)) * 10 : nullptr;
}

__device__ __forceinline__ void frontier_add_moments(u64* row, int sdx, int sdy, int x_lo, int x_hi, int y_lo, int y_hi) {
    atomicAdd(row + 2, (u64)sdx); atomicAdd(row + 3, (u64)sdy);
    atomicMin(row + 4, (u64)x_lo); atomicMax(row + 5, (u64)x_hi); atomicMin(row + 6, (u64)y_lo); atomicMax(row + 7, (u64)y_hi);
}

__global__ __launch_bounds__(BR_LANES) void frontier_moment_kernel(FrontierArgs a) {
    const int tid = threadIdx.x, pi = blockIdx.y;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int i = tid >> 2, j0 = 16 * (tid & 3), ri = BR_EDGE * bx + i, rj0 = BR_EDGE * by + j0;
    int l[16];
    const int wl = frontier_lane_labels(a, pi, bx, by, i, j0, l);
    if (wl == FRONTIER_NONE) return;                       // (uniform over the wave)
    if (wl >= 0) {
        u64* row = frontier_row(a, pi, wl);
        if (!row) return;                                  // (uniform over the wave)
        int n = 0, sdy = 0, y_lo = INT_MAX, y_hi = -1;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (l[k] != FRONTIER_NONE) { ++n; sdy += rj0 + k; y_lo = min(y_lo, rj0 + k); y_hi = rj0 + k; }
        const int sdx = wave_add(n * ri), x_lo = wave_min(n ? ri : INT_MAX), x_hi = wave_max(n ? ri : -1);
        sdy = wave_add(sdy); y_lo = wave_min(y_lo); y_hi = wave_max(y_hi);
        if ((tid & 63) == 0) frontier_add_moments(row, sdx, sdy, x_lo, x_hi, y_lo, y_hi);
        return;
    }
    int cur = FRONTIER_NONE, n = 0, sdy = 0, y_lo = 0;
#pragma unroll
    for (int k = 0; k <= 16; ++k) {                        // k == 16 closes the last run
        const int lk = k < 16 ? l[k] : FRONTIER_NONE;
        if (lk != cur) {
            if (cur != FRONTIER_NONE)
                if (u64* row = frontier_row(a, pi, cur)) frontier_add_moments(row, n * ri, sdy, ri, ri, y_lo, rj0 + k - 1);
            cur = lk; n = 0; sdy = 0; y_lo = rj0 + k;
        }
        ++n; sdy += rj0 + k;
    }
}

// the centroid of a row's region, rounded half up, packed as cx << 32 | cy; the key a cell offers to its region: squared
// distance to the centroid, then L
__device__ __forceinline__ u64 frontier_centroid(const u64* row) {
    const u64 size = row[1];
    return (((2 * row[2] + size) / (2 * size)) << 32) | ((2 * row[3] + size) / (2 * size));
}
__device__ __forceinline__ u64 frontier_rep_key(u64 centroid, int ri, int rj, int L) {
    const long long ex = ri - (long long)(centroid >> 32), ey = rj - (long long)(uint32_t)centroid;
    return ((u64)(ex * ex + ey * ey) << 27) | (u64)L;
}

__global__ __launch_bounds__(BR_LANES) void frontier_rep_kernel(FrontierArgs a) {
    const int tid = threadIdx.x, pi = blockIdx.y;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int i = tid >> 2, j0 = 16 * (tid & 3), ri = BR_EDGE * bx + i, rj0 = BR_EDGE * by + j0;
    int l[16];
    const int wl = frontier_lane_labels(a, pi, bx, by, i, j0, l);
    if (wl == FRONTIER_NONE) return;                       // (uniform over the wave)
    if (wl >= 0) {
        u64* row = frontier_row(a, pi, wl);
        if (!row) return;                                  // (uniform over the wave)
        const u64 centre = frontier_centroid(row);
        u64 best = ROW_UNSET;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (l[k] != FRONTIER_NONE) best = min(best, frontier_rep_key(centre, ri, rj0 + k, ri * a.ny + rj0 + k));
        best = wave_min64(best);
        if ((tid & 63) == 0) atomicMin(row + 8, best);
        return;
    }
    int cur = FRONTIER_NONE;
    u64* row = nullptr;
    u64 best = ROW_UNSET, centre = 0;
#pragma unroll
    for (int k = 0; k <= 16; ++k) {                        // k == 16 closes the last run
        const int lk = k < 16 ? l[k] : FRONTIER_NONE;
        if (lk != cur) {
            if (row) atomicMin(row + 8, best);
            cur = lk; best = ROW_UNSET;
            row = cur != FRONTIER_NONE ? frontier_row(a, pi, cur) : nullptr;
            if (row) centre = frontier_centroid(row);
        }
        if (row) best = min(best, frontier_rep_key(centre, ri, rj0 + k, ri * a.ny + rj0 + k));
    }
}

__global__ __launch_bounds__(BR_LANES) void frontier_finish_kernel(FrontierArgs a) {
    const long long t = (long long)blockIdx.x * BR_LANES + threadIdx.x;
    if (t >= (long long)a.n_part * a.max_regions) return;
    const int pi = (int)(t / a.max_regions), k = (int)(t - (long long)pi * a.max_regions);
    if (k >= a.counts[3 * (size_t)pi + 2]) return;
    u64* row = a.table + (size_t)t * 10;
    const int L = (int)(row[8] & ((1u << 27) - 1)), ri = L / a.ny;
    const u64 x0 = (u64)(long long)a.x0, y0 = (u64)(long long)a.y0;   // two's complement: the rows are read as int64
    row[4] += x0; row[5] += x0; row[6] += y0; row[7] += y0;
    row[8] = x0 + (u64)ri; row[9] = y0 + (u64)(L - ri * a.ny);
}

__global__ __launch_bounds__(BR_LANES) void frontier_label_out_kernel(FrontierArgs a) {
    const long long t = (long long)blockIdx.x * BR_LANES + threadIdx.x;
    if (t >= (long long)a.nx * a.ny) return;
    const int32_t lv = a.ras[frontier_at(a, (int)t)];
    a.label_out[t] = lv == FRONTIER_NONE ? -1 : lv;
}

void launch_frontier_mask(const DevView& v, const FrontierArgs& a, hipStream_t s) {
    frontier_mask_kernel<<<block_relax_grid(a), BR_LANES, 0, s>>>(v, a);
}

void launch_frontier_round(const FrontierArgs& a, int parity, int32_t* d_count, hipStream_t s) {
    frontier_label_kernel<<<block_relax_grid(a), BR_LANES, 0, s>>>(a, parity, d_count);
}

void launch_frontier_output(const FrontierArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(a.nbx * a.nby), (unsigned)a.n_part);
    if (a.table) {
        frontier_reduce_kernel<<<grid, BR_LANES, 0, s>>>(a);
        frontier_select_kernel<<<(unsigned)a.n_part, BR_LANES, 0, s>>>(a);
        frontier_moment_kernel<<<grid, BR_LANES, 0, s>>>(a);
        frontier_rep_kernel<<<grid, BR_LANES, 0, s>>>(a);
        frontier_finish_kernel<<<br_blocks((long long)a.n_part * a.max_regions), BR_LANES, 0, s>>>(a);
    }
    if (a.label_out) frontier_label_out_kernel<<<br_blocks((long long)a.nx * a.ny), BR_LANES, 0, s>>>(a);
}

}  // namespace rbpf
