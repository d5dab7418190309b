// kernels_score.hip -- map scores: a box of a particle's map compared cell by cell with a reference raster (include/rbpf_hip.h,
// rbpf_score_maps; the specification is DESIGN 3.14).
//
// The box is cut into 64 x 64 blocks; a 256-lane workgroup works on one block, and a lane owns 16 neighbouring cells of one row.
//   score_ref_kernel    once per call, one workgroup per block: the reference's occupied cells of the block with `tol` rows and
//                       columns round it (cells outside the box are not occupied: there is no reference there) as bits in LDS,
//                       widened by tol columns and or-ed over 2 tol + 1 rows: bit j of row i of the result says "a reference-occupied
//                       cell of the box within Chebyshev distance tol".  Writes those 64 words, and the sums of the block that need
//                       no map: reference cells of class F, U and O and the sum of |r|.  Checks the range of a device reference.
//   score_maps_kernel   one workgroup per (particle, block); blockIdx.y is the particle.  The window is the block grown by tol
//                       cells.  If no tile of the particle has a written cell in the window, v is 0 on all of it: every cell is of
//                       class U, nothing of the map is occupied, and the workgroup adds the reference's sums and leaves.  Otherwise
//                       it stages the tiles' occupancy words of the window (two words shifted together per 32 cells; bit by bit
//                       only at a tile seam), dilates them as above (near_m), and every lane reads its
//                       16 int8 cells through the tile table (one 16-byte load where the strip lies in one tile, aligned) and its 16
//                       reference cells, classifies, compares and counts: the nine class pairs in 5-bit fields of one 64-bit
//                       register (a lane sees 16 cells at the most).  Sums across the wave with lane shuffles, across the four waves
//                       through LDS; 13 lanes add the block's sums to the particle's row with 64-bit integer atomics.
// Integer adds commute: the result depends on no order.  No workgroup waits for another.
#include "rbpf_device.h"

namespace rbpf {

static const int SROWS = BR_EDGE + 2 * 16;   // rows of the window at the largest tol

// dilation shared by both kernels: s_occ rows of 192 bits (bit 64 + j of row r = column j of the block, row r = block row r - m)
// -> s_near[i] bit j: an occupied cell within Chebyshev distance m of block cell (i, j).  Whole workgroup (contains barriers).
__device__ __forceinline__ void score_dilate(const uint32_t* s_occ, uint64_t* s_wide, uint64_t* s_near, int m, int tid) {
    const int rows = BR_EDGE + 2 * m;
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
}

// the lane's reference cells: n (0 .. 16) of them from p
__device__ __forceinline__ void score_ref16(const int8_t* __restrict__ p, int n, int8_t (&r)[16]) {
    union { uint4 u; int8_t c[16]; } q;
    if (n == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) q.u = *reinterpret_cast<const uint4*>(p);
    else {
#pragma unroll
        for (int k = 0; k < 16; ++k) q.c[k] = k < n ? p[k] : (int8_t)0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) r[k] = q.c[k];
}

// occ_word32 where the 32 cells lie in one tile (all but the words at a tile seam): two occupancy words of the tile's row, shifted
// together, instead of 32 single bits
__device__ __forceinline__ uint32_t score_occ_word32(const DevView& v, const int32_t* __restrict__ tab, int u, int w0) {
    const int dim = v.dim, edge = v.L * dim;
    if (u < 0 || u >= edge || w0 < 0 || w0 + 31 >= edge) return occ_word32(v, tab, u, w0);
    const int b = w0 / dim, j = w0 - b * dim;
    if (j + 31 >= dim) return occ_word32(v, tab, u, w0);
    const int a = u / dim, tile = tab[a * v.L + b];
    if (tile < 0) return 0u;
    const uint32_t* __restrict__ row = v.occ + (size_t)tile * dim * v.ow + (size_t)(u - a * dim) * v.ow;
    const int wi = j >> 5, sh = j & 31;
    const uint32_t lo = row[wi];
    return sh ? (lo >> sh) | (row[wi + 1] << (32 - sh)) : lo;   // sh > 0: bit j + 31 lies in word wi + 1 < ow
}

__device__ __forceinline__ int score_class(int x, int thr) { return x < 0 ? 0 : x > thr ? 2 : 1; }

__device__ __forceinline__ int score_wave_add(int x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64); return x; }

__global__ __launch_bounds__(BR_LANES) void score_ref_kernel(ScoreArgs a, int vmin, int vmax, int thr) {
    __shared__ uint32_t s_occ[SROWS * 6];
    __shared__ uint64_t s_wide[SROWS];
    __shared__ uint64_t s_near[BR_EDGE];
    __shared__ int s_sum[4];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int m = a.tol, rows = BR_EDGE + 2 * m, wcols = BR_EDGE + 2 * m;
    for (int k = tid; k < rows * 6; k += BR_LANES) s_occ[k] = 0u;
    if (tid < 4) s_sum[tid] = 0;
    __syncthreads();
    for (int k = tid; k < rows * wcols; k += BR_LANES) {
        const int r = k / wcols, c = k - r * wcols;
        const int ri = BR_EDGE * bx - m + r, rj = BR_EDGE * by - m + c;          // box-relative
        if (ri < 0 || ri >= a.nx || rj < 0 || rj >= a.ny) continue;
        if (a.ref[(size_t)ri * a.ny + rj] > thr) {
            const int pos = BR_EDGE - m + c;
            atomicOr(&s_occ[6 * r + (pos >> 5)], 1u << (pos & 31));
        }
    }
    __syncthreads();
    score_dilate(s_occ, s_wide, s_near, m, tid);
    if (tid < BR_EDGE) a.near_r[(size_t)blockIdx.x * BR_EDGE + tid] = s_near[tid];
    const int i = tid >> 2, j0 = 16 * (tid & 3), ri = BR_EDGE * bx + i, rj0 = BR_EDGE * by + j0;
    int cnt[3] = {0, 0, 0}, sum = 0, bad = 0;
    if (ri < a.nx && rj0 < a.ny) {
        const int n = min(16, a.ny - rj0);
        int8_t r[16];
        score_ref16(a.ref + (size_t)ri * a.ny + rj0, n, r);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k >= n) break;
            const int x = r[k], c = score_class(x, thr);
            cnt[0] += c == 0; cnt[1] += c == 1; cnt[2] += c == 2;
            sum += x < 0 ? -x : x;
            bad |= x < vmin || x > vmax;
        }
    }
    for (int k = 0; k < 3; ++k) cnt[k] = score_wave_add(cnt[k]);
    sum = score_wave_add(sum);
    if ((tid & 63) == 0) {
        for (int k = 0; k < 3; ++k) atomicAdd(&s_sum[k], cnt[k]);
        atomicAdd(&s_sum[3], sum);
    }
    if (a.validate && bad) atomicOr(a.bad, 1);
    __syncthreads();
    if (tid < 4) a.ref_sums[(size_t)blockIdx.x * 4 + tid] = s_sum[tid];
}

__global__ __launch_bounds__(BR_LANES) void score_maps_kernel(DevView v, ScoreArgs a, int vmin, int nv, int thr) {
    __shared__ uint32_t s_occ[SROWS * 6];                 // row r = X0 - tol + r; bit 32 w + k of a row = column Y0 - 64 + 32 w + k
    __shared__ uint64_t s_wide[SROWS];
    __shared__ uint64_t s_near[BR_EDGE];                  // bit j of row i: a map-occupied cell within tol of (X0 + i, Y0 + j)
    __shared__ int32_t s_tab[256];
    __shared__ long long s_red[4][SCORE_FIELDS];
    const int tid = threadIdx.x, pi = blockIdx.y, p = a.particle + pi;
    const int bx = blockIdx.x / a.nby, by = blockIdx.x - bx * a.nby;
    const int X0 = a.x0 + BR_EDGE * bx, Y0 = a.y0 + BR_EDGE * by, m = a.tol, rows = BR_EDGE + 2 * m;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    const int dim = v.dim, off = v.R * dim + dim / 2, edge = v.L * dim;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(a.scores) + (size_t)pi * SCORE_FIELDS;

    // does any tile hold a written cell in the window?  (outside its written box a tile holds 0, its occupancy words too)
    const int u_lo = max(X0 - m + off, 0), u_hi = min(X0 + BR_EDGE - 1 + m + off, edge - 1);
    const int w_lo = max(Y0 - m + off, 0), w_hi = min(Y0 + BR_EDGE - 1 + m + off, edge - 1);
    const int ta_lo = u_lo / dim, ta_n = u_hi / dim - ta_lo + 1, tb_lo = w_lo / dim, tb_n = w_hi / dim - tb_lo + 1;
    int any = 0;
    for (int k = tid; k < ta_n * tb_n; k += BR_LANES) {
        const int ta = ta_lo + k / tb_n, tb = tb_lo + k % tb_n, tile = tab[ta * v.L + tb];
        if (tile < 0) continue;
        const int* bb = v.tile_bbox + 4 * (size_t)tile;
        // tile-local, so that the empty box (INT_MAX, -1) needs no care
        any |= max(u_lo - ta * dim, bb[0]) <= min(u_hi - ta * dim, bb[1]) && max(w_lo - tb * dim, bb[2]) <= min(w_hi - tb * dim, bb[3]);
    }
    if (!__syncthreads_or(any)) {
        if (tid < 5) {
            const int32_t* rs = a.ref_sums + (size_t)blockIdx.x * 4;
            long long add;
            if (tid < 3) add = rs[tid];                                          // n[U][F], n[U][U], n[U][O]
            else if (tid == 3) add = rs[3];                                      // l1 = sum |0 - r|
            else add = a.table ? (long long)a.table[-vmin] * (rs[0] + rs[1] + rs[2]) : 0;
            const int field = tid < 3 ? 3 + tid : tid == 3 ? 11 : 12;
            if (add) atomicAdd(out + field, (unsigned long long)add);
        }
        return;
    }

    for (int k = tid; k < rows * 4; k += BR_LANES) {       // words 1 .. 4 of a row: tol <= 16 reads columns Y0 - 32 .. Y0 + 95 at the most
        const int r = k >> 2, w = 1 + (k & 3);
        s_occ[6 * r + w] = score_occ_word32(v, tab, X0 - m + r + off, Y0 - BR_EDGE + 32 * w + off);
    }
    if (tid < nv) s_tab[tid] = a.table ? a.table[tid] : 0;
    __syncthreads();
    score_dilate(s_occ, s_wide, s_near, m, tid);

    const int i = tid >> 2, j0 = 16 * (tid & 3), ri = BR_EDGE * bx + i, rj0 = BR_EDGE * by + j0;
    unsigned long long pairs = 0ull;                      // nine 5-bit counters, field 3 class(v) + class(r)
    int hit_m = 0, hit_r = 0, l1 = 0;
    long long tsum = 0;
    if (ri < a.nx && rj0 < a.ny) {
        const int n = min(16, a.ny - rj0);
        union { uint4 u; int8_t c[16]; } q;
        q.u = make_uint4(0u, 0u, 0u, 0u);
        const int u = X0 + i + off, ta = u / dim, ti = u - ta * dim;              // inside the lattice: the host checked the box
        const int w0 = Y0 + j0 + off, tb0 = w0 / dim, tj0 = w0 - tb0 * dim;
        if (tj0 + 16 <= dim) {                                                   // the strip lies in one tile (and so in the lattice)
            const int tile = tab[ta * v.L + tb0];
            if (tile >= 0) {
                const int8_t* src = v.pool + (size_t)tile * dim * dim + (size_t)ti * dim + tj0;
                if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) q.u = *reinterpret_cast<const uint4*>(src);
                else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) q.c[k] = src[k];
                }
            }
        } else {
            int cur_b = -1, tile = -1;
            for (int k = 0; k < n; ++k) {                                        // cells of the box: inside the lattice
                const int w = w0 + k, b = w / dim, tj = w - b * dim;
                if (b != cur_b) { tile = tab[ta * v.L + b]; cur_b = b; }
                q.c[k] = tile >= 0 ? v.pool[(size_t)tile * dim * dim + (size_t)ti * dim + tj] : (int8_t)0;
            }
        }
        int8_t r[16];
        score_ref16(a.ref + (size_t)ri * a.ny + rj0, n, r);
        uint32_t occ_m = 0u, occ_r = 0u;
        int tacc = 0;                                                            // 16 entries of at most 2^20
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k >= n) break;
            const int x = q.c[k], y = r[k], cx = score_class(x, thr), cy = score_class(y, thr);
            pairs += 1ull << (5 * (3 * cx + cy));
            occ_m |= (uint32_t)(cx == 2) << k;
            occ_r |= (uint32_t)(cy == 2) << k;
            l1 += x > y ? x - y : y - x;
            tacc += s_tab[min(max(x - vmin, 0), nv - 1)];
        }
        tsum = tacc;
        const uint32_t near_m = (uint32_t)(s_near[i] >> j0), near_r = (uint32_t)(a.near_r[(size_t)blockIdx.x * BR_EDGE + i] >> j0);
        hit_m = __popc(occ_m & near_r);
        hit_r = __popc(occ_r & near_m);
    }
    int val[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) val[k] = (int)((pairs >> (5 * k)) & 31ull);
    val[9] = hit_m; val[10] = hit_r; val[11] = l1;
#pragma unroll
    for (int k = 0; k < 12; ++k) val[k] = score_wave_add(val[k]);
    for (int o = 32; o > 0; o >>= 1) tsum += __shfl_xor(tsum, o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s_red[tid >> 6][k] = val[k];
        s_red[tid >> 6][12] = tsum;
    }
    __syncthreads();
    if (tid < SCORE_FIELDS) {
        const long long add = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
        if (add) atomicAdd(out + tid, (unsigned long long)add);
    }
}

void launch_score_ref(const DevView& v, const ScoreArgs& a, hipStream_t s) {
    score_ref_kernel<<<(unsigned)(a.nbx * a.nby), BR_LANES, 0, s>>>(a, v.cc.vmin, v.cc.vmax, v.cc.thr);
}

void launch_score_maps(const DevView& v, const ScoreArgs& a, hipStream_t s) {
    score_maps_kernel<<<dim3((unsigned)(a.nbx * a.nby), (unsigned)a.n_part), BR_LANES, 0, s>>>(v, a, v.cc.vmin, v.cc.vmax - v.cc.vmin + 1, v.cc.thr);
}

}  // namespace rbpf
