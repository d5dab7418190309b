// kernels_gain.hip -- what a scan taken at a pose would observe in a particle's map (include/rbpf_hip.h, rbpf_view_gain;
// DESIGN 3.11): the SET of cells the pose's beams test, reduced against the map.
//
// One workgroup per (particle, pose), three phases:
//   1. zero a bitmap in LDS: one row per X of the window [X0 - M, X0 + M], bits along Y.  Bit 0 of a row is the lattice
//      column wbase = (w0 - M) rounded down to a multiple of 32 (w = Y + off counts cells from the lattice's first column),
//      so a row has W = ceil((2M + 1) / 32) + 1 words, and because dim is a multiple of 16 each half of a word is 16 cells of
//      ONE tile row, 16-byte aligned in the pool;
//   2. the waves take the beams 64 at a time from a counter in LDS; each lane runs walk_ray (rbpf_raywalk.h, the walk of
//      cast_scans_kernel) and ORs the bit of every cell it tests into the bitmap - bits of one bitmap word are gathered in a
//      register and stored with one non-returning LDS OR when the walk moves on to another word (every x step, every 32nd
//      y step);
//   3. after a barrier the lanes sweep the bitmap words: for every half word that is not 0 they load its 16 int8 cells (none
//      where there is no tile or the half lies outside tile_bbox: those cells are 0), look the marked ones up in the table
//      (LDS) and add up gain (64 bits), seen and unknown; the sums are reduced inside the wave, across the waves through LDS,
//      and lane 0 stores them.
// No global atomics and integer sums only: the result is the same whatever the order.
#include "rbpf_raywalk.h"

namespace rbpf {

static const int GB = 1024;            // 16 waves: with a window of more than 80 KB one workgroup has the CU to itself

union Cells16 { uint4 u; int8_t c[16]; };

__global__ __launch_bounds__(GB) void view_gain_kernel(DevView v, GainArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t* bits = reinterpret_cast<uint32_t*>(smem);                  // [2M + 1][W], padded to 16 bytes
    __shared__ int32_t s_tab[256];
    __shared__ unsigned long long s_gain[GB / 64];
    __shared__ int s_seen[GB / 64], s_unk[GB / 64], s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x % a.n_poses, p = a.particle >= 0 ? a.particle : (int)(blockIdx.x / a.n_poses);
    const int L = v.L, dim = v.dim, M = a.M, W = a.W, rows = 2 * M + 1, nw = rows * W;
    const double4 ps = reinterpret_cast<const double4*>(a.pose4)[n];     // x, y, cos(theta), sin(theta)
    const double fX = __builtin_floor(ps.x * a.inv), fY = __builtin_floor(ps.y * a.inv);   // the walk's origin cell
    const int off = v.R * dim + dim / 2;                                  // mosaic X + off = tile * dim + cell
    const double lo = -(double)off, hi = (double)(L * dim - off);
    if (!(fX >= lo && fX < hi && fY >= lo && fY < hi)) {                  // origin outside the lattice: nothing is seen
        if (tid == 0) {
            a.gain[blockIdx.x] = 0;
            if (a.seen) a.seen[blockIdx.x] = 0;
            if (a.unknown) a.unknown[blockIdx.x] = 0;
        }
        return;
    }
    const int u0 = (int)fX + off - M, w0 = (int)fY + off;                 // lattice row of bitmap row 0; the origin's column
    const int wbase = (w0 - M) & ~31;                                     // lattice column of bit 0 (may lie before the lattice)
    const int yb0 = w0 - wbase;                                           // the origin's bit in a row: M .. M + 31

    for (int k = tid; k < (nw + 3) / 4; k += GB) reinterpret_cast<uint4*>(bits)[k] = make_uint4(0u, 0u, 0u, 0u);
    if (tid < a.nv) s_tab[tid] = a.table[tid];
    if (tid == 0) s_next = 0;
    __syncthreads();

    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * L * L;
    for (;;) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_next, 64);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= a.B) break;
        const int b = base + lane;
        if (b < a.B) {
            const double2 bm = reinterpret_cast<const double2*>(a.beam2)[b]; // cos(angle), sin(angle)
            int cur = -1;
            uint32_t pend = 0u;
            double t;
            walk_ray(v, tab, ps, bm, a.inv, a.tlim, t, [&](int kx, int ky) {
                const int row = M + kx, yb = yb0 + ky;
                if ((unsigned)row >= (unsigned)rows || (unsigned)yb >= (unsigned)(32 * W)) return;   // never: DESIGN 3.11, the window bound
                const int k = row * W + (yb >> 5);
                if (k != cur) {
                    if (pend) atomicOr(&bits[cur], pend);
                    cur = k; pend = 0u;
                }
                pend |= 1u << (yb & 31);
            });
            if (pend) atomicOr(&bits[cur], pend);
        }
    }
    __syncthreads();

    unsigned long long gain = 0ull;
    int seen = 0, unk = 0;
    const int vmin = v.cc.vmin;
    const int32_t zero_gain = s_tab[0 - vmin];
    int cur_pos = -1, tile = -1, b0 = 0, b1 = -1, b2 = 0, b3 = -1;
    for (int k = tid; k < nw; k += GB) {
        const uint32_t m = bits[k];
        if (!m) continue;
        const int row = k / W, u = u0 + row, ta = u / dim, i = u - ta * dim;    // a marked cell lies in the lattice: 0 <= u < L dim
        const int ws = wbase + 32 * (k - row * W);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t mh = (m >> (16 * h)) & 0xffffu;
            if (!mh) continue;
            const int wh = ws + 16 * h, tb = wh / dim, j = wh - tb * dim;       // 16 cells of one tile row (dim % 16 == 0)
            const int pos = ta * L + tb;
            if (pos != cur_pos) {
                cur_pos = pos; tile = tab[pos]; b1 = b3 = -1; b0 = b2 = 0;
                if (tile >= 0) { const int* bb = v.tile_bbox + 4 * (size_t)tile; b0 = bb[0]; b1 = bb[1]; b2 = bb[2]; b3 = bb[3]; }
            }
            const int cnt = __popc(mh);
            seen += cnt;
            if (tile < 0 || i < b0 || i > b1 || j > b3 || j + 15 < b2) {        // no tile, or outside its written box: 0
                unk += cnt; gain += (unsigned long long)cnt * (unsigned)zero_gain;
                continue;
            }
            Cells16 c;
            c.u = *reinterpret_cast<const uint4*>(v.pool + (size_t)tile * dim * dim + (size_t)i * dim + j);
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if ((mh >> q) & 1u) {
                    const int val = c.c[q];
                    unk += val == 0;
                    gain += (unsigned)s_tab[val - vmin];
                }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        gain += __shfl_down(gain, d);
        seen += __shfl_down(seen, d);
        unk += __shfl_down(unk, d);
    }
    if (lane == 0) { s_gain[wave] = gain; s_seen[wave] = seen; s_unk[wave] = unk; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < GB / 64; ++q) { gain += s_gain[q]; seen += s_seen[q]; unk += s_unk[q]; }
        a.gain[blockIdx.x] = (int64_t)gain;
        if (a.seen) a.seen[blockIdx.x] = seen;
        if (a.unknown) a.unknown[blockIdx.x] = unk;
    }
}

size_t view_gain_lds_bytes(int M, int W) { return (((size_t)(2 * M + 1) * W * 4) + 15) & ~(size_t)15; }

void launch_view_gain(const DevView& v, const GainArgs& a, hipStream_t s) {
    const size_t lds = view_gain_lds_bytes(a.M, a.W);
    static size_t lds_set[MAX_DEVICES] = {};   // more than the default 64 KiB of dynamic LDS
    ensure_dynamic_lds(reinterpret_cast<const void*>(view_gain_kernel), lds, lds_set);
    const unsigned blocks = (unsigned)((a.particle >= 0 ? 1 : v.P) * (long long)a.n_poses);
    view_gain_kernel<<<blocks, GB, lds, s>>>(v, a);
}

}  // namespace rbpf
