// kernels_build.hip -- the map that a list of scans draws from a list of poses (include/rbpf_hip.h, rbpf_build_map):
// per cell of a box, in how many scans a return beam ended there (hits) and in how many scans any beam passed or ended there
// (seen).  Counts are per scan: a scan's beams form SETS of cells first, as in kernels_gain.hip, and the sets are added up.
//
// One workgroup per scan, one bitmap in LDS used twice (two bitmaps of the widest window do not fit 160 KB):
//   1. zero the bitmap: one row per X of the window [X0 - M, X0 + M] round the pose's cell, bits along Y, bit 0 of a row the
//      column ybase = (Y0 - M) rounded down to a multiple of 32, W = ceil((2M + 1) / 32) + 1 words per row;
//   2. the waves take the beams 64 at a time from a counter in LDS; each lane runs walk_free (rbpf_raywalk.h: the walk of DESIGN
//      3.7 with no map to test) to the beam's end and ORs every cell into the bitmap, the bits of one word gathered in a register
//      and issued as one non-returning LDS OR when the walk changes word.  The end cell of a return beam goes into `ends`;
//   3. sweep the bitmap into `seen` (below);
//   4. zero the bitmap again, mark the end cells listed in `ends` (no second walk), sweep it into `hits`.
// The sweep adds 1 to the cell of every set bit with a relaxed agent-scope integer atomic.  A wave instruction covers 64
// consecutive Y of one row, 256 contiguous bytes, the lanes of clear bits masked off.  Each lane first looks at one such pair of
// words; a ballot then names the pairs that hold a bit at all, and only those are issued.  Rows outside the box are not swept.
// Integer adds commute: the rasters are the same bits whatever the schedule.
#include "rbpf_raywalk.h"

namespace rbpf {

static const int BB = 1024;            // 16 waves: with a window of more than 80 KB one workgroup has the CU to itself

// adds the bitmap's rows [r_lo, r_hi) into out: row r is box row i0 + r, bit 0 of a row is box column j0 (either may be negative)
__device__ __forceinline__ void sweep_add(const uint32_t* bits, const int W, const int r_lo, const int r_hi, const long long i0,
                                          const long long j0, const int nx, const int ny, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int WP = (W + 1) / 2, npairs = (r_hi - r_lo) * WP;              // pairs of words: 64 cells
    for (int base = wave * 64; base < npairs; base += BB) {
        const int q = base + lane;
        bool any = false;
        if (q < npairs) {
            const int r = q / WP, wp = q - r * WP;
            const uint32_t* w = bits + (size_t)(r_lo + r) * W + 2 * wp;
            any = (w[0] | (2 * wp + 1 < W ? w[1] : 0u)) != 0u;
        }
        unsigned long long todo = __ballot(any);
        while (todo) {
            const int k = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int r = (base + k) / WP, wp = (base + k) - r * WP, wi = 2 * wp + (lane >> 5);
            const uint32_t word = wi < W ? bits[(size_t)(r_lo + r) * W + wi] : 0u;
            const long long i = i0 + r_lo + r, j = j0 + 64 * wp + lane;
            if (((word >> (lane & 31)) & 1u) && i >= 0 && i < nx && j >= 0 && j < ny)
                __hip_atomic_fetch_add(out + (size_t)i * ny + (size_t)j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ __launch_bounds__(BB) void build_map_kernel(BuildArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t* bits = reinterpret_cast<uint32_t*>(smem);                  // [2M + 1][W], padded to 16 bytes
    __shared__ int s_next;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = blockIdx.x;
    const int M = a.M, W = a.W, rows = 2 * M + 1, nw = rows * W;
    const double4 ps = reinterpret_cast<const double4*>(a.pose4)[n];     // x, y, cos(theta), sin(theta)
    const double fX = __builtin_floor(ps.x * a.inv), fY = __builtin_floor(ps.y * a.inv);   // the walk's origin cell
    // no cell of the scan lies farther than M from it (the window bound): a window that misses the box adds nothing
    if (!(fX >= (double)a.x0 - M && fX < (double)a.x0 + a.nx + M && fY >= (double)a.y0 - M && fY < (double)a.y0 + a.ny + M)) return;
    const long long X0 = (long long)fX, Y0 = (long long)fY;
    const long long ybase = (Y0 - M) & ~31LL;                             // column of bit 0 of a row
    const int yb0 = (int)(Y0 - ybase);                                    // the origin's bit in a row: M .. M + 31
    const long long i0 = X0 - M - a.x0, j0 = ybase - a.y0;                // box row of bitmap row 0, box column of bit 0
    const int r_lo = i0 < 0 ? (int)-i0 : 0, r_hi = i0 + rows > a.nx ? (int)(a.nx - i0) : rows;   // 0 <= r_lo < r_hi <= rows

    for (int k = tid; k < (nw + 3) / 4; k += BB) reinterpret_cast<uint4*>(bits)[k] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) s_next = 0;
    __syncthreads();

    const double* __restrict__ rng = a.ranges + (size_t)n * a.B;
    uint32_t* __restrict__ ends = a.ends + (size_t)n * a.B;
    for (;;) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_next, 64);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= a.B) break;
        const int b = base + lane;
        if (b < a.B) {
            const double r = rng[b];
            uint32_t end = 0u;
            if (!(r != r) && !(r < a.min_range)) {                        // NaN and r < min_range: the beam is skipped
                const bool ret = !(r > a.max_range);                      // beyond max_range (+inf too): free to max_range, no hit
                const double tend = ret ? r * a.inv : a.tlim;
                const RayStart rs = ray_start(ps, reinterpret_cast<const double2*>(a.beam2)[b], a.inv);
                int cur = -1, kx, ky;
                uint32_t pend = 0u;
                walk_free(rs, tend, kx, ky, [&](int cx, int cy) {
                    const int row = M + cx, yb = yb0 + cy;
                    if ((unsigned)row >= (unsigned)rows || (unsigned)yb >= (unsigned)(32 * W)) return;   // never: the window bound
                    const int k = row * W + (yb >> 5);
                    if (k != cur) {
                        if (pend) atomicOr(&bits[cur], pend);
                        cur = k; pend = 0u;
                    }
                    pend |= 1u << (yb & 31);
                });
                if (pend) atomicOr(&bits[cur], pend);
                const int row = M + kx, yb = yb0 + ky;
                if (ret && (unsigned)row < (unsigned)rows && (unsigned)yb < (unsigned)(32 * W))
                    end = ((uint32_t)(row * 32 * W + yb) << 1) | 1u;
            }
            ends[b] = end;
        }
    }
    __syncthreads();
    if (a.seen) sweep_add(bits, W, r_lo, r_hi, i0, j0, a.nx, a.ny, a.seen);
    if (!a.hits) return;
    __syncthreads();                                                      // the sweep has read the bitmap; `ends` is this workgroup's own
    for (int k = tid; k < (nw + 3) / 4; k += BB) reinterpret_cast<uint4*>(bits)[k] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (int b = tid; b < a.B; b += BB) {
        const uint32_t end = ends[b];
        if (end & 1u) atomicOr(&bits[end >> 6], 1u << ((end >> 1) & 31));   // (row * 32 W + yb) >> 5 = row * W + (yb >> 5)
    }
    __syncthreads();
    sweep_add(bits, W, r_lo, r_hi, i0, j0, a.nx, a.ny, a.hits);
}

static size_t build_map_lds_bytes(int M, int W) { return (((size_t)(2 * M + 1) * W * 4) + 15) & ~(size_t)15; }

void launch_build_map(const BuildArgs& a, hipStream_t s) {
    const size_t lds = build_map_lds_bytes(a.M, a.W);
    static size_t lds_set[MAX_DEVICES] = {};   // more than the default 64 KiB of dynamic LDS
    ensure_dynamic_lds(reinterpret_cast<const void*>(build_map_kernel), lds, lds_set);
    build_map_kernel<<<(unsigned)a.n_scans, BB, lds, s>>>(a);
}

}  // namespace rbpf
