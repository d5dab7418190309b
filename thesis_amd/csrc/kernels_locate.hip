// kernels_locate.hip -- global localization: one scan scored at every free cell and every heading of a search box in one
// particle's map (include/rbpf_hip.h, rbpf_locate_scan; the specification is DESIGN 3.8).
//
// The score of a candidate pose is an integer sum of field values F = occ + dil in {0, 1, 2} at the beams' end cells, and the
// end cell of beam b at rotation r is the candidate cell plus an integer offset (u, w)[r][b] that does not depend on the
// candidate.  So the search is organised over bit planes:
//   locate_field_kernel    the box grown by the largest offset M, as dense rows of {occ, dil} word pairs: bit k of word j of
//                          row i is the cell (x0 - M + i, y0 - M + 32 j + k).  Gathered from the tiles' occupancy words.
//   locate_cand_kernel     the candidate bits (cell < 0) of the box, 32 cells of one row per word, and the list of the words
//                          that hold a candidate at all: the search skips the others.
//   locate_offsets_kernel  (u, w) for every rotation and used beam, float64 with explicit single operations, packed as
//                          u << 16 | word << 5 | shift of the field position the beam reads.
//   locate_search_kernel   a lane owns one candidate word (32 neighbouring y), a workgroup one run of rotations (blockIdx.y).
//                          Rotation and beam are wave-uniform: the table entry is a scalar load, the shift a scalar.  Per
//                          beam a lane loads two neighbouring word pairs of one field row, funnel-shifts them into the F bits
//                          of its 32 candidates and adds them into bit-sliced counters: five low planes per beam, carried
//                          into sixteen high planes every 15 beams (2 * 15 < 32).  After the last beam the 32 scores are
//                          compared with the running best, still bit-sliced (strictly greater wins, rotations ascend: the
//                          smallest r is kept).  At the end the lane unpacks its candidates and merges them across the
//                          workgroups of other rotations with atomicMax on score << 16 | (n_rot - 1 - r).
//   locate_final_kernel    packed -> best, rot; -1 where the cell is no candidate.
// The field of a 16 m room is a few hundred KB and stays in L2; it is not staged in LDS.
#include "rbpf_internal.h"

namespace rbpf {

static const int LB = 256;
static const int LOW_BEAMS = 15;      // beams between two carries of the low planes: 2 * 15 fits their 5 bits

// bits k = 0 .. n-1: cell (u, w0 + k) of the particle's map is occupied.  (u, w) = mosaic (X, Y) + off count from the lattice's
// first cell; outside the lattice, without a tile and outside a tile's written box the occupancy words hold 0.
__device__ __forceinline__ uint64_t occ_run(const DevView& v, const int32_t* __restrict__ tab, int u, int w0, int n) {
    const int dim = v.dim, edge = v.L * dim;
    if (u < 0 || u >= edge) return 0ull;
    const int a = u / dim, i = u - a * dim;
    uint64_t bits = 0ull;
    int cur_b = -1, cur_w = -1, tile = -1;
    uint32_t word = 0u;
    for (int k = 0; k < n; ++k) {
        const int w = w0 + k;
        if (w < 0 || w >= edge) continue;
        const int b = w / dim, j = w - b * dim;
        if (b != cur_b) { tile = tab[a * v.L + b]; cur_b = b; cur_w = -1; }
        if ((j >> 5) != cur_w) {
            cur_w = j >> 5;
            word = tile >= 0 ? v.occ[(size_t)tile * dim * v.ow + (size_t)i * v.ow + cur_w] : 0u;
        }
        bits |= (uint64_t)((word >> (j & 31)) & 1u) << k;
    }
    return bits;
}

__global__ __launch_bounds__(LB) void locate_field_kernel(DevView v, LocateArgs a) {
    const long long t = (long long)blockIdx.x * LB + threadIdx.x;
    if (t >= (long long)a.rows * a.W) return;
    const int row = (int)(t / a.W), wj = (int)(t - (long long)row * a.W);
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[a.particle] * v.L * v.L;
    const int off = v.R * v.dim + v.dim / 2;
    const int u = a.x0 - a.M + row + off, w = a.y0 - a.M + 32 * wj + off;
    // 34 cells of three rows: bit k is column w - 1 + k
    const uint64_t mid = occ_run(v, tab, u, w - 1, 34);
    const uint64_t any = mid | occ_run(v, tab, u - 1, w - 1, 34) | occ_run(v, tab, u + 1, w - 1, 34);
    a.field[t] = make_uint2((uint32_t)(mid >> 1), (uint32_t)(any | (any >> 1) | (any >> 2)));
}

__global__ __launch_bounds__(LB) void locate_cand_kernel(DevView v, LocateArgs a) {
    const long long t = (long long)blockIdx.x * LB + threadIdx.x;
    if (t >= (long long)a.nx * a.nyw) return;
    const int row = (int)(t / a.nyw), kw = (int)(t - (long long)row * a.nyw);
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[a.particle] * v.L * v.L;
    const int dim = v.dim, off = v.R * dim + dim / 2;
    const int u = a.x0 + row + off, w0 = a.y0 + 32 * kw + off;       // inside the lattice: the host checked the box
    const int aa = u / dim, i = u - aa * dim;
    const int n = min(32, a.ny - 32 * kw);
    uint32_t bits = 0u;
    int cur_b = -1, tile = -1;
    for (int k = 0; k < n; ++k) {
        const int w = w0 + k, b = w / dim, j = w - b * dim;
        if (b != cur_b) { tile = tab[aa * v.L + b]; cur_b = b; }
        if (tile >= 0 && v.pool[(size_t)tile * dim * dim + (size_t)i * dim + j] < 0) bits |= 1u << k;
    }
    a.cand[t] = bits;
    if (bits) a.items[atomicAdd(a.n_items, 1)] = (int32_t)t;
}

__global__ __launch_bounds__(LB) void locate_offsets_kernel(LocateArgs a) {
    const long long t = (long long)blockIdx.x * LB + threadIdx.x;
    if (t >= (long long)a.n_rot * a.nb) return;
    const int r = (int)(t / a.nb), b = (int)(t - (long long)r * a.nb);
    const double2 cs = reinterpret_cast<const double2*>(a.cs)[r], xy = reinterpret_cast<const double2*>(a.bxy)[b];
    const double fu = __builtin_floor(__dadd_rn(0.5, __dmul_rn(__dsub_rn(__dmul_rn(cs.x, xy.x), __dmul_rn(cs.y, xy.y)), a.inv)));
    const double fw = __builtin_floor(__dadd_rn(0.5, __dmul_rn(__dadd_rn(__dmul_rn(cs.y, xy.x), __dmul_rn(cs.x, xy.y)), a.inv)));
    // |offset| <= M for every used beam (range < match_max_range); the clamp only keeps a read inside the field whatever comes
    const double m = (double)a.M;
    const int u = (int)fmin(fmax(fu, -m), m), w = (int)fmin(fmax(fw, -m), m);
    const int pos = a.M + w;                                             // bit of the field row that candidate bit 0 reads
    a.offs[t] = (int32_t)(((uint32_t)u << 16) | (uint32_t)((pos >> 5) << 5) | (uint32_t)(pos & 31));
}

// the F bits of beam entry e for the lane's 32 candidates, added into the low planes
#define LOCATE_BEAM(e)                                                                            \
    {                                                                                             \
        const int32_t e_ = (e);                                                                   \
        const uint2* p_ = base + (long long)(e_ >> 16) * a.W + ((e_ >> 5) & 2047);                \
        const uint2 lo_ = p_[0], hi_ = p_[1];                                                     \
        const uint32_t oc_ = __builtin_amdgcn_alignbit(hi_.x, lo_.x, (uint32_t)(e_ & 31));        \
        const uint32_t di_ = __builtin_amdgcn_alignbit(hi_.y, lo_.y, (uint32_t)(e_ & 31));        \
        const uint32_t x0_ = di_ & ~oc_;                       /* F = 2 occ + (dil and not occ) */ \
        uint32_t c_ = l0 & x0_; l0 ^= x0_;                                                        \
        const uint32_t t_ = l1 ^ oc_; const uint32_t c2_ = (l1 & oc_) | (t_ & c_); l1 = t_ ^ c_;  \
        c_ = l2 & c2_; l2 ^= c2_;                                                                 \
        const uint32_t c3_ = l3 & c_; l3 ^= c_;                                                   \
        l4 ^= c3_;                                                                                \
    }

__global__ __launch_bounds__(LB) void locate_search_kernel(LocateArgs a) {
    const int idx = blockIdx.x * LB + threadIdx.x;
    if (idx >= *a.n_items) return;
    const int item = a.items[idx], row = item / a.nyw, kw = item - row * a.nyw;
    const uint32_t cand = a.cand[item];
    const uint2* __restrict__ base = a.field + (size_t)(row + a.M) * a.W + kw;
    const int r0 = blockIdx.y * a.rpw, r1 = min(a.n_rot, r0 + a.rpw), nb = a.nb;
    uint32_t bs[16], br[12];                                             // best score and its rotation, bit-sliced
#pragma unroll
    for (int k = 0; k < 16; ++k) bs[k] = 0u;
#pragma unroll
    for (int k = 0; k < 12; ++k) br[k] = ((r0 >> k) & 1) ? ~0u : 0u;
    for (int r = r0; r < r1; ++r) {
        const int32_t* __restrict__ o = a.offs + (size_t)r * nb;
        uint32_t H[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) H[k] = 0u;
        for (int b0 = 0; b0 < nb; b0 += LOW_BEAMS) {
            uint32_t l0 = 0u, l1 = 0u, l2 = 0u, l3 = 0u, l4 = 0u;
            if (b0 + LOW_BEAMS <= nb) {
#pragma unroll
                for (int j = 0; j < LOW_BEAMS; ++j) LOCATE_BEAM(o[b0 + j])
            } else {
                for (int b = b0; b < nb; ++b) LOCATE_BEAM(o[b])
            }
            const uint32_t l[5] = {l0, l1, l2, l3, l4};
            uint32_t carry = 0u;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint32_t t = H[k] ^ l[k], cn = (H[k] & l[k]) | (t & carry);
                H[k] = t ^ carry; carry = cn;
            }
#pragma unroll
            for (int k = 5; k < 16; ++k) { const uint32_t cn = H[k] & carry; H[k] ^= carry; carry = cn; }
        }
        uint32_t gt = 0u, eq = ~0u;
#pragma unroll
        for (int k = 15; k >= 0; --k) { gt |= eq & H[k] & ~bs[k]; eq &= ~(H[k] ^ bs[k]); }
#pragma unroll
        for (int k = 0; k < 16; ++k) bs[k] = (H[k] & gt) | (bs[k] & ~gt);
#pragma unroll
        for (int k = 0; k < 12; ++k) br[k] = (((r >> k) & 1) ? gt : 0u) | (br[k] & ~gt);
    }
    uint32_t* __restrict__ out = a.packed + (size_t)row * a.ny + 32 * kw;
    for (int k = 0; k < 32; ++k) {
        if (!((cand >> k) & 1u)) continue;                               // (bits at Y >= y1 are never set)
        uint32_t sc = 0u, rr = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) sc |= ((bs[j] >> k) & 1u) << j;
#pragma unroll
        for (int j = 0; j < 12; ++j) rr |= ((br[j] >> k) & 1u) << j;
        atomicMax(out + k, (sc << 16) | (uint32_t)(a.n_rot - 1 - (int)rr));
    }
}
#undef LOCATE_BEAM

__global__ __launch_bounds__(LB) void locate_final_kernel(LocateArgs a) {
    const long long c = (long long)blockIdx.x * LB + threadIdx.x;
    if (c >= (long long)a.nx * a.ny) return;
    const int row = (int)(c / a.ny), y = (int)(c - (long long)row * a.ny);
    const bool is_cand = (a.cand[(size_t)row * a.nyw + (y >> 5)] >> (y & 31)) & 1u;
    const uint32_t p = a.packed[c];
    a.best[c] = is_cand ? (int32_t)(p >> 16) : -1;
    if (a.rot) a.rot[c] = is_cand ? a.n_rot - 1 - (int32_t)(p & 0xffffu) : -1;
}

static unsigned blocks_for(long long n) { return (unsigned)((n + LB - 1) / LB); }

void launch_locate_field(const DevView& v, const LocateArgs& a, hipStream_t s) {
    locate_field_kernel<<<blocks_for((long long)a.rows * a.W), LB, 0, s>>>(v, a);
}

void launch_locate_scan(const DevView& v, const LocateArgs& a, hipStream_t s) {
    const long long words = (long long)a.nx * a.nyw;
    locate_field_kernel<<<blocks_for((long long)a.rows * a.W), LB, 0, s>>>(v, a);
    locate_cand_kernel<<<blocks_for(words), LB, 0, s>>>(v, a);
    if (a.nb > 0) locate_offsets_kernel<<<blocks_for((long long)a.n_rot * a.nb), LB, 0, s>>>(a);
    locate_search_kernel<<<dim3(blocks_for(words), (unsigned)((a.n_rot + a.rpw - 1) / a.rpw)), LB, 0, s>>>(a);
    locate_final_kernel<<<blocks_for((long long)a.nx * a.ny), LB, 0, s>>>(a);
}

}  // namespace rbpf
