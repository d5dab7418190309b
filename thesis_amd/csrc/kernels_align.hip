// kernels_align.hip -- alignment of a point set of unknown pose to one particle's map: occupied and free points scored at every
// cell and every rotation of a search box (include/rbpf_hip.h, rbpf_align_points; the specification is DESIGN 3.10).
//
// score = hits - 2 clash, with hits = sum over occupied points of F = occ + dil and clash = free points that land on an occupied
// cell.  The kernels sum the biased score hits + 2 (n_free - clash) >= 0: an occupied point adds F, a free point adds 2 * !occ,
// both in {0, 1, 2}, so the search is locate's (kernels_locate.hip) over bit planes, without a candidate gate:
//   locate_field_kernel    (shared, launch_locate_field) the box grown by M as rows of {occ, dil} word pairs.
//   align_offsets_kernel   (u, w) for every rotation of the window and every point, float64 with explicit single operations,
//                          packed as u << 16 | word << 5 | shift of the field position the point reads.
//   align_search_kernel    a lane owns one word of the box (32 neighbouring Y), a workgroup one run of rotations (blockIdx.y).
//                          Rotation and point are wave-uniform: the table entry is a scalar load, the shift a scalar.  Per point
//                          a lane loads two neighbouring word pairs of one field row and funnel-shifts them onto its 32 cells;
//                          the occupied run adds F into five low planes, the free run adds 2 * !occ into the upper four of
//                          them, and either run is carried into sixteen high planes every 15 entries (2 * 15 < 32).  The running
//                          best stays bit-sliced (strictly greater wins, rotations ascend: the smallest r is kept); at the end
//                          the lane unpacks its cells and merges them across rotation runs with atomicMax on
//                          biased score << 16 | (n_rot - 1 - r).
//   align_final_kernel     packed -> best = biased score - 2 n_free, rot.
#include "rbpf_internal.h"

namespace rbpf {

static const int AB = 256;
static const int LOW_POINTS = 15;     // entries between two carries of the low planes: 2 * 15 fits their 5 bits

__global__ __launch_bounds__(AB) void align_offsets_kernel(AlignArgs a) {
    const long long t = (long long)blockIdx.x * AB + threadIdx.x;
    if (t >= (long long)a.r_count * a.np) return;
    const int r = (int)(t / a.np), k = (int)(t - (long long)r * a.np);
    const double2 cs = reinterpret_cast<const double2*>(a.cs)[r], xy = reinterpret_cast<const double2*>(a.pxy)[k];
    const double fu = __builtin_floor(__dadd_rn(0.5, __dmul_rn(__dsub_rn(__dmul_rn(cs.x, xy.x), __dmul_rn(cs.y, xy.y)), a.inv)));
    const double fw = __builtin_floor(__dadd_rn(0.5, __dmul_rn(__dadd_rn(__dmul_rn(cs.y, xy.x), __dmul_rn(cs.x, xy.y)), a.inv)));
    // |offset| <= M for every point (M = ceil(max hypot * inv) + 1); the clamp only keeps a read inside the field whatever comes
    const double m = (double)a.M;
    const int u = (int)fmin(fmax(fu, -m), m), w = (int)fmin(fmax(fw, -m), m);
    const int pos = a.M + w;                                             // bit of the field row that cell bit 0 reads
    a.offs[t] = (int32_t)(((uint32_t)u << 16) | (uint32_t)pos);          // pos = word << 5 | shift, at most 2 M <= 32768
}

// the {occ, dil} bits of table entry e for the lane's 32 cells
#define ALIGN_FETCH(e)                                                                            \
        const int32_t e_ = (e);                                                                   \
        const uint2* p_ = base + (long long)(e_ >> 16) * a.W + ((e_ >> 5) & 2047);                \
        const uint2 lo_ = p_[0], hi_ = p_[1];
// an occupied point: F = 2 occ + (dil and not occ) added into the low planes
#define ALIGN_OCC(e)                                                                              \
    {                                                                                             \
        ALIGN_FETCH(e)                                                                            \
        const uint32_t oc_ = __builtin_amdgcn_alignbit(hi_.x, lo_.x, (uint32_t)(e_ & 31));        \
        const uint32_t di_ = __builtin_amdgcn_alignbit(hi_.y, lo_.y, (uint32_t)(e_ & 31));        \
        const uint32_t x0_ = di_ & ~oc_;                                                          \
        uint32_t c_ = l0 & x0_; l0 ^= x0_;                                                        \
        const uint32_t t_ = l1 ^ oc_; const uint32_t c2_ = (l1 & oc_) | (t_ & c_); l1 = t_ ^ c_;  \
        c_ = l2 & c2_; l2 ^= c2_;                                                                 \
        const uint32_t c3_ = l3 & c_; l3 ^= c_;                                                   \
        l4 ^= c3_;                                                                                \
    }
// a free point: 2 * (not occ) added into the low planes (plane 0 stays 0 in a free group)
#define ALIGN_FREE(e)                                                                             \
    {                                                                                             \
        ALIGN_FETCH(e)                                                                            \
        const uint32_t nf_ = ~__builtin_amdgcn_alignbit(hi_.x, lo_.x, (uint32_t)(e_ & 31));       \
        uint32_t c_ = l1 & nf_; l1 ^= nf_;                                                        \
        const uint32_t c2_ = l2 & c_; l2 ^= c_;                                                   \
        const uint32_t c3_ = l3 & c2_; l3 ^= c2_;                                                 \
        l4 ^= c3_;                                                                                \
    }
// one run of n table entries o[0 .. n), in groups of LOW_POINTS, each group carried into the high planes H
#define ALIGN_RUN(o, n, POINT)                                                                    \
    for (int b0 = 0; b0 < (n); b0 += LOW_POINTS) {                                                \
        uint32_t l0 = 0u, l1 = 0u, l2 = 0u, l3 = 0u, l4 = 0u;                                     \
        if (b0 + LOW_POINTS <= (n)) {                                                             \
            _Pragma("unroll") for (int j = 0; j < LOW_POINTS; ++j) POINT((o)[b0 + j])             \
        } else {                                                                                  \
            for (int b = b0; b < (n); ++b) POINT((o)[b])                                          \
        }                                                                                         \
        const uint32_t l[5] = {l0, l1, l2, l3, l4};                                               \
        uint32_t carry = 0u;                                                                      \
        _Pragma("unroll") for (int k = 0; k < 5; ++k) {                                           \
            const uint32_t t = H[k] ^ l[k], cn = (H[k] & l[k]) | (t & carry);                     \
            H[k] = t ^ carry; carry = cn;                                                         \
        }                                                                                         \
        _Pragma("unroll") for (int k = 5; k < 16; ++k) { const uint32_t cn = H[k] & carry; H[k] ^= carry; carry = cn; } \
    }

__global__ __launch_bounds__(AB) void align_search_kernel(AlignArgs a) {
    const int idx = blockIdx.x * AB + threadIdx.x;
    if (idx >= a.nx * a.nyw) return;
    const int row = idx / a.nyw, kw = idx - row * a.nyw;
    const uint2* __restrict__ base = a.field + (size_t)(row + a.M) * a.W + kw;
    // rotations of this run, as indices into the window's tables; r_begin + q is the rotation itself
    const int q0 = blockIdx.y * a.rpw, q1 = min(a.r_count, q0 + a.rpw), n_occ = a.n_occ, n_free = a.np - a.n_occ;
    uint32_t bs[16], br[12];                                             // best biased score and its rotation, bit-sliced
#pragma unroll
    for (int k = 0; k < 16; ++k) bs[k] = 0u;
#pragma unroll
    for (int k = 0; k < 12; ++k) br[k] = (((a.r_begin + q0) >> k) & 1) ? ~0u : 0u;
    for (int q = q0; q < q1; ++q) {
        const int32_t* __restrict__ oo = a.offs + (size_t)q * a.np;
        const int32_t* __restrict__ of = oo + n_occ;
        const int r = a.r_begin + q;
        uint32_t H[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) H[k] = 0u;
        ALIGN_RUN(oo, n_occ, ALIGN_OCC)
        ALIGN_RUN(of, n_free, ALIGN_FREE)
        uint32_t gt = 0u, eq = ~0u;
#pragma unroll
        for (int k = 15; k >= 0; --k) { gt |= eq & H[k] & ~bs[k]; eq &= ~(H[k] ^ bs[k]); }
#pragma unroll
        for (int k = 0; k < 16; ++k) bs[k] = (H[k] & gt) | (bs[k] & ~gt);
#pragma unroll
        for (int k = 0; k < 12; ++k) br[k] = (((r >> k) & 1) ? gt : 0u) | (br[k] & ~gt);
    }
    uint32_t* __restrict__ out = a.packed + (size_t)row * a.ny + 32 * kw;
    const int n = min(32, a.ny - 32 * kw);                               // the last word of a row may be partial
    for (int k = 0; k < n; ++k) {
        uint32_t sc = 0u, rr = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) sc |= ((bs[j] >> k) & 1u) << j;
#pragma unroll
        for (int j = 0; j < 12; ++j) rr |= ((br[j] >> k) & 1u) << j;
        atomicMax(out + k, (sc << 16) | (uint32_t)(a.n_rot - 1 - (int)rr));
    }
}
#undef ALIGN_RUN
#undef ALIGN_FREE
#undef ALIGN_OCC
#undef ALIGN_FETCH

__global__ __launch_bounds__(AB) void align_final_kernel(AlignArgs a) {
    const long long c = (long long)blockIdx.x * AB + threadIdx.x;
    if (c >= (long long)a.nx * a.ny) return;
    const uint32_t p = a.packed[c];
    a.best[c] = (int32_t)(p >> 16) - 2 * (a.np - a.n_occ);
    if (a.rot) a.rot[c] = a.n_rot - 1 - (int32_t)(p & 0xffffu);
}

static unsigned blocks_for(long long n) { return (unsigned)((n + AB - 1) / AB); }

void launch_align_points(const DevView& v, const LocateArgs& f, const AlignArgs& a, hipStream_t s) {
    launch_locate_field(v, f, s);
    align_offsets_kernel<<<blocks_for((long long)a.r_count * a.np), AB, 0, s>>>(a);
    align_search_kernel<<<dim3(blocks_for((long long)a.nx * a.nyw), (unsigned)((a.r_count + a.rpw - 1) / a.rpw)), AB, 0, s>>>(a);
    align_final_kernel<<<blocks_for((long long)a.nx * a.ny), AB, 0, s>>>(a);
}

}  // namespace rbpf
