// kernels_pairs.hip -- batched scan-to-submap matching: M pairs of a query scan and a run of reference scans at their current
// poses, every candidate (i, j, k) of a window of translations and rotations round each pair's guess scored against the field the
// run's own end points draw (include/rbpf_hip.h, rbpf_match_pairs; the specification is DESIGN 3.18).  No particle's map is read.
//   pairs_field_kernel     one workgroup per pair.  It transforms the used beams of the run's scans (float64, explicit single
//                          operations, cos and sin from the host) and sets the bit of each end cell in an LDS bitmap over the
//                          pair's window grown by one cell on every side: 2 Mw + 3 rows of WW + 1 words, bit c of a row the cell
//                          Y0 - Mw - 1 + c.  Points outside the grown window are dropped: no candidate reads them (DESIGN 3.17,
//                          the window bound), and the ring is what the dilation of the window's border cells reads.  Then every
//                          lane forms words of the window: occ is the bitmap shifted by the ring, dil the OR of the three rows
//                          and three shifts round it, written as the rows of {occ, dil} word pairs that the search stages.
//   pairs_search_kernel    rbpf_refine_search.h's body, one workgroup per (pair, run of kpw rotations): it copies the pair's own
//                          field into LDS and reads the query's scan.
//   pairs_final_kernel     packed -> out_m8 and out_pose_m3.
// All stores are vector stores; the only atomics are integer.
#include "rbpf_refine_search.h"

namespace rbpf {

__global__ __launch_bounds__(PAIRS_BLOCK) void pairs_field_kernel(PairsArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t* occ = reinterpret_cast<uint32_t*>(smem);                    // [2 Mw + 3][WW + 1]
    __shared__ int s_ref;
    const int tid = threadIdx.x, m = blockIdx.x;
    const int Mw = a.Mw, WW = a.WW, OW = WW + 1, grows = 2 * Mw + 3, rows = 2 * Mw + 1;
    const int2 c0 = reinterpret_cast<const int2*>(a.cell0)[m];
    const int gx0 = c0.x - Mw - 1, gy0 = c0.y - Mw - 1;                   // cell of row 0 and of bit 0 of the grown window
    const int2 run = reinterpret_cast<const int2*>(a.runs)[m];
    if (tid == 0) s_ref = 0;
    for (int t = tid; t < grows * OW; t += PAIRS_BLOCK) occ[t] = 0u;
    __syncthreads();

    int used = 0;
    const int total = (run.y - run.x) * a.B;                              // < 2^31: the host checked n_scans * n_beams
    for (int e = tid; e < total; e += PAIRS_BLOCK) {
        const int sn = run.x + e / a.B, b = e - (e / a.B) * a.B;
        const double r = a.ranges[(size_t)sn * a.B + b];
        if (!(a.min_range < r && r < a.max_range)) continue;              // NaN, +-inf, 0 and negative ranges fail one of the two
        const double2 p = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)sn], cs = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)sn + 1];
        const double2 bm = reinterpret_cast<const double2*>(a.beam2)[b];
        const double bx = __dmul_rn(r, bm.x), by = __dmul_rn(r, bm.y);
        const double x = __dadd_rn(p.x, __dsub_rn(__dmul_rn(cs.x, bx), __dmul_rn(cs.y, by)));
        const double y = __dadd_rn(p.y, __dadd_rn(__dmul_rn(cs.y, bx), __dmul_rn(cs.x, by)));
        const int row = (int)__builtin_floor(__dmul_rn(x, a.inv)) - gx0;  // |floor| < 2^30: the host checked
        const int col = (int)__builtin_floor(__dmul_rn(y, a.inv)) - gy0;
        ++used;
        if ((unsigned)row < (unsigned)grows && (unsigned)col < (unsigned)grows) atomicOr(occ + row * OW + (col >> 5), 1u << (col & 31));
    }
    if (used) atomicAdd(&s_ref, used);
    __syncthreads();

    uint2* __restrict__ out = a.fields + (size_t)m * rows * WW;
    for (int t = tid; t < rows * WW; t += PAIRS_BLOCK) {
        const int r = t / WW, w = t - r * WW;                             // window row r is grown row r + 1, window bit c grown bit c + 1
        const uint32_t* q = occ + r * OW + w;
        const unsigned long long up = q[0] | ((unsigned long long)q[1] << 32);
        const unsigned long long at = q[OW] | ((unsigned long long)q[OW + 1] << 32);
        const unsigned long long dn = q[2 * OW] | ((unsigned long long)q[2 * OW + 1] << 32);
        const unsigned long long any = up | at | dn;
        out[t] = make_uint2((uint32_t)(at >> 1), (uint32_t)(any | (any >> 1) | (any >> 2)));
    }
    if (tid == 0) a.n_ref[m] = s_ref;
}

__global__ __launch_bounds__(REFINE_BLOCK) void pairs_search_kernel(RefineArgs a, const int32_t* query, const uint2* fields) {
    refine_search_body<true>(a, query, fields);
}

__global__ __launch_bounds__(256) void pairs_final_kernel(RefineArgs a, PairsArgs p) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= a.N) return;
    int i, j, k;
    const int score = refine_unkey(a.packed[m], a.R, a.Wt, i, j, k);
    if (p.out_m8) {
        int32_t* o = p.out_m8 + 8 * (size_t)m;
        o[0] = i; o[1] = j; o[2] = k; o[3] = score; o[4] = a.guess_score[m]; o[5] = a.n_used[m]; o[6] = p.n_ref[m]; o[7] = 0;
    }
    if (p.out_pose) {
        const double2 g = reinterpret_cast<const double2*>(a.guess)[m];
        double* o = p.out_pose + 3 * (size_t)m;
        o[0] = __dadd_rn(g.x, __ddiv_rn((double)i, a.invS));
        o[1] = __dadd_rn(g.y, __ddiv_rn((double)j, a.invS));
        o[2] = a.rot[((size_t)m * a.nk + (k + a.R)) * 4 + 2];             // theta_k, formed on the host
    }
}

size_t pairs_field_lds_bytes(int Mw, int WW) { return (size_t)(2 * Mw + 3) * (WW + 1) * 4; }

void launch_match_pairs(const PairsArgs& p, const RefineArgs& a, hipStream_t s) {
    const size_t flds = pairs_field_lds_bytes(p.Mw, p.WW), lds = refine_lds_bytes(a.Mw, a.WW);
    static size_t field_set[MAX_DEVICES] = {}, search_set[MAX_DEVICES] = {};   // more than the default 64 KiB of dynamic LDS
    ensure_dynamic_lds(reinterpret_cast<const void*>(pairs_field_kernel), flds, field_set);
    ensure_dynamic_lds(reinterpret_cast<const void*>(pairs_search_kernel), lds, search_set);
    pairs_field_kernel<<<(unsigned)p.M, PAIRS_BLOCK, flds, s>>>(p);
    pairs_search_kernel<<<dim3((unsigned)a.N, (unsigned)((a.nk + a.kpw - 1) / a.kpw)), REFINE_BLOCK, lds, s>>>(a, p.query, p.fields);
    pairs_final_kernel<<<(unsigned)((a.N + 255) / 256), 256, 0, s>>>(a, p);
}

}  // namespace rbpf
