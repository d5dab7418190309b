// rbpf_refine_search.h -- the candidate search shared by refine_search_kernel (kernels_refine.hip) and
// pairs_search_kernel (kernels_pairs.hip): one workgroup per (item, run of kpw rotations) scores every
// translation of its rotations against a window of {occ, dil} word pairs staged in LDS.  The two kernels differ in where the
// window comes from and in which scan an item reads, nothing else: OWN = false stages the window from one field shared by all
// items (the union of their windows, a.field), item n reading scan n; OWN = true copies item n's own field, rows of a.WW word
// pairs whose bit 0 is cell Y0 - Mw, and reads scan query[n].  kernels_refine.hip describes the body.
#pragma once
#include "rbpf_internal.h"

namespace rbpf {

static const int32_t REFINE_UNUSED = INT32_MIN;  // PX of a beam that is not used

// the tie order as the low 41 bits of the merge key, complemented: the largest key is the smallest (|k|, i^2 + j^2, k, i, j)
__device__ __forceinline__ unsigned long long refine_key(int score, int k, int i, int j, int R, int W) {
    const unsigned long long ak = (unsigned long long)(127 - (k < 0 ? -k : k));          // |k| <= 100
    const unsigned long long d2 = (unsigned long long)(4095 - (i * i + j * j));          // <= 2048
    const unsigned long long kk = (unsigned long long)(255 - (k + R));                   // <= 200
    const unsigned long long ii = (unsigned long long)(127 - (i + W)), jj = (unsigned long long)(127 - (j + W));   // <= 64
    return ((unsigned long long)score << 41) | (ak << 34) | (d2 << 22) | (kk << 14) | (ii << 7) | jj;
}

// `a` comes by value: through a reference the compiler reloads the arguments after the stores (71 instructions more in
// refine_search_kernel); by value the kernel is what it was before the body moved here
template <bool OWN>
__device__ __forceinline__ void refine_search_body(const RefineArgs a, const int32_t* __restrict__ query, const uint2* __restrict__ own) {
    const int RB = REFINE_BLOCK, RJ = REFINE_RUN;
    extern __shared__ __align__(16) unsigned char smem[];
    int2* tab = reinterpret_cast<int2*>(smem);                            // [kc][bc] (PX, PY) of the chunk's beams
    uint2* win = reinterpret_cast<uint2*>(smem + REFINE_TABLE * 8);       // [rows][WW] {occ, dil}
    __shared__ unsigned long long s_best;
    __shared__ int s_used;
    const int tid = threadIdx.x, n = blockIdx.x;
    const int W = a.Wt, R = a.R, s = a.s, nw = 2 * W + 1, njr = refine_runs(nw, s), t1 = nw * njr;
    const int q0 = blockIdx.y * a.kpw, kc = min(a.kpw, a.nk - q0);        // rotations q0 .. q0 + kc - 1, k = q - R
    const int Mw = a.Mw, WW = a.WW, rows = 2 * Mw + 1;
    const int2 c0 = reinterpret_cast<const int2*>(a.cell0)[n];            // floor(g * inv): the window's centre
    const int wx0 = c0.x - Mw;                                            // cell of window row 0
    const int wj0 = OWN ? 0 : (c0.y - Mw - a.fy0) >> 5;                   // field word of window word 0 (floor division)
    const int wy0 = OWN ? c0.y - Mw : a.fy0 + 32 * wj0;                   // cell of bit 0 of a window row: <= Y0 - Mw

    if (tid == 0) { s_best = 0ull; s_used = 0; }
    if (OWN) {
        const uint2* __restrict__ src = own + (size_t)n * rows * WW;
        for (int t = tid; t < rows * WW; t += RB) win[t] = src[t];
    } else {
        for (int t = tid; t < rows * WW; t += RB) {
            const int r = t / WW, w = t - r * WW;
            const int fr = wx0 + r - a.fx0, fw = wj0 + w;
            win[t] = (fr >= 0 && fr < a.frows && fw >= 0 && fw < a.fW) ? a.field[(size_t)fr * a.fW + fw] : make_uint2(0u, 0u);
        }
    }

    const double2 g = reinterpret_cast<const double2*>(a.guess)[n];
    const double* __restrict__ rng = a.ranges + (size_t)(OWN ? query[n] : n) * a.B;
    const double* __restrict__ rot = a.rot + ((size_t)n * a.nk + q0) * 4;
    const int bc = min(a.B, REFINE_TABLE / kc), nchunk = (a.B + bc - 1) / bc;
    const int ntask = kc * t1;
    for (int task0 = 0; task0 < ntask; task0 += RB) {
        const int task = task0 + tid;
        const bool live = task < ntask;
        const int kk = live ? task / t1 : 0, rem = task - kk * t1, ii = live ? rem / njr : 0, jr = rem - ii * njr;
        const int i = ii - W, j0 = (jr & ((1 << s) - 1)) + (((jr >> s) * RJ) << s) - W;     // the run: j0 + S t, t = 0 .. 7
        int acc[RJ];
#pragma unroll
        for (int t = 0; t < RJ; ++t) acc[t] = 0;
        for (int ch = 0; ch < nchunk; ++ch) {
            const int b0 = ch * bc, nb = min(bc, a.B - b0);
            if (task0 == 0 || nchunk > 1) {                               // a single chunk stays in the table for every pass
                __syncthreads();                                          // the last chunk's readers are done
                int used = 0;
                for (int e = tid; e < kc * nb; e += RB) {
                    const int ek = e / nb, eb = e - ek * nb;
                    const double r = rng[b0 + eb];
                    int2 p = make_int2(REFINE_UNUSED, 0);
                    if (a.min_range < r && r < a.max_range) {             // NaN, +-inf, 0 and negative ranges fail one of the two
                        const double2 cs = reinterpret_cast<const double2*>(rot + 4 * ek)[0];
                        const double2 bm = reinterpret_cast<const double2*>(a.beam2)[b0 + eb];
                        const double bx = __dmul_rn(r, bm.x), by = __dmul_rn(r, bm.y);
                        const double x = __dadd_rn(g.x, __dsub_rn(__dmul_rn(cs.x, bx), __dmul_rn(cs.y, by)));
                        const double y = __dadd_rn(g.y, __dadd_rn(__dmul_rn(cs.y, bx), __dmul_rn(cs.x, by)));
                        p = make_int2((int)__builtin_floor(__dmul_rn(x, a.invS)), (int)__builtin_floor(__dmul_rn(y, a.invS)));   // |.| < 2^30: the host checked
                        used += ek == 0;
                    }
                    tab[ek * bc + eb] = p;
                }
                if (blockIdx.y == 0 && task0 == 0 && used) atomicAdd(&s_used, used);
                __syncthreads();
            }
            if (!live) continue;
            const int2* __restrict__ tb = tab + kk * bc;
            for (int b = 0; b < nb; ++b) {
                const int2 p = tb[b];
                if (p.x == REFINE_UNUSED) continue;
                const int row = ((p.x + i) >> s) - wx0, py = p.y + j0;
                const int cf = (py >> s) - wy0;                            // window bit of the run's first column
                // 0 <= row < rows and 0 <= cf, cf + 7 < 32 (WW - 1) for every used beam (the window bound); the test
                // only keeps a read inside the window whatever comes
                if ((unsigned)row >= (unsigned)rows || (unsigned)cf >= (unsigned)(32 * (WW - 1))) continue;
                const uint2* q = win + row * WW + (cf >> 5);
                const uint2 lo = q[0], hi = q[1];
                const uint32_t oc = __builtin_amdgcn_alignbit(hi.x, lo.x, (uint32_t)(cf & 31));
                const uint32_t di = __builtin_amdgcn_alignbit(hi.y, lo.y, (uint32_t)(cf & 31));
#pragma unroll
                for (int t = 0; t < RJ; ++t) acc[t] += (int)((oc >> t) & 1u) + (int)((di >> t) & 1u);   // (py + S t) >> s is column cf + t
            }
        }
        if (live) {
            const int k = q0 + kk - R;
            unsigned long long best = 0ull;
#pragma unroll
            for (int t = 0; t < RJ; ++t)
                if (j0 + (t << s) <= W) {
                    const int j = j0 + (t << s);
                    const unsigned long long key = refine_key(acc[t], k, i, j, R, W);
                    best = key > best ? key : best;
                    if (a.scores) a.scores[(((size_t)n * a.nk + (q0 + kk)) * nw + ii) * nw + (j + W)] = acc[t];
                    if (k == 0 && i == 0 && j == 0) a.guess_score[n] = acc[t];
                }
            atomicMax(&s_best, best);
        }
    }
    __syncthreads();
    if (tid == 0) {
        atomicMax(a.packed + n, s_best);
        if (blockIdx.y == 0) a.n_used[n] = s_used;
    }
}

// the best candidate of a merge word: (i, j, k) and its score
__device__ __forceinline__ int refine_unkey(unsigned long long p, int R, int W, int& i, int& j, int& k) {
    k = 255 - (int)((p >> 14) & 255u) - R; i = 127 - (int)((p >> 7) & 127u) - W; j = 127 - (int)(p & 127u) - W;
    return (int)(p >> 41);
}

}  // namespace rbpf
