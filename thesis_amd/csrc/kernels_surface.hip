// kernels_surface.hip -- peaks and moments of score volumes (include/rbpf_hip.h, rbpf_score_surface; the specification is
// DESIGN 3.20).  The input is what rbpf_refine_poses and rbpf_match_pairs write: int32 [N][nk][nw][nw], nk = 2 R + 1 rotations and
// nw = 2 W + 1 translations a side, candidate (i, j, k) at [k + R][i + W][j + W].
//   surface_kernel   one workgroup per item, no word shared between workgroups and no global atomic.  At most K passes.  In pass
//                    p every lane strides over the flat volume with running (k, i, j) counters, forms the merge key of
//                    rbpf_refine_search.h for a candidate and, only where the key beats the lane's best so far, tests the
//                    candidate against the boxes of the p peaks found before (LDS): the free test runs for a handful of
//                    candidates a lane.  The keys are reduced with __shfl_xor inside a wave and through LDS across waves; a zero
//                    maximum (no key of a candidate is zero) says that nothing is free, and the item is done.  Then the lanes
//                    stride over the peak's box alone, clipped to the volume, with the same free test, and add the plateau's
//                    size and its ten weighted sums in int64; these are reduced the same way.  Integer sums do not depend on
//                    their order, so the record is the same whatever the tree.  Lane 0 writes the record with plain stores; the
//                    records behind the last peak are zeroed by all lanes.
// A score is compared, shifted into a key and subtracted, never used as an index: a value outside 0 .. 32768 gives meaningless
// numbers and no access outside the buffers.  Peak coordinates come out of the key's low 22 bits, which a score cannot reach.
#include "rbpf_refine_search.h"

namespace rbpf {

// a flat index t over [.][nb][nc] as running counters: set() by division once, step() adds the stride's own three digits
struct SurfaceWalk {
    int a, b, c, da, db, dc, nb, nc;
    __device__ __forceinline__ void set(int t, int stride, int nb_, int nc_) {
        nb = nb_; nc = nc_;
        const int r = nb * nc;
        a = t / r; b = (t - a * r) / nc; c = t - a * r - b * nc;
        da = stride / r; db = (stride - da * r) / nc; dc = stride - da * r - db * nc;
    }
    __device__ __forceinline__ void step() {
        c += dc; if (c >= nc) { c -= nc; ++b; }
        b += db; if (b >= nb) { b -= nb; ++a; }
        a += da;
    }
};

__device__ __forceinline__ unsigned long long surface_wave_max(unsigned long long v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ long long surface_wave_sum(long long v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(SURFACE_BLOCK) void surface_kernel(SurfaceArgs a) {
    const int NWAVE = SURFACE_BLOCK / 64;
    __shared__ int4 s_peak[SURFACE_MAX_PEAKS];                            // (i, j, k, score) of the peaks found
    __shared__ unsigned long long s_key[NWAVE];
    __shared__ long long s_sum[NWAVE][SURFACE_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
    const int R = a.R, W = a.W, nw = 2 * W + 1, vol = (2 * R + 1) * nw * nw;   // n_items * vol < 2^31: the host checked
    const int32_t* __restrict__ V = a.scores + (size_t)n * vol;
    const int drop = a.drop ? a.drop[n] : 0;
    long long* __restrict__ out = a.out + (size_t)n * a.K * 16;

    // free: in the box of none of the first p peaks
    auto is_free = [&](int i, int j, int k, int p) {
        for (int q = 0; q < p; ++q) {
            const int4 pk = s_peak[q];
            if (abs(i - pk.x) <= a.ex_t && abs(j - pk.y) <= a.ex_t && abs(k - pk.z) <= a.ex_r) return false;
        }
        return true;
    };

    int p = 0;
    for (; p < a.K; ++p) {
        unsigned long long best = 0ull;
        SurfaceWalk w;
        w.set(tid, SURFACE_BLOCK, nw, nw);
        for (int t = tid; t < vol; t += SURFACE_BLOCK, w.step()) {
            const int k = w.a - R, i = w.b - W, j = w.c - W;
            const unsigned long long key = refine_key(V[t], k, i, j, R, W);
            if (key > best && is_free(i, j, k, p)) best = key;
        }
        best = surface_wave_max(best);
        if (lane == 0) s_key[wave] = best;
        __syncthreads();
        best = s_key[0];
#pragma unroll
        for (int q = 1; q < NWAVE; ++q) best = s_key[q] > best ? s_key[q] : best;
        if (best == 0ull) break;                                          // uniform: nothing is free any more
        int pi, pj, pk;
        const int sp = refine_unkey(best, R, W, pi, pj, pk);
        if (tid == 0) s_peak[p] = make_int4(pi, pj, pk, sp);

        // the plateau: the free cells of the peak's own box within `drop` of its score
        const int k0 = max(-R, pk - a.ex_r), k1 = min(R, pk + a.ex_r), i0 = max(-W, pi - a.ex_t), i1 = min(W, pi + a.ex_t);
        const int j0 = max(-W, pj - a.ex_t), j1 = min(W, pj + a.ex_t);
        const int bi = i1 - i0 + 1, bj = j1 - j0 + 1, cells = (k1 - k0 + 1) * bi * bj;
        const int floor_s = sp - drop;
        long long sum[SURFACE_SUMS];
#pragma unroll
        for (int q = 0; q < SURFACE_SUMS; ++q) sum[q] = 0;
        w.set(tid, SURFACE_BLOCK, bi, bj);
        for (int t = tid; t < cells; t += SURFACE_BLOCK, w.step()) {
            const int k = k0 + w.a, i = i0 + w.b, j = j0 + w.c;
            const int v = V[((k + R) * nw + (i + W)) * nw + (j + W)];
            if (v < floor_s || !is_free(i, j, k, p)) continue;
            const long long wt = (long long)v - floor_s + 1, di = i - pi, dj = j - pj, dk = k - pk;
            sum[0] += 1; sum[1] += wt;
            sum[2] += wt * di; sum[3] += wt * dj; sum[4] += wt * dk;
            sum[5] += wt * di * di; sum[6] += wt * di * dj; sum[7] += wt * di * dk;
            sum[8] += wt * dj * dj; sum[9] += wt * dj * dk; sum[10] += wt * dk * dk;
        }
#pragma unroll
        for (int q = 0; q < SURFACE_SUMS; ++q) {
            const long long r = surface_wave_sum(sum[q]);
            if (lane == 0) s_sum[wave][q] = r;
        }
        __syncthreads();                                                  // s_sum and s_peak[p] are written; s_key has been read
        if (tid == 0) {
            long long* o = out + 16 * p;
            o[0] = pi; o[1] = pj; o[2] = pk; o[3] = sp;
            for (int q = 0; q < SURFACE_SUMS; ++q) {
                long long r = 0;
                for (int u = 0; u < NWAVE; ++u) r += s_sum[u][q];
                o[4 + q] = r;
            }
            o[15] = 0;
        }
        __syncthreads();                                                  // s_sum is free for the next pass
    }
    for (int t = 16 * p + tid; t < 16 * a.K; t += SURFACE_BLOCK) out[t] = 0;
    if (tid == 0 && a.count) a.count[n] = p;
}

void launch_score_surface(const SurfaceArgs& a, hipStream_t s) {
    surface_kernel<<<(unsigned)a.N, SURFACE_BLOCK, 0, s>>>(a);
}

}  // namespace rbpf
