// kernels_places.hip -- scans compared by appearance: a scan becomes a polar occupancy image of R rings of 64 sectors, one 64-bit
// word a ring, and every query image is scored against every reference image at all 64 turns (include/rbpf_hip.h,
// rbpf_describe_scans and rbpf_match_places; the specification is DESIGN 3.19).  No particle's map is read.
//   places_describe_kernel one workgroup per scan.  The used beams set bit sector[b] (host) of word ring(r) of an LDS image;
//                          wave 0 writes the words, n_used and the popcount.
//   places_field_kernel    one lane per reference: D' = D dilated 3 x 3 (sectors circular, rings clipped) and w = |D| + |D'|.
//   places_search_kernel   one workgroup per (four queries, chunk of references), one wave per query, lane = turn s.  A lane keeps
//                          its query turned back by s in registers (popcount(Q & rotl(D, s)) = popcount(rotr(Q, s) & D)), so a
//                          reference costs it 2 R ANDs and popcounts on words every lane reads at one LDS address.  The chunk's
//                          references pass through LDS in tiles of 32.  One ballot asks whether any turn could enter the wave's
//                          list; only then the wave reduces over its lanes (score, then the tie rank of the turn) and inserts.
//                          The list of the k best lives in the registers of lanes 0 .. k - 1, best first.
//   places_merge_kernel    one wave per query: the chunks' lists into one, n_bits of the query, the outputs.
// The rank is a strict total order, so neither the chunk length nor the order of insertion shows in the result.
// All stores are vector stores; the only atomics are integer, in LDS.
#include "rbpf_internal.h"

namespace rbpf {

static const int PLACES_BLOCK = 256;   // four waves: four queries of a search workgroup
static const int PLACES_TILE = 32;     // references staged at a time: 2 * 32 * 32 words, 16 KiB at 32 rings

__global__ __launch_bounds__(PLACES_BLOCK) void places_describe_kernel(const double* __restrict__ ranges, const int32_t* __restrict__ sector,
                                                                       int B, int R, double min_range, double max_range, double rings_per_m,
                                                                       unsigned long long* __restrict__ desc, int32_t* __restrict__ info) {
    __shared__ unsigned long long words[RBPF_PLACES_MAX_RINGS];
    __shared__ int s_used;
    const int tid = threadIdx.x, n = blockIdx.x;
    if (tid < RBPF_PLACES_MAX_RINGS) words[tid] = 0ull;
    if (tid == 0) s_used = 0;
    __syncthreads();
    int used = 0;
    const double* __restrict__ row = ranges + (size_t)n * B;
    for (int b = tid; b < B; b += PLACES_BLOCK) {
        const double r = row[b];
        if (!(min_range < r && r < max_range)) continue;                  // NaN, +-inf, 0 and negative ranges fail one of the two
        const int ring = min((int)__builtin_floor(__dmul_rn(r, rings_per_m)), R - 1);
        atomicOr(words + ring, 1ull << sector[b]);
        ++used;
    }
    if (used) atomicAdd(&s_used, used);
    __syncthreads();
    if (tid >= 64) return;
    const unsigned long long w = tid < R ? words[tid] : 0ull;
    int bits = __popcll(w);
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o);
    if (desc && tid < R) desc[(size_t)n * R + tid] = w;
    if (info && tid == 0) { info[2 * (size_t)n] = s_used; info[2 * (size_t)n + 1] = bits; }
}

__global__ __launch_bounds__(256) void places_field_kernel(PlacesArgs a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nr) return;
    const int R = a.R;
    const unsigned long long* __restrict__ d = a.rd + (size_t)r * R;
    unsigned long long below = 0ull, at = d[0];
    int w = 0;
    for (int g = 0; g < R; ++g) {
        const unsigned long long above = g + 1 < R ? d[g + 1] : 0ull;
        const unsigned long long any = below | at | above;
        const unsigned long long dl = any | (any << 1 | any >> 63) | (any >> 1 | any << 63);
        a.dil[(size_t)r * R + g] = dl;
        w += __popcll(at) + __popcll(dl);
        below = at; at = above;
    }
    a.w[r] = w;
}

// a is better than b: v_a^2 w_b > v_b^2 w_a, ties to the smaller r.  v <= 4096 and w <= 4096: both sides stay below 2^37
__device__ __forceinline__ bool places_better(int va, int wa, int ra, int vb, int wb, int rb) {
    const unsigned long long l = (unsigned long long)(va * va) * (unsigned)wb, r = (unsigned long long)(vb * vb) * (unsigned)wa;
    return l > r || (l == r && ra < rb);
}

// The wave's list: lane j < cnt holds the j-th best {r, s, v, w}.  Every lane calls this with the same new entry.
__device__ __forceinline__ void places_insert(int lane, int k, int4& e, int& cnt, int4 n) {
    const bool keep = lane < cnt && !places_better(n.z, n.w, n.x, e.z, e.w, e.x);
    const int pos = __popcll(__ballot(keep));                             // the list is sorted: the kept ones are a prefix
    if (pos >= k) return;
    const int4 up = make_int4(__shfl_up(e.x, 1), __shfl_up(e.y, 1), __shfl_up(e.z, 1), __shfl_up(e.w, 1));
    if (lane == pos) e = n; else if (lane > pos) e = up;
    cnt = min(cnt + 1, k);
}

__global__ __launch_bounds__(PLACES_BLOCK) void places_search_kernel(PlacesArgs a) {
    __shared__ unsigned long long s_d[PLACES_TILE * RBPF_PLACES_MAX_RINGS], s_p[PLACES_TILE * RBPF_PLACES_MAX_RINGS];
    __shared__ int s_w[PLACES_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = (int)(blockIdx.x % (unsigned)a.nch), q0 = (int)(blockIdx.x / (unsigned)a.nch) * 4, q = q0 + wave;
    const int R = a.R, k = a.k;
    int reach = 0;                                                        // the references any of the four queries admits
    for (int j = 0; j < 4; ++j)
        if (q0 + j < a.nq) reach = max(reach, a.limit[q0 + j]);
    const int mine = q < a.nq ? a.limit[q] : 0;
    const long long first = (long long)c * a.chunk;
    const int begin = (int)min(first, (long long)a.nr), end = (int)min(min(first + a.chunk, (long long)a.nr), (long long)reach);

    unsigned long long qr[RBPF_PLACES_MAX_RINGS];                         // the query turned back by this lane's s
#pragma unroll
    for (int g = 0; g < RBPF_PLACES_MAX_RINGS; ++g) {
        const unsigned long long x = (q < a.nq && g < R) ? a.qd[(size_t)q * R + g] : 0ull;
        qr[g] = (x >> lane) | (x << ((64 - lane) & 63));
    }
    const int turn = min(lane, 64 - lane) * 2 + (lane > 32 ? 1 : 0);       // the tie order of the turns: 0 is first
    int4 e = make_int4(-1, 0, 0, 0);
    int cnt = 0, kv = 0, kw = 1;                                          // kv, kw: the k-th entry once the list is full

    for (int t0 = begin; t0 < end; t0 += PLACES_TILE) {
        const int nt = min(PLACES_TILE, end - t0);
        __syncthreads();
        for (int t = tid; t < nt * R; t += PLACES_BLOCK) { s_d[t] = a.rd[(size_t)t0 * R + t]; s_p[t] = a.dil[(size_t)t0 * R + t]; }
        if (tid < nt) s_w[tid] = a.w[t0 + tid];
        __syncthreads();
        const int n_mine = min(nt, mine - t0);
        for (int i = 0; i < n_mine; ++i) {
            const int w = s_w[i];
            if (w == 0) continue;
            const unsigned long long* d = s_d + i * R;
            const unsigned long long* p = s_p + i * R;
            int v = 0;
#pragma unroll
            for (int g = 0; g < RBPF_PLACES_MAX_RINGS; ++g)
                if (g < R) v += __popcll(qr[g] & d[g]) + __popcll(qr[g] & p[g]);
            // a full list holds smaller r only: a tie with its last entry loses
            const bool could = cnt == k ? (unsigned long long)(v * v) * (unsigned)kw > (unsigned long long)(kv * kv) * (unsigned)w : v > 0;
            if (__ballot(could) == 0ull) continue;
            int key = (v << 7) | (127 - turn);
            for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o));
            const int best = 127 - (key & 127), s = (best & 1) ? 64 - (best >> 1) : best >> 1;
            places_insert(lane, k, e, cnt, make_int4(t0 + i, s, key >> 7, w));
            if (cnt == k) { kv = __shfl(e.z, k - 1); kw = __shfl(e.w, k - 1); }
        }
    }
    if (q < a.nq && lane < k)
        a.partial[((size_t)q * a.nch + c) * k + lane] = lane < cnt ? e : make_int4(-1, 0, 0, 0);
}

__global__ __launch_bounds__(PLACES_BLOCK) void places_merge_kernel(PlacesArgs a) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    const int k = a.k;
    const int n_chunks = (int)min((long long)a.nch, ((long long)a.limit[q] + a.chunk - 1) / a.chunk);
    int4 e = make_int4(-1, 0, 0, 0);
    int cnt = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const int4* __restrict__ part = a.partial + ((size_t)q * a.nch + c) * k;
        for (int j = 0; j < k; ++j) {
            const int4 n = part[j];                                       // one address for the wave
            if (n.x < 0) break;
            places_insert(lane, k, e, cnt, n);
        }
    }
    int bits = lane < a.R ? __popcll(a.qd[(size_t)q * a.R + lane]) : 0;
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o);
    if (a.out_qk4 && lane < k) {                                          // a caller's device pointer need not be 16-byte aligned
        int32_t* o = a.out_qk4 + 4 * ((size_t)q * k + lane);
        if (lane >= cnt) e = make_int4(-1, 0, 0, 0);
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    if (a.out_q2 && lane == 0) { a.out_q2[2 * (size_t)q] = bits; a.out_q2[2 * (size_t)q + 1] = cnt; }
}

void launch_describe_scans(const double* d_ranges, const int32_t* d_sector, int n_scans, int n_beams, int n_rings, double min_range,
                           double max_range, double rings_per_m, unsigned long long* d_desc, int32_t* d_info, hipStream_t s) {
    places_describe_kernel<<<(unsigned)n_scans, PLACES_BLOCK, 0, s>>>(d_ranges, d_sector, n_beams, n_rings, min_range, max_range, rings_per_m,
                                                                      d_desc, d_info);
}

void launch_match_places(const PlacesArgs& a, hipStream_t s) {
    places_field_kernel<<<(unsigned)((a.nr + 255) / 256), 256, 0, s>>>(a);
    places_search_kernel<<<(unsigned)((long long)((a.nq + 3) / 4) * a.nch), PLACES_BLOCK, 0, s>>>(a);
    places_merge_kernel<<<(unsigned)((a.nq + 3) / 4), PLACES_BLOCK, 0, s>>>(a);
}

}  // namespace rbpf
