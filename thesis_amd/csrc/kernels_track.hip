// kernels_track.hip -- the trajectory log: every particle's pose and parent per recorded step, the walk back through the parents,
// and the filter's pose estimate (include/rbpf_hip.h, rbpf_track_* and rbpf_estimate; the specification is DESIGN 3.15).
//
//   track_compose_kernel   behind every local resample: pending' [j] = pending[idx[j]] where the DEVICE flag `did` is set, pending[j]
//                          otherwise.  The host never reads the flag; it swaps the two buffers either way.
//   track_record_kernel    one workgroup: bit copies of px, py, pth into the record, parent = pending, pending = identity, and the
//                          estimate row of the moment (RBPF_W_RESAMPLE, n_alive -1).
//   estimate_kernel        one workgroup: the estimate row of the current state (rbpf_estimate).
//   The walk back (rbpf_track_lineage, rbpf_track_summary) is a chain of dependent gathers cur = parent[t][cur], one per record.
//   Maps compose associatively, so it is cut into chunks of RBPF_TRACK_CHUNK records (chunk c = records 64 c .. 64 c + 63):
//   walk_compose_kernel    per chunk c above the first and index j: comp[c][j], the index at the last record of chunk c - 1 of the
//                          ancestor of index j at the last record of chunk c.  A workgroup owns a slab of 256 indices of one chunk; a
//                          lane follows one chain, so the slab reads each parent row of the chunk once.  A row is 4 P bytes (16 KB on
//                          the bench scene) and stays in L2; the chain is bound by the latency of its 64 gathers, which the other
//                          waves of the CU hide: slabs of one index per lane give the most waves.
//   walk_start_kernel      one lane per walked particle: start[last] = pending[particle], start[c - 1] = comp[c][start[c]].
//   walk_output_kernel     per chunk and walked particle again: from start[c] down through the chunk, writes the index and, if asked,
//                          the gathered pose of every record in [t0, t1).  Stores are contiguous in the particle; the gathers coalesce
//                          better the further back they go, because lineages merge.
//   track_summary_kernel   one workgroup per record: the estimate row over the lineages' poses at that record with the FINAL weights,
//                          and n_alive = the distinct values of the lineage row, counted through a P-bit bitmap in LDS.
// The estimate row itself and its deterministic sums live in rbpf_estrow.h (kernels_modes.hip computes one row per pose mode).
#include "rbpf_estrow.h"

namespace rbpf {

static const int WALK_SLAB = 256;              // indices (= lanes) of a walk workgroup

__device__ __forceinline__ const double* rec_x(const TrackLog& g, int t) { return reinterpret_cast<const double*>(g.base + (size_t)t * g.stride); }
__device__ __forceinline__ const int32_t* rec_parent(const TrackLog& g, int t) { return reinterpret_cast<const int32_t*>(g.base + (size_t)t * g.stride + track_parent_offset(g.P)); }

__global__ __launch_bounds__(256) void track_compose_kernel(int P, const int32_t* __restrict__ did, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ pend, int32_t* __restrict__ pend2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    int i = j;
    if (*did) { const int s = idx[j]; if (s >= 0 && s < P) i = s; }
    pend2[j] = pend[i];
}

__global__ __launch_bounds__(TT) void track_record_kernel(TrackLog g, int t, const double* __restrict__ px, const double* __restrict__ py,
                                                          const double* __restrict__ pth, const double* __restrict__ weight, int32_t* pend) {
    __shared__ double s_red[TW * EST_SUMS * 2];
    __shared__ int s_arg[TW];
    unsigned char* rec = g.base + (size_t)t * g.stride;
    double* x = reinterpret_cast<double*>(rec);
    int32_t* parent = reinterpret_cast<int32_t*>(rec + track_parent_offset(g.P));
    const int P = g.P;
    for (int j = threadIdx.x; j < P; j += TT) {
        x[j] = px[j]; x[P + j] = py[j]; x[2 * (size_t)P + j] = pth[j];
        parent[j] = pend[j]; pend[j] = j;
    }
    estimate_row(P, [&](int j, double& a, double& b, double& c) { a = px[j]; b = py[j]; c = pth[j]; }, weight, nullptr, RBPF_W_RESAMPLE, EveryParticle(), -1,
                 x + 3 * (size_t)P, parent + P, s_red, s_arg);
}

__global__ __launch_bounds__(TT) void estimate_kernel(int P, const double* __restrict__ px, const double* __restrict__ py,
                                                      const double* __restrict__ pth, const double* __restrict__ weight,
                                                      const double* __restrict__ given, int mode, double* out16, int32_t* out4) {
    __shared__ double s_red[TW * EST_SUMS * 2];
    __shared__ int s_arg[TW];
    estimate_row(P, [&](int j, double& a, double& b, double& c) { a = px[j]; b = py[j]; c = pth[j]; }, weight, given, mode, EveryParticle(), -1, out16, out4,
                 s_red, s_arg);
}

// ---- the walk back -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WALK_SLAB) void walk_compose_kernel(TrackWalk q) {
    const int c = q.c0 + 1 + blockIdx.y, j = blockIdx.x * WALK_SLAB + threadIdx.x;
    if (j >= q.g.P) return;
    const int a = c * RBPF_TRACK_CHUNK, b = min(a + RBPF_TRACK_CHUNK, q.N);
    int cur = j;
    for (int t = b - 1; t >= a; --t) cur = rec_parent(q.g, t)[cur];
    q.comp[(size_t)(c - q.c0) * q.g.P + j] = cur;
}

__global__ __launch_bounds__(WALK_SLAB) void walk_start_kernel(TrackWalk q) {
    const int j = blockIdx.x * WALK_SLAB + threadIdx.x;
    if (j >= q.n) return;
    int cur = q.pending[q.particles ? q.particles[j] : j];
    for (int c = q.c1; ; --c) {
        q.start[(size_t)(c - q.c0) * q.n + j] = cur;
        if (c == q.c0) break;
        cur = q.comp[(size_t)(c - q.c0) * q.g.P + cur];
    }
}

__global__ __launch_bounds__(WALK_SLAB) void walk_output_kernel(TrackWalk q) {
    const int c = q.c0 + blockIdx.y, j = blockIdx.x * WALK_SLAB + threadIdx.x;
    if (j >= q.n) return;
    const int a = max(c * RBPF_TRACK_CHUNK, q.t0), b = min((c + 1) * RBPF_TRACK_CHUNK, q.N);
    const size_t P = (size_t)q.g.P;
    int cur = q.start[(size_t)(c - q.c0) * q.n + j];
    for (int t = b - 1; t >= a; --t) {
        if (t < q.t1) {
            const size_t o = (size_t)(t - q.t0) * q.n + j;
            if (q.out_idx) q.out_idx[o] = cur;
            if (q.out_pose) {
                const double* x = rec_x(q.g, t);
                q.out_pose[3 * o] = x[cur]; q.out_pose[3 * o + 1] = x[P + cur]; q.out_pose[3 * o + 2] = x[2 * P + cur];
            }
        }
        if (t > a) cur = rec_parent(q.g, t)[cur];
    }
}

__global__ __launch_bounds__(TT) void track_summary_kernel(TrackLog g, int t0, const int32_t* __restrict__ lineage, const double* __restrict__ weight,
                                                           const double* __restrict__ given, int mode, double* out_f, int32_t* out_i) {
    __shared__ double s_red[TW * EST_SUMS * 2];
    __shared__ int s_arg[TW];
    __shared__ uint32_t s_bits[TRACK_SUMMARY_MAX_P / 32];
    __shared__ int s_alive;
    const int P = g.P, t = t0 + blockIdx.x, words = (P + 31) / 32;
    const int32_t* lin = lineage + (size_t)blockIdx.x * P;
    for (int k = threadIdx.x; k < words; k += TT) s_bits[k] = 0;
    if (threadIdx.x == 0) s_alive = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < P; j += TT) { const int i = lin[j]; atomicOr(&s_bits[i >> 5], 1u << (i & 31)); }
    __syncthreads();
    int n = 0;
    for (int k = threadIdx.x; k < words; k += TT) n += __popc(s_bits[k]);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_alive, n);
    __syncthreads();
    const double* x = rec_x(g, t);
    estimate_row(P, [&](int j, double& a, double& b, double& c) { const int i = lin[j]; a = x[i]; b = x[(size_t)P + i]; c = x[2 * (size_t)P + i]; },
                 weight, given, mode, EveryParticle(), s_alive, out_f + (size_t)blockIdx.x * RBPF_EST_F64, out_i + (size_t)blockIdx.x * RBPF_EST_I32, s_red, s_arg);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
void launch_track_compose(int P, const int32_t* d_did, const int32_t* d_idx, const int32_t* d_pend, int32_t* d_pend2, hipStream_t s) {
    hipLaunchKernelGGL(track_compose_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, d_did, d_idx, d_pend, d_pend2);
}

void launch_track_record(const DevView& v, const TrackLog& g, int t, int32_t* d_pend, hipStream_t s) {
    hipLaunchKernelGGL(track_record_kernel, dim3(1), dim3(TT), 0, s, g, t, v.px, v.py, v.pth, v.weight, d_pend);
}

void launch_estimate(const DevView& v, const double* d_given, int mode, double* d_out16, int32_t* d_out4, hipStream_t s) {
    hipLaunchKernelGGL(estimate_kernel, dim3(1), dim3(TT), 0, s, v.P, v.px, v.py, v.pth, v.weight, d_given, mode, d_out16, d_out4);
}

void launch_track_walk(const TrackWalk& q, hipStream_t s) {
    const int slabs_p = (q.g.P + WALK_SLAB - 1) / WALK_SLAB, slabs_n = (q.n + WALK_SLAB - 1) / WALK_SLAB;
    if (q.c1 > q.c0) hipLaunchKernelGGL(walk_compose_kernel, dim3(slabs_p, q.c1 - q.c0), dim3(WALK_SLAB), 0, s, q);
    hipLaunchKernelGGL(walk_start_kernel, dim3(slabs_n), dim3(WALK_SLAB), 0, s, q);
    hipLaunchKernelGGL(walk_output_kernel, dim3(slabs_n, (q.t1 - 1) / RBPF_TRACK_CHUNK - q.c0 + 1), dim3(WALK_SLAB), 0, s, q);
}

void launch_track_summary(const TrackLog& g, int t0, int t1, const int32_t* d_lineage, const double* d_weight, const double* d_given,
                          int mode, double* d_out_f, int32_t* d_out_i, hipStream_t s) {
    hipLaunchKernelGGL(track_summary_kernel, dim3(t1 - t0), dim3(TT), 0, s, g, t0, d_lineage, d_weight, d_given, mode, d_out_f, d_out_i);
}

}  // namespace rbpf
