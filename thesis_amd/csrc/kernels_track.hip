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
// Sums are deterministic: a lane adds its elements in index order, a wave reduces by a fixed butterfly (a + b == b + a, so every
// lane holds the same bits), and every lane adds the 8 wave sums in wave order.  The partial sums are double-double, rounded once.
// No floating-point atomics.
#include <math.h>

#include "rbpf_device.h"

namespace rbpf {

static const int TT = 512;                     // lanes of the one-workgroup kernels: 8 waves (256 VGPRs each: the float64 sincos, atan2 and
                                               // remainder beside 13 double-double sums spill at 1024 lanes)
static const int TW = TT / 64;
static const int WALK_SLAB = 256;              // indices (= lanes) of a walk workgroup
static const int EST_SUMS = 7;                 // the widest block sum

__device__ __forceinline__ const double* rec_x(const TrackLog& g, int t) { return reinterpret_cast<const double*>(g.base + (size_t)t * g.stride); }
__device__ __forceinline__ const int32_t* rec_parent(const TrackLog& g, int t) { return reinterpret_cast<const int32_t*>(g.base + (size_t)t * g.stride + track_parent_offset(g.P)); }

// every lane ends with the same N sums over the workgroup, carried in double-double (error-free additions, rbpf_math.h) and
// rounded to float64 once at the end: the order of the additions is fixed and barely matters.  s_red: [TW][N][2] doubles
template <int N>
__device__ __forceinline__ void block_sum(dd (&a)[N], double* s_red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int o = 32; o > 0; o >>= 1) a[k] = dd_add(a[k], dd{__shfl_xor(a[k].hi, o, 64), __shfl_xor(a[k].lo, o, 64)});
    __syncthreads();                           // the last use of s_red is over
    if (lane == 0)
        for (int k = 0; k < N; ++k) { s_red[(wave * N + k) * 2] = a[k].hi; s_red[(wave * N + k) * 2 + 1] = a[k].lo; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        dd s = {s_red[k * 2], s_red[k * 2 + 1]};
        for (int w = 1; w < TW; ++w) s = dd_add(s, dd{s_red[(w * N + k) * 2], s_red[(w * N + k) * 2 + 1]});
        a[k] = s;
    }
}

// np.argmax: the first largest value, a NaN counting as the largest.  i < 0: no candidate
__device__ __forceinline__ bool arg_better(double wa, int ia, double wb, int ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    const bool na = wa != wa, nb = wb != wb;
    if (na != nb) return na;
    if (!na && wa != wb) return wa > wb;
    return ia < ib;
}

static const double TWO_PI = 6.283185307179586, PI = 3.141592653589793;

// The estimate row: whole workgroup of TT lanes, contains barriers.  pose(j, x, y, th) gives particle j's pose;
// w_raw are the filter's weights (best and RBPF_W_RESAMPLE read them), w_given the caller's (RBPF_W_GIVEN).  Lane 0 writes
// out16 / out4.  s_red: [TW][EST_SUMS][2] doubles, s_arg: [TW] ints
template <class Pose>
__device__ void estimate_row(int P, Pose pose, const double* __restrict__ w_raw, const double* __restrict__ w_given, int mode,
                             int n_alive, double* out16, int32_t* out4, double* s_red, int* s_arg) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the smallest weight after -inf -> 0 (the shift of main.py:53-55), and the first argmax of the raw weights
    double mn = INFINITY, bw = 0.0; int bi = -1;
    for (int j = tid; j < P; j += TT) {
        const double w = w_raw[j];
        mn = fmin(mn, w == -INFINITY ? 0.0 : w);
        if (arg_better(w, j, bw, bi)) { bw = w; bi = j; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        const double ow = __shfl_xor(bw, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (arg_better(ow, oi, bw, bi)) { bw = ow; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) { s_red[wave] = mn; s_red[TW + wave] = bw; s_arg[wave] = bi; }
    __syncthreads();
    mn = s_red[0]; bw = s_red[TW]; bi = s_arg[0];
    for (int w = 1; w < TW; ++w) {
        mn = fmin(mn, s_red[w]);
        if (arg_better(s_red[TW + w], s_arg[w], bw, bi)) { bw = s_red[TW + w]; bi = s_arg[w]; }
    }
    const double shift = (mode == RBPF_W_RESAMPLE && mn < 0) ? fabs(mn) : 0.0;
    auto weight_of = [&](int j) -> double {
        if (mode == RBPF_W_UNIFORM) return 1.0;
        if (mode == RBPF_W_GIVEN) return w_given[j];
        double w = w_raw[j];
        if (w == -INFINITY) w = 0.0;
        if (shift != 0.0 && w != 0.0) w += shift;
        return w;
    };
    auto used = [&](double w, double x, double y, double th) { return isfinite(w) && w > 0.0 && isfinite(x) && isfinite(y) && isfinite(th); };

    dd acc[EST_SUMS] = {};                               // W, sum w x, w y, w sin, w cos, w^2, contributing particles
    for (int j = tid; j < P; j += TT) {
        double x, y, th;
        pose(j, x, y, th);
        const double w = weight_of(j);
        if (!used(w, x, y, th)) continue;
        double s, c;
        sincos(th, &s, &c);
        const double term[EST_SUMS] = {w, w * x, w * y, w * s, w * c, w * w, 1.0};
#pragma unroll
        for (int k = 0; k < EST_SUMS; ++k) acc[k] = dd_add_d(acc[k], term[k]);
    }
    block_sum<EST_SUMS>(acc, s_red);
    double a[EST_SUMS];
#pragma unroll
    for (int k = 0; k < EST_SUMS; ++k) a[k] = acc[k].hi;
    const double W = a[0];
    const bool any = W > 0.0;
    const double mx = a[1] / W, my = a[2] / W, mth = atan2(a[3], a[4]);
    dd cacc[6] = {};                                     // xx, xy, xth, yy, yth, thth
    if (any)
        for (int j = tid; j < P; j += TT) {
            double x, y, th;
            pose(j, x, y, th);
            const double w = weight_of(j);
            if (!used(w, x, y, th)) continue;
            const double dx = x - mx, dy = y - my;
            double dt = remainder(th - mth, TWO_PI);     // [-pi, pi]
            if (dt <= -PI) dt += TWO_PI;                 // (-pi, pi]
            const double term[6] = {w * (dx * dx), w * (dx * dy), w * (dx * dt), w * (dy * dy), w * (dy * dt), w * (dt * dt)};
#pragma unroll
            for (int k = 0; k < 6; ++k) cacc[k] = dd_add_d(cacc[k], term[k]);
        }
    block_sum<6>(cacc, s_red);
    double c6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cacc[k].hi;
    if (tid == 0) {
        const double nan = NAN;
        out16[0] = any ? mx : nan; out16[1] = any ? my : nan; out16[2] = any ? mth : nan;
        for (int k = 0; k < 6; ++k) out16[3 + k] = any ? c6[k] / W : nan;
        out16[9] = any ? hypot(a[3], a[4]) / W : nan;
        out16[10] = any ? W : nan;
        out16[11] = any ? (W * W) / a[5] : nan;
        out16[12] = out16[13] = out16[14] = out16[15] = 0.0;
        out4[0] = bi; out4[1] = (int32_t)a[6]; out4[2] = n_alive; out4[3] = 0;
    }
}

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
    estimate_row(P, [&](int j, double& a, double& b, double& c) { a = px[j]; b = py[j]; c = pth[j]; }, weight, nullptr, RBPF_W_RESAMPLE, -1,
                 x + 3 * (size_t)P, parent + P, s_red, s_arg);
}

__global__ __launch_bounds__(TT) void estimate_kernel(int P, const double* __restrict__ px, const double* __restrict__ py,
                                                      const double* __restrict__ pth, const double* __restrict__ weight,
                                                      const double* __restrict__ given, int mode, double* out16, int32_t* out4) {
    __shared__ double s_red[TW * EST_SUMS * 2];
    __shared__ int s_arg[TW];
    estimate_row(P, [&](int j, double& a, double& b, double& c) { a = px[j]; b = py[j]; c = pth[j]; }, weight, given, mode, -1, out16, out4,
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
                 weight, given, mode, s_alive, out_f + (size_t)blockIdx.x * RBPF_EST_F64, out_i + (size_t)blockIdx.x * RBPF_EST_I32, s_red, s_arg);
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
