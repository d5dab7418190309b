// rbpf_estrow.h -- the estimate row of a one-workgroup kernel: shared by kernels_track.hip (rbpf_estimate, the
// records, the smoothed trajectory) and kernels_modes.hip (one row per pose mode).
// Sums are deterministic: a lane adds its elements in index order, a wave reduces by a fixed butterfly (a + b == b + a, so every
// lane holds the same bits), and every lane adds the 8 wave sums in wave order.  The partial sums are double-double, rounded once.
// No floating-point atomics.
#pragma once
#include <math.h>

#include "rbpf_device.h"

namespace rbpf {

static const int TT = 512;                     // lanes of the one-workgroup kernels: 8 waves (256 VGPRs each: the float64 sincos, atan2 and
                                               // remainder beside 13 double-double sums spill at 1024 lanes)
static const int TW = TT / 64;
static const int EST_SUMS = 7;                 // the widest block sum

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

struct EveryParticle { __device__ __forceinline__ bool operator()(int) const { return true; } };

// The effective weight of a particle under weights_mode: 1, the caller's, or the resample distribution of the raw weights
// (-inf -> 0, then `shift`, the magnitude of a negative minimum over ALL P, onto every non-zero value: main.py:53-55)
struct EffWeight {
    const double* w_raw; const double* w_given; int mode; double shift;
    __device__ __forceinline__ double operator()(int j) const {
        if (mode == RBPF_W_UNIFORM) return 1.0;
        if (mode == RBPF_W_GIVEN) return w_given[j];
        double w = w_raw[j];
        if (w == -INFINITY) w = 0.0;
        if (shift != 0.0 && w != 0.0) w += shift;
        return w;
    }
};
__device__ __forceinline__ bool est_used(double w, double x, double y, double th) {
    return isfinite(w) && w > 0.0 && isfinite(x) && isfinite(y) && isfinite(th);
}

// Whole workgroup, contains barriers: the effective weights of a set (the smallest raw weight after -inf -> 0 is taken over all
// P) and `best`, the first argmax of the raw weights among the particles member(j) admits (-1: none).  s_red: [2 TW] doubles,
// s_arg: [TW] ints
template <class Member>
__device__ __forceinline__ EffWeight weights_scan(int P, const double* __restrict__ w_raw, const double* __restrict__ w_given, int mode,
                                                  Member member, int& best, double* s_red, int* s_arg) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double mn = INFINITY, bw = 0.0; int bi = -1;
    for (int j = tid; j < P; j += TT) {
        const double w = w_raw[j];
        mn = fmin(mn, w == -INFINITY ? 0.0 : w);
        if (member(j) && arg_better(w, j, bw, bi)) { bw = w; bi = j; }
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
    best = bi;
    return EffWeight{w_raw, w_given, mode, (mode == RBPF_W_RESAMPLE && mn < 0) ? fabs(mn) : 0.0};
}

// The estimate row: whole workgroup of TT lanes, contains barriers.  pose(j, x, y, th) gives particle j's pose;
// w_raw are the filter's weights (best and RBPF_W_RESAMPLE read them), w_given the caller's (RBPF_W_GIVEN).  Only the particles
// member(j) admits take part: to the sums everyone else is a particle of weight 0, and `best` is taken among the admitted.
// Lane 0 writes out16 / out4.  s_red: [TW][EST_SUMS][2] doubles, s_arg: [TW] ints
template <class Pose, class Member>
__device__ void estimate_row(int P, Pose pose, const double* __restrict__ w_raw, const double* __restrict__ w_given, int mode,
                             Member member, int n_alive, double* out16, int32_t* out4, double* s_red, int* s_arg) {
    const int tid = threadIdx.x;
    int bi;
    const EffWeight weight_of = weights_scan(P, w_raw, w_given, mode, member, bi, s_red, s_arg);

    dd acc[EST_SUMS] = {};                               // W, sum w x, w y, w sin, w cos, w^2, contributing particles
    for (int j = tid; j < P; j += TT) {
        if (!member(j)) continue;
        double x, y, th;
        pose(j, x, y, th);
        const double w = weight_of(j);
        if (!est_used(w, x, y, th)) continue;
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
            if (!member(j)) continue;
            double x, y, th;
            pose(j, x, y, th);
            const double w = weight_of(j);
            if (!est_used(w, x, y, th)) continue;
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

}  // namespace rbpf
