// kernels_scancheck.hip -- measured scans checked against the particles' maps: a class and an integer cost per beam, reduced per
// pose and per beam (include/rbpf_hip.h, rbpf_check_scans; the specification is DESIGN 3.23).
//
// One lane per ray, ray r = pose * B + beam, 256-lane workgroups over the flat ray index, as cast_scans_kernel and for its
// reasons.  A lane reads its measured range, decides whether and how far to walk - to the measured end plus the
// tolerance, not to max_range - runs walk_ray_to (rbpf_raywalk.h) and, only where the walk met nothing, loads the one int8
// cell its measured end lies in.
//   reduction   lanes of a wave hold consecutive rays, so the lanes of one pose form a run.  A segmented shuffle reduction
//               (a lane adds its neighbour at distance 1, 2, 4, .. 32 while that neighbour belongs to the same pose) leaves
//               the run's sums in its first lane: the cost as an int32 (64 beams of at most 2^21) and the eight class counts
//               as the bytes of one 64-bit word (a run has at most 64 beams).  The first lane of a run adds them to the
//               pose's outputs with integer atomics; the outputs are zeroed on the stream before the launch.  Correct for
//               any B >= 1: with B >= 64 a wave holds at most two runs, with B = 1 sixty-four.
//   votes       one int32 atomic per ray into votes[beam][class]; the lanes of a wave hold different beams unless B < 64.
// Integer sums only: the result is the same whatever the order.
#include "rbpf_raywalk.h"

namespace rbpf {

static const int SB = 256;

__global__ __launch_bounds__(SB) void check_scans_kernel(DevView v, ScanCheckArgs a) {
    const long long r = (long long)blockIdx.x * SB + threadIdx.x;
    const bool live = r < (long long)a.n_poses * a.B;
    const int lane = threadIdx.x & 63;
    int n = -1, b = 0, cls = RBPF_SCAN_SKIP, cost = 0;
    if (live) {
        n = (int)(r / a.B); b = (int)(r - (long long)n * a.B);
        const double z = a.ranges[(a.scan_each ? (size_t)n * a.B : (size_t)0) + b];
        if (z > 0.0 && !(z < a.min_range)) {                              // (a NaN is skipped)
            const int p = a.particle >= 0 ? a.particle : n;
            const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
            const double4 ps = reinterpret_cast<const double4*>(a.pose4)[n];     // x, y, cos(theta), sin(theta)
            const double2 bm = reinterpret_cast<const double2*>(a.beam2)[b];     // cos(angle), sin(angle)
            const bool returned = z < a.max_range;
            const double tz = z * a.inv, tend = tz + a.ttol;
            const double tlim = returned ? (tend < a.tmax ? tend : a.tmax) : a.tmax;
            double t;
            int e_tile, e_i, e_j;
            const int st = walk_ray_to(v, tab, ps, bm, a.inv, tlim, tz, t, e_tile, e_i, e_j);
            if (st == 2) cls = RBPF_SCAN_OFF;
            else if (!returned) cls = st == 1 ? RBPF_SCAN_MISSING : RBPF_SCAN_CLEAR;
            else if (st == 1) {
                const double d = t - tz, hb = (double)a.half_bins;
                cls = d >= -a.ttol ? RBPF_SCAN_MATCH : RBPF_SCAN_LONG;
                double q = __builtin_floor(d * a.bins_per_cell + 0.5);
                q = q < -hb ? -hb : q > hb ? hb : q;                      // clamped as a float64: d may be thousands of cells
                cost = a.tabs[8 + (int)q + a.half_bins];
            } else cls = scan_end_value(v, e_tile, e_i, e_j) < 0 ? RBPF_SCAN_SHORT : RBPF_SCAN_NEW;
        }
        cost += a.tabs[cls];
        if (a.classes) a.classes[r] = (uint8_t)cls;
        if (a.votes) atomicAdd(&a.votes[8 * (size_t)b + cls], 1);
    }
    unsigned long long cnt = live ? 1ull << (8 * cls) : 0ull;
    for (int off = 1; off < 64; off <<= 1) {
        const int n2 = __shfl_down(n, off, 64), c2 = __shfl_down(cost, off, 64);
        const unsigned long long k2 = __shfl_down(cnt, off, 64);
        if (lane + off < 64 && n2 == n) { cost += c2; cnt += k2; }
    }
    if (live && (lane == 0 || b == 0)) {                                  // the first lane of a run
        atomicAdd(&a.cost[n], (unsigned long long)cost);
        if (a.counts)
            for (int c = 0; c < 8; ++c) {
                const int k = (int)((cnt >> (8 * c)) & 0xffull);
                if (k) atomicAdd(&a.counts[8 * (size_t)n + c], k);
            }
    }
}

void launch_check_scans(const DevView& v, const ScanCheckArgs& a, hipStream_t s) {
    const long long rays = (long long)a.n_poses * a.B;
    check_scans_kernel<<<(unsigned)((rays + SB - 1) / SB), SB, 0, s>>>(v, a);
}

}  // namespace rbpf
