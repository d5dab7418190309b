// kernels_cast.hip -- lidar scans cast from the particles' occupancy maps (include/rbpf_hip.h, rbpf_cast_scans).
//
// One lane per ray; ray r = pose * B + beam, so the beams of a pose lie in consecutive lanes: neighbouring beams walk
// neighbouring cells and share the occupancy words they load.  The walk itself - the supercover (4-connected) grid traversal
// of DESIGN 3.7 in float64 against the occupancy bit planes - is walk_ray of rbpf_raywalk.h, shared with kernels_gain.hip.
#include "rbpf_raywalk.h"

namespace rbpf {

static const int CB = 256;

__global__ __launch_bounds__(CB) void cast_scans_kernel(DevView v, CastArgs a) {
    const long long r = (long long)blockIdx.x * CB + threadIdx.x;
    if (r >= (long long)a.n_poses * a.B) return;
    const int n = (int)(r / a.B), b = (int)(r - (long long)n * a.B);
    const int p = a.particle >= 0 ? a.particle : n;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    const double4 ps = reinterpret_cast<const double4*>(a.pose4)[n];     // x, y, cos(theta), sin(theta)
    const double2 bm = reinterpret_cast<const double2*>(a.beam2)[b];     // cos(angle), sin(angle)
    double t;
    const int st = walk_ray(v, tab, ps, bm, a.inv, a.tlim, t, [](int, int) {});
    const double range = st == 1 ? t / a.inv : a.max_range;
    a.ranges[r] = range;
    if (a.status) a.status[r] = (uint8_t)st;
}

void launch_cast_scans(const DevView& v, const CastArgs& a, hipStream_t s) {
    const long long rays = (long long)a.n_poses * a.B;
    cast_scans_kernel<<<(unsigned)((rays + CB - 1) / CB), CB, 0, s>>>(v, a);
}

}  // namespace rbpf
