// kernels_paths.hip -- path checks: polylines of waypoint cells walked through a particle's map, every step's cell tested for
// "known free and clear of the walls" (include/rbpf_hip.h, rbpf_check_paths and rbpf_check_rollouts; the specification is
// DESIGN 3.22, the rollouts' placement 3.24).
//
// One wave works on one path, four waves to a 256-lane workgroup, so that a rollout of 60 steps leaves no wave of its workgroup
// idle.  Lane l takes the steps l, l + 64, ...  A step's cell follows in closed form from the step's number alone: the segment is
// found by a binary search over the steps at which the path reaches its waypoints (staged in LDS for paths of up to PATH_STAGE
// waypoints, read from memory beyond that), the cell on the segment by path_cell.  No lane waits for another.  The walk, the
// clearance and the reduction are rbpf_pathwalk.h's, for both kernels.
//   check_paths_kernel      (particle, path): waypoint cells and their steps come from the host
//   check_rollouts_kernel   (pose, template): the lanes place the template's waypoints at the pose, a wave-wide prefix sum of the
//                           segment lengths gives their steps, both straight into LDS; lane 0 also stores `steps`
#include "rbpf_pathwalk.h"

namespace rbpf {

__global__ __launch_bounds__(64 * PATH_WAVES) void check_paths_kernel(DevView v, PathArgs a) {
    __shared__ int32_t s_step[PATH_WAVES][PATH_STAGE];
    __shared__ int32_t s_cell[PATH_WAVES][PATH_STAGE][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * PATH_WAVES + wv;          // the result this wave writes
    const bool live = r < a.pairs;
    int k = 0, p = a.particle;
    if (live) {
        if (a.own_k) { k = (int)r; p = (int)(r / a.own_k); }
        else { const int pi = (int)(r / a.n_paths); k = (int)(r - (long long)pi * a.n_paths); p += pi; }
    }
    const int first = live ? a.path_start[k] : 0, nw = live ? a.path_start[k + 1] - first : 0;
    const int32_t* __restrict__ g_step = a.wstep + first;
    const int32_t* __restrict__ g_cell = a.cells + 2 * (size_t)first;
    const bool staged = nw <= PATH_STAGE;
    if (staged)
        for (int j = lane; j < nw; j += 64) { s_step[wv][j] = g_step[j]; s_cell[wv][j][0] = g_cell[2 * j]; s_cell[wv][j][1] = g_cell[2 * j + 1]; }
    __syncthreads();
    if (!live) return;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    auto step_of = [&](int j) { return staged ? s_step[wv][j] : g_step[j]; };
    auto cell_of = [&](int j, int& x, int& y) { if (staged) { x = s_cell[wv][j][0]; y = s_cell[wv][j][1]; } else { x = g_cell[2 * j]; y = g_cell[2 * j + 1]; } };
    path_walk(v, tab, PathRule{a.inflate, a.clear_max, a.through_unknown, a.start_exempt}, nw, lane, step_of, cell_of, a.out + 4 * (size_t)r);
}

// Waypoint j of template k at pose n (include/rbpf_hip.h, rbpf_check_rollouts: the placement), every operation a float64 operation
// rounded on its own, as kernels_pairs.hip places a beam's end.  The host has seen to it that no pose can put a waypoint of these
// templates outside the lattice (rbpf_rolloutbatch.h), so the conversion and the sum with `off` stay far inside 32 bits.
__global__ __launch_bounds__(64 * PATH_WAVES) void check_rollouts_kernel(DevView v, RolloutArgs a) {
    __shared__ int32_t s_step[PATH_WAVES][PATH_STAGE];
    __shared__ int32_t s_cell[PATH_WAVES][PATH_STAGE][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * PATH_WAVES + wv;          // the result this wave writes
    const bool live = r < a.pairs;
    const int n = live ? (int)(r / a.n_tmpl) : 0, k = live ? (int)(r - (long long)n * a.n_tmpl) : 0;
    const int first = live ? a.tmpl_start[k] : 0, nw = live ? a.tmpl_start[k + 1] - first : 0;      // nw <= PATH_STAGE: the host checked
    if (live) {
        const double2 ps = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)n], cs = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)n + 1];
        const double2* __restrict__ xy = reinterpret_cast<const double2*>(a.tmpl_xy) + first;
        int carry = 0, lx = 0, ly = 0;                                      // the step and the cell of the waypoint before this round's first
        for (int base = 0; base < nw; base += 64) {                        // nw is the wave's: every lane runs every round
            const int j = base + lane;
            int cx = 0, cy = 0;
            if (j < nw) {
                const double2 q = xy[j];
                const double wx = __dadd_rn(ps.x, __dsub_rn(__dmul_rn(cs.x, q.x), __dmul_rn(cs.y, q.y)));
                const double wy = __dadd_rn(ps.y, __dadd_rn(__dmul_rn(cs.y, q.x), __dmul_rn(cs.x, q.y)));
                cx = (int)__builtin_floor(__dmul_rn(wx, a.inv)) + a.off;
                cy = (int)__builtin_floor(__dmul_rn(wy, a.inv)) + a.off;
            }
            int qx = __shfl_up(cx, 1, 64), qy = __shfl_up(cy, 1, 64);      // the waypoint before this lane's
            if (lane == 0) { qx = base ? lx : cx; qy = base ? ly : cy; }
            int sum = j < nw ? max(abs(cx - qx), abs(cy - qy)) : 0;        // the segment that ends at waypoint j; 0 for waypoint 0
            for (int off = 1; off < 64; off <<= 1) {                       // inclusive prefix sum over the wave
                const int t = __shfl_up(sum, off, 64);
                if (lane >= off) sum += t;
            }
            sum += carry;
            if (j < nw) { s_step[wv][j] = sum; s_cell[wv][j][0] = cx; s_cell[wv][j][1] = cy; }
            carry = __shfl(sum, 63, 64); lx = __shfl(cx, 63, 64); ly = __shfl(cy, 63, 64);      // read only if a round follows: lane 63 held a waypoint
        }
    }
    __syncthreads();
    if (!live) return;
    const int p = a.particle >= 0 ? a.particle : n;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    auto step_of = [&](int j) { return s_step[wv][j]; };
    auto cell_of = [&](int j, int& x, int& y) { x = s_cell[wv][j][0]; y = s_cell[wv][j][1]; };
    path_walk(v, tab, PathRule{a.inflate, a.clear_max, a.through_unknown, a.start_exempt}, nw, lane, step_of, cell_of, a.out + 4 * (size_t)r);
    if (lane == 0 && a.steps) a.steps[r] = s_step[wv][nw - 1] + 1;
}

void launch_check_paths(const DevView& v, const PathArgs& a, hipStream_t s) {
    check_paths_kernel<<<(unsigned)((a.pairs + PATH_WAVES - 1) / PATH_WAVES), 64 * PATH_WAVES, 0, s>>>(v, a);
}

void launch_check_rollouts(const DevView& v, const RolloutArgs& a, hipStream_t s) {
    check_rollouts_kernel<<<(unsigned)((a.pairs + PATH_WAVES - 1) / PATH_WAVES), 64 * PATH_WAVES, 0, s>>>(v, a);
}

}  // namespace rbpf
