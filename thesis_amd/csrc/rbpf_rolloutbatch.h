// rbpf_rolloutbatch.h -- the host side of rbpf_check_rollouts (rbpf_api.hip; include/rbpf_hip.h): the argument
// checks and their messages, how far a template can reach from a pose, the test that keeps every placed waypoint inside the
// lattice without placing one, the bound on a rollout's steps, and a host copy of the placement.  Plain C++17 and nothing of
// HIP, so that a program without a GPU can include it (tests/host/rolloutbatch_test.cpp).
#pragma once
#include "rbpf_pathbatch.h"

static const int ROLLOUT_MAX_WAYPOINTS = 128;            // waypoints of one template at the most: what PATH_STAGE stages in LDS
static const int ROLLOUT_MARGIN = 2;                     // cells added to a template's reach for the placement's rounding

// The scalar arguments: the message, or null where they are good.  P is the number of particles.
static inline const char* check_rollout_args(const void* poses_n3, const void* tmpl_xy, const void* tmpl_start, const void* out,
                                             int32_t particle, int P, long long n_poses, long long n_tmpl, int32_t inflate,
                                             int32_t clear_max, uint32_t flags) {
    if (!poses_n3 || !tmpl_xy || !tmpl_start || !out) return "poses, tmpl_xy, tmpl_start or out is NULL";
    if (flags & ~(PATHS_DEVICE_OUT | PATHS_THROUGH_UNKNOWN | PATHS_START_EXEMPT)) return "unknown flags (RBPF_PATHS_OWN belongs to rbpf_check_paths)";
    if (particle < -1 || particle >= P) return "particle index out of range";
    if (inflate < 0 || clear_max <= inflate || clear_max > 320) return "0 <= inflate < clear_max <= 320 is required";
    if (n_poses < 1 || n_tmpl < 1) return "n_poses >= 1 and n_tmpl >= 1 are required";
    if (particle < 0 && n_poses != P) return "particle -1 checks pose n in particle n's map: n_poses must equal n_particles";
    return nullptr;
}
static inline long long rollout_results(long long n_poses, long long n_tmpl) { return n_poses * n_tmpl; }     // both below 2^31
static inline const char* check_rollout_results(long long n_poses, long long n_tmpl) {
    return rollout_results(n_poses, n_tmpl) >= PATHS_MAX_RESULTS ? "n_poses * n_tmpl < 2^29 is required" : nullptr;
}

// What the templates of a call come to.  reach is a whole number of cells kept in float64: it may exceed any integer type before
// the tests below turn the call down.
struct RolloutBatch {
    int m_max = 0;                    // waypoints of the longest template
    double rmax = 0.0;                // max |lx| + |ly| over all waypoints, metres
    double reach = 0.0;               // ceil(rmax * inv) + ROLLOUT_MARGIN cells: no placed waypoint's cell lies farther from its pose's on either axis
    std::string msg;
    const char* error() const { return msg.empty() ? nullptr : msg.c_str(); }
};

// The offset table and the coordinates of the templates; fills b, or returns false with b.msg set.  inv: cells per metre.
// |cos| and |sin| are <= 1, so |lx| + |ly| bounds both rotated coordinates whatever the heading.  A rollout's consecutive
// waypoints both lie within `reach` cells of the pose's cell, so a segment has at most 2 reach steps and a rollout of m waypoints
// at most (m - 1) 2 reach: below 2^20 for the longest template, or the call is turned down.
static inline bool rollout_templates(RolloutBatch& b, const double* tmpl_xy, const int32_t* tmpl_start, long long n_tmpl, double inv) {
    b = RolloutBatch();
    if (tmpl_start[0] != 0) { b.msg = "tmpl_start[0] must be 0"; return false; }
    for (long long k = 0; k < n_tmpl; ++k) {
        const long long m = (long long)tmpl_start[k + 1] - tmpl_start[k];
        if (m < 1) { b.msg = "tmpl_start must increase strictly: template " + std::to_string(k) + " has no waypoint"; return false; }
        if (m > ROLLOUT_MAX_WAYPOINTS) { b.msg = "template " + std::to_string(k) + " has more than 128 waypoints"; return false; }
        b.m_max = std::max(b.m_max, (int)m);
    }
    for (long long k = 0; k < n_tmpl; ++k)
        for (long long w = tmpl_start[k]; w < tmpl_start[k + 1]; ++w) {
            const double lx = tmpl_xy[2 * w], ly = tmpl_xy[2 * w + 1];
            if (!std::isfinite(lx) || !std::isfinite(ly)) {
                b.msg = "template " + std::to_string(k) + ", waypoint " + std::to_string(w - tmpl_start[k]) + ": coordinates must be finite";
                return false;
            }
            b.rmax = std::max(b.rmax, fabs(lx) + fabs(ly));
        }
    const double cells = b.rmax * inv;
    if (!std::isfinite(cells)) { b.msg = "the templates reach farther than a float64 holds in cells"; return false; }
    b.reach = ceil(cells) + (double)ROLLOUT_MARGIN;
    if ((double)(b.m_max - 1) * 2.0 * b.reach >= (double)PATHS_MAX_STEPS) {
        b.msg = "a rollout could have more than 2^20 steps: (waypoints - 1) * 2 * reach < 2^20 is required, reach = " + std::to_string((long long)std::min(b.reach, 9e18)) + " cells";
        return false;
    }
    return true;
}

// A pose may be used if the square of half-side reach round its own cell lies in the lattice [lo, hi) on both axes; reach as
// rollout_templates left it.  Everything is compared in float64 before anything is converted: x * inv may be infinite.
static inline bool rollout_pose_ok(double x, double y, double inv, double reach, long long lo, long long hi) {
    const double fx = floor(x * inv), fy = floor(y * inv);
    return fx - reach >= (double)lo && fx + reach < (double)hi && fy - reach >= (double)lo && fy + reach < (double)hi;
}
static inline bool rollout_poses(RolloutBatch& b, const double* poses_n3, long long n_poses, double inv, long long lo, long long hi) {
    for (long long n = 0; n < n_poses; ++n) {
        const double* p = poses_n3 + 3 * n;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) { b.msg = "pose " + std::to_string(n) + " must be finite"; return false; }
        if (!rollout_pose_ok(p[0], p[1], inv, b.reach, lo, hi)) {
            b.msg = "pose " + std::to_string(n) + ": the templates placed there could leave the tile lattice (reach " + std::to_string((long long)std::min(b.reach, 9e18)) + " cells; raise lattice_radius)";
            return false;
        }
    }
    return true;
}

// The placement (include/rbpf_hip.h, rbpf_check_rollouts), every operation a float64 operation rounded on its own: the mosaic cell
// of the template waypoint (lx, ly) at the pose (x, y) with c = cos(theta), s = sin(theta).  The kernel's copy is in
// check_rollouts_kernel (kernels_paths.hip).  Only for poses rollout_pose_ok accepts: the conversion needs the cell in range.
static inline void rollout_place(double x, double y, double c, double s, double lx, double ly, double inv, long long& X, long long& Y) {
    const double cx = c * lx, sy = s * ly, sx = s * lx, cy = c * ly;
    const double rx = cx - sy, ry = sx + cy;
    const double wx = x + rx, wy = y + ry;
    X = (long long)floor(wx * inv); Y = (long long)floor(wy * inv);
}
