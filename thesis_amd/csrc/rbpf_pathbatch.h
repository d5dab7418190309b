// rbpf_pathbatch.h -- the host side of rbpf_check_paths (rbpf_api.hip; include/rbpf_hip.h): the argument checks and
// their messages, the cells of the waypoints, the step at which a path reaches each waypoint, `steps`, and which particle a path
// belongs to.  Plain C++17 and nothing of HIP, so that a program without a GPU can include it (tests/host/pathbatch_test.cpp).
#pragma once
#include <cmath>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

// the flags of include/rbpf_hip.h, repeated so that this header stands alone (rbpf_api.hip asserts that they agree)
static const uint32_t PATHS_DEVICE_OUT = 1u, PATHS_THROUGH_UNKNOWN = 2u, PATHS_START_EXEMPT = 4u, PATHS_OWN = 8u;
static const int PATHS_MAX_STEPS = 1 << 20;              // steps of one path at the most
static const long long PATHS_MAX_RESULTS = 1LL << 29;    // (particle, path) pairs of one call, exclusive

// The scalar arguments: the message, or null where they are good.  P is the number of particles.
static inline const char* check_path_args(const void* xy, const void* path_start, const void* out, int32_t particle, int P,
                                          long long n_paths, int32_t inflate, int32_t clear_max, uint32_t flags) {
    if (!xy || !path_start || !out) return "xy, path_start or out is NULL";
    if (flags & ~(PATHS_DEVICE_OUT | PATHS_THROUGH_UNKNOWN | PATHS_START_EXEMPT | PATHS_OWN)) return "unknown flags";
    if (particle < -1 || particle >= P) return "particle index out of range";
    if (inflate < 0 || clear_max <= inflate || clear_max > 320) return "0 <= inflate < clear_max <= 320 is required";
    if (n_paths < 1) return "n_paths >= 1 is required";
    if (flags & PATHS_OWN) {
        if (particle != -1) return "RBPF_PATHS_OWN needs particle -1";
        if (n_paths % P != 0) return "with RBPF_PATHS_OWN n_paths must be a multiple of the number of particles";
    }
    return nullptr;
}

// (particle, path) pairs of a call: every path in one map, every path in every map, or with OWN every path in its own particle's
static inline long long path_results(int32_t particle, int P, long long n_paths, uint32_t flags) {
    return particle >= 0 || (flags & PATHS_OWN) ? n_paths : (long long)P * n_paths;
}
static inline const char* check_path_results(int32_t particle, int P, long long n_paths, uint32_t flags) {
    return path_results(particle, P, n_paths, flags) >= PATHS_MAX_RESULTS ? "n_particles * n_paths < 2^29 is required (n_paths < 2^29 for one map or with RBPF_PATHS_OWN)" : nullptr;
}
// with OWN the paths come in P groups of K = n_paths / P, and path k belongs to particle k / K; 0 without the flag
static inline int path_group_size(long long n_paths, int P, uint32_t flags) { return flags & PATHS_OWN ? (int)(n_paths / P) : 0; }

// What the kernel reads, and `steps`.  Cells count from the lattice's first cell (u = X - lo): none is negative.
struct PathBatch {
    std::vector<int32_t> cells;       // [n_waypoints][2]
    std::vector<int32_t> wstep;       // [n_waypoints] the step of its path at which the walk stands on the waypoint; 0 at a path's first
    std::vector<int32_t> steps;       // [n_paths] 1 + the last waypoint's step
    std::string msg;
    const char* error() const { return msg.empty() ? nullptr : msg.c_str(); }
};

// Checks the offset table and the coordinates and fills b; false with b.msg set otherwise.  inv: cells per metre; the lattice
// holds the mosaic cells lo <= X, Y < hi.  A waypoint lies in cell floor(x * inv), in float64: the product of two finite doubles
// may still be infinite, which the range test catches before anything is converted to an integer.
static inline bool path_batch_build(PathBatch& b, const double* xy, const int32_t* path_start, long long n_paths, double inv,
                                    long long lo, long long hi) {
    b.msg.clear();
    if (path_start[0] != 0) { b.msg = "path_start[0] must be 0"; return false; }
    for (long long k = 0; k < n_paths; ++k)
        if (path_start[k + 1] <= path_start[k]) {
            b.msg = "path_start must increase strictly: path " + std::to_string(k) + " has no waypoint";
            return false;
        }
    const size_t nw = (size_t)path_start[n_paths];
    b.cells.resize(2 * nw); b.wstep.resize(nw); b.steps.resize((size_t)n_paths);
    for (long long k = 0; k < n_paths; ++k) {
        long long at = 0;                                                  // the step of the last waypoint
        for (long long w = path_start[k]; w < path_start[k + 1]; ++w) {
            const auto bad = [&](const char* what) {
                b.msg = "path " + std::to_string(k) + ", waypoint " + std::to_string(w - path_start[k]) + what;
                return false;
            };
            if (!std::isfinite(xy[2 * w]) || !std::isfinite(xy[2 * w + 1])) return bad(": coordinates must be finite");
            const double fx = floor(xy[2 * w] * inv), fy = floor(xy[2 * w + 1] * inv);
            if (!(fx >= (double)lo && fx < (double)hi && fy >= (double)lo && fy < (double)hi))
                return bad(": its cell lies outside the tile lattice (raise lattice_radius)");
            const long long u = (long long)fx - lo, v = (long long)fy - lo;    // exact: integers in float64
            if (w > path_start[k]) at += std::max(llabs(u - b.cells[2 * w - 2]), llabs(v - b.cells[2 * w - 1]));
            if (at >= PATHS_MAX_STEPS) { b.msg = "path " + std::to_string(k) + " has more than 2^20 steps"; return false; }
            b.cells[2 * w] = (int32_t)u; b.cells[2 * w + 1] = (int32_t)v; b.wstep[w] = (int32_t)at;
        }
        b.steps[(size_t)k] = (int32_t)(at + 1);
    }
    return true;
}

// The cell of step t = 0 .. n of the segment from cell A to cell B, n = max(|XB - XA|, |YB - YA|) >= 1: the major coordinate moves
// by one a step, the minor one by floor((2 t a + n) / (2 n)), a its whole change.  t <= n < 2^20 and a <= n (a path has at most
// 2^20 steps), so 2 t a + n < 2^42: the product is formed in 64 bits and cannot overflow whatever the lattice.  The kernel's copy of
// this function is path_cell in rbpf_pathwalk.h.
static inline void path_segment_cell(int32_t xa, int32_t ya, int32_t xb, int32_t yb, int32_t t, int32_t& x, int32_t& y) {
    const int32_t dx = xb - xa, dy = yb - ya, ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, n = ax > ay ? ax : ay;
    const int32_t minor = (int32_t)((2ull * (uint64_t)t * (uint64_t)(ax >= ay ? ay : ax) + (uint64_t)n) / (2ull * (uint64_t)n));
    const int32_t sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    if (ax >= ay) { x = xa + sx * t; y = ya + sy * minor; }
    else { y = ya + sy * t; x = xa + sx * minor; }
}
