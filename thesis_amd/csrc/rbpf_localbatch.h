// rbpf_localbatch.h -- the host side of rbpf_local_map (rbpf_api.hip; include/rbpf_hip.h): the argument checks
// and their messages, the sample tables gx / gy, how far a window can reach from its pose's cell, the LDS a window needs, the
// batch split, and a host copy of the placement.  Plain C++17 and nothing of HIP, so that a program without a GPU can include it
// (tests/host/localbatch_test.cpp).
#pragma once
#include "rbpf_scanbatch.h"

#include <vector>

static const uint32_t LOCAL_DEVICE_OUT = 1u;             // RBPF_LOCAL_DEVICE_OUT (rbpf_api.hip asserts that it is)
static const int LOCAL_MAX_SIDE = 384;                   // RBPF_LOCAL_MAX_SIDE: 2 reach + 1 cells at the most
static const int LOCAL_MARGIN = 2;                       // cells added to a window's reach for the placement's rounding
static const int LOCAL_GROUP = 64;                       // poses whose weighted crops one workgroup of the fusion adds up
static const size_t LOCAL_SCRATCH = (size_t)256 << 20;   // crops and group sums of one batch of poses at the most
static const size_t LOCAL_LDS = 160 * 1024;              // LDS of one gfx950 workgroup

// What the scalar arguments of a call come to.  reach is a whole number of cells kept in float64: it may exceed any integer
// type before local_plan turns the call down.
struct LocalPlan {
    int n = 0, S = 0, nq = 0;         // output cells a side, samples a cell and axis, samples an axis (n S)
    double reach = 0.0;               // ceil(hypot(|fx| + h, |fy| + h) inv) + LOCAL_MARGIN cells, h = 0.5 n cell_out
    int side = 0;                     // 2 reach + 1: rows of the LDS window
    std::vector<double> gx, gy;       // [nq] sample coordinates in the robot's frame, metres
    unsigned long long total = 0;     // sum of wq
    std::string msg;
    const char* error() const { return msg.empty() ? nullptr : msg.c_str(); }
};

// The scalar arguments: the message, or null where they are good.  P is the number of particles.
static inline const char* check_local_args(const void* poses_n3, const void* fused, const void* crops, int32_t particle, int P,
                                           long long n_poses, long long n, double cell_out, long long samples, const double* offset2,
                                           uint32_t flags) {
    if (!poses_n3) return "poses_n3 is NULL";
    if (!fused && !crops) return "fused and crops are both NULL";
    if (flags & ~LOCAL_DEVICE_OUT) return "unknown flags";
    if (particle < -1 || particle >= P) return "particle index out of range";
    if (n_poses < 1 || n < 1) return "n_poses >= 1 and n >= 1 are required";
    if (samples < 1 || samples > 8) return "1 <= samples <= 8 is required";
    if (!std::isfinite(cell_out) || !(cell_out > 0.0)) return "cell_out must be finite and > 0";
    if (offset2 && (!std::isfinite(offset2[0]) || !std::isfinite(offset2[1]))) return "offset2 must be finite";
    if (particle < 0 && n_poses != P) return "particle -1 reads pose n in particle n's map: n_poses must equal n_particles";
    if (n > 32768 || n_poses * n * n >= (1LL << 31)) return "n_poses * n * n < 2^31 is required";
    return nullptr;
}

// The tables and the window; fills p, or returns false with p.msg set.  inv: cells per metre.  Every operation is a float64
// operation rounded on its own, in the order of include/rbpf_hip.h.
static inline bool local_plan(LocalPlan& p, int n, double cell_out, int samples, const double* offset2, double inv) {
    p = LocalPlan();
    p.n = n; p.S = samples; p.nq = n * samples;
    const double fx = offset2 ? offset2[0] : 0.0, fy = offset2 ? offset2[1] : 0.0;
    const double h = 0.5 * (double)n * cell_out;
    const double cells = hypot(fabs(fx) + h, fabs(fy) + h) * inv;
    if (!std::isfinite(cells)) { p.msg = "the window reaches farther than a float64 holds in cells"; return false; }
    p.reach = ceil(cells) + (double)LOCAL_MARGIN;
    if (2.0 * p.reach + 1.0 > (double)LOCAL_MAX_SIDE) {
        p.msg = "the window needs " + std::to_string((long long)std::min(2.0 * p.reach + 1.0, 9e18)) + " map cells a side, the limit is " +
                std::to_string(LOCAL_MAX_SIDE) + " (RBPF_LOCAL_MAX_SIDE): use a smaller window or offset";
        return false;
    }
    p.side = 2 * (int)p.reach + 1;
    p.gx.resize((size_t)p.nq); p.gy.resize((size_t)p.nq);
    const double Sd = (double)samples, half = 0.5 * (double)n;
    for (int q = 0; q < p.nq; ++q) {
        const double u = (((double)(q / samples) + ((double)(q % samples) + 0.5) / Sd) - half) * cell_out;
        p.gx[(size_t)q] = u + fx; p.gy[(size_t)q] = u + fy;
    }
    return true;
}

// The poses and the weights: false with p.msg set at the first bad one.  |x inv| < 2^30 keeps the cell and everything within
// `reach` of it inside 32 bits; the lattice need not hold the window.
static inline bool local_poses(LocalPlan& p, const double* poses_n3, long long n_poses, double inv) {
    for (long long k = 0; k < n_poses; ++k) {
        const double* q = poses_n3 + 3 * k;
        if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) { p.msg = "pose " + std::to_string(k) + " must be finite"; return false; }
        if (!(fabs(q[0] * inv) < 1073741824.0) || !(fabs(q[1] * inv) < 1073741824.0)) {
            p.msg = "pose " + std::to_string(k) + ": |x| and |y| must stay below 2^30 cells";
            return false;
        }
    }
    return true;
}
static inline bool local_weights(LocalPlan& p, const uint32_t* wq, long long n_poses) {
    p.total = 0;
    for (long long k = 0; k < n_poses; ++k) p.total += wq ? wq[k] : 1u;     // n_poses < 2^31 values below 2^32: no overflow
    if (p.total == 0) { p.msg = "the weights wq sum to 0"; return false; }
    if (p.total > 2147483647ULL) { p.msg = "the weights wq sum to " + std::to_string(p.total) + ", more than 2^31 - 1"; return false; }
    return true;
}

// The LDS window of a pose: `side` rows of `local_row_bytes` bytes.  Its first column is the pose's first cell rounded down to
// a multiple of 16, so that a 16-byte strip of a tile row lands on a 16-byte strip of the window: up to 15 columns in front.
static inline int local_row_bytes(int side) { return (side + 15 + 15) & ~15; }
static inline size_t local_window_bytes(int side) { return (size_t)side * local_row_bytes(side); }
// the tables go into LDS behind the window where both fit, else the lanes read them from memory once per output cell
static inline size_t local_table_bytes(int nq) { return (size_t)nq * 16; }
static inline bool local_tables_fit(int side, int nq) { return local_window_bytes(side) + local_table_bytes(nq) <= LOCAL_LDS; }

// One pose's crop in scratch (padded so that every crop starts on a 16-byte strip) and the fusion's group sums: three uint32 and
// one int64 per cell and group of LOCAL_GROUP poses.
static inline size_t local_crop_stride(int n, bool dense) { const size_t c = (size_t)n * n; return dense ? c : (c + 15) & ~(size_t)15; }
static inline size_t local_cells_padded(int n) { return ((size_t)n * n + 15) & ~(size_t)15; }
static inline long long local_groups(long long poses) { return (poses + LOCAL_GROUP - 1) / LOCAL_GROUP; }
static inline size_t local_batch_bytes(long long poses, int n, bool scratch_crops, bool fuse) {
    return pad256(scratch_crops ? (size_t)poses * local_crop_stride(n, false) : 0) +
           pad256(fuse ? (size_t)local_groups(poses) * local_cells_padded(n) * 20 : 0);
}
// poses per batch: all of them, halved (to a multiple of LOCAL_GROUP while above it) until the batch's scratch stays under
// LOCAL_SCRATCH or one pose is left - the caller turns down a pose that does not fit alone; cap > 0 (RBPF_LOCAL_BATCH) caps
// it, for tests
static inline long long local_batch(long long n_poses, int n, bool scratch_crops, bool fuse, long long cap) {
    long long b = n_poses;
    while (b > 1 && local_batch_bytes(b, n, scratch_crops, fuse) > LOCAL_SCRATCH)
        b = b > LOCAL_GROUP ? (b / 2 + LOCAL_GROUP - 1) / LOCAL_GROUP * LOCAL_GROUP : b / 2;
    if (cap > 0) b = std::min(b, cap);
    return b;
}

// The placement (include/rbpf_hip.h, rbpf_local_map; that of rbpf_check_rollouts), every operation a float64 operation rounded
// on its own: the mosaic cell of the sample (gx, gy) at the pose (x, y) with c = cos(theta), s = sin(theta).  The kernel's copy
// is in local_crop_kernel (kernels_local.hip).
static inline void local_place(double x, double y, double c, double s, double gx, double gy, double inv, long long& X, long long& Y) {
    const double cx = c * gx, sy = s * gy, sx = s * gx, cy = c * gy;
    const double rx = cx - sy, ry = sx + cy;
    const double wx = x + rx, wy = y + ry;
    X = (long long)floor(wx * inv); Y = (long long)floor(wy * inv);
}
