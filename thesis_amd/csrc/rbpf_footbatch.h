// rbpf_footbatch.h -- the host side of rbpf_check_footprints (rbpf_api.hip; include/rbpf_hip.h): the argument
// checks that rbpf_check_rollouts does not already make and their messages, the footprint table's validation, its reach and its
// packed form, the heading bin of a pose, and the results of the three pairings.  Templates, poses and the step bound are
// rbpf_rolloutbatch.h's, called from here.  Plain C++17 and nothing of HIP, so that a program without a GPU can include it
// (tests/host/footbatch_test.cpp).
#pragma once
#include "rbpf_rolloutbatch.h"

static const int FOOT_MAX_BINS = 256;        // heading bins of a table
static const int FOOT_MAX_SPANS = 256;       // spans of one bin
static const int FOOT_MAX_OFFSET = 127;      // |dx|, |y0|, |y1| of a span: a span packs into three bytes
static const int FOOT_MAX_WIDTH = 64;        // cells of a span: one occ_run64
static const int FOOT_MAX_EXEMPT = 255;

// The scalar arguments: the message, or null where they are good.  P is the number of particles.  The flags and the pairing are
// this call's own; everything else is check_rollout_args's, asked with the pose count the pairing stands for.
static inline const char* check_footprint_args(const void* poses_n3, const void* tmpl_xy, const void* tmpl_bin, const void* tmpl_start,
                                               const void* fp_span, const void* fp_start, const void* out, int32_t particle, int P,
                                               long long n_poses, long long n_tmpl, long long n_bins, int32_t inflate, int32_t clear_max,
                                               int32_t exempt, uint32_t flags) {
    if (!tmpl_bin || !fp_span || !fp_start) return "tmpl_bin, fp_span or fp_start is NULL";
    if (flags & ~(PATHS_DEVICE_OUT | PATHS_THROUGH_UNKNOWN)) return "unknown flags (the exemption is the argument exempt; RBPF_PATHS_OWN belongs to rbpf_check_paths)";
    if (n_bins < 1 || n_bins > FOOT_MAX_BINS) return "1 <= n_bins <= 256 is required";
    if (exempt < -1 || exempt > FOOT_MAX_EXEMPT) return "-1 <= exempt <= 255 is required";
    if (particle == -1 && n_poses != 1 && n_poses != P)
        return "particle -1 checks one pose in every particle's map or pose n in particle n's: n_poses must be 1 or n_particles";
    return check_rollout_args(poses_n3, tmpl_xy, tmpl_start, out, particle, P, particle == -1 && n_poses == 1 ? P : n_poses, n_tmpl, inflate,
                              clear_max, flags);
}

// rows of `out`: the poses of one map, or the particles (one pose in every map, or each pose in its own)
static inline long long footprint_rows(int32_t particle, int P, long long n_poses) { return particle >= 0 ? n_poses : P; }
static inline long long footprint_results(int32_t particle, int P, long long n_poses, long long n_tmpl) { return footprint_rows(particle, P, n_poses) * n_tmpl; }
static inline const char* check_footprint_results(int32_t particle, int P, long long n_poses, long long n_tmpl) {
    return footprint_results(particle, P, n_poses, n_tmpl) >= PATHS_MAX_RESULTS ? "rows * n_tmpl < 2^29 is required (rows: n_poses for one map, n_particles with particle -1)" : nullptr;
}

// The heading bin of theta among H: floor(theta * (H / (2 pi)) + 0.5) mod H, in float64 and in this order, reduced into 0 .. H - 1
// for negative headings.  False where |theta * H / (2 pi)| >= 2^31 (or theta is not finite).
static inline bool pose_bin(double theta, int H, int32_t& bin) {
    const double q = theta * ((double)H / (2.0 * M_PI));
    if (!(fabs(q) < 2147483648.0)) return false;
    const long long k = (long long)floor(q + 0.5);
    bin = (int32_t)(((k % H) + H) % H);
    return true;
}

// What the table of a call comes to
struct FootTable {
    int reach = 0;                    // max over the spans of max(|dx|, |y0|, |y1|): no covered cell lies farther from its centre on either axis
    int max_spans = 0;                // spans of the largest bin
    std::string msg;
    const char* error() const { return msg.empty() ? nullptr : msg.c_str(); }
};

// The offset table and the spans; fills t, or returns false with t.msg set
static inline bool footprint_table(FootTable& t, const int32_t* fp_span, const int32_t* fp_start, int H) {
    t = FootTable();
    if (fp_start[0] != 0) { t.msg = "fp_start[0] must be 0"; return false; }
    for (int b = 0; b < H; ++b) {
        const long long n = (long long)fp_start[b + 1] - fp_start[b];
        if (n < 1) { t.msg = "fp_start must increase strictly: bin " + std::to_string(b) + " has no span"; return false; }
        if (n > FOOT_MAX_SPANS) { t.msg = "bin " + std::to_string(b) + " has more than 256 spans"; return false; }
        t.max_spans = std::max(t.max_spans, (int)n);
    }
    for (int b = 0; b < H; ++b)
        for (int32_t k = fp_start[b]; k < fp_start[b + 1]; ++k) {
            const long long dx = fp_span[3 * (size_t)k], y0 = fp_span[3 * (size_t)k + 1], y1 = fp_span[3 * (size_t)k + 2];
            if (dx < -FOOT_MAX_OFFSET || dx > FOOT_MAX_OFFSET || y0 < -FOOT_MAX_OFFSET || y1 > FOOT_MAX_OFFSET || y0 > y1 || y1 - y0 >= FOOT_MAX_WIDTH) {
                t.msg = "bin " + std::to_string(b) + ", span " + std::to_string(k - fp_start[b]) + ": |dx| <= 127, -127 <= y0 <= y1 <= 127 and y1 - y0 <= 63 are required";
                return false;
            }
            t.reach = std::max(t.reach, (int)std::max(std::max(dx < 0 ? -dx : dx, y0 < 0 ? -y0 : y0), y1 < 0 ? -y1 : y1));
        }
    return true;
}

// a span as the kernel reads it: dx, y0 and y1 as signed bytes 0, 1 and 2 of one word
static inline int32_t footprint_pack(const int32_t* span3) {
    return (int32_t)(((uint32_t)span3[0] & 255u) | (((uint32_t)span3[1] & 255u) << 8) | (((uint32_t)span3[2] & 255u) << 16));
}

// every template waypoint's bin lies in [0, H); the message names the first that does not
static inline bool footprint_template_bins(FootTable& t, const int32_t* tmpl_bin, const int32_t* tmpl_start, long long n_tmpl, int H) {
    for (long long k = 0; k < n_tmpl; ++k)
        for (long long w = tmpl_start[k]; w < tmpl_start[k + 1]; ++w)
            if (tmpl_bin[w] < 0 || tmpl_bin[w] >= H) {
                t.msg = "template " + std::to_string(k) + ", waypoint " + std::to_string(w - tmpl_start[k]) + ": the heading bin must lie in [0, n_bins)";
                return false;
            }
    return true;
}

// the poses' bins into pb[n_poses]; the poses are finite (rollout_poses saw to it)
static inline bool footprint_pose_bins(FootTable& t, int32_t* pb, const double* poses_n3, long long n_poses, int H) {
    for (long long n = 0; n < n_poses; ++n)
        if (!pose_bin(poses_n3[3 * n + 2], H, pb[n])) {
            t.msg = "pose " + std::to_string(n) + ": |theta * n_bins / (2 pi)| < 2^31 is required";
            return false;
        }
    return true;
}
