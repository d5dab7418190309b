// rbpf_scanbatch.h -- what the entry points over a batch of scans share on the host (rbpf_api.hip: cast, view gain, map building,
// pose refinement, pair matching, scan description, scan checks): the layout of a scratch block, the argument checks, the staging loops and
// the set-up of the pose search.  Plain C++17 and nothing of HIP, so that a program without a GPU can include it
// (tests/host/scanbatch_test.cpp).
#pragma once
#include <cmath>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

static inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// The layout of one scratch block, walked once: the offsets an entry point uses and the size it reserves come from the same calls.
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += pad256(bytes); return o; }   // a region of its own, 256-aligned
    size_t pack(size_t bytes) { const size_t o = at; at += bytes; return o; }           // right behind the last one: inside the upload
    size_t close() { const size_t b = at; at = pad256(at); return b; }                  // the upload's bytes; the next region is aligned
    size_t total() const { return at; }
};

// ---- argument checks: the message, or null where the arguments are good ---------------------------------------------------------
// n items of n_beams beams (beams_max 0: no limit).  The entry points word this differently, so the message is theirs.
static inline const char* check_counts(long long n, int n_min, long long n_beams, int beams_max, const char* msg) {
    return n < n_min || n_beams < 1 || (beams_max && n_beams > beams_max) || n * n_beams >= (1LL << 31) ? msg : nullptr;
}
static inline const char* check_max_range(double r) { return !std::isfinite(r) || !(r > 0.0) ? "max_range must be finite and > 0" : nullptr; }
static inline const char* check_min_range(double r) { return !std::isfinite(r) || r < 0.0 ? "min_range must be finite and >= 0" : nullptr; }
static inline const char* check_ranges(double max_range, double min_range) {     // the order every entry point checks them in
    const char* m = check_max_range(max_range);
    return m ? m : check_min_range(min_range);
}
static inline const char* check_finite(const double* p, long long n, const char* msg) {
    for (long long k = 0; k < n; ++k)
        if (!std::isfinite(p[k])) return msg;
    return nullptr;
}
static inline const char* check_poses(const double* poses_n3, int n) { return check_finite(poses_n3, 3LL * n, "poses must be finite"); }
static inline const char* check_angles(const double* angles, int n) { return check_finite(angles, n, "angles must be finite"); }
// scan checks (rbpf_check_scans): the tolerance, the pairing of scans with poses, and the two cost tables; the tables are read
// only once their sizes are known to be good
static inline const char* check_tol(double t) { return !std::isfinite(t) || t < 0.0 ? "tol must be finite and >= 0" : nullptr; }
static inline const char* check_scan_count(long long n_scans, long long n_poses) {
    return n_scans != 1 && n_scans != n_poses ? "n_scans must be 1 or n_poses" : nullptr;
}
static const int SCAN_HALF_BINS_MAX = 4096, SCAN_BINS_PER_CELL_MAX = 64, SCAN_COST_MAX = 1 << 20;
static inline const char* check_beam_tables(const int32_t* hit_tab, int half_bins, int bins_per_cell, const int32_t* class_cost8) {
    if (half_bins < 1 || half_bins > SCAN_HALF_BINS_MAX) return "1 <= half_bins <= 4096 is required";
    if (bins_per_cell < 1 || bins_per_cell > SCAN_BINS_PER_CELL_MAX) return "1 <= bins_per_cell <= 64 is required";
    for (int k = 0; k < 2 * half_bins + 1; ++k)
        if (hit_tab[k] < 0 || hit_tab[k] > SCAN_COST_MAX) return "hit_tab entries must lie in 0 .. 2^20";
    for (int k = 0; k < 8; ++k)
        if (class_cost8[k] < 0 || class_cost8[k] > SCAN_COST_MAX) return "class_cost8 entries must lie in 0 .. 2^20";
    return nullptr;
}
static inline bool search_substeps_ok(int S) { return S == 1 || S == 2 || S == 4 || S == 8 || S == 16; }
static inline const char* check_search(int substeps, int n_trans, int n_rot) {
    if (!search_substeps_ok(substeps)) return "substeps must be 1, 2, 4, 8 or 16";
    if (n_trans < 0 || n_trans > 32) return "0 <= n_trans <= 32 is required";
    return n_rot < 0 || n_rot > 100 ? "0 <= n_rot <= 100 is required" : nullptr;
}
static inline const char* check_rot_step(double s) { return !std::isfinite(s) || s < 0.0 ? "rot_step must be finite and >= 0" : nullptr; }
// RBPF_ESTATE of a call that reads or queues behind the step's buffers while a scan update is half done
static inline std::string mid_step_message(const char* what) { return std::string(what) + " between rbpf_scan_update_begin and rbpf_scan_update_end"; }

// ---- staging: host libm, the device never sees an angle.  Each returns the end of what it wrote -------------------------------------
static inline double* stage_pose4(double* dst, const double* poses_n3, size_t n) {       // [x, y, cos th, sin th]
    for (size_t k = 0; k < n; ++k, dst += 4) {
        dst[0] = poses_n3[3 * k]; dst[1] = poses_n3[3 * k + 1];
        dst[2] = cos(poses_n3[3 * k + 2]); dst[3] = sin(poses_n3[3 * k + 2]);
    }
    return dst;
}
static inline double* stage_beam2(double* dst, const double* angles, size_t n) {         // [cos a, sin a]
    for (size_t b = 0; b < n; ++b, dst += 2) { dst[0] = cos(angles[b]); dst[1] = sin(angles[b]); }
    return dst;
}
static inline int32_t* stage_beam_tables(int32_t* dst, const int32_t* class_cost8, const int32_t* hit_tab, int half_bins) {   // [class costs] [hit_tab]
    for (int k = 0; k < 8; ++k) *dst++ = class_cost8[k];
    for (int k = 0; k < 2 * half_bins + 1; ++k) *dst++ = hit_tab[k];
    return dst;
}
static inline double* stage_rotations(double* dst, double th0, int n_rot, double rot_step) {   // [cos, sin, th, 0] of th0 + (q - n_rot) rot_step
    for (int q = 0; q < 2 * n_rot + 1; ++q, dst += 4) {
        const double th = th0 + (double)(q - n_rot) * rot_step;
        dst[0] = cos(th); dst[1] = sin(th); dst[2] = th; dst[3] = 0.0;
    }
    return dst;
}

// ---- the pose search of refinement and pair matching (rbpf_refine_search.h) ---------------------------------------------------------
static inline int search_shift(int substeps) { return substeps == 1 ? 0 : substeps == 2 ? 1 : substeps == 4 ? 2 : substeps == 8 ? 3 : 4; }
static inline int refine_row_words(long long Mw) { return (int)((((2 * Mw + 1 + 31) >> 5) + 2) | 1); }
// rotations per workgroup: as many as fit (lanes over the tasks of one rotation), fewer while the grid would not fill the GPU;
// the environment variable `knob` overrides it (tests)
static inline int search_kpw(long long items, int nk, int fit, const char* knob) {
    int kpw = std::max(1, std::min(std::min(16, nk), fit));
    while (kpw > 1 && items * ((nk + kpw - 1) / kpw) < 1024) --kpw;
    if (const char* e = knob ? getenv(knob) : nullptr) kpw = std::max(1, std::min(std::min(16, nk), atoi(e)));
    return kpw;
}
// The fields of a RefineArgs that follow from the checked arguments: `items` scans or pairs, `inv` cells per metre, `fit` as above.
// False, and nothing filled, where the window exceeds max_reach = rbpf_refine_max_reach(substeps, n_trans).
template <class Args>
static bool search_setup(Args& a, int items, int n_beams, int substeps, int n_trans, int n_rot, double inv, double min_range,
                         double max_range, int max_reach, int fit, const char* knob) {
    const double reach = ceil(max_range * inv);
    if (!(reach <= (double)max_reach)) return false;
    a.N = items; a.B = n_beams; a.Wt = n_trans; a.R = n_rot; a.nk = 2 * n_rot + 1; a.s = search_shift(substeps);
    a.Mw = (int)reach + (n_trans + substeps - 1) / substeps + 2; a.WW = refine_row_words(a.Mw);
    a.invS = inv * (double)substeps;                                       // exact: a power of two
    a.min_range = min_range; a.max_range = max_range;
    a.kpw = search_kpw(items, a.nk, fit, knob);
    return true;
}
