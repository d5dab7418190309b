// The host side of rbpf_check_footprints, thesis_amd/csrc/rbpf_footbatch.h, run on the CPU under -fsanitize=address,undefined
// (tests/test_footbatch_host.py compiles and starts this program).  Expected numbers and messages are literals worked out by hand
// from the specification in include/rbpf_hip.h.
#include "rbpf_footbatch.h"

#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static bool same(const char* got, const char* want) { return want ? got && strcmp(got, want) == 0 : got == nullptr; }
static const double nan_ = std::numeric_limits<double>::quiet_NaN(), inf_ = std::numeric_limits<double>::infinity();

static void test_scalar_checks() {
    const double ps[3] = {0, 0, 0}, xy[2] = {0, 0};
    const int32_t tb[1] = {0}, ts[2] = {0, 1}, sp[3] = {0, 0, 0}, fs[2] = {0, 1};
    int32_t out[4];
    const int P = 4;
    auto chk = [&](const void* a_tb, const void* a_sp, const void* a_fs, int32_t particle, long long n_poses, long long H, int32_t exempt, uint32_t flags) {
        return check_footprint_args(ps, xy, a_tb, ts, a_sp, a_fs, out, particle, P, n_poses, 1, H, 0, 1, exempt, flags);
    };
    EXPECT(same(chk(tb, sp, fs, 0, 1, 1, -1, 0), nullptr) && same(chk(tb, sp, fs, 3, 1000, 256, 255, 3), nullptr));
    EXPECT(same(chk(tb, sp, fs, -1, 4, 64, 0, 2), nullptr) && same(chk(tb, sp, fs, -1, 1, 64, 3, 1), nullptr));
    const char* const null = "tmpl_bin, fp_span or fp_start is NULL";
    EXPECT(same(chk(nullptr, sp, fs, 0, 1, 1, -1, 0), null) && same(chk(tb, nullptr, fs, 0, 1, 1, -1, 0), null) && same(chk(tb, sp, nullptr, 0, 1, 1, -1, 0), null));
    const char* const flag = "unknown flags (the exemption is the argument exempt; RBPF_PATHS_OWN belongs to rbpf_check_paths)";
    EXPECT(same(chk(tb, sp, fs, 0, 1, 1, -1, PATHS_START_EXEMPT), flag) && same(chk(tb, sp, fs, -1, 4, 1, -1, PATHS_OWN), flag));
    EXPECT(same(chk(tb, sp, fs, 0, 1, 1, -1, 16), flag) && same(chk(tb, sp, fs, 0, 1, 1, -1, 0x80000000u), flag));
    const char* const bins = "1 <= n_bins <= 256 is required";
    EXPECT(same(chk(tb, sp, fs, 0, 1, 0, -1, 0), bins) && same(chk(tb, sp, fs, 0, 1, 257, -1, 0), bins) && same(chk(tb, sp, fs, 0, 1, -3, -1, 0), bins));
    const char* const ex = "-1 <= exempt <= 255 is required";
    EXPECT(same(chk(tb, sp, fs, 0, 1, 1, -2, 0), ex) && same(chk(tb, sp, fs, 0, 1, 1, 256, 0), ex));
    const char* const pairing = "particle -1 checks one pose in every particle's map or pose n in particle n's: n_poses must be 1 or n_particles";
    EXPECT(same(chk(tb, sp, fs, -1, 3, 1, -1, 0), pairing) && same(chk(tb, sp, fs, -1, 5, 1, -1, 0), pairing) && same(chk(tb, sp, fs, -1, 0, 1, -1, 0), pairing));
    // what rbpf_check_rollouts rejects comes through with its own words
    EXPECT(same(check_footprint_args(nullptr, xy, tb, ts, sp, fs, out, 0, P, 1, 1, 1, 0, 1, -1, 0), "poses, tmpl_xy, tmpl_start or out is NULL"));
    EXPECT(same(check_footprint_args(ps, xy, tb, ts, sp, fs, nullptr, 0, P, 1, 1, 1, 0, 1, -1, 0), "poses, tmpl_xy, tmpl_start or out is NULL"));
    EXPECT(same(chk(tb, sp, fs, P, 1, 1, -1, 0), "particle index out of range") && same(chk(tb, sp, fs, -2, 1, 1, -1, 0), "particle index out of range"));
    EXPECT(same(check_footprint_args(ps, xy, tb, ts, sp, fs, out, 0, P, 1, 1, 1, 4, 4, -1, 0), "0 <= inflate < clear_max <= 320 is required"));
    EXPECT(same(check_footprint_args(ps, xy, tb, ts, sp, fs, out, 0, P, 1, 1, 1, 0, 321, -1, 0), "0 <= inflate < clear_max <= 320 is required"));
    EXPECT(same(check_footprint_args(ps, xy, tb, ts, sp, fs, out, 0, P, 0, 1, 1, 0, 1, -1, 0), "n_poses >= 1 and n_tmpl >= 1 are required"));
    EXPECT(same(check_footprint_args(ps, xy, tb, ts, sp, fs, out, -1, P, 1, 0, 1, 0, 1, -1, 0), "n_poses >= 1 and n_tmpl >= 1 are required"));
}

static void test_results_of_the_three_pairings() {
    const int P = 4096;
    EXPECT(footprint_rows(7, P, 1024) == 1024 && footprint_results(7, P, 1024, 256) == 262144);      // every pose in one map
    EXPECT(footprint_rows(-1, P, P) == P && footprint_results(-1, P, P, 256) == 1048576);            // each pose in its own map
    EXPECT(footprint_rows(-1, P, 1) == P && footprint_results(-1, P, 1, 256) == 1048576);            // one pose in every map
    EXPECT(footprint_results(0, P, 1, 1) == 1);
    const char* const many = "rows * n_tmpl < 2^29 is required (rows: n_poses for one map, n_particles with particle -1)";
    EXPECT(same(check_footprint_results(-1, 1024, 1, (1 << 19) - 1), nullptr) && same(check_footprint_results(-1, 1024, 1, 1 << 19), many));
    EXPECT(same(check_footprint_results(-1, 1024, 1024, 1 << 19), many) && same(check_footprint_results(0, 1024, 1, 1 << 19), nullptr));
    EXPECT(same(check_footprint_results(0, 1024, (1LL << 29) - 1, 1), nullptr) && same(check_footprint_results(0, 1024, 1LL << 29, 1), many));
    EXPECT(same(check_footprint_results(3, 4, 2147483647LL, 2147483647LL), many));
}

static void test_pose_bin() {
    int32_t b = -7;
    const double step = 2.0 * M_PI / 8.0;
    EXPECT(pose_bin(0.0, 8, b) && b == 0);
    EXPECT(pose_bin(step, 8, b) && b == 1);
    EXPECT(pose_bin(-step, 8, b) && b == 7);                               // negative headings come back into 0 .. H - 1
    EXPECT(pose_bin(-3.0 * step, 8, b) && b == 5);
    EXPECT(pose_bin(-M_PI, 8, b) && b == 4);
    EXPECT(pose_bin(M_PI, 8, b) && b == 4);
    EXPECT(pose_bin(2.0 * M_PI, 8, b) && b == 0);                          // multiples of 2 pi
    EXPECT(pose_bin(-2.0 * M_PI, 8, b) && b == 0);
    EXPECT(pose_bin(200.0 * M_PI, 8, b) && b == 0);
    EXPECT(pose_bin(-200.0 * M_PI, 64, b) && b == 0);
    EXPECT(pose_bin(0.49 * step, 8, b) && b == 0);
    EXPECT(pose_bin(0.51 * step, 8, b) && b == 1);
    EXPECT(pose_bin(-0.49 * step, 8, b) && b == 0);
    EXPECT(pose_bin(-0.51 * step, 8, b) && b == 7);
    EXPECT(pose_bin(7.51 * step, 8, b) && b == 0);
    // the half-bin points: q = +-0.5 exactly (pi / 4 * (4 / (2 pi)) with M_PI in both), floor(q + 0.5) = 1 and 0
    EXPECT(M_PI / 4.0 * (4.0 / (2.0 * M_PI)) == 0.5);
    EXPECT(pose_bin(M_PI / 4.0, 4, b) && b == 1);
    EXPECT(pose_bin(-M_PI / 4.0, 4, b) && b == 0);
    EXPECT(pose_bin(3.0 * M_PI / 4.0, 4, b) && (b == 2 || b == 1));        // 1.5 up to rounding of the product
    for (double th : {-50.0, -1.0, 0.0, 3.3, 1e6}) EXPECT(pose_bin(th, 1, b) && b == 0);
    EXPECT(pose_bin(1e6, 256, b) && b >= 0 && b < 256);
    // |theta * H / (2 pi)| >= 2^31
    const double edge = 2147483648.0 * (2.0 * M_PI);                       // q = 2^31 for H = 1 up to rounding
    b = -7;
    EXPECT(!pose_bin(edge * 1.0000001, 1, b) && !pose_bin(-edge * 1.0000001, 1, b) && !pose_bin(edge, 256, b) && b == -7);
    EXPECT(pose_bin(edge * 0.9999999, 1, b) && b == 0);
    EXPECT(!pose_bin(nan_, 8, b) && !pose_bin(inf_, 8, b) && !pose_bin(-inf_, 8, b));
    FootTable t;
    int32_t pb[3] = {-7, -7, -7};
    const double good[] = {0, 0, -step, 1, 1, 2.0 * M_PI, 5, 5, 3.0 * step}, bad[] = {0, 0, 0, 0, 0, 1e12, 0, 0, 0};
    EXPECT(footprint_pose_bins(t, pb, good, 3, 8) && pb[0] == 7 && pb[1] == 0 && pb[2] == 3 && t.error() == nullptr);
    EXPECT(!footprint_pose_bins(t, pb, bad, 3, 8) && same(t.error(), "pose 1: |theta * n_bins / (2 pi)| < 2^31 is required"));
}

static void test_table() {
    FootTable t;
    {   // the bounds' edges: 127, width 64, 256 spans
        const int32_t sp[] = {127, -127, -64, -127, 64, 127, 0, -31, 32, 5, 0, 0};
        const int32_t fs[] = {0, 1, 4};
        EXPECT(footprint_table(t, sp, fs, 2) && t.error() == nullptr && t.reach == 127 && t.max_spans == 3);
        const int32_t one[] = {0, 0, 0}, f1[] = {0, 1};
        EXPECT(footprint_table(t, one, f1, 1) && t.reach == 0 && t.max_spans == 1);
        const int32_t small[] = {-3, -2, 5, 4, -6, -1}, f2[] = {0, 2};
        EXPECT(footprint_table(t, small, f2, 1) && t.reach == 6);
    }
    {   // spans outside their bounds: the message names the bin and the span
        const char* const want = "bin 1, span 2: |dx| <= 127, -127 <= y0 <= y1 <= 127 and y1 - y0 <= 63 are required";
        const int32_t fs[] = {0, 1, 4};
        const int32_t bad[][3] = {{128, 0, 0}, {-128, 0, 0}, {0, -128, -100}, {0, 100, 128}, {0, 3, 2}, {0, -32, 32}, {0, 0, 64}, {2147483647, 0, 0}, {0, -2147483647 - 1, 2147483647}};
        for (const auto& s : bad) {
            int32_t sp[12] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 0, 0, 0};
            memcpy(sp + 9, s, sizeof s);
            EXPECT(!footprint_table(t, sp, fs, 2) && same(t.error(), want));
        }
        int32_t sp[12] = {0, 0, 64, 1, 1, 1, 2, 2, 2, 0, 0, 0};
        EXPECT(!footprint_table(t, sp, fs, 2) && same(t.error(), "bin 0, span 0: |dx| <= 127, -127 <= y0 <= y1 <= 127 and y1 - y0 <= 63 are required"));
    }
    {   // the offset table
        std::vector<int32_t> sp(3 * 600, 0);
        const int32_t from_one[] = {1, 2, 3}, empty[] = {0, 2, 2, 3}, back[] = {0, 2, 1, 3}, full[] = {0, 256, 257}, over[] = {0, 1, 258};
        EXPECT(!footprint_table(t, sp.data(), from_one, 2) && same(t.error(), "fp_start[0] must be 0"));
        EXPECT(!footprint_table(t, sp.data(), empty, 3) && same(t.error(), "fp_start must increase strictly: bin 1 has no span"));
        EXPECT(!footprint_table(t, sp.data(), back, 3) && same(t.error(), "fp_start must increase strictly: bin 1 has no span"));
        EXPECT(footprint_table(t, sp.data(), full, 2) && t.max_spans == 256);
        EXPECT(!footprint_table(t, sp.data(), over, 2) && same(t.error(), "bin 1 has more than 256 spans"));
    }
    {   // the packed span: three signed bytes
        const int32_t a[] = {-127, -127, 127}, b[] = {127, -1, 0}, c[] = {0, 0, 0}, d[] = {-1, 5, 68};
        EXPECT(footprint_pack(a) == 0x007f8181 && footprint_pack(b) == 0x0000ff7f && footprint_pack(c) == 0 && footprint_pack(d) == 0x004405ff);
        for (const int32_t* s : {a, b, c, d}) {
            const int32_t w = footprint_pack(s);
            EXPECT((int)(int8_t)(w & 255) == s[0] && (int)(int8_t)((w >> 8) & 255) == s[1] && (int)(int8_t)((w >> 16) & 255) == s[2]);
        }
    }
    {   // the templates' bins
        const int32_t ts[] = {0, 2, 5}, good[] = {0, 7, 3, 3, 0}, high[] = {0, 7, 3, 8, 0}, low[] = {0, -1, 3, 3, 0};
        EXPECT(footprint_template_bins(t = FootTable(), good, ts, 2, 8) && t.error() == nullptr);
        EXPECT(!footprint_template_bins(t, high, ts, 2, 8) && same(t.error(), "template 1, waypoint 1: the heading bin must lie in [0, n_bins)"));
        EXPECT(!footprint_template_bins(t, low, ts, 2, 8) && same(t.error(), "template 0, waypoint 1: the heading bin must lie in [0, n_bins)"));
        EXPECT(!footprint_template_bins(t, good, ts, 2, 7) && same(t.error(), "template 0, waypoint 1: the heading bin must lie in [0, n_bins)"));
    }
}

int main() {
    test_scalar_checks();
    test_results_of_the_three_pairings();
    test_pose_bin();
    test_table();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("footbatch ok");
    return 0;
}
