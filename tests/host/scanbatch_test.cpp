// The host-only helpers of thesis_amd/csrc/rbpf_scanbatch.h, run on the CPU under -fsanitize=address,undefined
// (tests/test_scanbatch_host.py compiles and starts this program).  Every expected number is a literal worked out from the
// expressions the entry points held before the header existed; every message is the text of rbpf_api.hip.
#include "rbpf_scanbatch.h"

#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static bool same(const char* got, const char* want) { return want ? got && strcmp(got, want) == 0 : got == nullptr; }
static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static void test_carve() {
    EXPECT(pad256(0) == 0 && pad256(1) == 256 && pad256(255) == 256 && pad256(256) == 256 && pad256(257) == 512);
    const size_t sizes[] = {0, 1, 255, 256, 257, 0, 1000, 4096};
    Carve c;
    size_t end = 0;
    for (size_t b : sizes) {                             // regions of their own
        const size_t at = c.take(b);
        EXPECT(at >= end && at % 256 == 0 && c.total() >= at + b && c.total() % 256 == 0);
        end = at + b;
    }
    EXPECT(c.total() == 256 * (0 + 1 + 1 + 1 + 2 + 0 + 4 + 16));
    Carve p;                                             // packed regions, then the end of the upload
    end = 0;
    for (size_t b : sizes) {
        const size_t at = p.pack(b);
        EXPECT(at == end && p.total() == at + b);
        end = at + b;
    }
    EXPECT(end == 5865 && p.close() == 5865 && p.total() == 5888 && p.take(1) == 5888 && p.total() == 6144);
    Carve z;
    EXPECT(z.close() == 0 && z.total() == 0 && z.take(0) == 0 && z.pack(0) == 0 && z.total() == 0);
}

// the walks of rbpf_refine_poses, rbpf_match_pairs and rbpf_build_map at 3 items of 5 beams, n_rot 1, n_trans 1, host outputs
static void test_layouts() {
    const size_t N = 3, B = 5, nk = 3, nw = 3, nray = N * B, vol = N * nk * nw * nw;
    {   // refinement with a field of 37 rows of 2 word pairs
        Carve c;
        const size_t guess_at = c.pack(N * 16), rot_at = c.pack(N * nk * 32), beam_at = c.pack(B * 16), range_at = c.pack(nray * 8);
        const size_t cell_at = c.pack(N * 8), in_b = c.close(), field_at = c.take(37 * 2 * 8);
        const size_t packed_at = c.take(N * 8), gscore_at = c.take(N * 4), used_at = c.take(N * 4), merge_b = c.total() - packed_at;
        const size_t pose_at = c.take(N * 24), n6_at = c.take(N * 24), score_at = c.take(vol * 4);
        EXPECT(guess_at == 0 && rot_at == 48 && beam_at == 336 && range_at == 416 && cell_at == 536 && in_b == 560);
        EXPECT(field_at == 768 && packed_at == 1536 && gscore_at == 1792 && used_at == 2048 && merge_b == 768);
        EXPECT(pose_at == 2304 && n6_at == 2560 && score_at == 2816 && c.total() == 3328);
        Carve d;                                         // device outputs, no field: nothing behind the merge words
        d.pack(560); d.close();
        EXPECT(d.take(0) == 768 && d.take(N * 8) == 768 && d.take(N * 4) == 1024 && d.take(N * 4) == 1280);
        EXPECT(d.take(0) == 1536 && d.take(0) == 1536 && d.take(0) == 1536 && d.total() == 1536);
    }
    {   // pair matching: 3 pairs over 3 scans, windows of Mw 10 (21 rows of 3 word pairs)
        const size_t M = 3;
        EXPECT(refine_row_words(10) == 3);
        Carve c;
        const size_t guess_at = c.pack(M * 16), rot_at = c.pack(M * nk * 32), pose_at = c.pack(N * 32), beam_at = c.pack(B * 16);
        const size_t range_at = c.pack(nray * 8), cell_at = c.pack(M * 8), run_at = c.pack(M * 8), query_at = c.pack(M * 4), in_b = c.close();
        const size_t field_at = c.take(M * 21 * 3 * 8);
        const size_t packed_at = c.take(M * 8), gscore_at = c.take(M * 4), used_at = c.take(M * 4), ref_at = c.take(M * 4), merge_b = c.total() - packed_at;
        const size_t out_pose_at = c.take(M * 24), m8_at = c.take(M * 32), score_at = c.take(vol * 4);
        EXPECT(guess_at == 0 && rot_at == 48 && pose_at == 336 && beam_at == 432 && range_at == 512 && cell_at == 632);
        EXPECT(run_at == 656 && query_at == 680 && in_b == 692 && field_at == 768 && packed_at == 2304 && gscore_at == 2560);
        EXPECT(used_at == 2816 && ref_at == 3072 && merge_b == 1024 && out_pose_at == 3328 && m8_at == 3584 && score_at == 3840);
        EXPECT(c.total() == 4352);
    }
    {   // map building into a box of 7 x 5 cells
        Carve c;
        const size_t pose_at = c.pack(N * 32), beam_at = c.pack(B * 16), range_at = c.pack(nray * 8), in_b = c.close();
        const size_t ends_at = c.take(nray * 4), hits_at = c.take(35 * 4), seen_at = c.take(35 * 4);
        EXPECT(pose_at == 0 && beam_at == 96 && range_at == 176 && in_b == 296 && ends_at == 512 && hits_at == 768 && seen_at == 1024);
        EXPECT(c.total() == 1280);
        Carve s;                                         // seen alone: it takes the place hits had
        s.pack(296); s.close(); s.take(nray * 4);
        EXPECT(s.take(0) == 768 && s.take(35 * 4) == 768 && s.total() == 1024);
    }
}

static void test_staging() {
    const double pi = 3.14159265358979323846;
    const std::vector<double> th = {0.0, pi, -pi, 7.5, -100.25, 2.0 * pi + 1e-9, 1e6, -0.0, 0.3};
    std::vector<double> poses, want, got(4 * th.size() + 1, -7.0);
    for (size_t k = 0; k < th.size(); ++k) { poses.push_back(0.5 * (double)k - 1.0); poses.push_back(-3.25 + (double)k); poses.push_back(th[k]); }
    for (size_t n = 0; n < th.size(); ++n) {             // the loop rbpf_cast_scans held
        want.push_back(poses[3 * n]); want.push_back(poses[3 * n + 1]);
        want.push_back(cos(poses[3 * n + 2])); want.push_back(sin(poses[3 * n + 2]));
    }
    want.push_back(-7.0);                                // nothing behind the last pose is written
    EXPECT(stage_pose4(got.data(), poses.data(), th.size()) == got.data() + 4 * th.size() && same_bits(got, want));
    EXPECT(stage_pose4(got.data(), poses.data(), 0) == got.data());

    want.clear(); got.assign(2 * th.size() + 1, -7.0);
    for (size_t b = 0; b < th.size(); ++b) { want.push_back(cos(th[b])); want.push_back(sin(th[b])); }
    want.push_back(-7.0);
    EXPECT(stage_beam2(got.data(), th.data(), th.size()) == got.data() + 2 * th.size() && same_bits(got, want));

    for (double th0 : th)
        for (int n_rot : {0, 1, 10})
            for (double step : {0.0, 0.004363323129985824, 1.5}) {
                const int nk = 2 * n_rot + 1;
                want.clear(); got.assign(4 * (size_t)nk + 1, -7.0);
                for (int q = 0; q < nk; ++q) {           // the loop rbpf_refine_poses held
                    const double t = th0 + (double)(q - n_rot) * step;
                    want.push_back(cos(t)); want.push_back(sin(t)); want.push_back(t); want.push_back(0.0);
                }
                want.push_back(-7.0);
                EXPECT(stage_rotations(got.data(), th0, n_rot, step) == got.data() + 4 * nk && same_bits(got, want));
            }
}

static void test_checks() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const char* const refine = "n_scans >= 1, 1 <= n_beams <= 16384 and n_scans * n_beams < 2^31 are required";
    const char* const cast = "n_poses >= 0, n_beams >= 1 and n_poses * n_beams < 2^31 are required";
    EXPECT(same(check_counts(1, 1, 16384, 16384, refine), nullptr) && same(check_counts(1, 1, 16385, 16384, refine), refine));
    EXPECT(same(check_counts(0, 1, 5, 16384, refine), refine) && same(check_counts(-1, 1, 5, 16384, refine), refine));
    EXPECT(same(check_counts(3, 1, 0, 16384, refine), refine) && same(check_counts(3, 1, 1, 16384, refine), nullptr));
    EXPECT(same(check_counts(1 << 17, 1, 16384, 16384, refine), refine) && same(check_counts((1 << 17) - 1, 1, 16384, 16384, refine), nullptr));
    EXPECT(same(check_counts(0, 0, 5, 0, cast), nullptr) && same(check_counts(-1, 0, 5, 0, cast), cast) && same(check_counts(1, 0, 16385, 0, cast), nullptr));
    EXPECT(same(check_counts(1 << 27, 0, 16, 0, cast), cast) && same(check_counts(1, 0, 2147483647LL, 0, cast), nullptr));
    EXPECT(same(check_counts(1, 0, 2147483648LL, 0, cast), cast));

    const char* const max_msg = "max_range must be finite and > 0";
    const char* const min_msg = "min_range must be finite and >= 0";
    EXPECT(same(check_max_range(11.0), nullptr) && same(check_max_range(5e-324), nullptr));
    for (double r : {0.0, -0.0, -1.0, nan, inf, -inf}) EXPECT(same(check_max_range(r), max_msg));
    EXPECT(same(check_min_range(0.0), nullptr) && same(check_min_range(-0.0), nullptr) && same(check_min_range(0.3), nullptr));
    for (double r : {-0.1, -5e-324, nan, inf, -inf}) EXPECT(same(check_min_range(r), min_msg));
    EXPECT(same(check_ranges(11.0, 0.0), nullptr) && same(check_ranges(0.0, -1.0), max_msg) && same(check_ranges(11.0, -1.0), min_msg));
    EXPECT(same(check_ranges(nan, nan), max_msg) && same(check_ranges(1.0, 2.0), nullptr));

    std::vector<double> poses = {0.5, 0.4, 0.3, -1.0, 2.0, 1.0}, angles = {-2.0, 0.0, 1e300, 2.0};
    EXPECT(same(check_poses(poses.data(), 2), nullptr) && same(check_poses(poses.data(), 0), nullptr) && same(check_angles(angles.data(), 4), nullptr));
    for (double bad : {nan, inf, -inf})
        for (size_t k = 0; k < poses.size(); ++k) {
            std::vector<double> p = poses;
            p[k] = bad;
            EXPECT(same(check_poses(p.data(), 2), "poses must be finite"));
            EXPECT(same(check_poses(p.data(), 1), k < 3 ? "poses must be finite" : nullptr));   // only the first n poses are read
            std::vector<double> a = angles;
            a[k % 4] = bad;
            EXPECT(same(check_angles(a.data(), 4), "angles must be finite"));
        }
    EXPECT(same(check_finite(poses.data(), 6, "guesses must be finite"), nullptr));
    poses[5] = nan;
    EXPECT(same(check_finite(poses.data(), 6, "guesses must be finite"), "guesses must be finite") && same(check_finite(poses.data(), 5, "x"), nullptr));

    for (int S : {1, 2, 4, 8, 16}) EXPECT(search_substeps_ok(S) && same(check_search(S, 32, 100), nullptr) && same(check_search(S, 0, 0), nullptr));
    for (int S : {0, 3, 5, 32, -1, -2}) EXPECT(!search_substeps_ok(S) && same(check_search(S, 1, 1), "substeps must be 1, 2, 4, 8 or 16"));
    EXPECT(same(check_search(16, 33, 1), "0 <= n_trans <= 32 is required") && same(check_search(4, -1, 1), "0 <= n_trans <= 32 is required"));
    EXPECT(same(check_search(4, 32, 101), "0 <= n_rot <= 100 is required") && same(check_search(4, 1, -1), "0 <= n_rot <= 100 is required"));
    EXPECT(same(check_search(3, 33, 101), "substeps must be 1, 2, 4, 8 or 16") && same(check_search(4, 33, 101), "0 <= n_trans <= 32 is required"));
    EXPECT(same(check_rot_step(0.0), nullptr) && same(check_rot_step(0.01), nullptr));
    for (double s : {-0.01, nan, inf, -inf}) EXPECT(same(check_rot_step(s), "rot_step must be finite and >= 0"));

    EXPECT(mid_step_message("pose refinement") == "pose refinement between rbpf_scan_update_begin and rbpf_scan_update_end");
    EXPECT(mid_step_message("pair matching") == "pair matching between rbpf_scan_update_begin and rbpf_scan_update_end");
}

struct Args { int N, B, Wt, R, s, nk, kpw, Mw, WW; double invS, min_range, max_range; };

// fit is REFINE_BLOCK / (nw * refine_runs(nw, s)) = 512 / (nw * (((((nw + (1 << s) - 1) >> s) + 7) / 8) << s)), by hand:
//   substeps 4, n_trans 12: nw 25, s 2, 4 runs, 100 tasks: 5      substeps 2, n_trans 32: nw 65, s 1, 10 runs, 650 tasks: 0
//   substeps 1, n_trans 0: one task: 512                           substeps 2, n_trans 1: nw 3, s 1, 2 runs, 6 tasks: 85
static void test_search() {
    const char* knob = "RBPF_SCANBATCH_TEST_KPW";
    unsetenv(knob);
    EXPECT(search_kpw(2000, 21, 5, knob) == 5);          // a full batch at the defaults: as many rotations as fit
    EXPECT(search_kpw(12, 21, 5, knob) == 1);            // 12 x ceil(21 / k) stays below 1024 for every k
    EXPECT(search_kpw(100, 21, 5, knob) == 2);           // 100 x 11 = 1100 is the first count of workgroups to reach 1024
    EXPECT(search_kpw(5000, 201, 0, knob) == 1);         // a rotation's tasks exceed the lanes: passes, one rotation each
    EXPECT(search_kpw(5000, 201, 512, knob) == 16);      // never more than 16
    EXPECT(search_kpw(400, 3, 512, knob) == 1 && search_kpw(1024, 3, 512, knob) == 3 && search_kpw(1023, 3, 512, knob) == 2);
    EXPECT(search_kpw(3, 3, 85, knob) == 1 && search_kpw(1 << 20, 1, 85, knob) == 1 && search_kpw(2000, 21, 5, nullptr) == 5);
    setenv(knob, "7", 1);
    EXPECT(search_kpw(12, 21, 5, knob) == 7 && search_kpw(12, 3, 5, knob) == 3 && search_kpw(12, 21, 5, nullptr) == 1);
    setenv(knob, "99", 1);
    EXPECT(search_kpw(12, 21, 5, knob) == 16);
    setenv(knob, "0", 1);
    EXPECT(search_kpw(2000, 21, 5, knob) == 1);
    unsetenv(knob);

    EXPECT(search_shift(1) == 0 && search_shift(2) == 1 && search_shift(4) == 2 && search_shift(8) == 3 && search_shift(16) == 4);
    EXPECT(refine_row_words(225) == 17 && refine_row_words(367) == 25 && refine_row_words(0) == 3 && refine_row_words(16) == 5);
    Args a;
    memset(&a, 0xff, sizeof a);
    EXPECT(!search_setup(a, 12, 181, 4, 12, 10, 20.0, 0.3, 11.0, 219, 5, knob) && a.N == -1 && a.kpw == -1);   // ceil(11 x 20) = 220 > 219
    EXPECT(search_setup(a, 12, 181, 4, 12, 10, 20.0, 0.3, 11.0, 220, 5, knob));
    EXPECT(a.N == 12 && a.B == 181 && a.Wt == 12 && a.R == 10 && a.nk == 21 && a.s == 2 && a.Mw == 225 && a.WW == 17 && a.kpw == 1);
    EXPECT(a.invS == 80.0 && a.min_range == 0.3 && a.max_range == 11.0);
    EXPECT(search_setup(a, 3, 5, 2, 1, 1, 40.0, 0.0, 9.0, 362, 85, knob));                    // reach 360, ceil(1 / 2) + 2 more
    EXPECT(a.N == 3 && a.B == 5 && a.Wt == 1 && a.R == 1 && a.nk == 3 && a.s == 1 && a.Mw == 363 && a.WW == 25 && a.invS == 80.0);
    EXPECT(!search_setup(a, 3, 5, 2, 1, 1, 40.0, 0.0, std::numeric_limits<double>::quiet_NaN(), 362, 85, knob));
}

int main() {
    test_carve();
    test_layouts();
    test_staging();
    test_checks();
    test_search();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("scanbatch ok");
    return 0;
}
