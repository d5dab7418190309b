// The helpers rbpf_check_scans added to thesis_amd/csrc/rbpf_scanbatch.h, run on the CPU under -fsanitize=address,undefined
// (tests/test_scancheck_host.py compiles and starts this program).  The tables are heap arrays of exactly the size the entry point
// documents, so a read past 2 * half_bins + 1 or 8 entries is the sanitizer's to report; every message is the text of rbpf_api.hip.
#include "rbpf_scanbatch.h"

#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static bool same(const char* got, const char* want) { return want ? got && strcmp(got, want) == 0 : got == nullptr; }

static void test_checks() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const char* const tol_msg = "tol must be finite and >= 0";
    EXPECT(same(check_tol(0.0), nullptr) && same(check_tol(-0.0), nullptr) && same(check_tol(0.1), nullptr) && same(check_tol(1e300), nullptr));
    for (double t : {-0.1, -5e-324, nan, inf, -inf}) EXPECT(same(check_tol(t), tol_msg));

    const char* const scans_msg = "n_scans must be 1 or n_poses";
    EXPECT(same(check_scan_count(1, 1), nullptr) && same(check_scan_count(1, 4096), nullptr) && same(check_scan_count(4096, 4096), nullptr));
    for (long long n : {0LL, -1LL, 2LL, 4095LL, 4097LL}) EXPECT(same(check_scan_count(n, 4096), scans_msg));
    EXPECT(same(check_scan_count(2, 1), scans_msg) && same(check_scan_count(0, 0), nullptr));
}

static void test_tables() {
    const char* const hb_msg = "1 <= half_bins <= 4096 is required";
    const char* const bpc_msg = "1 <= bins_per_cell <= 64 is required";
    const char* const hit_msg = "hit_tab entries must lie in 0 .. 2^20";
    const char* const cc_msg = "class_cost8 entries must lie in 0 .. 2^20";
    const std::vector<int32_t> cc = {0, 0, 1 << 20, 5, 6, 7, 8, 9};
    for (int hb : {1, 2, 7, 16, 4096}) {
        std::vector<int32_t> hit(2 * (size_t)hb + 1, 3);
        hit[0] = hit.back() = 1 << 20;
        EXPECT(same(check_beam_tables(hit.data(), hb, 1, cc.data()), nullptr) && same(check_beam_tables(hit.data(), hb, 64, cc.data()), nullptr));
        EXPECT(same(check_beam_tables(hit.data(), hb, 0, cc.data()), bpc_msg) && same(check_beam_tables(hit.data(), hb, 65, cc.data()), bpc_msg));
        EXPECT(same(check_beam_tables(hit.data(), hb, -4, cc.data()), bpc_msg));
        for (size_t k : {(size_t)0, (size_t)hb, hit.size() - 1})
            for (int32_t bad : {-1, (1 << 20) + 1, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()}) {
                std::vector<int32_t> h2 = hit;
                h2[k] = bad;
                EXPECT(same(check_beam_tables(h2.data(), hb, 4, cc.data()), hit_msg));
            }
        for (size_t k = 0; k < 8; ++k)
            for (int32_t bad : {-1, (1 << 20) + 1}) {
                std::vector<int32_t> c2 = cc;
                c2[k] = bad;
                EXPECT(same(check_beam_tables(hit.data(), hb, 4, c2.data()), cc_msg));
            }
        // staged as [class costs] [hit_tab], nothing behind it
        std::vector<int32_t> got(8 + hit.size() + 1, -7), want(cc);
        want.insert(want.end(), hit.begin(), hit.end());
        want.push_back(-7);
        EXPECT(stage_beam_tables(got.data(), cc.data(), hit.data(), hb) == got.data() + 8 + hit.size() && got == want);
    }
    // a bad size is refused before either table is read: one-entry tables stand in for the caller's
    const std::vector<int32_t> one = {1 << 30};
    for (int hb : {0, -1, 4097, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()})
        EXPECT(same(check_beam_tables(one.data(), hb, 4, one.data()), hb_msg));
    const std::vector<int32_t> three = {0, 0, 0};
    EXPECT(same(check_beam_tables(three.data(), 1, 0, one.data()), bpc_msg));
}

// the walk of rbpf_check_scans over its scratch block at 3 poses of 5 beams, half_bins 2
static void test_layout() {
    const size_t N = 3, B = 5, ntab = 8 + 5;
    {   // one scan for every pose, host outputs, all four asked for
        Carve c;
        const size_t pose_at = c.pack(N * 32), beam_at = c.pack(B * 16), range_at = c.pack(1 * B * 8), tab_at = c.pack(ntab * 4), in_b = c.close();
        const size_t cost_at = c.take(N * 8), counts_at = c.take(N * 32), votes_at = c.take(B * 32), classes_at = c.take(N * B);
        EXPECT(pose_at == 0 && beam_at == 96 && range_at == 176 && tab_at == 216 && in_b == 268);
        EXPECT(cost_at == 512 && counts_at == 768 && votes_at == 1024 && classes_at == 1280 && c.total() == 1536);
    }
    {   // a scan per pose, device outputs: nothing behind the upload
        Carve c;
        c.pack(N * 32); c.pack(B * 16);
        const size_t range_at = c.pack(N * B * 8), tab_at = c.pack(ntab * 4), in_b = c.close();
        EXPECT(range_at == 176 && tab_at == 296 && in_b == 348 && tab_at % 8 == 0);
        EXPECT(c.take(0) == 512 && c.take(0) == 512 && c.total() == 512);
    }
}

int main() {
    test_checks();
    test_tables();
    test_layout();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("scancheck ok");
    return 0;
}
