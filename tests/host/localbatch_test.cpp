// The host side of rbpf_local_map, thesis_amd/csrc/rbpf_localbatch.h, run on the CPU under -fsanitize=address,undefined
// (tests/test_localbatch_host.py compiles and starts this program).  Expected numbers are literals worked out by hand from the
// specification in include/rbpf_hip.h; the seeded sweep holds the host copy of the placement to the square of half-side reach.
#include "rbpf_localbatch.h"

#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>
#include <vector>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static bool same(const char* got, const char* want) { return want ? got && strcmp(got, want) == 0 : got == nullptr; }
static const double nan_ = std::numeric_limits<double>::quiet_NaN(), inf_ = std::numeric_limits<double>::infinity();

static void test_scalar_checks() {
    const double ps[3] = {0, 0, 0}, off[2] = {0.5, -0.25};
    long long fused[4]; signed char crops[1];
    const int P = 4;
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1, 1, 0.05, 1, nullptr, 0), nullptr));
    EXPECT(same(check_local_args(ps, fused, nullptr, -1, P, 4, 128, 0.05, 8, off, LOCAL_DEVICE_OUT), nullptr));
    EXPECT(same(check_local_args(ps, nullptr, crops, 3, P, 1000, 16, 1e-3, 2, off, 0), nullptr));
    EXPECT(same(check_local_args(nullptr, fused, crops, 0, P, 1, 1, 0.05, 1, nullptr, 0), "poses_n3 is NULL"));
    EXPECT(same(check_local_args(ps, nullptr, nullptr, 0, P, 1, 1, 0.05, 1, nullptr, 0), "fused and crops are both NULL"));
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1, 1, 0.05, 1, nullptr, 2), "unknown flags"));
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1, 1, 0.05, 1, nullptr, 0x80000000u), "unknown flags"));
    EXPECT(same(check_local_args(ps, fused, crops, P, P, 1, 1, 0.05, 1, nullptr, 0), "particle index out of range"));
    EXPECT(same(check_local_args(ps, fused, crops, -2, P, 1, 1, 0.05, 1, nullptr, 0), "particle index out of range"));
    const char* const counts = "n_poses >= 1 and n >= 1 are required";
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, 0, 1, 0.05, 1, nullptr, 0), counts) && same(check_local_args(ps, fused, crops, 0, P, 1, 0, 0.05, 1, nullptr, 0), counts));
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, -3, 1, 0.05, 1, nullptr, 0), counts) && same(check_local_args(ps, fused, crops, 0, P, 1, -1, 0.05, 1, nullptr, 0), counts));
    const char* const samp = "1 <= samples <= 8 is required";
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1, 1, 0.05, 0, nullptr, 0), samp) && same(check_local_args(ps, fused, crops, 0, P, 1, 1, 0.05, 9, nullptr, 0), samp));
    const char* const cell = "cell_out must be finite and > 0";
    for (double bad : {0.0, -0.05, nan_, inf_, -inf_}) EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1, 1, bad, 1, nullptr, 0), cell));
    for (double bad : {nan_, inf_, -inf_})
        for (int k = 0; k < 2; ++k) {
            double o[2] = {0, 0};
            o[k] = bad;
            EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1, 1, 0.05, 1, o, 0), "offset2 must be finite"));
        }
    const char* const each = "particle -1 reads pose n in particle n's map: n_poses must equal n_particles";
    EXPECT(same(check_local_args(ps, fused, crops, -1, P, 3, 1, 0.05, 1, nullptr, 0), each) && same(check_local_args(ps, fused, crops, -1, P, 5, 1, 0.05, 1, nullptr, 0), each));
    const char* const many = "n_poses * n * n < 2^31 is required";
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1 << 17, 128, 0.05, 1, nullptr, 0), many));                 // 2^17 * 2^14 = 2^31
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, (1 << 17) - 1, 128, 0.05, 1, nullptr, 0), nullptr));
    EXPECT(same(check_local_args(ps, fused, crops, 0, P, 1, 46341, 0.05, 1, nullptr, 0), many) && same(check_local_args(ps, fused, crops, 0, P, 2147483647LL, 2147483647LL, 0.05, 1, nullptr, 0), many));
}

static void test_tables_and_reach() {
    LocalPlan p;
    // n = 4, S = 1, cells of 0.5 m, 2 cells per metre: (q + 0.5 - 2) * 0.5; h = 1, hypot(1, 1) * 2 = 2.83 -> 3 + 2 cells
    EXPECT(local_plan(p, 4, 0.5, 1, nullptr, 2.0) && p.error() == nullptr && p.n == 4 && p.S == 1 && p.nq == 4);
    EXPECT(p.gx == std::vector<double>({-0.75, -0.25, 0.25, 0.75}) && p.gy == p.gx && p.reach == 5.0 && p.side == 11);
    // n = 2, S = 2, offset (1, -0.5): (q / 2 + (q % 2 + 0.5) / 2 - 1) * 0.5 + f; h = 0.5, hypot(1.5, 1.0) * 2 = 3.61 -> 4 + 2 cells
    const double off[2] = {1.0, -0.5};
    EXPECT(local_plan(p, 2, 0.5, 2, off, 2.0) && p.nq == 4);
    EXPECT(p.gx == std::vector<double>({0.625, 0.875, 1.125, 1.375}) && p.gy == std::vector<double>({-0.875, -0.625, -0.375, -0.125}));
    EXPECT(p.reach == 6.0 && p.side == 13);
    // S = 3 is no power of two: the table holds what the written order of operations gives
    EXPECT(local_plan(p, 1, 0.3, 3, nullptr, 20.0) && p.gx.size() == 3);
    for (int q = 0; q < 3; ++q) EXPECT(p.gx[(size_t)q] == ((0.0 + ((double)q + 0.5) / 3.0) - 0.5) * 0.3 + 0.0);
    // the limit's two sides at 0.05 m, 20 cells per metre: n = 267: h = 6.675, 188.80 -> 189 + 2 cells, side 383;
    // n = 268: h = 6.7, 189.50 -> 190 + 2, side 385
    EXPECT(local_plan(p, 267, 0.05, 1, nullptr, 20.0) && p.reach == 191.0 && p.side == 383);
    EXPECT(!local_plan(p, 268, 0.05, 1, nullptr, 20.0) &&
           same(p.error(), "the window needs 385 map cells a side, the limit is 384 (RBPF_LOCAL_MAX_SIDE): use a smaller window or offset"));
    const double far[2] = {-9.0, 0.0};                 // a small window far ahead: hypot(9.05, 0.05) * 20 = 181.0 -> 182 + 2, side 369
    EXPECT(local_plan(p, 2, 0.05, 1, far, 20.0) && p.side == 369);
    const double farther[2] = {0.0, 9.6};              // hypot(0.05, 9.65) * 20 = 193.0 -> 194 + 2, side 393
    EXPECT(!local_plan(p, 2, 0.05, 1, farther, 20.0) &&
           same(p.error(), "the window needs 393 map cells a side, the limit is 384 (RBPF_LOCAL_MAX_SIDE): use a smaller window or offset"));
    const double huge[2] = {1e308, 1e308};
    EXPECT(!local_plan(p, 2, 0.05, 1, huge, 20.0) && same(p.error(), "the window reaches farther than a float64 holds in cells"));
    EXPECT(!local_plan(p, 32768, 1e300, 1, nullptr, 20.0) && p.error() != nullptr);
}

static void test_poses_and_weights() {
    LocalPlan p;
    const double good[] = {0, 0, 0, 53687091.0, -53687091.0, 7.0};          // 53687091 * 20 = 1073741820 < 2^30
    EXPECT(local_poses(p, good, 2, 20.0) && p.error() == nullptr);
    for (double bad : {nan_, inf_, -inf_})
        for (int k = 0; k < 6; ++k) {
            double ps[6] = {0, 0, 0, 1, 1, 1};
            ps[k] = bad;
            p.msg.clear();
            const std::string want = std::string("pose ") + (k < 3 ? "0" : "1") + " must be finite";
            EXPECT(!local_poses(p, ps, 2, 20.0) && same(p.error(), want.c_str()));
        }
    const double edge[] = {0, 0, 0, 0, 53687091.2, 0};                       // 53687091.2 * 20 = 2^30
    p.msg.clear();
    EXPECT(!local_poses(p, edge, 2, 20.0) && same(p.error(), "pose 1: |x| and |y| must stay below 2^30 cells"));
    const double neg[] = {-1e300, 0, 0};
    p.msg.clear();
    EXPECT(!local_poses(p, neg, 1, 20.0) && same(p.error(), "pose 0: |x| and |y| must stay below 2^30 cells"));

    p.msg.clear();
    EXPECT(local_weights(p, nullptr, 130) && p.total == 130);
    const uint32_t w[] = {0, 2147483647u, 0}, z[] = {0, 0}, over[] = {2147483647u, 1}, big[] = {4294967295u, 4294967295u};
    EXPECT(local_weights(p, w, 3) && p.total == 2147483647ULL);
    EXPECT(!local_weights(p, z, 2) && same(p.error(), "the weights wq sum to 0"));
    p.msg.clear();
    EXPECT(!local_weights(p, over, 2) && same(p.error(), "the weights wq sum to 2147483648, more than 2^31 - 1"));
    p.msg.clear();
    EXPECT(!local_weights(p, big, 2) && same(p.error(), "the weights wq sum to 8589934590, more than 2^31 - 1"));
}

static void test_window_and_batches() {
    EXPECT(local_row_bytes(1) == 16 && local_row_bytes(11) == 32 && local_row_bytes(17) == 32 && local_row_bytes(19) == 48 && local_row_bytes(383) == 400);
    for (int side = 1; side <= 383; side += 2) EXPECT(local_row_bytes(side) % 16 == 0 && local_row_bytes(side) >= side + 15 && local_row_bytes(side) < side + 31);
    EXPECT(local_window_bytes(383) == 153200);
    EXPECT(local_tables_fit(383, 267) && !local_tables_fit(383, 267 * 8));   // 153200 + 4272 <= 163840 < 153200 + 34176
    EXPECT(local_tables_fit(187, 256) && local_table_bytes(256) == 4096);
    EXPECT(local_crop_stride(5, true) == 25 && local_crop_stride(5, false) == 32 && local_crop_stride(16, false) == 256 && local_cells_padded(33) == 1104);
    EXPECT(local_groups(1) == 1 && local_groups(64) == 1 && local_groups(65) == 2 && local_groups(130) == 3 && local_groups(4096) == 64);
    // 4096 poses, n = 128: 64 MiB of crops, 64 groups * 16384 cells * 20 bytes of sums
    EXPECT(local_batch_bytes(4096, 128, true, true) == 67108864u + 20971520u && local_batch_bytes(4096, 128, false, true) == 20971520u);
    EXPECT(local_batch_bytes(4096, 128, true, false) == 67108864u && local_batch_bytes(3, 5, true, true) == 256 + 768);
    EXPECT(local_batch(4096, 128, true, true, 0) == 4096 && local_batch(4096, 128, true, true, 7) == 7 && local_batch(4096, 128, true, true, 1) == 1);
    EXPECT(local_batch(3, 16, true, true, 100) == 3);
    // n = 256: 4096 crops are 256 MiB by themselves; half of them and their sums (128 + 40 MiB) fit
    EXPECT(local_batch(4096, 256, true, true, 0) == 2048 && local_batch(4096, 256, false, true, 0) == 4096);
    EXPECT(local_batch(100, 2048, true, true, 0) == 32 && local_batch_bytes(32, 2048, true, true) <= LOCAL_SCRATCH && local_batch_bytes(50, 2048, true, true) > LOCAL_SCRATCH);
    for (long long b : {1LL, 63LL, 64LL, 65LL, 4096LL, 100000LL})
        for (int n : {1, 17, 128, 300, 1000}) {
            const long long k = local_batch(b, n, true, true, 0);
            EXPECT(k >= 1 && k <= b && (k == 1 || local_batch_bytes(k, n, true, true) <= LOCAL_SCRATCH));
        }
    EXPECT(local_batch_bytes(1, 32768, true, true) > LOCAL_SCRATCH);          // what rbpf_local_map answers with RBPF_ENOMEM
}

// 10^5 seeded windows and poses: every sample the tables hold, placed by the six operations, lies within `reach` cells of the
// pose's own cell on both axes - the corners and the edge midpoints always, and a random sample
static void test_reach_holds_the_samples() {
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    const double invs[] = {20.0, 40.0, 1000.0 / 130.0, 2.0, 12.5};
    int done = 0, refused = 0;
    double tightest = 1e9;
    for (int trial = 0; done < 100000; ++trial) {
        const double inv = invs[trial % 5];
        const int n = 1 + (int)(u01(rng) * 64), S = 1 + (int)(u01(rng) * 8);
        const double cell_out = (0.1 + 2.9 * u01(rng)) / inv;                       // 0.1 .. 3 map cells
        const double off[2] = {(u01(rng) - 0.5) * 160.0 / inv, (u01(rng) - 0.5) * 160.0 / inv};
        LocalPlan p;
        if (!local_plan(p, n, cell_out, S, trial % 7 ? off : nullptr, inv)) { ++refused; continue; }
        const double scale = trial % 11 == 0 ? 1e9 / inv : trial % 3 == 0 ? 1.0 : 300.0;  // up to 10^9 cells from the origin
        double ps[3] = {(u01(rng) - 0.5) * 2.0 * scale, (u01(rng) - 0.5) * 2.0 * scale, (u01(rng) - 0.5) * 40.0};
        if (trial % 13 == 0) ps[2] = (double)((trial / 13) % 9 - 4) * (M_PI / 4.0);  // the headings where c or s all but vanishes
        if (trial % 17 == 0) { ps[0] = floor(ps[0] * inv) / inv; ps[1] = (floor(ps[1] * inv) + 1.0) / inv; }   // on cell boundaries
        if (!local_poses(p, ps, 1, inv)) { ++failures; fprintf(stderr, "trial %d: %s\n", trial, p.error()); continue; }
        const double c = cos(ps[2]), s = sin(ps[2]);
        const long long X0 = (long long)floor(ps[0] * inv), Y0 = (long long)floor(ps[1] * inv), reach = (long long)p.reach;
        const int last = p.nq - 1, mid = p.nq / 2;
        const int qs[9][2] = {{0, 0}, {0, last}, {last, 0}, {last, last}, {0, mid}, {last, mid}, {mid, 0}, {mid, last},
                              {(int)(u01(rng) * p.nq), (int)(u01(rng) * p.nq)}};
        for (const int* q : qs) {
            long long X, Y;
            local_place(ps[0], ps[1], c, s, p.gx[(size_t)q[0]], p.gy[(size_t)q[1]], inv, X, Y);
            const long long far = std::max(std::llabs(X - X0), std::llabs(Y - Y0));
            if (far > reach) { ++failures; fprintf(stderr, "trial %d: sample (%d, %d) lies %lld cells from the pose's cell, reach %lld\n", trial, q[0], q[1], far, reach); }
            tightest = std::min(tightest, (double)(reach - far));
        }
        ++done;
    }
    EXPECT(refused > 0 && refused < 100000);            // the sweep meets the window limit too
    EXPECT(tightest >= 0.0 && tightest <= 2.0);         // and windows whose corner uses the bound up to the spare cells
}

int main() {
    test_scalar_checks();
    test_tables_and_reach();
    test_poses_and_weights();
    test_window_and_batches();
    test_reach_holds_the_samples();
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    puts("localbatch ok");
    return 0;
}
