// The host side of rbpf_check_rollouts, thesis_amd/csrc/rbpf_rolloutbatch.h, run on the CPU under -fsanitize=address,undefined
// (tests/test_rolloutbatch_host.py compiles and starts this program).  Expected numbers are literals worked out by hand from the
// specification in include/rbpf_hip.h; the seeded sweep holds the placement to the lattice wherever the pose test said yes.
#include "rbpf_rolloutbatch.h"

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
    const double ps[3] = {0, 0, 0}, xy[2] = {0, 0};
    const int32_t ts[2] = {0, 1};
    int32_t out[4];
    const int P = 4;
    EXPECT(same(check_rollout_args(ps, xy, ts, out, 0, P, 1, 1, 0, 1, 0), nullptr) && same(check_rollout_args(ps, xy, ts, out, -1, P, 4, 9, 20, 320, 7), nullptr));
    EXPECT(same(check_rollout_args(ps, xy, ts, out, 3, P, 1000, 1, 319, 320, 0), nullptr));
    const char* const null = "poses, tmpl_xy, tmpl_start or out is NULL";
    EXPECT(same(check_rollout_args(nullptr, xy, ts, out, 0, P, 1, 1, 0, 1, 0), null) && same(check_rollout_args(ps, nullptr, ts, out, 0, P, 1, 1, 0, 1, 0), null));
    EXPECT(same(check_rollout_args(ps, xy, nullptr, out, 0, P, 1, 1, 0, 1, 0), null) && same(check_rollout_args(ps, xy, ts, nullptr, 0, P, 1, 1, 0, 1, 0), null));
    const char* const flag = "unknown flags (RBPF_PATHS_OWN belongs to rbpf_check_paths)";
    EXPECT(same(check_rollout_args(ps, xy, ts, out, -1, P, 4, 1, 0, 1, PATHS_OWN), flag) && same(check_rollout_args(ps, xy, ts, out, 0, P, 1, 1, 0, 1, 16), flag));
    EXPECT(same(check_rollout_args(ps, xy, ts, out, 0, P, 1, 1, 0, 1, 0x80000000u), flag));
    EXPECT(same(check_rollout_args(ps, xy, ts, out, P, P, 1, 1, 0, 1, 0), "particle index out of range") && same(check_rollout_args(ps, xy, ts, out, -2, P, 1, 1, 0, 1, 0), "particle index out of range"));
    const char* const range = "0 <= inflate < clear_max <= 320 is required";
    EXPECT(same(check_rollout_args(ps, xy, ts, out, 0, P, 1, 1, -1, 1, 0), range) && same(check_rollout_args(ps, xy, ts, out, 0, P, 1, 1, 4, 4, 0), range));
    EXPECT(same(check_rollout_args(ps, xy, ts, out, 0, P, 1, 1, 0, 321, 0), range));
    const char* const counts = "n_poses >= 1 and n_tmpl >= 1 are required";
    EXPECT(same(check_rollout_args(ps, xy, ts, out, 0, P, 0, 1, 0, 1, 0), counts) && same(check_rollout_args(ps, xy, ts, out, 0, P, 1, 0, 0, 1, 0), counts));
    EXPECT(same(check_rollout_args(ps, xy, ts, out, 0, P, -5, 1, 0, 1, 0), counts) && same(check_rollout_args(ps, xy, ts, out, -1, P, 4, -1, 0, 1, 0), counts));
    const char* const each = "particle -1 checks pose n in particle n's map: n_poses must equal n_particles";
    EXPECT(same(check_rollout_args(ps, xy, ts, out, -1, P, 3, 1, 0, 1, 0), each) && same(check_rollout_args(ps, xy, ts, out, -1, P, 5, 1, 0, 1, 0), each));

    EXPECT(rollout_results(4096, 256) == 1048576 && rollout_results(1, 1) == 1);
    const char* const many = "n_poses * n_tmpl < 2^29 is required";
    EXPECT(same(check_rollout_results(1024, (1 << 19) - 1), nullptr) && same(check_rollout_results(1024, 1 << 19), many));
    EXPECT(same(check_rollout_results(1 << 19, 1024), many) && same(check_rollout_results((1LL << 29) - 1, 1), nullptr));
    EXPECT(same(check_rollout_results(2147483647LL, 2147483647LL), many));
}

static void test_templates() {
    RolloutBatch b;
    {   // the offset table
        const double xy[] = {0, 0, 1, 1, 2, 2};
        const int32_t good[] = {0, 1, 3}, from_one[] = {1, 2, 3}, empty[] = {0, 2, 2, 3}, back[] = {0, 2, 1, 3};
        EXPECT(rollout_templates(b, xy, good, 2, 20.0) && b.error() == nullptr && b.m_max == 2 && b.rmax == 4.0 && b.reach == 82.0);
        EXPECT(!rollout_templates(b, xy, from_one, 2, 20.0) && same(b.error(), "tmpl_start[0] must be 0"));
        EXPECT(!rollout_templates(b, xy, empty, 3, 20.0) && same(b.error(), "tmpl_start must increase strictly: template 1 has no waypoint"));
        EXPECT(!rollout_templates(b, xy, back, 3, 20.0) && same(b.error(), "tmpl_start must increase strictly: template 1 has no waypoint"));
        const std::vector<double> zeros(2 * 130, 0.0);
        const int32_t full[] = {0, 1, 129}, over[] = {0, 1, 130};
        EXPECT(rollout_templates(b, zeros.data(), full, 2, 20.0) && b.m_max == 128 && b.rmax == 0.0 && b.reach == 2.0);
        EXPECT(!rollout_templates(b, zeros.data(), over, 2, 20.0) && same(b.error(), "template 1 has more than 128 waypoints"));
    }
    {   // coordinates: the message names the template and the waypoint
        const int32_t ts[] = {0, 1, 3};
        for (double bad : {nan_, inf_, -inf_})
            for (int k = 0; k < 6; ++k) {
                double xy[] = {0, 0, 1, 1, 2, 2};
                xy[k] = bad;
                const std::string want = std::string("template ") + (k < 2 ? "0" : "1") + ", waypoint " + (k < 4 ? "0" : "1") + ": coordinates must be finite";
                EXPECT(!rollout_templates(b, xy, ts, 2, 20.0) && same(b.error(), want.c_str()));
            }
        const char* const far = "the templates reach farther than a float64 holds in cells";
        double xy[] = {0, 0, 1, 1, 1.7e308, 0};                            // finite, but 1.7e308 * 20 is not
        EXPECT(!rollout_templates(b, xy, ts, 2, 20.0) && same(b.error(), far));
        xy[4] = 1e308; xy[5] = -1e308;                                     // |lx| + |ly| is infinite already
        EXPECT(!rollout_templates(b, xy, ts, 2, 1.0) && same(b.error(), far));
    }
    {   // reach where the farthest waypoint sits on a cell boundary: ceil adds nothing there, and a whole cell an ulp beyond
        const int32_t ts[] = {0, 2};
        double xy[] = {0.0, 0.0, 0.25, 0.0};                               // 0.25 m * 20 = 5 cells exactly
        EXPECT(rollout_templates(b, xy, ts, 1, 20.0) && b.rmax == 0.25 && b.reach == 7.0);
        xy[2] = -0.125; xy[3] = 0.125;                                     // |lx| + |ly| counts, not the larger of them
        EXPECT(rollout_templates(b, xy, ts, 1, 20.0) && b.rmax == 0.25 && b.reach == 7.0);
        xy[2] = 0.0; xy[3] = -std::nextafter(0.25, 1.0);
        EXPECT(rollout_templates(b, xy, ts, 1, 20.0) && b.reach == 8.0);
        xy[3] = std::nextafter(0.25, 0.0);
        EXPECT(rollout_templates(b, xy, ts, 1, 20.0) && b.reach == 7.0);
        xy[3] = 1e-300;                                                    // any reach at all is a cell
        EXPECT(rollout_templates(b, xy, ts, 1, 20.0) && b.reach == 3.0);
    }
    {   // the step bound at its edge, (m_max - 1) * 2 * reach < 2^20, with inv = 16 so that every product is exact
        const char* const steps = "a rollout could have more than 2^20 steps: (waypoints - 1) * 2 * reach < 2^20 is required, reach = ";
        std::vector<double> xy(2 * 128, 0.0);
        const int32_t two[] = {0, 2}, full[] = {0, 128}, one[] = {0, 1};
        xy[0] = 524285.0 / 16.0;                                           // reach 524287: 2 * 524287 = 2^20 - 2
        EXPECT(rollout_templates(b, xy.data(), two, 1, 16.0) && b.reach == 524287.0);
        xy[0] = std::nextafter(524285.0 / 16.0, 1e9);                      // reach 524288: 2^20
        EXPECT(!rollout_templates(b, xy.data(), two, 1, 16.0) && same(b.error(), (std::string(steps) + "524288 cells").c_str()));
        xy[0] = 4126.0 / 16.0;                                             // reach 4128: 127 * 2 * 4128 = 2^20 - 64
        EXPECT(rollout_templates(b, xy.data(), full, 1, 16.0) && b.reach == 4128.0 && b.m_max == 128);
        xy[0] = std::nextafter(4126.0 / 16.0, 1e9);                        // reach 4129: 127 * 2 * 4129 = 2^20 + 190
        EXPECT(!rollout_templates(b, xy.data(), full, 1, 16.0) && same(b.error(), (std::string(steps) + "4129 cells").c_str()));
        xy[0] = 1e15;                                                      // a single waypoint takes no step, whatever its reach
        EXPECT(rollout_templates(b, xy.data(), one, 1, 16.0) && b.reach == 1.6e16 + 2.0);
        xy[0] = 1e300;
        EXPECT(!rollout_templates(b, xy.data(), two, 1, 16.0) && same(b.error(), (std::string(steps) + "9000000000000000000 cells").c_str()));
    }
}

static void test_poses() {
    // cells per metre 20; the lattice holds the cells -1400 <= X, Y < 1400; the templates reach 7 cells
    const double inv = 20.0;
    const long long lo = -1400, hi = 1400;
    RolloutBatch b;
    const int32_t ts[] = {0, 2};
    const double xy[] = {0.0, 0.0, 0.25, 0.0};
    EXPECT(rollout_templates(b, xy, ts, 1, inv) && b.reach == 7.0);
    {
        double ps[] = {0, 0, 0, 1, -2, 3.5, -69.6, 69.6, -7.0};
        EXPECT(rollout_poses(b, ps, 3, inv, lo, hi) && b.error() == nullptr);
        for (double bad : {nan_, inf_, -inf_})
            for (int k = 0; k < 9; ++k) {
                double q[9];
                memcpy(q, ps, sizeof q);
                q[k] = bad;
                EXPECT(!rollout_poses(b, q, 3, inv, lo, hi) && same(b.error(), ("pose " + std::to_string(k / 3) + " must be finite").c_str()));
            }
    }
    // the cell of the pose exactly `reach` cells from each edge, and one cell beyond: cells lo + 7 = -1393 and hi - 1 - 7 = 1392
    const double first = -1393 / inv + 0.01, last = 1392 / inv + 0.01, below = -1394 / inv + 0.01, above = 1393 / inv + 0.01;
    EXPECT(rollout_pose_ok(first, 0, inv, 7.0, lo, hi) && rollout_pose_ok(last, 0, inv, 7.0, lo, hi) && rollout_pose_ok(0, first, inv, 7.0, lo, hi) && rollout_pose_ok(0, last, inv, 7.0, lo, hi));
    EXPECT(rollout_pose_ok(first, last, inv, 7.0, lo, hi) && rollout_pose_ok(last, first, inv, 7.0, lo, hi));
    EXPECT(!rollout_pose_ok(below, 0, inv, 7.0, lo, hi) && !rollout_pose_ok(above, 0, inv, 7.0, lo, hi) && !rollout_pose_ok(0, below, inv, 7.0, lo, hi) && !rollout_pose_ok(0, above, inv, 7.0, lo, hi));
    EXPECT(!rollout_pose_ok(1e300, 0, inv, 7.0, lo, hi) && !rollout_pose_ok(0, -1.7e308, inv, 7.0, lo, hi) && !rollout_pose_ok(0, 0, inv, 1.6e16, lo, hi));
    EXPECT(rollout_pose_ok(0, 0, inv, 1399.0, lo, hi) && !rollout_pose_ok(0, 0, inv, 1400.0, lo, hi));
    EXPECT(rollout_pose_ok(-0.01, -0.01, inv, 1399.0, lo, hi) && !rollout_pose_ok(0.06, 0, inv, 1399.0, lo, hi) && !rollout_pose_ok(0, -0.06, inv, 1399.0, lo, hi));   // cells -1, 1 and -2
    const char* const outside = "pose 2: the templates placed there could leave the tile lattice (reach 7 cells; raise lattice_radius)";
    for (double edge : {below, above, 1e300, -1.7e308}) {
        double ps[] = {0, 0, 0, first, last, 1.0, 0, edge, 2.0, 0, 0, 0};
        EXPECT(!rollout_poses(b, ps, 4, inv, lo, hi) && same(b.error(), outside));
        ps[7] = first;
        EXPECT(rollout_poses(b, ps, 4, inv, lo, hi));
    }
}

// 10^5 and more (pose, heading, waypoint) triples the pose test accepts, a third of them with the pose's cell exactly `reach` cells
// from an edge of the lattice, the waypoints out to |lx| + |ly| = rmax: the placed cell lies in the lattice, within reach of the pose's.
static void test_placement_stays_inside() {
    std::mt19937_64 rng(20240521);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    struct Case { double inv; long long lo, hi; double rmax; };
    const Case cases[] = {{20.0, -1400, 1400, 0.25}, {20.0, -1400, 1400, 7.3}, {10.0, -600, 600, 3.0}, {16.0, -4096, 4096, 200.0},
                          {20.0, -(1LL << 30), 1LL << 30, 12.5}, {20.0, -(1LL << 30), 1LL << 30, 0.0}, {1.0 / 3.0, -50, 50, 17.0}};
    long long accepted = 0, at_edge = 0;
    for (const Case& c : cases) {
        const double reach = ceil(c.rmax * c.inv) + 2.0;
        const long long first = c.lo + (long long)reach, last = c.hi - 1 - (long long)reach;
        EXPECT(first <= last);
        for (int it = 0; it < 30000; ++it) {
            long long cell[2];
            double p[2];
            for (int k = 0; k < 2; ++k) {
                const int where = (int)(unit(rng) * 6);                  // 0, 1: an edge; else anywhere between
                cell[k] = where == 0 ? first : where == 1 ? last : first + (long long)(unit(rng) * (double)(last - first + 1));
                const int f = (int)(unit(rng) * 4);
                const double frac = f == 0 ? 0.0 : f == 1 ? std::nextafter(1.0, 0.0) : unit(rng);
                p[k] = ((double)cell[k] + frac) / c.inv;
            }
            if (!rollout_pose_ok(p[0], p[1], c.inv, reach, c.lo, c.hi)) continue;      // the division's rounding moved the pose over the edge
            const double fx = floor(p[0] * c.inv), fy = floor(p[1] * c.inv);
            const int h = (int)(unit(rng) * 12);
            const double th = h < 8 ? (h - 4) * 0.78539816339744830962 : (unit(rng) * 2.0 - 1.0) * 3.14159265358979323846;
            const int w = (int)(unit(rng) * 4);                           // on an axis, on the diagonal of the diamond, or inside it
            const double u = unit(rng) * 2.0 - 1.0, share = unit(rng);
            double lx = w == 0 ? c.rmax : w == 1 ? 0.0 : w == 2 ? share * c.rmax : u * c.rmax;
            double ly = w == 0 ? 0.0 : w == 1 ? -c.rmax : w == 2 ? c.rmax - share * c.rmax : (unit(rng) * 2.0 - 1.0) * (c.rmax - fabs(u * c.rmax));
            if (unit(rng) < 0.5) lx = -lx;
            if (!(fabs(lx) + fabs(ly) <= c.rmax)) continue;               // the sum's rounding: rmax is the largest such sum by definition
            long long X, Y;
            rollout_place(p[0], p[1], cos(th), sin(th), lx, ly, c.inv, X, Y);
            ++accepted;
            if (fx == (double)first || fx == (double)last || fy == (double)first || fy == (double)last) ++at_edge;
            const bool inside = X >= c.lo && X < c.hi && Y >= c.lo && Y < c.hi;
            const bool near = fabs((double)X - fx) <= reach && fabs((double)Y - fy) <= reach;
            if (!inside || !near) {
                ++failures;
                fprintf(stderr, "placement: pose (%.17g, %.17g, %.17g) waypoint (%.17g, %.17g) inv %.17g -> cell (%lld, %lld), lattice [%lld, %lld), reach %.0f\n",
                        p[0], p[1], th, lx, ly, c.inv, X, Y, c.lo, c.hi, reach);
            }
        }
    }
    EXPECT(accepted >= 100000 && at_edge >= 20000);
}

int main() {
    test_scalar_checks();
    test_templates();
    test_poses();
    test_placement_stays_inside();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("rolloutbatch ok");
    return 0;
}
