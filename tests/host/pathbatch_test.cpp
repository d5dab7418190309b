// The host side of rbpf_check_paths, thesis_amd/csrc/rbpf_pathbatch.h, run on the CPU under -fsanitize=address,undefined
// (tests/test_pathbatch_host.py compiles and starts this program).  Every expected number is a literal worked out by hand from
// the specification in include/rbpf_hip.h; the walk is checked against an incremental Bresenham written out here.
#include "rbpf_pathbatch.h"

#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static bool same(const char* got, const char* want) { return want ? got && strcmp(got, want) == 0 : got == nullptr; }

static void test_scalar_checks() {
    const double xy[2] = {0, 0};
    const int32_t ps[2] = {0, 1};
    int32_t out[4];
    const int P = 4;
    EXPECT(same(check_path_args(xy, ps, out, 0, P, 1, 0, 1, 0), nullptr) && same(check_path_args(xy, ps, out, -1, P, 8, 20, 320, 15), nullptr));
    EXPECT(same(check_path_args(nullptr, ps, out, 0, P, 1, 0, 1, 0), "xy, path_start or out is NULL"));
    EXPECT(same(check_path_args(xy, nullptr, out, 0, P, 1, 0, 1, 0), "xy, path_start or out is NULL"));
    EXPECT(same(check_path_args(xy, ps, nullptr, 0, P, 1, 0, 1, 0), "xy, path_start or out is NULL"));
    EXPECT(same(check_path_args(xy, ps, out, 0, P, 1, 0, 1, 16), "unknown flags"));
    EXPECT(same(check_path_args(xy, ps, out, P, P, 1, 0, 1, 0), "particle index out of range") && same(check_path_args(xy, ps, out, -2, P, 1, 0, 1, 0), "particle index out of range"));
    const char* const range = "0 <= inflate < clear_max <= 320 is required";
    EXPECT(same(check_path_args(xy, ps, out, 0, P, 1, -1, 1, 0), range) && same(check_path_args(xy, ps, out, 0, P, 1, 4, 4, 0), range));
    EXPECT(same(check_path_args(xy, ps, out, 0, P, 1, 0, 321, 0), range) && same(check_path_args(xy, ps, out, 0, P, 1, 319, 320, 0), nullptr));
    EXPECT(same(check_path_args(xy, ps, out, 0, P, 0, 0, 1, 0), "n_paths >= 1 is required") && same(check_path_args(xy, ps, out, 0, P, -3, 0, 1, 0), "n_paths >= 1 is required"));
    EXPECT(same(check_path_args(xy, ps, out, 2, P, 8, 0, 1, PATHS_OWN), "RBPF_PATHS_OWN needs particle -1"));
    EXPECT(same(check_path_args(xy, ps, out, -1, P, 6, 0, 1, PATHS_OWN), "with RBPF_PATHS_OWN n_paths must be a multiple of the number of particles"));
    EXPECT(same(check_path_args(xy, ps, out, -1, P, 4, 0, 1, PATHS_OWN | PATHS_START_EXEMPT), nullptr));

    EXPECT(path_results(2, 4096, 1000, 0) == 1000 && path_results(-1, 4096, 1000, 0) == 4096000 && path_results(-1, 4096, 8192, PATHS_OWN) == 8192);
    const char* const many = "n_particles * n_paths < 2^29 is required (n_paths < 2^29 for one map or with RBPF_PATHS_OWN)";
    EXPECT(same(check_path_results(-1, 65536, 8191, 0), nullptr) && same(check_path_results(-1, 65536, 8192, 0), many));
    EXPECT(same(check_path_results(3, 65536, 8192, 0), nullptr) && same(check_path_results(-1, 65536, 65536 * 4096LL, PATHS_OWN), nullptr));
    EXPECT(same(check_path_results(0, 1, (1LL << 29) - 1, 0), nullptr) && same(check_path_results(0, 1, 1LL << 29, 0), many));
    EXPECT(path_group_size(12, 4, PATHS_OWN) == 3 && path_group_size(6, 6, PATHS_OWN | PATHS_DEVICE_OUT) == 1 && path_group_size(12, 4, PATHS_START_EXEMPT) == 0);
}

static void test_build() {
    // cells per metre 20; the lattice holds the cells -1400 <= X, Y < 1400 (three tiles of 800 and a half on either side)
    const double inv = 20.0;
    const long long lo = -1400, hi = 1400;
    PathBatch b;
    {   // three paths: a bend with a repeated waypoint, a single point, a diagonal back to its first cell
        const double xy[] = {0.26, -0.01, 0.26, -0.01, 0.41, 0.12, 0.41, 0.64,   -70.0, 69.99,   1.0, 1.0, 1.26, 0.74, 1.0, 1.0};
        const int32_t ps[] = {0, 4, 5, 8};
        EXPECT(path_batch_build(b, xy, ps, 3, inv, lo, hi) && b.error() == nullptr);
        const std::vector<int32_t> cells = {1405, 1399, 1405, 1399, 1408, 1402, 1408, 1412,   0, 2799,   1420, 1420, 1425, 1414, 1420, 1420};
        const std::vector<int32_t> wstep = {0, 0, 3, 13, 0, 0, 6, 12}, steps = {14, 1, 13};
        EXPECT(b.cells == cells && b.wstep == wstep && b.steps == steps);
    }
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    {   // the offset table
        const double xy[] = {0, 0, 1, 1, 2, 2};
        const int32_t from_one[] = {1, 2, 3}, empty[] = {0, 2, 2, 3}, back[] = {0, 2, 1, 3};
        EXPECT(!path_batch_build(b, xy, from_one, 2, inv, lo, hi) && same(b.error(), "path_start[0] must be 0"));
        EXPECT(!path_batch_build(b, xy, empty, 3, inv, lo, hi) && same(b.error(), "path_start must increase strictly: path 1 has no waypoint"));
        EXPECT(!path_batch_build(b, xy, back, 3, inv, lo, hi) && same(b.error(), "path_start must increase strictly: path 1 has no waypoint"));
    }
    {   // coordinates: the message names the path and the waypoint
        const int32_t ps[] = {0, 1, 3};
        for (double bad : {nan, inf, -inf})
            for (int k = 0; k < 6; ++k) {
                double xy[] = {0, 0, 1, 1, 2, 2};
                xy[k] = bad;
                const std::string want = std::string("path ") + (k < 2 ? "0" : "1") + ", waypoint " + (k < 4 ? "0" : "1") + ": coordinates must be finite";
                EXPECT(!path_batch_build(b, xy, ps, 2, inv, lo, hi) && same(b.error(), want.c_str()));
            }
        const char* const outside = "path 1, waypoint 1: its cell lies outside the tile lattice (raise lattice_radius)";
        for (double edge : {70.0, -70.01, 1e300, -1e300, 1.7e308}) {       // 1.7e308 * 20 is infinite
            double xy[] = {0, 0, 1, 1, 2, edge};
            EXPECT(!path_batch_build(b, xy, ps, 2, inv, lo, hi) && same(b.error(), outside));
        }
        double xy[] = {0, 0, 1, 1, 69.99, -70.0};                          // the lattice's last and first cell
        EXPECT(path_batch_build(b, xy, ps, 2, inv, lo, hi) && b.cells[4] == 2799 && b.cells[5] == 0 && b.steps[1] == 1 + 1420);
    }
    {   // 2^20 steps are the most: a zigzag over 2047 cells, 512 times and once more
        const long long lo2 = 0, hi2 = 4096;
        std::vector<double> xy;
        std::vector<int32_t> ps = {0};
        for (int k = 0; k <= 512; ++k) { xy.push_back(k % 2 ? 2047.5 : 0.5); xy.push_back(3.5); }
        xy.push_back(0.5 + 62); xy.push_back(3.5);                         // the last leg: 62 cells on from X = 0
        ps.push_back((int32_t)(xy.size() / 2));
        EXPECT(path_batch_build(b, xy.data(), ps.data(), 1, 1.0, lo2, hi2) && b.steps[0] == 512 * 2047 + 62 + 1);
        xy[xy.size() - 2] = 0.5 + 62 + 449;                                // 512 * 2047 + 511 = 2^20 - 1: 2^20 steps exactly
        EXPECT(path_batch_build(b, xy.data(), ps.data(), 1, 1.0, lo2, hi2) && b.steps[0] == (1 << 20));
        xy[xy.size() - 2] = 0.5 + 62 + 450;
        EXPECT(!path_batch_build(b, xy.data(), ps.data(), 1, 1.0, lo2, hi2) && same(b.error(), "path 0 has more than 2^20 steps"));
    }
}

// an incremental Bresenham: the error term in units of 1 / (2 n) starts at a half and carries the minor axis at 2 n
static void walk(int32_t xa, int32_t ya, int32_t xb, int32_t yb, std::vector<int32_t>& out) {
    const long long ax = llabs((long long)xb - xa), ay = llabs((long long)yb - ya), n = std::max(ax, ay);
    const int32_t sx = xb >= xa ? 1 : -1, sy = yb >= ya ? 1 : -1;
    long long err = n;
    int32_t x = xa, y = ya;
    out = {x, y};
    for (long long t = 0; t < n; ++t) {
        if (ax >= ay) { x += sx; err += 2 * ay; if (err >= 2 * n) { err -= 2 * n; y += sy; } }
        else { y += sy; err += 2 * ax; if (err >= 2 * n) { err -= 2 * n; x += sx; } }
        out.push_back(x); out.push_back(y);
    }
}

static void test_segment_cells() {
    std::vector<int32_t> want;
    auto same_walk = [&](int32_t xa, int32_t ya, int32_t xb, int32_t yb) {
        walk(xa, ya, xb, yb, want);
        const int32_t n = (int32_t)(want.size() / 2) - 1;
        bool ok = true;
        for (int32_t t = 0; t <= n && ok; ++t) {
            int32_t x, y;
            path_segment_cell(xa, ya, xb, yb, t, x, y);
            ok = x == want[2 * t] && y == want[2 * t + 1];
        }
        return ok;
    };
    for (int dx = -12; dx <= 12; ++dx)
        for (int dy = -12; dy <= 12; ++dy)
            if (dx || dy) EXPECT(same_walk(5, 7, 5 + dx, 7 + dy));
    // the longest segments a path may hold: 2 t a reaches 2^41, beyond 32 bits
    const int32_t far = (1 << 20) - 1;
    EXPECT(same_walk(0, 0, far, far - 1) && same_walk(far, 3, 0, far / 2 + 3) && same_walk(0, far, far / 3, 0) && same_walk(17, 0, 17, far));
    EXPECT(same_walk(0, 0, far, 1) && same_walk(0, 0, far, far) && same_walk(far, far, 0, 1));
    int32_t x, y;
    path_segment_cell(0, 0, far, far - 1, far, x, y);
    EXPECT(x == far && y == far - 1);
}

int main() {
    test_scalar_checks();
    test_build();
    test_segment_cells();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("pathbatch ok");
    return 0;
}
