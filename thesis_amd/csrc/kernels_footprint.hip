// kernels_footprint.hip -- rollout checks with an oriented footprint (include/rbpf_hip.h, rbpf_check_footprints).
//
// One wave works on one (pose or particle, template), four waves to a 256-lane workgroup.  The lanes place the template's
// waypoints and form their steps by a wave-wide prefix sum, as check_rollouts_kernel does (kernels_paths.hip), and store the
// heading bin of every waypoint, (pose bin + template bin) mod H, beside them in LDS.  Lane l then takes the steps l, l + 64, ...:
// the segment by the binary search, the centre cell by path_cell, the inscribed-radius test by path_clearance, and then the
// bins the step tests and their spans.  A span lies along y, the contiguous axis of a tile row: its occupied cells are one
// occ_run64, its unknown and not-known-free cells come from the int8 row a 4-byte word at a time.
//
// The span table is read from memory, a span one packed word: the lanes of a wave stand on different steps and so in different
// bins, which a bin staged in LDS cannot serve, and lanes in the same bin read the same word (one request).  The table of a call
// is a few KB that every wave reads; it stays in the caches.
#include "rbpf_pathwalk.h"

namespace rbpf {

typedef uint32_t __attribute__((may_alias)) cell_word;

// Of the n <= 64 cells of lattice row u from column w0 on: bit k of `zero` = cell (u, w0 + k) has v == 0, of `nonneg` = it has
// v >= 0.  v is 0 outside the lattice and without a tile.  A tile's part is read as aligned 4-byte words of the pool (the pool
// is an allocation of its own, so the word that holds a cell of it lies in it) and the bytes outside the part are masked off.
__device__ __forceinline__ void val_run64(const DevView& v, const int32_t* __restrict__ tab, int u, int w0, int n, uint64_t& zero, uint64_t& nonneg) {
    const int dim = v.dim, edge = v.L * dim;
    zero = nonneg = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    if (u < 0 || u >= edge) return;
    const int a = u / dim, i = u - a * dim, hi = min(w0 + n, edge);
    for (int w = max(w0, 0); w < hi; ) {
        const int b = w / dim, j = w - b * dim, end = min((b + 1) * dim, hi);      // the end of this tile's part, or of the run
        const int tile = tab[a * v.L + b];
        if (tile >= 0) {
            const uintptr_t p0 = (uintptr_t)(v.pool + (size_t)tile * dim * dim + (size_t)i * dim + j), p1 = p0 + (uintptr_t)(end - w);
            for (uintptr_t q = p0 & ~(uintptr_t)3; q < p1; q += 4) {
                const uint32_t x = *reinterpret_cast<const cell_word*>(q);
                const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;      // bit 7 of a byte: the byte is not 0
                uint32_t not_zero = (((nz >> 7) * 0x01020408u) >> 24) & 15u;                    // bit k: byte k (no carries: the partial products do not meet)
                uint32_t negative = ((((x & 0x80808080u) >> 7) * 0x01020408u) >> 24) & 15u;
                uint32_t keep = 15u;
                if (q < p0) keep &= 15u << (int)(p0 - q);
                if (p1 - q < 4) keep &= (1u << (int)(p1 - q)) - 1u;
                not_zero &= keep; negative &= keep;
                const int sh = (int)((long long)q - (long long)p0) + (w - w0);                  // the bit of byte 0; >= -3, and >= 0 where a kept byte needs it
                if (sh >= 0) { zero &= ~((uint64_t)not_zero << sh); nonneg &= ~((uint64_t)negative << sh); }
                else { zero &= ~((uint64_t)not_zero >> -sh); nonneg &= ~((uint64_t)negative >> -sh); }
            }
        }
        w = end;
    }
}

__global__ __launch_bounds__(64 * PATH_WAVES) void check_footprints_kernel(DevView v, FootArgs a) {
    __shared__ int32_t s_step[PATH_WAVES][PATH_STAGE];
    __shared__ int32_t s_cell[PATH_WAVES][PATH_STAGE][2];
    __shared__ int32_t s_bin[PATH_WAVES][PATH_STAGE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * PATH_WAVES + wv;          // the result this wave writes
    const bool live = r < a.pairs;
    const int row = live ? (int)(r / a.n_tmpl) : 0, k = live ? (int)(r - (long long)row * a.n_tmpl) : 0;
    const int n = a.one_pose ? 0 : row;                                   // the pose; the map is that of `particle`, or of particle `row`
    const int first = live ? a.tmpl_start[k] : 0, nw = live ? a.tmpl_start[k + 1] - first : 0;      // nw <= PATH_STAGE: the host checked
    if (live) {
        const double2 ps = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)n], cs = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)n + 1];
        const double2* __restrict__ xy = reinterpret_cast<const double2*>(a.tmpl_xy) + first;
        const int pb = a.pose_bin[n];
        int carry = 0, lx = 0, ly = 0;                                      // the step and the cell of the waypoint before this round's first
        for (int base = 0; base < nw; base += 64) {                        // nw is the wave's: every lane runs every round
            const int j = base + lane;
            int cx = 0, cy = 0;
            if (j < nw) {
                const double2 q = xy[j];
                const double wx = __dadd_rn(ps.x, __dsub_rn(__dmul_rn(cs.x, q.x), __dmul_rn(cs.y, q.y)));
                const double wy = __dadd_rn(ps.y, __dadd_rn(__dmul_rn(cs.y, q.x), __dmul_rn(cs.x, q.y)));
                cx = (int)__builtin_floor(__dmul_rn(wx, a.inv)) + a.off;
                cy = (int)__builtin_floor(__dmul_rn(wy, a.inv)) + a.off;
            }
            int qx = __shfl_up(cx, 1, 64), qy = __shfl_up(cy, 1, 64);      // the waypoint before this lane's
            if (lane == 0) { qx = base ? lx : cx; qy = base ? ly : cy; }
            int sum = j < nw ? max(abs(cx - qx), abs(cy - qy)) : 0;        // the segment that ends at waypoint j; 0 for waypoint 0
            for (int off = 1; off < 64; off <<= 1) {                       // inclusive prefix sum over the wave
                const int t = __shfl_up(sum, off, 64);
                if (lane >= off) sum += t;
            }
            sum += carry;
            if (j < nw) {
                int bin = pb + a.tmpl_bin[first + j];                      // both in [0, H)
                if (bin >= a.n_bins) bin -= a.n_bins;
                s_step[wv][j] = sum; s_cell[wv][j][0] = cx; s_cell[wv][j][1] = cy; s_bin[wv][j] = bin;
            }
            carry = __shfl(sum, 63, 64); lx = __shfl(cx, 63, 64); ly = __shfl(cy, 63, 64);      // read only if a round follows: lane 63 held a waypoint
        }
    }
    __syncthreads();
    if (!live) return;
    const int p = a.particle >= 0 ? a.particle : row;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    const int dim = v.dim, E = a.exempt;
    const int x0 = s_cell[wv][0][0], y0 = s_cell[wv][0][1];
    const int S = s_step[wv][nw - 1] + 1;
    int blocked = INT32_MAX, unknown = INT32_MAX, clear = a.clear_max, n_unknown = 0;
    for (int s = lane; s < S; s += 64) {
        // the centre, and the waypoints [j0, j1] whose bins the step tests
        int x = x0, y = y0, j0 = 0, j1 = 0;
        if (s > 0) {
            int lo = 1, hi = nw - 1;                      // the first waypoint j with step j >= s: the step lies on segment j - 1 -> j
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_step[wv][mid] < s) lo = mid + 1; else hi = mid; }
            const int sa = s_step[wv][lo - 1], sb = s_step[wv][lo];
            path_cell(s_cell[wv][lo - 1][0], s_cell[wv][lo - 1][1], s_cell[wv][lo][0], s_cell[wv][lo][1], s - sa, x, y);
            j0 = j1 = sb == s || 2 * (s - sa) >= sb - sa ? lo : lo - 1;      // on waypoint lo, or strictly between: the nearer end, the later at the middle
        }
        if (s_step[wv][j1] == s) while (j1 + 1 < nw && s_step[wv][j1 + 1] == s) ++j1;      // every waypoint the step stands on
        const int ta = x / dim, tb = y / dim, tile = tab[ta * v.L + tb];   // the centre lies in the lattice (the host sees to it)
        const int val = tile >= 0 ? (int)v.pool[(size_t)tile * dim * dim + (size_t)(x - ta * dim) * dim + (y - tb * dim)] : 0;
        const int d = path_clearance(v, tab, x, y, a.clear_max);
        const bool centre_exempt = E >= 0 && abs(x - x0) <= E && abs(y - y0) <= E;
        bool bad = !centre_exempt && ((!a.through_unknown && val >= 0) || d <= a.inflate);      // an occupied centre has d = 0
        bool unk = val == 0;
        int last = -1;
        for (int j = j0; j <= j1; ++j) {
            const int bin = s_bin[wv][j];
            if (bin == last) continue;                    // a waypoint held with its heading: the same cells again
            last = bin;
            const int k0 = a.fp_start[bin], k1 = a.fp_start[bin + 1];
            for (int q = k0; q < k1; ++q) {
                const int32_t sp = a.fp_span[q];
                const int u = x + (int)(int8_t)(sp & 255), w0 = y + (int)(int8_t)((sp >> 8) & 255), nn = (int)(int8_t)((sp >> 16) & 255) - (int)(int8_t)((sp >> 8) & 255) + 1;
                uint64_t zero, nonneg;
                val_run64(v, tab, u, w0, nn, zero, nonneg);
                uint64_t stop = a.through_unknown ? occ_run64(v, tab, u, w0, nn) : nonneg;
                if (E >= 0 && abs(u - x0) <= E) {          // the columns y0 - E .. y0 + E of this row are exempt
                    const int c0 = max(w0, y0 - E) - w0, c1 = min(w0 + nn - 1, y0 + E) - w0;
                    if (c0 <= c1) stop &= ~((c1 - c0 >= 63 ? ~0ull : (1ull << (c1 - c0 + 1)) - 1ull) << c0);
                }
                bad = bad || stop != 0ull;
                unk = unk || zero != 0ull;
            }
        }
        if (bad) blocked = min(blocked, s);
        if (unk) { unknown = min(unknown, s); ++n_unknown; }
        clear = min(clear, d);
    }
    for (int off = 32; off > 0; off >>= 1) {
        blocked = min(blocked, __shfl_down(blocked, off, 64));
        unknown = min(unknown, __shfl_down(unknown, off, 64));
        clear = min(clear, __shfl_down(clear, off, 64));
        n_unknown += __shfl_down(n_unknown, off, 64);
    }
    if (lane == 0) {
        int32_t* __restrict__ o = a.out + 4 * (size_t)r;
        o[0] = blocked == INT32_MAX ? -1 : blocked; o[1] = unknown == INT32_MAX ? -1 : unknown; o[2] = clear; o[3] = n_unknown;
        if (a.steps) a.steps[r] = S;
    }
}

void launch_check_footprints(const DevView& v, const FootArgs& a, hipStream_t s) {
    check_footprints_kernel<<<(unsigned)((a.pairs + PATH_WAVES - 1) / PATH_WAVES), 64 * PATH_WAVES, 0, s>>>(v, a);
}

}  // namespace rbpf
