// kernels_modes.hip -- pose modes: the connected components of a set of weighted poses on a lattice of bin_xy x bin_xy x 2 pi / n_th
// bins, and one estimate row per component (include/rbpf_hip.h, rbpf_pose_modes and rbpf_track_modes; the specification is DESIGN 3.21).
//
//   pose_modes_kernel      one workgroup: the filter's current poses.
//   track_modes_kernel     one workgroup per record: the poses the current particles' ancestors had at that record (the lineage
//                          table of the walk back, kernels_track.hip), with the FINAL weights.
// Both run modes_set: keys -> bin table -> union-find -> labels and tallies -> selection -> rows, workgroup barriers in between.
// The tables of a set lie in global scratch (rbpf_internal.h, ModesArgs) and stay in L2.  What lanes exchange through them is
// written by integer atomics or before a barrier and read past the lane's L1 (ld below); every result is a set membership, a
// minimum or an integer sum, so the order in which the atomics land cannot change an output.  No floating-point atomics, no
// waiting on anyone: every loop is bounded by the table or the particle count.
#include "rbpf_estrow.h"

namespace rbpf {

static const unsigned long long KEY_EMPTY = ~0ull;   // a key has its top 4 bits clear
static const int NO_ROOT = 0x7fffffff;
static const long long XY_BIAS = 1ll << 23;

template <class T>
__device__ __forceinline__ T ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct ModeTables {
    unsigned long long* keys; unsigned long long* Q;
    int32_t* broot; int32_t* up; int32_t* pslot; int32_t* cnt; int32_t* nb; int32_t* lab;
};
__device__ __forceinline__ ModeTables mode_tables(const ModesArgs& a, int set) {
    unsigned char* b = a.tables + (size_t)set * modes_set_bytes(a.P, a.S);
    ModeTables t;
    t.keys = reinterpret_cast<unsigned long long*>(b);
    t.Q = t.keys + a.S;
    t.broot = reinterpret_cast<int32_t*>(t.Q + a.P);
    t.up = t.broot + a.S; t.pslot = t.up + a.P; t.cnt = t.pslot + a.P; t.nb = t.cnt + a.P;
    t.lab = a.label ? a.label : reinterpret_cast<int32_t*>(b + modes_label_offset(a.P, a.S));
    return t;
}

// the bin of a contributing particle as one key: ix + 2^23 (24 bits) | iy + 2^23 (24 bits) | it (12 bits); false: it contributes nothing
__device__ __forceinline__ bool bin_key(const ModesArgs& a, double w, double x, double y, double th, unsigned long long& key) {
    if (!est_used(w, x, y, th)) return false;
    const double fx = x * a.inv, fy = y * a.inv, ft = th * a.kth;
    if (!(fabs(fx) < 8388608.0 && fabs(fy) < 8388608.0 && fabs(ft) < 1099511627776.0)) return false;
    const long long ix = (long long)floor(fx) + XY_BIAS, iy = (long long)floor(fy) + XY_BIAS;
    long long it = (long long)floor(ft) % a.n_th;
    if (it < 0) it += a.n_th;
    key = ((unsigned long long)ix << 36) | ((unsigned long long)iy << 12) | (unsigned long long)it;
    return true;
}

__device__ __forceinline__ unsigned slot_hash(unsigned long long k, int S) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k & (unsigned)(S - 1);
}

// the slot that holds `key`, claimed if nobody has it yet; the table is at most half full, so a free slot is met within S probes
__device__ __forceinline__ int claim_slot(unsigned long long* keys, int S, unsigned long long key) {
    unsigned s = slot_hash(key, S);
    for (int i = 0; i < S; ++i) {
        const unsigned long long prev = atomicCAS(&keys[s], KEY_EMPTY, key);
        if (prev == KEY_EMPTY || prev == key) return (int)s;
        s = (s + 1) & (unsigned)(S - 1);
    }
    return -1;
}
__device__ __forceinline__ int find_slot(const unsigned long long* keys, int S, unsigned long long key) {
    unsigned s = slot_hash(key, S);
    for (int i = 0; i < S; ++i) {
        const unsigned long long k = ld(keys + s);
        if (k == key) return (int)s;
        if (k == KEY_EMPTY) return -1;
        s = (s + 1) & (unsigned)(S - 1);
    }
    return -1;
}

// up[r] <= r always, so a chain ends at its smallest element after at most `bound` steps
__device__ __forceinline__ int find_root(const int32_t* up, int x, int bound) {
    for (int i = 0; i < bound; ++i) {
        const int p = ld(up + x);
        if (p == x) break;
        x = p;
    }
    return x;
}
// Hooks the larger root under the smaller.  If somebody got to `a` first (old != a), a now hangs under min(old, b) and the pair
// (old, b) is still to be joined: a' + b < a + b, so the loop ends by itself.  True: a hook was tried, the round is not the last
__device__ __forceinline__ bool unite(int32_t* up, int a, int b, int bound) {
    bool hooked = false;
    for (int i = 0; i < bound; ++i) {
        a = find_root(up, a, bound); b = find_root(up, b, bound);
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&up[a], b);
        hooked = true;
        if (old == a) break;
        a = old;
    }
    return hooked;
}

// Whole workgroup of TT lanes.  pose(j, x, y, th) gives the pose of particle j of the set
template <class Pose>
__device__ void modes_set(const ModesArgs& a, int set, Pose pose) {
    __shared__ double s_red[TW * EST_SUMS * 2];
    __shared__ int s_arg[TW];
    __shared__ unsigned long long s_q[TW];
    __shared__ unsigned long long s_qtot;
    __shared__ int s_cnt[3];                             // contributing particles, bins, modes
    __shared__ int s_changed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = a.P, S = a.S;
    const ModeTables t = mode_tables(a, set);

    for (int s = tid; s < S; s += TT) { t.keys[s] = KEY_EMPTY; t.broot[s] = NO_ROOT; }
    for (int j = tid; j < P; j += TT) { t.Q[j] = 0; t.up[j] = j; t.cnt[j] = 0; t.nb[j] = 0; }
    if (tid == 0) { s_qtot = 0; s_cnt[0] = s_cnt[1] = s_cnt[2] = 0; }
    int unused;
    const EffWeight weight_of = weights_scan(P, a.w_raw, a.w_given, a.mode, EveryParticle(), unused, s_red, s_arg);   // barriers: the tables are clear

    // 1, 2. keys into the bin table, the bin's root = its smallest particle; wmax.  Along a wave, a run of lanes with one key (a
    // converged cloud: the whole wave) sends its head alone to the table: the head holds the run's smallest index
    double wmax = 0.0;
    for (int base = 0; base < P; base += TT) {
        const int j = base + tid;
        unsigned long long key = KEY_EMPTY;             // no particle here, or one that contributes nothing
        if (j < P) {
            double x, y, th;
            pose(j, x, y, th);
            const double w = weight_of(j);
            if (bin_key(a, w, x, y, th, key)) wmax = fmax(wmax, w);
        }
        const unsigned long long before = __shfl_up(key, 1, 64);
        const bool head = key != KEY_EMPTY && (lane == 0 || before != key);
        int slot = -1;
        if (head && (slot = claim_slot(t.keys, S, key)) >= 0) atomicMin(&t.broot[slot], j);
        const unsigned long long heads = __ballot(head) & (~0ull >> (63 - lane));   // the heads at or below this lane
        slot = __shfl(slot, heads ? 63 - __clzll((long long)heads) : lane, 64);
        if (j < P) t.pslot[j] = key != KEY_EMPTY ? slot : -1;
    }
    for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, o, 64));
    __syncthreads();                                     // the last use of s_red is over; the table is complete
    if (lane == 0) s_red[wave] = wmax;
    __syncthreads();
    for (int w = 0; w < TW; ++w) wmax = fmax(wmax, s_red[w]);

    // 3. union-find over the occupied bins, a bin standing for its root.  A round joins every bin to its 13 forward neighbours
    // and then points every bin at its tree's root; the round that hooks nothing is the proof that all are joined
    for (int round = 0; round <= P; ++round) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        bool hooked = false;
        for (int j = tid; j < P; j += TT) {
            const int s = t.pslot[j];
            if (s < 0 || ld(t.broot + s) != j) continue; // one lane per bin: the one that holds its root
            const unsigned long long key = ld(t.keys + s);
            const long long ix = (long long)(key >> 36), iy = (long long)((key >> 12) & 0xffffff);
            const int it = (int)(key & 0xfff);
            for (int n = 14; n < 27; ++n) {              // (dx, dy, dt) after (0, 0, 0) in lexicographic order
                const int dx = n / 9 - 1, dy = (n / 3) % 3 - 1, dt = n % 3 - 1;
                const long long nx = ix + dx, ny = iy + dy;
                if (nx < 0 || nx >= 2 * XY_BIAS || ny < 0 || ny >= 2 * XY_BIAS) continue;
                int nt = it + dt;
                if (nt < 0) nt += a.n_th; else if (nt >= a.n_th) nt -= a.n_th;
                const int ns = find_slot(t.keys, S, ((unsigned long long)nx << 36) | ((unsigned long long)ny << 12) | (unsigned long long)nt);
                if (ns >= 0 && ns != s) hooked |= unite(t.up, j, ld(t.broot + ns), P);
            }
        }
        if (hooked) s_changed = 1;
        __syncthreads();
        const int changed = s_changed;
        for (int j = tid; j < P; j += TT) {
            const int s = t.pslot[j];
            if (s < 0 || ld(t.broot + s) != j) continue;
            const int r = find_root(t.up, j, P);
            if (r != j) __hip_atomic_store(t.up + j, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (!changed) break;
    }

    // 4. labels and tallies: integer atomics only
    int n_used = 0, n_bins = 0, n_modes = 0;
    unsigned long long q_sum = 0;
    for (int base = 0; base < P; base += TT) {
        const int j = base + tid, s = j < P ? t.pslot[j] : -1;
        int r = -1;
        unsigned long long q = 0;
        if (s >= 0) {
            const int b = ld(t.broot + s);
            r = find_root(t.up, b, P);
            q = (unsigned long long)floor((weight_of(j) / wmax) * 4294967296.0);
            if (b == j) { atomicAdd(&t.nb[r], 1); ++n_bins; }
            ++n_used; q_sum += q; n_modes += r == j;
        }
        // a wave whose members all lie in one mode (a converged cloud) adds once
        const unsigned long long members = __ballot(s >= 0);
        const int first = members ? __ffsll((long long)members) - 1 : 0;
        const int r0 = __shfl(r, first, 64);
        if (members && __ballot(s >= 0 && r != r0) == 0) {
            unsigned long long qs = q; int c = s >= 0;
            for (int o = 32; o > 0; o >>= 1) { qs += __shfl_xor(qs, o, 64); c += __shfl_xor(c, o, 64); }
            if (lane == first) { atomicAdd(&t.Q[r0], qs); atomicAdd(&t.cnt[r0], c); }
        } else if (s >= 0) {
            atomicAdd(&t.Q[r], q);
            atomicAdd(&t.cnt[r], 1);
        }
        if (j < P) t.lab[j] = r;
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_used += __shfl_xor(n_used, o, 64); n_bins += __shfl_xor(n_bins, o, 64); n_modes += __shfl_xor(n_modes, o, 64);
        q_sum += __shfl_xor(q_sum, o, 64);
    }
    if (lane == 0) { atomicAdd(&s_cnt[0], n_used); atomicAdd(&s_cnt[1], n_bins); atomicAdd(&s_cnt[2], n_modes); atomicAdd(&s_qtot, q_sum); }
    __syncthreads();
    const unsigned long long q_total = s_qtot;
    if (tid == 0) {
        long long* info = a.info + (size_t)set * 4;
        info[0] = s_cnt[2]; info[1] = s_cnt[1]; info[2] = s_cnt[0]; info[3] = (long long)q_total;
    }
    if (!a.rows_f) return;

    // 5, 6. K times: the heaviest mode behind the one before in the order (Q descending, root ascending), and its row
    unsigned long long prev_q = ~0ull; int prev_r = -1;
    bool more = true;
    for (int k = 0; k < a.K; ++k) {
        double* out16 = a.rows_f + ((size_t)set * a.K + k) * RBPF_EST_F64;
        int32_t* out4 = a.rows_i + ((size_t)set * a.K + k) * RBPF_EST_I32;
        unsigned long long bq = 0; int br = -1;
        if (more) {
            for (int j = tid; j < P; j += TT) {
                if (t.lab[j] != j) continue;
                const unsigned long long q = ld(t.Q + j);
                if (!(q < prev_q || (q == prev_q && j > prev_r))) continue;
                if (br < 0 || q > bq || (q == bq && j < br)) { bq = q; br = j; }
            }
            auto better = [](unsigned long long qa, int ra, unsigned long long qb, int rb) {
                return ra >= 0 && (rb < 0 || qa > qb || (qa == qb && ra < rb));
            };
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long oq = __shfl_xor(bq, o, 64); const int orr = __shfl_xor(br, o, 64);
                if (better(oq, orr, bq, br)) { bq = oq; br = orr; }
            }
            __syncthreads();                             // the last use of s_q and s_arg is over
            if (lane == 0) { s_q[wave] = bq; s_arg[wave] = br; }
            __syncthreads();
            bq = s_q[0]; br = s_arg[0];
            for (int w = 1; w < TW; ++w)
                if (better(s_q[w], s_arg[w], bq, br)) { bq = s_q[w]; br = s_arg[w]; }
            more = br >= 0;
        }
        if (br >= 0) {
            const int root = br;
            const int32_t* lab = t.lab;
            estimate_row(P, pose, a.w_raw, a.w_given, a.mode, [=](int j) { return lab[j] == root; }, ld(t.nb + root), out16, out4, s_red, s_arg);
            if (tid == 0) { out16[12] = (double)bq; out16[13] = (double)bq / (double)q_total; out4[3] = root; }
            prev_q = bq; prev_r = br;
        } else if (tid == 0) {
            for (int c = 0; c < RBPF_EST_F64; ++c) out16[c] = c < 12 ? NAN : 0.0;
            out4[0] = -1; out4[1] = 0; out4[2] = 0; out4[3] = -1;
        }
    }
}

__global__ __launch_bounds__(TT) void pose_modes_kernel(ModesArgs a, const double* __restrict__ px, const double* __restrict__ py,
                                                        const double* __restrict__ pth) {
    modes_set(a, 0, [=](int j, double& x, double& y, double& th) { x = px[j]; y = py[j]; th = pth[j]; });
}

__global__ __launch_bounds__(TT) void track_modes_kernel(ModesArgs a, TrackLog g, int t0, const int32_t* __restrict__ lineage) {
    const size_t P = (size_t)g.P;
    const int32_t* lin = lineage + (size_t)blockIdx.x * P;
    const double* rec = reinterpret_cast<const double*>(g.base + (size_t)(t0 + (int)blockIdx.x) * g.stride);
    modes_set(a, blockIdx.x, [=](int j, double& x, double& y, double& th) { const int i = lin[j]; x = rec[i]; y = rec[P + i]; th = rec[2 * P + i]; });
}

void launch_pose_modes(const DevView& v, const ModesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pose_modes_kernel, dim3(1), dim3(TT), 0, s, a, v.px, v.py, v.pth);
}

void launch_track_modes(const TrackLog& g, int t0, int n_sets, const int32_t* d_lineage, const ModesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(track_modes_kernel, dim3(n_sets), dim3(TT), 0, s, a, g, t0, d_lineage);
}

}  // namespace rbpf
