// kernels_mapev.hip -- a5: HybridMap.update (hybridmap.py:95-145): the event-detecting walk (round 3).
//
// One 1024-thread workgroup at a time per particle (resident workgroups take particles from a queue), LDS window of 8-bit hit fields in GLOBAL cell-index space (as
// kernels_mapray.hip: a ray step is pure arithmetic, the index map is folded in by the write-back).  Same exact
// semantics as the other map kernels (kernels_mapupdate.hip has the ordered-replay argument).  What is different:
//
//   * The cells that receive an "occupied" / "nearby" hit in this scan (the only ones whose clamped adds do not commute)
//     carry a FLAG BIT in their field before the walk starts; every add of the walk RETURNS the old field, and a step that
//     sees the flag appends (beam, step) to an event list.  No slope buckets, no sort, no gather: a scan of 1081 beams in a
//     room leaves ~130 such passes per particle.
//   * Unflagged cells are written back from their counts: max(v + n * emp, min).  The flagged cells get a value from their
//     counts too; their real value follows.
//   * After the write-back the window's LDS is free: the flagged cells are grouped by storage cell through a hash table,
//     each listed pass is counted into the INTERVAL between two occupied / nearby events that its beam falls into - all
//     unoccupied passes are the same clamped add, so only their number between consecutive occupied / nearby events (in
//     beam order) matters - and one lane per flagged cell folds emp^n0 . ev0 . emp^n1 . ev1 ... from the cell's old value
//     and stores the byte (and its occupancy bit).
//   * A beam's own last step (occupied) and the step before it (the pass that precedes its own "nearby" hit) are not
//     walked at all: they are known without looking (the fold adds that pass in front of the beam's first event).
//   * Any partition of the ray steps may be written back on its own (clamped adds of one sign compose), so a fan larger than
//     the window is processed in strips of rows, each with its own read-modify-write.
//   * dim need not be a multiple of 32 (0.1 m cells: dim 400): the last 32-cell group of a tile row is partial.
//
//   Reference: hybridmap.py:95-145 (update), :274-301 (Bresenham), gridmap.py:86-117 (clamped adds).
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "rbpf_mapupdate.h"

namespace rbpf {

#if defined(RBPF_STAMPS) && defined(EV_BARRIER_WAITS)   // diagnostic: cycles every wave spends at the workgroup's barriers (printed by workgroup 0)
#undef BAR_LDS
#define BAR_LDS() do { const long long t0_ = clock64(); asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); { const long long d_ = clock64() - t0_; bar_wait += d_; if (bar_n < 12) bar_w[bar_n] = (int)d_; } ++bar_n; } while (0)
#endif

// Diagnostic (-DRBPF_STAMPS -DEV_STAMP_TURNOVER): per particle the constant-rate clock and the cycle counter when its workgroup
// takes it up and when the last of the sixteen waves is through with it, and the workgroup; the launcher writes the last launch's
// records to the file RBPF_EV_TURNOVER_OUT names (tools/probe_stamps.py reads it).  The product build has none of this.
#if defined(RBPF_STAMPS) && defined(EV_STAMP_TURNOVER)
static const int EV_TURN_MAX = 16384, EV_TURN_WORDS = 5;
__device__ unsigned long long ev_turn[EV_TURN_WORDS * EV_TURN_MAX];      // realtime in, realtime out, cycles in, cycles out, workgroup
#define EV_TURN_IN(p) do { if (threadIdx.x == 0 && (p) < EV_TURN_MAX) { unsigned long long* r_ = ev_turn + EV_TURN_WORDS * (p); r_[0] = wall_clock64(); r_[2] = (unsigned long long)clock64(); r_[4] = blockIdx.x; } } while (0)
#define EV_TURN_OUT(p) do { if ((threadIdx.x & 63) == 0 && (p) < EV_TURN_MAX) { unsigned long long* r_ = ev_turn + EV_TURN_WORDS * (p); atomicMax(&r_[1], (unsigned long long)wall_clock64()); atomicMax(&r_[3], (unsigned long long)clock64()); } } while (0)
static void ev_turnover_begin(hipStream_t s) {
    void* d = nullptr;
    if (getenv("RBPF_EV_TURNOVER_OUT") && hipGetSymbolAddress(&d, HIP_SYMBOL(ev_turn)) == hipSuccess) (void)hipMemsetAsync(d, 0, sizeof(unsigned long long) * EV_TURN_WORDS * EV_TURN_MAX, s);
}
static void ev_turnover_end(const DevView& v, int grid, hipStream_t s) {
    const char* path = getenv("RBPF_EV_TURNOVER_OUT");
    void* d = nullptr;
    if (!path || hipGetSymbolAddress(&d, HIP_SYMBOL(ev_turn)) != hipSuccess) return;
    const int n = std::min(v.P, EV_TURN_MAX);
    std::vector<unsigned long long> rec((size_t)EV_TURN_WORDS * n);
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(rec.data(), d, rec.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    int dev = 0, cus = 0, khz = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) { (void)hipGetLastError(); khz = 0; }
    if (FILE* f = fopen(path, "w")) {
        fprintf(f, "particles %d workgroups %d cus %d wall_clock_khz %d\n", n, grid, cus, khz);
        for (int p = 0; p < n; ++p) fprintf(f, "%llu %llu %llu %llu %llu\n", rec[5 * p], rec[5 * p + 1], rec[5 * p + 2], rec[5 * p + 3], rec[5 * p + 4]);
        fclose(f);
    }
}
#else
#define EV_TURN_IN(p) do { } while (0)
#define EV_TURN_OUT(p) do { } while (0)
static inline void ev_turnover_begin(hipStream_t) { }
static inline void ev_turnover_end(const DevView&, int, hipStream_t) { }
#endif

#ifndef EV_RUN                                  // (4 measured slower than 2: DESIGN.md section 6)
#define EV_RUN 2
#endif
static const int EB = 1024;                    // threads per particle
static const int HIT_BOUND = 62;               // per direction class; two classes can meet in a cell, +1 for the flag's count bit: 125 < 128
static const int EVCAP = 3072;                 // passes over flagged cells kept per particle (more: exact replay of every flagged cell)
static const int NPAIR = 3;                    // pairs (beam, e) per thread kept in registers: 3 * EB pairs = 1536 beams
static const int EV_R = EV_RUN;                // whole chunks of a ray that one work item of the level walk takes
static const int EV_LGR = EV_R == 4 ? 2 : EV_R == 2 ? 1 : 0;
static_assert(EV_R == 1 << EV_LGR, "the run length is 1, 2 or 4");
static const int FOLD_SPAN = 64;               // a flagged cell whose pairs lie within this many of each other is folded from a 64-bit set in registers

struct EvGeom {
    int fanw, bpad, ncell, T, logT, E;
    int o_mini, o_fs, o_end, o_nE, o_perm, o_kl, o_info, o_ux, o_uy, o_gxb, o_gyb, o_gym, o_evl, o_cnt;
    int p_keys, p_cnta, p_offs, p_oldv, p_rlist, p_evl, p_ic, p_bytes;              // the window's LDS after the write-back
    int bytes;
    bool ok;
};
__host__ __device__ inline EvGeom ev_geom(int B, int reach) {
    EvGeom g;
    g.fanw = (2 * reach + 8 + 7) & ~7;
    g.bpad = (B + 3) & ~3;
    int o = 0;
    g.o_mini = o;  o += al16(((NEAR_W * NEAR_W + 1) / 2) * 4);
    g.o_fs = o;    o += al16(g.bpad * 4);
    g.o_end = o;   o += al16(g.bpad * 4);
    g.o_nE = o;    o += al16(g.bpad * 2);
    g.o_perm = o;  o += al16(g.bpad * 2);
    g.o_kl = o;    o += al16(g.bpad * 2);
    g.o_info = o;  o += al16(g.bpad);
    g.o_ux = o;    o += al16(g.fanw * 2);
    g.o_uy = o;    o += al16(g.fanw * 2);
    g.o_gxb = o;   o += al16(g.fanw);
    g.o_gyb = o;   o += al16(g.fanw);
    g.o_gym = o;   o += al16(g.fanw + 16);
    g.o_evl = o;   o += EVCAP * 4;
    g.o_cnt = o;
    const int avail = 160 * 1024 - 2560 - o - 64;      // 2.5 KB for the kernel's static LDS
    g.ncell = avail > 0 ? avail & ~127 : 0;
    g.bytes = o + g.ncell;
    // after the write-back: hash table over the flagged storage cells (at most 2 B of them)
    int T = 1024, lt = 10;
    while (T < 3 * g.bpad) { T <<= 1; ++lt; }
    g.T = T; g.logT = lt;
    g.E = NPAIR * EB;                                  // pairs (beam, e)
    int q = 0;
    g.p_keys = q;  q += T * 4;                         // storage cell of the slot
    g.p_cnta = q;  q += T * 4;                         // head of the slot's list of pairs
    g.p_offs = q;  q += T * 2;                         // passes after the cell's last event
    g.p_oldv = q;  q += T;
    g.p_rlist = q; q += T * 2;
    g.p_evl = q;   q += al16(g.E * 2) * 2;          // next pair of the list; the lists laid out for the fold
    g.p_ic = q;    q += al16(g.E * 2);              // passes right before the pair's event
    g.p_bytes = q;
    g.ok = g.ncell >= 24576 && g.p_bytes <= g.ncell && 2 * 8 * NBIN * 2 <= g.ncell && 2 * B <= NPAIR * EB && reach >= NEAR_R + 4 && reach < 1000;
    return g;
}

bool map_update_ev_available(const DevView& v) {
    const EvGeom g = ev_geom(v.B, v.reach);
    const int gpt = (v.dim + 31) >> 5;
    return g.ok && lattice_fits_byte_fields(v.cc) && v.dim % 8 == 0 && 3 * gpt <= 192 && v.L * v.L <= 49;
}

// 32-bit fixed-point slope: ceil(dmin * 2^32 / dmaj), the diagonal clamped to 2^32 - 1.  With it
//   minor(j) = (slope * j + 2^31) >> 32  ==  (2 * dmin * j + dmaj) / (2 * dmaj)     (hybridmap.py:286-300 in closed form)
// for every j <= dmaj as long as 2 * j * dmaj < 2^32: the slope errs upwards by less than 2^-32 per step and a value
// (2 dmin j + dmaj) / (2 dmaj) that is not an integer lies at least 1 / (2 dmaj) below the next one.
__device__ __forceinline__ uint32_t ev_fix_slope(int dmin, int dmaj) {
    if (dmaj <= 0 || dmin <= 0) return 0u;
    if (dmin >= dmaj) return 0xFFFFFFFFu;
    const unsigned long long num = (unsigned long long)(unsigned)dmin << 32;
    unsigned long long q = (unsigned long long)((double)num / (double)dmaj);      // within one of the quotient
    long long r = (long long)num - (long long)(q * (unsigned)dmaj);
    if (r < 0) { --q; r += dmaj; }
    if (r >= dmaj) { ++q; r -= dmaj; }
    return (uint32_t)(q + (r > 0 ? 1u : 0u));
}
__device__ __forceinline__ int ev_minor(uint32_t fs, int j) {
    return (int)(((unsigned long long)fs * (unsigned)j + 0x80000000ull) >> 32);
}

__device__ __forceinline__ uint32_t ev_lds_add_rtn(int byte_addr, uint32_t val) {
    return __hip_atomic_fetch_add((lds_u32*)(uintptr_t)(uint32_t)byte_addr, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The flag of a field from the word an add returned: bit (sh mod 32) of it.  The bit-field extract reads only the low five bits
// of its offset, so the field's bit address goes in as it is (a shift by `sh & 31` costs a masking instruction per step).
__device__ __forceinline__ uint32_t ev_flag_bit(uint32_t word, int sh) {
    return __builtin_amdgcn_ubfe(word, (uint32_t)sh, 1u);
}

// open addressing, linear probing, keys never ~0
__device__ __forceinline__ int ev_hash_insert(uint32_t* keys, int T, int logT, uint32_t sc, bool& created) {
    uint32_t h = (sc * 2654435761u) >> (32 - logT);
    for (;;) {
        const uint32_t old = atomicCAS(&keys[h], 0xFFFFFFFFu, sc);
        created = old == 0xFFFFFFFFu;
        if (created || old == sc) return (int)h;
        h = (h + 1) & (uint32_t)(T - 1);
    }
}
__device__ __forceinline__ int ev_hash_find(const uint32_t* keys, int T, int logT, uint32_t sc) {
    uint32_t h = (sc * 2654435761u) >> (32 - logT);
    for (int it = 0; it < T; ++it) {
        const uint32_t k = keys[h];
        if (k == sc) return (int)h;
        if (k == 0xFFFFFFFFu) return -1;
        h = (h + 1) & (uint32_t)(T - 1);
    }
    return -1;
}


// What a particle's preamble needs from global memory before it can start: made by ONE wave, for the workgroup's next particle
// while the current one is written back, so that the chains slot -> tile-table row and pose -> sine / cosine are through when
// the next particle starts (rec->p says whose record it is).
struct EvNext { double px, py, sn, cs; int p, slot; int32_t tab[49]; };
__device__ __forceinline__ void ev_prefetch(const DevView& v, int p, EvNext* rec, int lane) {
    const int LL = v.L * v.L, slot = v.slot[p];
    if (lane < LL) rec->tab[lane] = v.tile_tab[(size_t)slot * LL + lane];
    double sn, cs_;
    sincos(v.upd_pose[2 * v.P + p], &sn, &cs_);
    if (lane == 0) { rec->px = v.upd_pose[p]; rec->py = v.upd_pose[v.P + p]; rec->sn = sn; rec->cs = cs_; rec->slot = slot; rec->p = p; }
}

// The particle a position of the launch stands for: itself, or - when the coming resample discards some particles (DevView::
// mu_keep) - the position's entry in the list of the others; v.P behind the last one.
__device__ __forceinline__ int ev_position(const DevView& v, int pos) {
    if (!v.mu_keep) return pos;
    return pos < *v.mu_n_keep ? v.mu_keep[pos] : v.P;
}

// One particle's update by the whole workgroup.  `draw`: thread 0 takes the workgroup's NEXT particle from the queue (its first
// one is position blockIdx.x, the queue hands out positions gridDim.x, gridDim.x + 1, ...) before anything else, so that the
// add's round trip - and the look-up of the position behind it - lies under the preamble's loads, and leaves it in *s_next
// (v.P or more: none) before the particle's first barrier - or before it returns ahead of that barrier.  Every return is
// uniform over the workgroup; the caller's barrier follows.
__device__ __forceinline__ void map_update_ev_particle(const DevView& v, const int p, const bool draw, int* s_next, EvNext* rec) {
    extern __shared__ __align__(16) unsigned char smem[];
    int tid_ = threadIdx.x;
    asm volatile("" : "+v"(tid_));                 // (what hangs on the thread's number is worked out per particle too: kept across the caller's loop it spilled)
    __builtin_assume((unsigned)tid_ < (unsigned)EB);
    const int tid = tid_, lane = tid & 63, wave = tid >> 6;
    int nxt = v.P;
    if (draw && tid == 0) nxt = ev_position(v, (int)gridDim.x + (int)atomicAdd(&v.ev_queue[0], 1u));
    const EvGeom G = ev_geom(v.B, v.reach);
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(smem + G.o_cnt);     // 8-bit fields: bit 0 = flagged, bits 1-7 = passes; [row = global x][col = global y]
    uint8_t*  const cnt8 = smem + G.o_cnt;
    uint32_t* const mini = reinterpret_cast<uint32_t*>(smem + G.o_mini);   // [NEAR_W^2] 16-bit fields round the start cell, same format
    uint32_t* const r_fs = reinterpret_cast<uint32_t*>(smem + G.o_fs);     // [B] 32-bit fixed-point slope
    int32_t*  const r_end = reinterpret_cast<int32_t*>(smem + G.o_end);    // [B] packed end cell relative to the start
    uint16_t* const r_nE = reinterpret_cast<uint16_t*>(smem + G.o_nE);     // [B] steps the walk takes
    uint16_t* const perm = reinterpret_cast<uint16_t*>(smem + G.o_perm);   // the rays with a run, ordered by falling count of runs (EV_R whole chunks each)
    uint8_t*  const r_info = smem + G.o_info;                              // [B]
    uint16_t* const r_kl = reinterpret_cast<uint16_t*>(smem + G.o_kl);     // [B] first whole chunk of the ray's share of the level walk | chunks << 8 (a strip: those inside it)
    uint16_t* const ux = reinterpret_cast<uint16_t*>(smem + G.o_ux);       // U of global column fxl + i
    uint16_t* const uy = reinterpret_cast<uint16_t*>(smem + G.o_uy);
    uint8_t*  const gxb = smem + G.o_gxb;                                  // G of global column fxl + i (0 / 1)
    uint8_t*  const gyb = smem + G.o_gyb;
    uint8_t*  const gym = smem + G.o_gym;                                  // G of window column lc as a byte mask (0 / 0xFF)
    uint32_t* const evlist = reinterpret_cast<uint32_t*>(smem + G.o_evl);  // [EVCAP] beam << 10 | step: passes over flagged cells

    __shared__ int s_fb, s_exact;
    __shared__ int s_need[49], s_tab[49];
    __shared__ int s_fan[4];
    __shared__ int s_wsum[EB / 64], s_wsum2[EB / 64];
    __shared__ int s_lcnt[MAXLEV + 1], s_lfill[MAXLEV + 1], s_nk[MAXLEV + 2], s_lp[MAXLEV + 3], s_nlev;
    __shared__ int s_nev, s_written, s_wbq;
    __shared__ unsigned long long s_cells;
    __shared__ uint8_t s_ggf[192];                    // per (tile column, 32-column group): a glitched column among its 33

    const int LL = v.L * v.L;
    STAMP_DECL;
    // No record of this particle (the workgroup's first one, or the one before it left early): wave 0 makes it on the spot.  Every wave
    // reads rec->p while nobody writes the record - the last writer is behind the caller's barrier, the next one behind the first
    // barrier here, which a wave reaches only after its read - so all sixteen take the same branch and the same barriers.
    const int rec_p = UNI(rec->p);
    if (rec_p != p) {
        __syncthreads();                           // every wave has read rec->p
        if (wave == 0) ev_prefetch(v, p, rec, lane);
        __syncthreads();
    }
    int32_t* tab = v.tile_tab + (size_t)UNI(rec->slot) * LL;
#if defined(RBPF_STAMPS) && defined(EV_BARRIER_WAITS)
    long long bar_wait = 0; int bar_n = 0; const long long t_begin = clock64(); int bar_w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    // =============================================== setup ===============================================
    // this thread's beams: one per thread (two for the first few)
    const int pb0 = tid, pb1 = tid + EB;
    const double pre_x0 = pb0 < v.B ? v.bx[pb0] : 0.0, pre_y0 = pb0 < v.B ? v.by[pb0] : 0.0, pre_s0 = pb0 < v.B ? v.bscale[pb0] : 0.0;
    const double pre_x1 = pb1 < v.B ? v.bx[pb1] : 0.0, pre_y1 = pb1 < v.B ? v.by[pb1] : 0.0, pre_s1 = pb1 < v.B ? v.bscale[pb1] : 0.0;
    const int pre_f0 = pb0 < v.B ? v.bflags[pb0] : 0, pre_f1 = pb1 < v.B ? v.bflags[pb1] : 0;
    const double s_px = rec->px, s_py = rec->py;
    int x0, y0;
    // (the LUT must cover the index map's margin here, only the rays' reach in the other kernels: which poses are RBPF_ERANGE depends on it)
    if (!fan_preamble_from<EB>(v, rec->tab, p, tid, s_px, s_py, v.reach + 2, G.fanw, ux, uy, x0, y0)) { if (tid == 0) *s_next = nxt; return; }
    const int fxl = x0 - v.reach - 2, fyl = y0 - v.reach - 2, nfx = 2 * v.reach + 5;
    uint16_t* const s_bins = reinterpret_cast<uint16_t*>(cnt);               // [8 NBIN] rays per (class, slope bucket) (the window is not in use yet)
    uint16_t* const s_far = s_bins + 8 * NBIN;                               // ... of the rays that reach the 8-bit fields
    if (tid == 0) {
        s_fan[0] = x0; s_fan[1] = x0; s_fan[2] = y0; s_fan[3] = y0;
        s_cells = 0; s_fb = 0; s_exact = 0; s_nev = 0; s_written = 0;
        *s_next = nxt;
    }
    for (int i = tid; i < LL; i += EB) { s_need[i] = 0; s_tab[i] = rec->tab[i]; }
    for (int i = tid; i < 8 * NBIN; i += EB) reinterpret_cast<uint32_t*>(s_bins)[i] = 0;     // both bucket arrays
    if (tid < 192) s_ggf[tid] = 0;
    if (tid <= MAXLEV) s_lcnt[tid] = 0;
    for (int i = tid; i < (NEAR_W * NEAR_W + 1) / 2; i += EB) mini[i] = 0;
    __syncthreads();
#ifndef EV_STAMP_FLAGS
    STAMP(0);
#endif
    const double s_s = rec->sn, s_c = rec->cs;
    const int nxt_p = UNI(*s_next);                // the workgroup's next particle (v.P or more: none)

    const int C = v.R * v.dim + v.dim / 2;
    const int Uxs = UNI(ux[x0 - fxl]), Uys = UNI(uy[y0 - fyl]);
    const int a0 = Uxs / v.dim, b0 = Uys / v.dim;
    auto lat_x = [&](int g) { const int U = ux[g - fxl]; return a0 + (U >= (a0 + 1) * v.dim ? 1 : 0) - (U < a0 * v.dim ? 1 : 0); };   // (rays are shorter than a tile)
    auto lat_y = [&](int g) { const int U = uy[g - fyl]; return b0 + (U >= (b0 + 1) * v.dim ? 1 : 0) - (U < b0 * v.dim ? 1 : 0); };
    {
        FanBox fan = {x0, x0, y0, y0, 0ull};
        for (int b = tid; b < v.B; b += EB) {
            const double x = b == pb0 ? pre_x0 : b == pb1 ? pre_x1 : v.bx[b], y = b == pb0 ? pre_y0 : b == pb1 ? pre_y1 : v.by[b];
            const int bf = b == pb0 ? pre_f0 : b == pb1 ? pre_f1 : (int)v.bflags[b];
            auto scale = [&] { return b == pb0 ? pre_s0 : b == pb1 ? pre_s1 : v.bscale[b]; };
            const BeamRay br = beam_ray(v, x, y, bf, scale, s_s, s_c, s_px, s_py, x0, y0, a0, b0, lat_x, lat_y, s_need, fan);
            const Ray& r = br.r;
            const int ddx = br.x1 - x0, ddy = br.y1 - y0, info = br.info;
            int nE = 0;
            uint32_t fs = 0;
            if (r.n > 0) {
                fs = ev_fix_slope(r.dmin, r.dmaj);
                // steps the walk takes: all of them but the beam's own occupied step and the pass before its own nearby hit
                nE = r.n - ((info & RI_OCC) ? 1 : 0) - ((info & RI_NEAR) ? 1 : 0);
                const int cls = (r.steep ? 4 : 0) | (ddx > 0 ? 2 : 0) | (ddy > 0 ? 1 : 0);
                const int key = cls * NBIN + (int)(fs >> 24);
                atomicAdd(reinterpret_cast<unsigned int*>(s_bins) + (key >> 1), 1u << ((key & 1) * 16));
                if (nE > NEAR_R) atomicAdd(reinterpret_cast<unsigned int*>(s_far) + (key >> 1), 1u << ((key & 1) * 16));   // only these reach the 8-bit fields
                const int nfull = (nE - NEAR_R) / LCH;                               // whole chunks beyond the 16-bit block
                if (nE > NEAR_R && nfull >= EV_R) atomicAdd(&s_lcnt[min(nfull / EV_R, MAXLEV)], 1);   // the levels of the runs (a strip makes its own)
            }
            r_fs[b] = fs;
            r_end[b] = (int32_t)(((uint32_t)ddx & 0xFFFFu) | ((uint32_t)ddy << 16));
            r_nE[b] = (uint16_t)nE;
            r_info[b] = (uint8_t)info;
            r_kl[b] = (uint16_t)(1 | ((nE > NEAR_R ? (nE - NEAR_R) / LCH : 0) << 8));
        }
        fan_box_join(fan, lane, s_fan, &s_cells);
    }
    __syncthreads();
    // ---- the window (rbpf_mapupdate.h: strips of storage rows if the fan does not fit) ----
    const StripGeom sg = strip_geom<EB>(ux, uy, gxb, gyb, G.fanw, fxl, fyl, C, s_fan, &s_fb, G.ncell, tid);
    const int S_lo = sg.S_lo, S_hi = sg.S_hi, T_lo = sg.T_lo, T_hi = sg.T_hi, gy_base = sg.gy_base, stride = sg.stride, rows_cap = sg.rows_cap;
    const int gpt = (v.dim + 31) >> 5, ggf_base = T_lo / v.dim * gpt;        // 32-cell groups per tile row (the last one may be partial); s_ggf[0]'s group
    if (wave == 0) level_sums(lane, s_lcnt, s_lfill, s_nk, s_lp, &s_nlev);
    {   // no 8-bit field can overflow: a cell at major distance j >= NEAR_R is hit, per direction class, only by rays
        // whose slope lies in a window of width 2^32 / j + 1, i.e. in at most NB_WIN consecutive buckets: bounded with all
        // rays of those buckets, or (the smaller of the two) with the rays long enough to reach an 8-bit field.
        // inclusive prefix sums over the 2048 (class, bucket) counts, two per thread
        const int c0 = s_bins[2 * tid], c1 = s_bins[2 * tid + 1], f0 = s_far[2 * tid], f1 = s_far[2 * tid + 1];
        int incl = c0 + c1, incl2 = f0 + f1;
        for (int o = 1; o < 64; o <<= 1) { int n = __shfl_up(incl, o, 64), n2 = __shfl_up(incl2, o, 64); if (lane >= o) { incl += n; incl2 += n2; } }
        if (lane == 63) { s_wsum[wave] = incl; s_wsum2[wave] = incl2; }
        __syncthreads();
        int base = incl - (c0 + c1), base2 = incl2 - (f0 + f1);
        for (int k = 0; k < wave; ++k) { base += s_wsum[k]; base2 += s_wsum2[k]; }
        s_bins[2 * tid] = (uint16_t)(base + c0); s_bins[2 * tid + 1] = (uint16_t)(base + c0 + c1);
        s_far[2 * tid] = (uint16_t)(base2 + f0); s_far[2 * tid + 1] = (uint16_t)(base2 + f0 + f1);
        __syncthreads();
        int mx2 = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = 2 * tid + i, cls = key / NBIN, bin = key % NBIN;
            const int hi = cls * NBIN + min(bin + NB_WIN - 1, NBIN - 1);
            mx2 = max(mx2, min((int)s_bins[hi] - (key ? (int)s_bins[key - 1] : 0), (int)s_far[hi] - (key ? (int)s_far[key - 1] : 0)));
        }
        mx2 = wave_max(mx2);
        if (lane == 0 && mx2 > HIT_BOUND) s_exact = 1;
    }
    // rays ordered by falling count of runs
    for (int b = tid; b < v.B; b += EB) {
        const int nE = r_nE[b];
        const int nfull = (nE - NEAR_R) / LCH;
        if (nE > NEAR_R && nfull >= EV_R) perm[atomicAdd(&s_lfill[min(nfull / EV_R, MAXLEV)], 1)] = (uint16_t)b;
    }
    glitch_mask<EB>(gyb, gym, s_ggf, ggf_base, 192, sg, G.fanw, fyl, nfx, C, v.dim, gpt, tid);
    __syncthreads();
    if (UNI(s_fb) || rows_cap < 8) { GIVE_BACK(1); }
    if (UNI(s_exact)) { GIVE_BACK(2); }
    alloc_missing_tiles(v, tab, s_need, s_tab, tid);
    STAMP(1);

    // pairs (beam, e) and the storage cells they flag, flagged cells and their sources (rbpf_mapupdate.h)
    auto pair_cell = [&](int pr) { return flagged_cell(pr, r_info, r_end, x0, y0, ux, uy, fxl, fyl); };
    auto sources = [&](uint32_t sc, FCell& f) { cell_sources(sc, C, gxb, gyb, fxl, fyl, f); };
    // tile and offset of a storage cell (rays are shorter than a tile: the lattice coordinate moves by at most one)
    auto cell_addr = [&](int sx, int sy, int& tile, int& row_t, int& col_t) {
        const int a = a0 + (sx >= (a0 + 1) * v.dim ? 1 : 0) - (sx < a0 * v.dim ? 1 : 0);
        const int bb = b0 + (sy >= (b0 + 1) * v.dim ? 1 : 0) - (sy < b0 * v.dim ? 1 : 0);
        tile = ((unsigned)a < (unsigned)v.L && (unsigned)bb < (unsigned)v.L) ? s_tab[a * v.L + bb] : -1;
        row_t = sx - a * v.dim; col_t = sy - bb * v.dim;
    };
    // direction of a ray: steps of the major / minor axis in global cells
    struct RayDir { int steep, sx, sy; };
    auto ray_dir = [&](int b) {
        const int32_t re = r_end[b];
        const int ex = (int)(int16_t)(re & 0xFFFF), ey = (int)(int16_t)((uint32_t)re >> 16);
        const int aex = ex < 0 ? -ex : ex, aey = ey < 0 ? -ey : ey;
        RayDir d; d.steep = aey > aex; d.sx = ex > 0 ? 1 : -1; d.sy = ey > 0 ? 1 : -1;          // hybridmap.py:282-283
        return d;
    };
    const int sat = sat_passes(v.cc);
    const WbConsts wbk = wb_consts(v.cc);
    const int cnt_lds = lds_addr(cnt), mini_lds = lds_addr(mini);
    // a thin fan: fewer ray cells than two fifths of the fan's box (181 beams on a 0.025 m grid: a seventh)
    const bool sparse = (long long)UNI((int)s_cells) * 5 < 2LL * (long long)(S_hi - S_lo + 1) * (long long)(T_hi - T_lo + 1);
    // a lane's steps that met a flagged cell (bit 16 + u of m = step j0 + u): into the event list
    auto log_events = [&](uint32_t m, int b, int j0, int ev_lo, int ev_hi, int gx_base, bool filter) {
        while (m) {
            const int lb = __ffs((int)m) - 1;
            m &= m - 1;
            const int j = j0 + lb - 16;
            if (filter) {   // strips share a global row with their neighbours: the strip that owns its storage row reports
                const RayDir d = ray_dir(b);
                const int row = x0 + d.sx * (d.steep ? ev_minor(r_fs[b], j) : j) - gx_base;
                if (row < ev_lo || row > ev_hi) continue;
            }
            const int pos = atomicAdd(&s_nev, 1);
            if (pos < EVCAP) evlist[pos] = ((uint32_t)b << 10) | (uint32_t)j;
        }
    };
    // this thread's pairs (beam, e): pair = tid, tid + EB, tid + 2 EB; cell and old value stay in registers until the
    // flagged cells are folded (the old value must be read before the write-back)
    uint32_t my_sc[NPAIR]; int my_old[NPAIR];
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
        const int pr = tid + i * EB;
        my_sc[i] = pr < 2 * v.B ? pair_cell(pr) : 0xFFFFFFFFu;
        my_old[i] = 0;
        if (my_sc[i] != 0xFFFFFFFFu) {
            int tile, row_t, col_t;
            cell_addr((int)(my_sc[i] >> 16), (int)(my_sc[i] & 0xFFFFu), tile, row_t, col_t);
            if (tile >= 0) my_old[i] = (int)v.pool[(size_t)tile * v.dim * v.dim + (size_t)row_t * v.dim + col_t];   // (in flight until the fold)
        }
    }

#ifdef EV_STAMP_FLAGS                                                           // diagnostic: slot 0 = the pairs' set-up (slot 1 then holds the whole set-up), slot 2 = clearing the window and the flags
    STAMP(0);
#endif
    // =============================================== windows ==============================================
    int n_win = 0;
    for (int S0 = S_lo; S0 <= S_hi; S0 += rows_cap - 1, ++n_win) {
        const int S1 = min(S_hi, S0 + rows_cap - 2);                             // storage rows S0..S1
        const int gx_base = S0 - C, rows_w = S1 - S0 + 2;                        // global rows gx_base .. gx_base + rows_w - 1
        const bool whole = S0 == S_lo && S1 == S_hi;                             // one window holds the fan
        BAR_LDS();                                                               // the previous window (or the slope buckets) is done with the counters
        for (int i = tid; i < (rows_w * stride + 15) >> 4; i += EB) reinterpret_cast<uint4*>(cnt)[i] = make_uint4(0, 0, 0, 0);
        BAR_LDS();
        // ---- flags: every global cell that maps to a storage cell with an occupied / nearby hit; the flag comes with a
        //      count of one, so a flagged field is never zero (the write-back takes "touched" from the field) ----
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) {
            uint32_t sc = my_sc[i];
            asm volatile("" : "+v"(sc));                                         // (the cell's sources are worked out here, strip by strip: hoisted out of the strips' loop they were 24 registers spilled to scratch)
            if (sc == 0xFFFFFFFFu) continue;
            FCell f;
            sources(sc, f);
#pragma unroll
            for (int ix = 0; ix < 2; ++ix)
#pragma unroll
            for (int iy = 0; iy < 2; ++iy) {
                if (ix >= f.ngx || iy >= f.ngy) continue;
                const int sgx = ix ? f.gx1 : f.gx0, sgy = iy ? f.gy1 : f.gy0;
                const int ddx = sgx - x0, ddy = sgy - y0;
                if (max(ddx < 0 ? -ddx : ddx, ddy < 0 ? -ddy : ddy) < NEAR_R) {
                    if (n_win == 0) { const int mi = (ddx + NEAR_R) * NEAR_W + (ddy + NEAR_R); atomicOr(&mini[mi >> 1], 3u << ((mi & 1) * 16)); }
                } else {
                    const int row = sgx - gx_base, col = sgy - gy_base;
                    if ((unsigned)row < (unsigned)rows_w && (unsigned)col < (unsigned)stride) { const int c = row * stride + col; atomicOr(&cnt[c >> 2], 3u << ((c & 3) * 8)); }
                }
            }
        }
        BAR_LDS();
        STAMP(2);
        // rows of this window whose passes are reported from here (the first and the last global row belong to two strips)
        const int ev_lo = (!whole && gxb[gx_base - fxl]) ? 1 : 0, ev_hi = (!whole && !gxb[gx_base + rows_w - 1 - fxl]) ? rows_w - 2 : rows_w - 1;
        // ---- the 16-bit block: steps 0 .. NEAR_R - 1 of every ray, once ----
        if (n_win == 0) {
            const int nw0 = (v.B + 63) >> 6;
            for (int q = wave; q < nw0; q += EB / 64) {
                const int b = lane * nw0 + q;                                          // the 64 rays of an instruction point in different directions
                const bool valid = b < v.B;
                const int nE = valid ? (int)r_nE[b] : 0;
                if (__ballot(nE > 0) == 0ull) continue;
                const uint32_t fs = valid ? r_fs[b] : 0u;
                const RayDir d = ray_dir(valid ? b : 0);
                const int mj = d.steep ? d.sy : d.sx * NEAR_W, mm = d.steep ? d.sx * NEAR_W : d.sy;
                const int d0 = mj, d1 = mj + mm;
                uint32_t acc = 0x80000000u, m = 0;
                int c = NEAR_R * NEAR_W + NEAR_R + (mini_lds >> 1);                    // field index, the array's LDS address folded in
                uint32_t ret[NEAR_R]; int sh[NEAR_R];
#pragma unroll
                for (int u = 0; u < NEAR_R; ++u) {
                    sh[u] = c << 4;
                    ret[u] = ev_lds_add_rtn((c << 1) & ~3, (u < nE ? 2u : 0u) << (sh[u] & 31));
                    const uint32_t nacc = acc + fs;
                    c += nacc < acc ? d1 : d0;
                    acc = nacc;
                }
                __builtin_amdgcn_sched_barrier(0);                                     // sixteen adds in flight, then their answers
#pragma unroll
                for (int u = 0; u < NEAR_R; ++u) m = __builtin_amdgcn_alignbit(u < nE ? ev_flag_bit(ret[u], sh[u]) : 0u, m, 1);
                if (m) log_events(m, b, 0, 0, 0, 0, false);
            }
        }
        // ---- walk: lanes are rays, chunk k >= 1 of a ray = its steps NEAR_R + 16 (k - 1) .. + 15.  A work item is a run of EV_R whole
        //      chunks of 64 rays (or one left-over chunk: see the level walk); the rays that own an r-th run are perm[0 .. N_r); lane l of
        //      the w-th wave of a level takes ray l * waves + w.
        //      A step: field += 2 with the old word returned, bit 0 of the old field = flagged; the address moves by one of two
        //      constants, chosen by the carry of the slope accumulator. ----
        {
            const int rx0 = x0 - gx_base, ry0 = y0 - gy_base;
            const int base0 = rx0 * stride + ry0 + cnt_lds;
            const int win_lo = cnt_lds, win_n = rows_w * stride;
            // one predicated chunk of ray b (steps j0 .. j0 + 15, those in [jlo, jhi] and inside the window count): the tail of a
            // ray, or - in a strip - a chunk the strip's edge cuts.  Branch-free: a dead step adds nothing to a word of the lane's own.
            // `strip` (a constant where it is called) = false: one window holds the fan, the chunk is a ray's tail and a step counts if it lies
            // below the ray's end - no lower bound, no test against the window.
            auto walk_pred = [&](int b, int j0, int jlo, int jhi, const bool strip) {
                const uint32_t fs = r_fs[b];
                const RayDir d = ray_dir(b);
                const int sxs = d.sx * stride;
                const int cj = d.steep ? d.sy : sxs, cm = d.steep ? sxs : d.sy;
                const unsigned long long pr64 = (unsigned long long)fs * (unsigned)j0 + 0x80000000ull;
                uint32_t acc = (uint32_t)pr64, m = 0, inm = 0;
                int c = base0 + __mul24(j0, cj) + __mul24((int)(pr64 >> 32), cm);
                const int d0 = cj, d1 = cj + cm;
                uint32_t ret[LCH]; int sh[LCH];
#pragma unroll
                for (int u = 0; u < LCH; ++u) {
                    const bool in = strip ? j0 + u >= jlo && j0 + u <= jhi && (unsigned)(c - win_lo) < (unsigned)win_n : j0 + u <= jhi;
                    sh[u] = c << 3;
                    ret[u] = ev_lds_add_rtn(in ? c & ~3 : win_lo + 4 * lane, (in ? 2u : 0u) << (sh[u] & 31));
                    inm |= in ? 1u << u : 0u;
                    const uint32_t nacc = acc + fs;
                    c += nacc < acc ? d1 : d0;
                    acc = nacc;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < LCH; ++u) m = __builtin_amdgcn_alignbit((inm >> u) & ev_flag_bit(ret[u], sh[u]), m, 1);
                if (m) log_events(m, b, j0, ev_lo, ev_hi, gx_base, !whole);
            };
            if (whole) {
                // the tail of every ray with more than NEAR_R steps (its whole chunks follow, level by level)
                for (int b = tid; b < v.B; b += EB) {
                    const int nE = (int)r_nE[b];
                    if (nE <= NEAR_R) continue;
                    const int j0 = NEAR_R + ((nE - NEAR_R) / LCH) * LCH;            // first step after the whole chunks
                    if (j0 < nE) walk_pred(b, j0, j0, nE - 1, false);
                }
            } else {
                // A strip holds a part of every ray: the steps NEAR_R .. nE - 1 whose row lies in the strip are a run
                // [lo, hi] (rows never turn back along a ray).  The whole chunks inside the run are the ray's share of the
                // strip's level walk (relative levels: rays ordered by how many runs of such chunks they have); the one or two chunks
                // that the strip's edge or the ray's end cuts are walked here, predicated.
                if (tid <= MAXLEV) s_lcnt[tid] = 0;
                BAR_LDS();
                auto first_j = [&](uint32_t fs, int mval) -> int {               // first step with minor(j) >= mval (mval >= 1)
                    if (fs == 0u) return 1 << 20;
                    const double jd = ((double)mval * 4294967296.0 - 2147483648.0) / (double)fs;
                    if (jd > 4000.0) return 1 << 20;
                    int j = (int)jd;
                    while (ev_minor(fs, j) < mval) ++j;
                    while (j > 0 && ev_minor(fs, j - 1) >= mval) --j;
                    return j;
                };
                for (int b = tid; b < v.B; b += EB) {
                    const int nE = (int)r_nE[b];
                    int ka = 1, len = 0;
                    if (nE > NEAR_R) {
                        const uint32_t fs = r_fs[b];
                        const RayDir d = ray_dir(b);
                        int lo = NEAR_R, hi = nE - 1;
                        if (!d.steep) {                                            // row = rx0 + sx * j
                            if (d.sx > 0) { lo = max(lo, -rx0); hi = min(hi, rows_w - 1 - rx0); }
                            else { lo = max(lo, rx0 - (rows_w - 1)); hi = min(hi, rx0); }
                        } else {                                                   // row = rx0 + sx * minor(j), minor never decreases
                            const int mlo = d.sx > 0 ? -rx0 : rx0 - (rows_w - 1), mhi = d.sx > 0 ? rows_w - 1 - rx0 : rx0;
                            if (mhi < 0) hi = -1;
                            else {
                                if (mlo > 0) lo = max(lo, first_j(fs, mlo));
                                hi = min(hi, first_j(fs, mhi + 1) - 1);
                            }
                        }
                        if (lo <= hi) {
                            const int nfull = (nE - NEAR_R) / LCH;
                            const int kf = (lo - NEAR_R) / LCH + 1, kl = (hi - NEAR_R) / LCH + 1;   // the chunks that hold the first / the last step
                            const int a = lo == NEAR_R + (kf - 1) * LCH ? kf : kf + 1;             // first chunk that lies inside as a whole
                            const int e = min(hi == NEAR_R + kl * LCH - 1 ? kl : kl - 1, nfull);   // last one
                            if (e >= a) { ka = a; len = e - a + 1; }
                            if (kf < a || kf > e) walk_pred(b, NEAR_R + (kf - 1) * LCH, lo, hi, true);
                            if (kl != kf && (kl < a || kl > e)) walk_pred(b, NEAR_R + (kl - 1) * LCH, lo, hi, true);
                        }
                    }
                    r_kl[b] = (uint16_t)(ka | (len << 8));
                    if (len >= EV_R) atomicAdd(&s_lcnt[min(len / EV_R, MAXLEV)], 1);
                }
                BAR_LDS();
                if (wave == 0) level_sums(lane, s_lcnt, s_lfill, s_nk, s_lp, &s_nlev);   // relative levels: rays with at least k runs of whole chunks inside the strip
                BAR_LDS();
                for (int b = tid; b < v.B; b += EB) {
                    const int len = (int)r_kl[b] >> 8;
                    if (len >= EV_R) perm[atomicAdd(&s_lfill[min(len / EV_R, MAXLEV)], 1)] = (uint16_t)b;
                }
                BAR_LDS();
            }
            // ---- the level walk: every lane runs all 16 steps of whole chunks (inside the window as a whole).  A ray's share of `len`
            //      whole chunks from chunk `ka` on (r_kl) is len / R RUNS of R consecutive chunks and len % R left-over chunks behind them.
            //      A work item is a run of 64 rays - direction, start address and the next item's fetch once, the slope accumulator and the
            //      address carried from chunk to chunk - or one left-over chunk of 64 rays.  The runs are levelled by their number (s_lp,
            //      s_nk, perm: run level r holds the rays with at least r runs); behind them come R - 1 levels of left-overs over ALL
            //      rays in beam order, lane l of a level's w-th wave asks ray l * waves + w and sits idle unless that ray has more than
            //      `level` left-overs (no second order of the rays: (R - 1) * B / 64 items, a few of a thousand). ----
            const int nlev_w = UNI(s_nlev);
            const int nruns = UNI(s_lp[nlev_w + 1]);                              // the runs' items (levels above nlev have no waves: s_lp stays flat)
            const int nwb = (v.B + 63) >> 6;
            const int nitems = nruns + (EV_R - 1) * nwb;
            const int wave_u = UNI(wave);                                         // (the items' numbers and the levels' bookkeeping in scalar registers)
            // the next item's ray is fetched while this one's adds are in flight
            int kn = 1;
            int lp_c = UNI(s_lp[1]), lp_n = UNI(s_lp[2]), nk_c = UNI(s_nk[1]);    // first item of the level, of the next level; rays of the level
            int nb = -1, nk0 = 1; uint32_t nfs = 0; int32_t nend = 0;             // the next item: ray, its first chunk, slope, end cell
            auto fetch_item = [&](int q) {
                nb = -1;
                if (q >= nitems) return;
                if (q < nruns) {
                    while (kn < nlev_w && q >= lp_n) { ++kn; lp_c = lp_n; lp_n = UNI(s_lp[kn + 1]); nk_c = UNI(s_nk[kn]); }
                    const int nwk = (nk_c + 63) >> 6, wslot = q - lp_c;
                    const int ii = lane * nwk + wslot;
                    if (ii < nk_c) { nb = perm[ii]; nfs = r_fs[nb]; nend = r_end[nb]; nk0 = ((int)r_kl[nb] & 0xFF) + ((kn - 1) << EV_LGR); }
                } else {
                    int wslot = q - nruns, lv = 0;                                // left-over level lv: the rays with more than lv left-overs
                    while (wslot >= nwb) { wslot -= nwb; ++lv; }
                    const int bb = lane * nwb + wslot;
                    if (bb < v.B) {
                        const int kl = (int)r_kl[bb], len = kl >> 8;
                        if ((len & (EV_R - 1)) > lv) { nb = bb; nfs = r_fs[bb]; nend = r_end[bb]; nk0 = (kl & 0xFF) + (len & ~(EV_R - 1)) + lv; }
                    }
                }
            };
            // (Drawing the items from a queue balances the waves - the oldest wave of every SIMD is served first and waits a third
            // of the walk for the youngest - and was 0.7 % faster, at the price of 20 spilled registers: 330 MB of scratch traffic per
            // 4096-particle launch.  A fixed share per wave it is.)
            fetch_item(wave_u);
            for (int q = wave_u; q < nitems; q = UNI(q + EB / 64)) {
                const int b = nb; const uint32_t fs = nfs; const int32_t re = nend;
                const int k = nk0;                                                // the item's first chunk
                const int nch = q < nruns ? EV_R : 1;                               // its chunks
                if (b < 0) { fetch_item(q + EB / 64); continue; }
                const int ex = (int)(int16_t)(re & 0xFFFF), ey = (int)(int16_t)((uint32_t)re >> 16);
                const int aex = ex < 0 ? -ex : ex, aey = ey < 0 ? -ey : ey;
                const int sxs = ex > 0 ? stride : -stride, sy1 = ey > 0 ? 1 : -1;
                const int cj = aey > aex ? sy1 : sxs, cm = aey > aex ? sxs : sy1;
                int j0 = NEAR_R + (k - 1) * LCH;
                const unsigned long long pr64 = (unsigned long long)fs * (unsigned)j0 + 0x80000000ull;
                uint32_t acc = (uint32_t)pr64;
                int c = base0 + __mul24(j0, cj) + __mul24((int)(pr64 >> 32), cm);
                const int d0 = cj, d1 = cj + cm;
                // chunk after chunk: sixteen adds in flight, one wait, their sixteen answers; after step 15 the accumulator and the
                // address are those of the next chunk's step 0 (not unrolled: one set of answers' registers)
#pragma nounroll
                for (int i = 0; i < nch; ++i, j0 += LCH) {
                    uint32_t m = 0;
                    uint32_t ret[LCH]; int sh[LCH];
#pragma unroll
                    for (int u = 0; u < LCH; ++u) {
                        sh[u] = c << 3;
                        ret[u] = ev_lds_add_rtn(c & ~3, 2u << (sh[u] & 31));
                        const uint32_t nacc = acc + fs;
                        c += nacc < acc ? d1 : d0;
                        acc = nacc;
                    }
                    if (i == 0) fetch_item(q + EB / 64);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_waitcnt(0xC07F);                            // lgkmcnt(0): one wait, then the sixteen answers
#pragma unroll
                    for (int u = 0; u < LCH; ++u) m = __builtin_amdgcn_alignbit(ev_flag_bit(ret[u], sh[u]), m, 1);
                    if (m) log_events(m, b, j0, ev_lo, ev_hi, gx_base, !whole);
                }
            }
        }
        BAR_LDS();
        STAMP(3);
        // ---- the 16-bit block's counts go into the window (saturated: only min(n, sat) matters for an unflagged cell;
        //      a flagged one arrives with its count of one and stays "touched") ----
        for (int mi = tid; mi < NEAR_W * NEAR_W; mi += EB) {
            const int row = x0 + mi / NEAR_W - NEAR_R - gx_base, col = y0 + mi % NEAR_W - NEAR_R - gy_base;
            if ((unsigned)row >= (unsigned)rows_w || (unsigned)col >= (unsigned)stride) continue;
            const uint32_t f = ((mini[mi >> 1] >> ((mi & 1) * 16)) & 0xFFFFu) >> 1;
            if (f) cnt8[row * stride + col] = (uint8_t)(min(f, (uint32_t)sat) << 1);
        }
        if (tid == 0) s_wbq = 0;
        BAR_LDS();
        // the next particle's record, as one more item of the write-back's queue: the wave that makes it joins the others a batch or so later
        if (S1 == S_hi && wave == EB / 64 - 1 && nxt_p < v.P) ev_prefetch(v, nxt_p, rec, lane);
        // ---- write-back (rbpf_mapupdate.h): the flagged cells get a value from their counts like all others; their real value
        //      follows after the windows.  A tile row of whole 32-cell groups under a fan that is not thin (both uniform over the
        //      workgroup; 0.05 m cells: dim 800) takes the instantiation without the partial group's word tests and the thin fan's branch ----
        if (v.dim % 32 == 0 && !sparse)
            strip_write_back<FIELD_COUNT_HI, false, false, false>(v, sg, S0, S1, gx_base, C, fxl, ggf_base, wbk, cnt, gxb, gym, s_ggf, s_tab, s_need,
                                                                  &s_wbq, &s_written, false, lane);
        else
            strip_write_back<FIELD_COUNT_HI, true, true, false>(v, sg, S0, S1, gx_base, C, fxl, ggf_base, wbk, cnt, gxb, gym, s_ggf, s_tab, s_need,
                                                                &s_wbq, &s_written, sparse, lane);
        STAMP(4);
    }
    BAR_LDS();                                                                // the window's LDS is free (the write-back's stores are still on their way)
#ifdef EV_STAMP_SPLIT
    STAMP(5);
#endif

    // ======================================== flagged cells ========================================
    uint32_t* const keys = reinterpret_cast<uint32_t*>(smem + G.o_cnt + G.p_keys);    // [T] storage cell, ~0 = empty
    uint32_t* const head = reinterpret_cast<uint32_t*>(smem + G.o_cnt + G.p_cnta);    // [T] first pair of the cell's list, 0xFFFF = none
    uint16_t* const iclast = reinterpret_cast<uint16_t*>(smem + G.o_cnt + G.p_offs);  // [T] passes after the cell's last event
    int8_t*   const oldc = reinterpret_cast<int8_t*>(smem + G.o_cnt + G.p_oldv);      // [T] the cell's value before the scan
    uint16_t* const rlist = reinterpret_cast<uint16_t*>(smem + G.o_cnt + G.p_rlist);  // [records] slots in use
    uint16_t* const nextp = reinterpret_cast<uint16_t*>(smem + G.o_cnt + G.p_evl);    // [pairs] next pair (beam << 1 | nearby) on the same cell
    uint16_t* const evl = nextp + al16(G.E * 2) / 2;                               // [pairs] the lists, one after the other (laid out by the fold)
    uint16_t* const ic16 = reinterpret_cast<uint16_t*>(smem + G.o_cnt + G.p_ic);      // [pairs] passes right before the pair's event
    const int T = G.T;
    const int nev_all = UNI(s_nev);
    const bool overflow = nev_all > EVCAP;
    for (int i = tid; i < T / 4; i += EB) { reinterpret_cast<uint4*>(keys)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu); reinterpret_cast<uint4*>(head)[i] = make_uint4(0xFFFFu, 0xFFFFu, 0xFFFFu, 0xFFFFu); }
    for (int i = tid; i < T / 8; i += EB) reinterpret_cast<uint4*>(iclast)[i] = make_uint4(0, 0, 0, 0);
    for (int i = tid; i < al16(G.E * 2) / 16; i += EB) reinterpret_cast<uint4*>(ic16)[i] = make_uint4(0, 0, 0, 0);
    if (tid == 0) { s_wsum[0] = 0; s_wsum[1] = 0; }
    BAR_LDS();
    // every pair joins the list of its cell (the cell's first pair lists the cell and leaves its old value)
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
        if (my_sc[i] == 0xFFFFFFFFu) continue;
        bool created;
        const int h = ev_hash_insert(keys, T, G.logT, my_sc[i], created);
        {   // a record per new cell: the wave's new cells take their places in the record list with ONE add (1300 returning adds
            // on one LDS word stand in line otherwise)
            const unsigned long long mk = __ballot(created);
            if (created) {
                const int first = __ffsll((long long)mk) - 1;
                int base = 0;
                if (lane == first) base = atomicAdd(&s_wsum[1], __popcll(mk));
                base = __shfl(base, first, 64);
                rlist[base + __popcll(mk & ((1ull << lane) - 1ull))] = (uint16_t)h; oldc[h] = (int8_t)my_old[i];
            }
        }
        nextp[tid + i * EB] = (uint16_t)atomicExch(&head[h], (uint32_t)(tid + i * EB));
    }
    BAR_LDS();
#ifndef EV_STAMP_SPLIT
    STAMP(5);
#endif
    if (!overflow) {
        // every listed pass is counted in front of the first event of a beam that is not smaller than its own (a beam's own
        // passes come before its own occupied / nearby hit), or behind the cell's last event
        for (int e = tid; e < nev_all; e += EB) {
            const uint32_t ev = evlist[e];
            const int b = (int)(ev >> 10), j = (int)(ev & 1023u);
            const RayDir d = ray_dir(b);
            const int mn = ev_minor(r_fs[b], j);
            const int gx = x0 + d.sx * (d.steep ? mn : j), gy = y0 + d.sy * (d.steep ? j : mn);
            const int h = ev_hash_find(keys, T, G.logT, ((uint32_t)ux[gx - fxl] << 16) | (uint32_t)uy[gy - fyl]);
            if (h < 0) continue;                                                 // (cannot happen: only flagged fields report)
            int best = 0xFFFF;
            for (int m = (int)head[h]; m != 0xFFFF; m = nextp[m]) if (m >= 2 * b && m < best) best = m;
            uint16_t* const slot = best != 0xFFFF ? &ic16[best] : &iclast[h];
            atomicAdd(reinterpret_cast<unsigned int*>(reinterpret_cast<uintptr_t>(slot) & ~(uintptr_t)3), (reinterpret_cast<uintptr_t>(slot) & 2) ? 0x10000u : 1u);
        }
    }
    __syncthreads();                                                          // every store of the write-back has landed: the flagged cells' bytes follow
    STAMP(6);
    // the byte and the occupancy bit of a flagged cell
    auto store_cell = [&](uint32_t key, int val) {
        int tile, row_t, col_t;
        cell_addr((int)(key >> 16), (int)(key & 0xFFFFu), tile, row_t, col_t);
        if (tile < 0) return;
        v.pool[(size_t)tile * v.dim * v.dim + (size_t)row_t * v.dim + col_t] = (int8_t)val;
        uint32_t* ow = &v.occ[((size_t)tile * v.dim + row_t) * v.ow + (col_t >> 5)];
        if (val > v.cc.thr) atomicOr(ow, 1u << (col_t & 31)); else atomicAnd(ow, ~(1u << (col_t & 31)));
    };
    const int NR = UNI(s_wsum[1]);
    if (!overflow) {
        for (int r = tid; r < NR; r += EB) {
            const int h = rlist[r];
            int val = (int)oldc[h];
            // ONE walk of the cell's list: its length, its smallest and largest pair, and the pairs as bits of a 128-bit set
            // round the first one (w0: pairs first - 64 .. first - 1, w1: first .. first + 63)
            const int first = (int)head[h];
            int n = 0, plo = 0xFFFF, phi = 0;
            unsigned long long w0 = 0, w1 = 0;
            for (int m = first; m != 0xFFFF; m = nextp[m]) {
                ++n; plo = min(plo, m); phi = max(phi, m);
                const int d = m - first;
                if ((unsigned)(d + 64) < 64u) w0 |= 1ull << ((d + 64) & 63);
                if ((unsigned)d < 64u) w1 |= 1ull << (d & 63);
            }
            if (phi - plo < FOLD_SPAN) {
                // the cell's pairs lie within 64 of each other (the beams that end in one cell are neighbours in the scan):
                // bit i of the set = pair plo + i.  Its bits in rising order are the events in (beam, nearby) order, and
                // the neighbours of a bit say what the list's order said: pair e - 1 of the same beam right before an
                // odd e, pair e + 1 right after an even one.
                const int s = plo - first + 64;                                       // 1 .. 64
                const unsigned long long set = s == 64 ? w1 : (w0 >> (s & 63)) | (w1 << ((64 - s) & 63));
                unsigned long long rest = set;
                while (rest) {
                    const int bit = __ffsll((long long)rest) - 1;
                    rest &= rest - 1;
                    const int ek = plo + bit;
                    const bool below = bit > 0 && ((set >> ((bit - 1) & 63)) & 1ull), above = bit < 63 && ((set >> ((bit + 1) & 63)) & 1ull);
                    // the beam's own pass over the cell before its nearby hit is not in the list: it precedes the beam's first event here
                    const bool own_pass = (ek & 1) ? !below : above;
                    const int np = (int)ic16[ek] + (own_pass ? 1 : 0);
                    val = max(val + min(np, sat) * v.cc.emp, v.cc.vmin);              // gridmap.py:97-101, np times
                    val = min(val + ((ek & 1) ? v.cc.nearby : v.cc.occ), v.cc.vmax);  // gridmap.py:86-90 / 108-112
                }
                val = max(val + min((int)iclast[h], sat) * v.cc.emp, v.cc.vmin);
                store_cell(keys[h], val);
                continue;
            }
            // pairs further apart (beams out of angular order, a scan that wraps round): laid out one after the other
            const int o2 = atomicAdd(&s_wsum[0], n);
            { int i = 0; for (int m = (int)head[h]; m != 0xFFFF; m = nextp[m]) evl[o2 + i++] = (uint16_t)m; }
            // the events in ascending (beam, nearby) order: the smallest one above the last, n times (a handful per cell)
            int cur = -2;
            for (int i = 0; i < n; ++i) {
                int ek = 0x7FFFFFFF, nx = 0x7FFFFFFF;                                 // the next event and the one after it
                for (int q = 0; q < n; ++q) { const int e = evl[o2 + q]; if (e > cur) { if (e < ek) { nx = ek; ek = e; } else if (e < nx) nx = e; } }
                const int beam = ek >> 1;
                // the beam's own pass over the cell before its nearby hit is not in the list: it precedes the beam's first event here
                const bool has_near = (ek & 1) || nx == ek + 1;
                const int np = (int)ic16[ek] + ((beam != (cur >> 1) && has_near) ? 1 : 0);
                val = max(val + min(np, sat) * v.cc.emp, v.cc.vmin);              // gridmap.py:97-101, np times
                val = min(val + ((ek & 1) ? v.cc.nearby : v.cc.occ), v.cc.vmax);  // gridmap.py:86-90 / 108-112
                cur = ek;
            }
            val = max(val + min((int)iclast[h], sat) * v.cc.emp, v.cc.vmin);
            store_cell(keys[h], val);
        }
    } else {
        // more passes over flagged cells than the list holds: every flagged cell is replayed by a wave with the exact
        // closed-form membership test over all beams (rbpf_mapupdate.h), whatever the list says
        for (int r = wave; r < NR; r += EB / 64) {
            const int h = rlist[r];
            const uint32_t key = keys[h];
            FCell f;
            sources(key, f);
            const int gxc[2] = {f.gx0, f.gx1}, gyc[2] = {f.gy0, f.gy1};
            const int val = replay_cell_wave(v, r_info, r_end, x0, y0, gxc, f.ngx, gyc, f.ngy, (int)oldc[h], lane);
            if (lane == 0) store_cell(key, val);
        }
        if (tid == 0) atomicAdd(&v.stats[ST_SLOW_CELLS], (unsigned long long)NR);
    }
    STAMP(7);
#if defined(RBPF_STAMPS) && defined(EV_BARRIER_WAITS)
    if (p == 0 && lane == 0) printf("wave %2d: %6lld cycles at %d barriers of %lld: %d %d %d %d %d %d %d %d\n", wave, bar_wait, bar_n, clock64() - t_begin, bar_w[0], bar_w[1], bar_w[2], bar_w[3], bar_w[4], bar_w[5], bar_w[6], bar_w[7]);
#endif
    if (tid == 0) {
        if (s_cells) atomicAdd(&v.stats[ST_RAY_CELLS], s_cells);
        if (s_written) atomicAdd(&v.stats[ST_CELLS_WRITTEN], (unsigned long long)s_written);
        atomicAdd(&v.stats[ST_MAP_WINDOWS], (unsigned long long)n_win);
        atomicAdd(&v.stats[ST_MAP_EVENTS], (unsigned long long)nev_all);
        if (overflow) atomicAdd(&v.stats[ST_EV_OVERFLOWS], 1ull);
        STAMP_FLUSH();
    }
}

// Resident workgroups (`resident` != 0, grid = min(P, CUs)): a workgroup fills a CU (1024 threads, ~157 KB of LDS), so with
// one workgroup per particle nothing covers the time between a workgroup's last wave and the first instruction of the next
// one on that CU.  Here a workgroup runs particle blockIdx.x, then whatever the queue word v.ev_queue[0] hands it, until an
// index >= P comes back.  The barrier between two particles waits for LDS traffic only: the static __shared__ words and
// the window are reused, the previous particle's stores to its own tiles stay in flight.  No workgroup waits for
// another one, so nothing depends on how many of them run at the same time.  The queue re-arms itself: a workgroup
// that leaves has made its last draw, so the one that counts itself last in v.ev_queue[1] puts both words back to
// zero for the next launch in the stream.  resident == 0: one workgroup per particle, no draw (A/B runs, tests).
// Both count in positions of the launch (ev_position): a workgroup whose first position lies behind the last particle that
// stays runs nothing and leaves.
// THE KERNEL HAS ONE ARGUMENT, this struct: the loop below reads `v` through the kernel-argument segment's own address, where a
// sole argument lies by construction (and `v` first in it: the static_assert).  Do not add a second argument; add a member.
struct EvKernArgs { DevView v; int resident; };
static_assert(offsetof(EvKernArgs, v) == 0 && std::is_standard_layout<EvKernArgs>::value, "map_update_ev_kernel reads DevView at offset 0 of its argument segment");
__global__ __launch_bounds__(EB) void map_update_ev_kernel(EvKernArgs ka_) {
    const DevView& v = ka_.v;
    const int resident = ka_.resident;
    __shared__ int s_next[2];                      // the next particle, by parity of the round: a wave may still read one while thread 0 writes the other
    __shared__ EvNext s_rec;
    if (threadIdx.x == 0) s_rec.p = -1;
    __syncthreads();
    int p = ev_position(v, (int)blockIdx.x);
    for (int it = 0; p < v.P; ++it) {
        // The particle's code reads the kernel's arguments through a pointer the compiler cannot see through: whatever it works out
        // from them is worked out per particle, as in a kernel of its own.  (Known to be the same for every particle it was kept in
        // registers across the whole loop: 79 of them spilled to scratch.)
#if __HIP_DEVICE_COMPILE__
        const __attribute__((address_space(4))) DevView* ka = (const __attribute__((address_space(4))) DevView*)__builtin_amdgcn_kernarg_segment_ptr();   // (EvKernArgs::v, offset 0)
        asm volatile("" : "+s"(ka));
        const DevView& vp = *(const DevView*)ka;
#else
        const DevView& vp = v;
#endif
        EV_TURN_IN(p);
        map_update_ev_particle(vp, p, resident != 0, &s_next[it & 1], &s_rec);
        EV_TURN_OUT(p);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // (BAR_LDS; the barrier-wait diagnostic redefines that for the particle's own)
        p = UNI(s_next[it & 1]);
    }
    if (resident && threadIdx.x == 0 && atomicAdd(&v.ev_queue[1], 1u) == gridDim.x - 1u) { atomicExch(&v.ev_queue[0], 0u); atomicExch(&v.ev_queue[1], 0u); }
}

static int device_cu_count() {
    static int cus[MAX_DEVICES] = {};
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < MAX_DEVICES && cus[dev] > 0) return cus[dev];
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) { (void)hipGetLastError(); n = 1; }
    if (dev >= 0 && dev < MAX_DEVICES) cus[dev] = n;
    return n;
}

// t0 / t1 (or nullptr): timing events that take the kernel's own start and end (hipExtLaunchKernelGGL: the dispatch carries
// them, no event records - and their barriers - in the stream)
// Returns the workgroups it launched.
int launch_map_update_ev(const DevView& v, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
    const EvGeom g = ev_geom(v.B, v.reach);
    static size_t lds_set[MAX_DEVICES] = {};
    ensure_dynamic_lds(reinterpret_cast<const void*>(map_update_ev_kernel), (size_t)g.bytes, lds_set);
    int grid = v.P;
    if (v.ev_resident) {
        grid = std::min(v.P, device_cu_count());
        if (v.ev_grid > 0) grid = std::min(grid, v.ev_grid);
    }
    ev_turnover_begin(s);
    const EvKernArgs args = {v, v.ev_resident};
    if (t0 && t1) hipExtLaunchKernelGGL(map_update_ev_kernel, dim3(grid), dim3(EB), (size_t)g.bytes, s, t0, t1, 0, args);
    else hipLaunchKernelGGL(map_update_ev_kernel, dim3(grid), dim3(EB), (size_t)g.bytes, s, args);
    ev_turnover_end(v, grid, s);
    return grid;
}

}  // namespace rbpf
