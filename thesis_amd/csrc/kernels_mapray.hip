// kernels_mapray.hip -- a5: HybridMap.update (hybridmap.py:95-145), counters in GLOBAL cell-index space.
//
// One 1024-thread workgroup per particle (16 waves, one workgroup per CU).  Same exact semantics as the other two map
// kernels (kernels_mapupdate.hip has the ordered-replay argument); what differs:
//
//   * The LDS hit counters are indexed by the reference's global integer cell index (hybridmap.py:102,106,123), the
//     space its Bresenham walks in, not by storage index.  A ray step is then pure arithmetic - no index-map lookups,
//     no "irregular" path on the negative side of a tile where the reference's float index formula (gridmap.py:93,
//     SURVEY quirk 3) mis-rounds.  The index map is verified per particle to have the form U(g) = g + C - G(g),
//     G(g) in {0,1} (it can only round DOWN); the write-back folds it in: storage cell s receives global cell s - C
//     when that one is not glitched, plus global cell s - C + 1 when that one is.
//   * Walk: lanes are rays, a work item is a 16-step chunk of 64 rays, each step from the closed form
//     minor(j) = (fstep * j + 2^21) >> 22 (rbpf_math.h / fix_slope); the adds are fire-and-forget LDS atomics: nothing
//     waits for a returned value, nothing is detected.
//   * Cells that receive an "occupied" / "nearby" hit (the only ones whose clamped adds do not commute) are not found
//     by the walk.  The rays through a cell at major distance j, minor offset c are exactly those of the matching
//     direction class whose fixed-point slope lies in [ceil((c*2^22 - 2^21)/j), ceil(((c+1)*2^22 - 2^21)/j)) and that
//     are longer than j; rays are bucketed by (class, slope >> 14) and sorted once per particle, so each such cell
//     GATHERS its few rays from a contiguous run, sorts the (beam, rank) events in registers and replays them.  Cells
//     next to the sensor, which most rays cross, take their events from a second walk of the 16-bit block instead and
//     need only the number of unoccupied passes between consecutive occupied / nearby events.  This happens before
//     anything is written, so every table overflow still hands the particle back untouched.
//   * A fan larger than the LDS window is processed in strips of storage rows (one launch, any fan size): cell sizes
//     of 0.025 m and 15 m rays included.  8-bit counters cannot overflow: a bound on the hits of any cell with j >= 16
//     is checked from the slope buckets first (cells nearer than NEAR_R steps live in a 16-bit block).
#include <hip/hip_ext.h>

#include "rbpf_mapupdate.h"

namespace rbpf {

static const int RB = 1024;                    // threads per particle
static const int RFIX = 22;                    // fixed-point bits of the slope (fix_slope)
static const int BIN_SHIFT = RFIX - 8;
static const int RSLOW = 256;                  // flagged cells replayed by the wave-wide exact scan, per particle
static const int ECAP = 16;                    // events per flagged cell kept in its list (more: the wave-wide scan)
static const int NNEAR = 128;                  // flagged cells inside the 16-bit block that collect their events from the block's walk
static const int NSPC = 32;                    // occupied / nearby events of such a cell
static const int NPOOL = 48;                   // flagged cells with more than ECAP events: lists of PCAP events, sorted and folded by a wave
static const int PCAP = 64;
static const int RSPEC = 512;                  // flagged cells on an axis or a diagonal through the sensor, per particle
static const int HIT_BOUND = 63;               // per direction class; two classes can meet in one cell: 126 < 128

struct RayGeom {
    int fanw, bpad, ncell;
    int o_cnt, o_mini, o_rend, o_rinfo, o_fstep, o_ux, o_uy, o_gxb, o_gyb, o_gym, o_bins, o_brays, o_oval, o_slow, o_oldv, o_rcc, o_rdmaj, o_perm, o_rpos, o_pflag, o_nid, o_nearl;
    int bytes;
    bool ok;
};

__host__ __device__ inline RayGeom ray_geom(int B, int reach) {
    RayGeom g;
    g.fanw = (2 * reach + 8 + 7) & ~7;
    g.bpad = (B + 3) & ~3;
    int o = 0;
    g.o_mini = o;  o += al16(((NEAR_W * NEAR_W + 1) / 2) * 4);
    g.o_rend = o;  o += al16(g.bpad * 4);
    g.o_fstep = o; o += al16(g.bpad * 4);
    g.o_rinfo = o; o += al16(g.bpad);
    g.o_ux = o;    o += al16(g.fanw * 2);
    g.o_uy = o;    o += al16(g.fanw * 2);
    g.o_gxb = o;   o += al16(g.fanw);
    g.o_gyb = o;   o += al16(g.fanw);
    g.o_gym = o;   o += al16(g.fanw + 16);
    g.o_bins = o;  o += 8 * NBIN * 2;                  // 2048 packed 16-bit fill pointers = one 32-bit word per thread
    g.o_brays = o; o += al16(g.bpad * 2);
    g.o_oval = o;  o += al16(g.bpad * 2);
    g.o_slow = o;  o += RSLOW * 2;
    g.o_oldv = o;  o += al16(g.bpad * 2);
    g.o_rcc = o;   o += al16(g.bpad * 4);
    g.o_rdmaj = o; o += al16(g.bpad * 2);
    g.o_perm = o;  o += al16(g.bpad * 2);
    g.o_rpos = o;  o += al16(g.bpad * 2);
    g.o_pflag = o; o += al16(g.bpad * 2);
    g.o_nid = o;   o += al16(NEAR_W * NEAR_W);
    g.o_nearl = o; o += NNEAR * 2;
    g.o_cnt = o;
    const int avail = 160 * 1024 - 2048 - o - 64;      // 2 KB for the kernel's static LDS
    g.ncell = avail > 0 ? avail & ~127 : 0;
    g.bytes = o + g.ncell;
    g.ok = g.ncell >= 24576 && B <= 4095 && reach >= NEAR_R + 4 && reach < 1000 && 2LL * reach * reach < (1LL << RFIX);
    return g;
}

// the flagged-cell pass borrows the counter window: 16-bit event counts, ECAP events per pair, the special list
__host__ __device__ inline bool ray_lists_fit(const RayGeom& g) {
    const int npair = 2 * g.bpad;
    return npair * 2 + npair * ECAP * 2 + RSPEC * 2 + g.bpad * 8 + npair * 2 + NPOOL * (PCAP * 2 + 4) + 64 <= g.ncell &&   // + the sorted ray records, the list of pairs in play, the long lists
           npair * 2 + npair * ECAP * 2 + RSPEC * 2 + (RB / 64) * 256 * 4 <= g.ncell;                                      // the bucket sort's key scratch in the records' place
}

bool map_update_ray_available(const DevView& v) {
    const RayGeom g = ray_geom(v.B, v.reach);
    return g.ok && ray_lists_fit(g) && lattice_fits_byte_fields(v.cc) && v.dim % 32 == 0 && v.L * v.L <= 49;
}

__device__ __forceinline__ uint32_t ray_fix_slope(int dmin, int dmaj) {
    return dmaj ? (((uint32_t)dmin << RFIX) + (uint32_t)dmaj - 1u) / (uint32_t)dmaj : 0u;
}

// Fire-and-forget adds on hit fields, addressed by field index + the array's LDS address folded into the index (the
// addresses are multiples of 4, so the field's position inside its word is unchanged): the LDS instruction takes the
// masked index as its address, without a separate add of the array's base.
__device__ __forceinline__ void fld8_add(int cabs, uint32_t one) {      // 8-bit fields; cabs = index + lds_addr(array); one = 1 or 0
    __hip_atomic_fetch_add((lds_u32*)(uintptr_t)(uint32_t)(cabs & ~3), one << ((cabs & 3) * 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void fld16_add(int cabs, uint32_t one) {     // 16-bit fields; cabs = index + lds_addr(array) / 2
    __hip_atomic_fetch_add((lds_u32*)(uintptr_t)(uint32_t)((cabs << 1) & ~3), one << ((cabs & 1) * 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(RB) void map_update_ray_kernel(DevView v, const int32_t* __restrict__ only) {
    if (only && !only[blockIdx.x]) return;                                 // the kernel that ran first did this particle
    if (v.mu_skip && v.mu_skip[blockIdx.x]) return;                        // the coming resample discards it (DevView::mu_skip)
    extern __shared__ __align__(16) unsigned char smem[];
    const RayGeom G = ray_geom(v.B, v.reach);
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(smem + G.o_cnt);     // 8-bit hit fields, [row = global x][col = global y]
    uint8_t*  const cnt8 = smem + G.o_cnt;
    uint32_t* const mini = reinterpret_cast<uint32_t*>(smem + G.o_mini);   // [NEAR_W^2] 16-bit fields around the start cell
    int32_t*  const r_end = reinterpret_cast<int32_t*>(smem + G.o_rend);   // [B] packed end cell relative to the start
    uint32_t* const r_fstep = reinterpret_cast<uint32_t*>(smem + G.o_fstep); // [B] fixed-point slope
    uint8_t*  const r_info = smem + G.o_rinfo;                             // [B]
    uint16_t* const ux = reinterpret_cast<uint16_t*>(smem + G.o_ux);       // U of global column fxl + i
    uint16_t* const uy = reinterpret_cast<uint16_t*>(smem + G.o_uy);
    uint8_t*  const gxb = smem + G.o_gxb;                                  // G of global column fxl + i (0 / 1)
    uint8_t*  const gyb = smem + G.o_gyb;
    uint8_t*  const gym = smem + G.o_gym;                                  // G of window column lc as a byte mask (0 / 0xFF)
    uint32_t* const bins32 = reinterpret_cast<uint32_t*>(smem + G.o_bins); // [8 * NBIN] 16-bit counts, then fill pointers
    uint16_t* const bins16 = reinterpret_cast<uint16_t*>(smem + G.o_bins);
    uint16_t* const brays = reinterpret_cast<uint16_t*>(smem + G.o_brays); // ray ids ordered by (class, slope bucket)
    uint8_t*  const oval = smem + G.o_oval;                                // [2 * B] replayed value - vmin of the cell flagged by (beam, e); 0xFF = none / not the owner
    uint16_t* const slowl = reinterpret_cast<uint16_t*>(smem + G.o_slow);  // [RSLOW] (beam << 1) | e
    uint8_t*  const oldv8 = smem + G.o_oldv;                               // [2 * B] its value before the scan
    uint32_t* const r_cc = reinterpret_cast<uint32_t*>(smem + G.o_rcc);    // [B] window-address steps of the ray: per major step | per minor step << 16
    uint16_t* const r_dmaj = reinterpret_cast<uint16_t*>(smem + G.o_rdmaj); // [B] last step of the ray
    uint16_t* const perm = reinterpret_cast<uint16_t*>(smem + G.o_perm);   // rays ordered by falling count of whole 16-step chunks
    uint16_t* const rpos = reinterpret_cast<uint16_t*>(smem + G.o_rpos);   // [B] position of the ray in brays
    uint8_t*  const nid = smem + G.o_nid;                                  // [NEAR_W^2] list position of the flagged cell a block cell is a source of, 0xFF = none
    uint16_t* const nearl = reinterpret_cast<uint16_t*>(smem + G.o_nearl); // [NNEAR] owner pairs of those cells
    uint8_t*  const pflag = smem + G.o_pflag;                              // [2 * B] 0 = pair not in play, 1 = gathered, 2 = other classes too

    __shared__ int s_fb;
    __shared__ int s_need[49], s_tab[49];
    __shared__ int s_fan[4];
    __shared__ int s_wsum[RB / 64];
    __shared__ int s_nslow, s_written, s_nspec, s_nact, s_exact, s_nnear, s_npool, s_wbq;
    __shared__ int s_npoolf, s_nnearf;                // cells folded from a pool list / from the block's second walk (tallies only)
    __shared__ int s_lcnt[MAXLEV + 1], s_lfill[MAXLEV + 1], s_nk[MAXLEV + 2], s_lp[MAXLEV + 3], s_nlev;
    __shared__ unsigned long long s_cells;
    __shared__ double s_sincos[2];
    __shared__ uint8_t s_ggf[96];                     // 32-column storage group g (from T_lo >> 5): a glitched column among its 33

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int LL = v.L * v.L;
    int32_t* tab = v.tile_tab + (size_t)v.slot[p] * LL;

    STAMP_DECL;
    // =============================================== setup ===============================================
    const int pb0 = tid, pb1 = tid + RB;
    const double pre_x0 = pb0 < v.B ? v.bx[pb0] : 0.0, pre_y0 = pb0 < v.B ? v.by[pb0] : 0.0;
    const double pre_x1 = pb1 < v.B ? v.bx[pb1] : 0.0, pre_y1 = pb1 < v.B ? v.by[pb1] : 0.0;
    const int pre_f0 = pb0 < v.B ? v.bflags[pb0] : 0, pre_f1 = pb1 < v.B ? v.bflags[pb1] : 0;
    const double s_px = v.upd_pose[p], s_py = v.upd_pose[v.P + p];
    int x0, y0;
    if (!fan_preamble<RB>(v, tab, p, tid, s_px, s_py, v.reach, G.fanw, s_sincos, ux, uy, x0, y0)) return;
    const int fxl = x0 - v.reach - 2, fyl = y0 - v.reach - 2, nfx = 2 * v.reach + 5;
    if (tid == 0) {
        s_fan[0] = x0; s_fan[1] = x0; s_fan[2] = y0; s_fan[3] = y0;
        s_cells = 0; s_fb = 0; s_written = 0; s_nslow = 0; s_nspec = 0; s_nact = 0; s_exact = 0; s_nnear = 0; s_npool = 0; s_npoolf = 0; s_nnearf = 0;
    }
    for (int i = tid; i < LL; i += RB) { s_need[i] = 0; s_tab[i] = tab[i]; }
    bins32[tid] = 0;
    if (tid < 96) s_ggf[tid] = 0;
    if (tid <= MAXLEV) s_lcnt[tid] = 0;
    for (int i = tid; i < (NEAR_W * NEAR_W + 1) / 2; i += RB) mini[i] = 0;
    for (int i = tid; i < (NEAR_W * NEAR_W + 3) / 4; i += RB) reinterpret_cast<uint32_t*>(nid)[i] = 0xFFFFFFFFu;
    for (int i = tid; i < (2 * G.bpad + 3) / 4; i += RB) reinterpret_cast<uint32_t*>(oval)[i] = 0xFFFFFFFFu;
    __syncthreads();
    STAMP(0);
    const double s_s = s_sincos[0], s_c = s_sincos[1];

    const int C = v.R * v.dim + v.dim / 2;
    const int Uxs = UNI(ux[x0 - fxl]), Uys = UNI(uy[y0 - fyl]);
    const int a0 = Uxs / v.dim, b0 = Uys / v.dim;
    auto lat_x = [&](int g) { const int U = ux[g - fxl]; return a0 + (U >= (a0 + 1) * v.dim ? 1 : 0) - (U < a0 * v.dim ? 1 : 0); };
    auto lat_y = [&](int g) { const int U = uy[g - fyl]; return b0 + (U >= (b0 + 1) * v.dim ? 1 : 0) - (U < b0 * v.dim ? 1 : 0); };
    // pairs (beam, e) and the storage cells they flag, flagged cells and their sources (rbpf_mapupdate.h)
    auto pair_cell = [&](int pr) { return flagged_cell(pr, r_info, r_end, x0, y0, ux, uy, fxl, fyl); };
    auto pair_gcell = [&](int pr) -> uint32_t {          // the same as a global cell relative to the start, biased: never ~0
        int dx, dy;
        return pair_offset(pr, r_info, r_end, dx, dy) ? (uint32_t)(dx + 0x4000) | ((uint32_t)(dy + 0x4000) << 16) : 0xFFFFFFFFu;
    };
    // direction class and slope bucket of a ray
    auto ray_key = [&](int ddx, int ddy, uint32_t fstep) {
        const int adx = ddx < 0 ? -ddx : ddx, ady = ddy < 0 ? -ddy : ddy;
        const int cls = (ady > adx ? 4 : 0) | (ddx > 0 ? 2 : 0) | (ddy > 0 ? 1 : 0);
        const int bin = min((int)(fstep >> BIN_SHIFT), NBIN - 1);
        return cls * NBIN + bin;
    };
    {
        FanBox fan = {x0, x0, y0, y0, 0ull};
        for (int b = tid; b < v.B; b += RB) {
            const double x = b == pb0 ? pre_x0 : b == pb1 ? pre_x1 : v.bx[b], y = b == pb0 ? pre_y0 : b == pb1 ? pre_y1 : v.by[b];
            const int bf = b == pb0 ? pre_f0 : b == pb1 ? pre_f1 : (int)v.bflags[b];
            const BeamRay br = beam_ray(v, x, y, bf, [&] { return v.bscale[b]; }, s_s, s_c, s_px, s_py, x0, y0, a0, b0, lat_x, lat_y, s_need, fan);
            const Ray& r = br.r;
            const int ddx = br.x1 - x0, ddy = br.y1 - y0;
            r_end[b] = (int32_t)(((uint32_t)ddx & 0xFFFFu) | ((uint32_t)ddy << 16));
            uint32_t fstep = 0;
            if (r.n > 0) {
                fstep = ray_fix_slope(r.dmin, r.dmaj);
                const int key = ray_key(ddx, ddy, fstep);
                atomicAdd(&bins32[key >> 1], 1u << ((key & 1) * 16));
                const int nfull = (r.dmaj + 1 - NEAR_R) / LCH;                       // whole chunks beyond the 16-bit block
                if (nfull >= 1) atomicAdd(&s_lcnt[min(nfull, MAXLEV)], 1);
            }
            r_dmaj[b] = (uint16_t)(r.n > 0 ? r.dmaj : 0);
            r_info[b] = (uint8_t)br.info;
            r_fstep[b] = fstep;
        }
        fan_box_join(fan, lane, s_fan, &s_cells);
    }
    __syncthreads();
    STAMP(0);
    // ---- the window (rbpf_mapupdate.h: strips of storage rows if the fan does not fit) ----
    const StripGeom sg = strip_geom<RB>(ux, uy, gxb, gyb, G.fanw, fxl, fyl, C, s_fan, &s_fb, G.ncell, tid);
    const int S_lo = sg.S_lo, S_hi = sg.S_hi, T_lo = sg.T_lo, gy_base = sg.gy_base, stride = sg.stride, rows_cap = sg.rows_cap;
    BAR_LDS();
    if (UNI(s_fb) || rows_cap < 8) { GIVE_BACK(1); }
    alloc_missing_tiles(v, tab, s_need, s_tab, tid);
    if (wave == 0) level_sums(lane, s_lcnt, s_lfill, s_nk, s_lp, &s_nlev);
    glitch_mask<RB>(gyb, gym, s_ggf, T_lo >> 5, 96, sg, G.fanw, fyl, nfx, C, v.dim, v.dim >> 5, tid);
    uint32_t* const farh = cnt;                                                // [8 * NBIN] 16-bit counts of the rays longer than the 16-bit block (the window is not in use yet)
    farh[tid] = 0;
    {   // bucket fill pointers: exclusive prefix sum over the 2048 (class, bucket) counts, two per thread
        const uint32_t w2 = bins32[tid];
        const int c0 = (int)(w2 & 0xFFFFu), c1 = (int)(w2 >> 16), pc = c0 + c1;
        int incl = pc;
        for (int o = 1; o < 64; o <<= 1) { int n = __shfl_up(incl, o, 64); if (lane >= o) incl += n; }
        if (lane == 63) s_wsum[wave] = incl;
        BAR_LDS();
        int wbase = 0;
        for (int k = 0; k < wave; ++k) wbase += s_wsum[k];
        const int excl = wbase + incl - pc;
        bins32[tid] = (uint32_t)excl | ((uint32_t)(excl + c0) << 16);
    }
    BAR_LDS();
    // window-address steps of a ray: per major step (cj) and per minor step (cm)
    auto ray_steps = [&](int b, int& cj, int& cm) {
        const int32_t re = r_end[b];
        const int ex = (int)(int16_t)(re & 0xFFFF), ey = (int)(int16_t)((uint32_t)re >> 16);
        const int aex = ex < 0 ? -ex : ex, aey = ey < 0 ? -ey : ey;
        const int sxs = ex > 0 ? stride : -stride, sy1 = ey > 0 ? 1 : -1;
        cj = aey > aex ? sy1 : sxs; cm = aey > aex ? sxs : sy1;
    };
    for (int b = tid; b < v.B; b += RB) {
        if (!(r_info[b] & RI_VALID)) continue;
        const int32_t e = r_end[b];
        const int key = ray_key((int)(int16_t)(e & 0xFFFF), (int)(int16_t)((uint32_t)e >> 16), r_fstep[b]);
        const int sh = (key & 1) * 16;
        const int pos = (int)((atomicAdd(&bins32[key >> 1], 1u << sh) >> sh) & 0xFFFFu);
        brays[pos] = (uint16_t)b;
        { int cj, cm; ray_steps(b, cj, cm); r_cc[b] = ((uint32_t)cj & 0xFFFFu) | ((uint32_t)cm << 16); }
        const int nfull = ((int)r_dmaj[b] + 1 - NEAR_R) / LCH;
        if (nfull >= 1) perm[atomicAdd(&s_lfill[min(nfull, MAXLEV)], 1)] = (uint16_t)b;
        if ((int)r_dmaj[b] >= NEAR_R) atomicAdd(&farh[key >> 1], 1u << sh);            // only these reach the 8-bit fields
    }
    BAR_LDS();
    // bucket key -> [start, end) in brays (the fill pointers have advanced to the bucket ends)
    auto bkt_start = [&](int key) { return key ? (int)bins16[key - 1] : 0; };
    auto bkt_end = [&](int key) { return (int)bins16[key]; };
    {   // no 8-bit field can overflow: a cell at major distance j >= NEAR_R is hit, per direction class, only by rays
        // that are at least that long and whose slope lies in a window of width 2^RFIX / j + 1 <= 2^RFIX / NEAR_R + 1, i.e. in
        // at most NB_WIN consecutive buckets.  First with all rays of the buckets (two reads of the fill pointers); only when that
        // bound fails, with the rays that are long enough to reach an 8-bit field.
        int mx = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int key = 2 * tid + k, cls = key / NBIN, bin = key % NBIN;
            mx = max(mx, bkt_end(cls * NBIN + min(bin + NB_WIN - 1, NBIN - 1)) - bkt_start(key));
        }
        mx = wave_max(mx);
        if (lane == 0 && mx > HIT_BOUND) s_exact = 1;
        BAR_LDS();
        if (UNI(s_exact)) {
            const uint16_t* fh = reinterpret_cast<const uint16_t*>(farh);
            mx = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int key = 2 * tid + k, cls = key / NBIN, bin = key % NBIN;
                int sum = 0;
                for (int d = 0; d < NB_WIN && bin + d < NBIN; ++d) sum += fh[cls * NBIN + bin + d];
                mx = max(mx, sum);
            }
            mx = wave_max(mx);
            if (lane == 0 && mx > HIT_BOUND) s_fb = 1;
        }
    }
    BAR_LDS();                                                                 // the window's first words become event counts next
    STAMP(1);

    // ---- flagged cells: those that receive an "occupied" or "nearby" hit (hybridmap.py:113,137,139-142) --------------
    // Pair (beam b, e) flags the storage cell of b's end cell (e = 0) or of the cell before it (e = 1); the smallest pair
    // that flags a storage cell owns it.  The rays of a direction class are sorted by slope, and the rays through a cell at
    // major distance j are exactly those with minor(j) = c: a contiguous run in that order around b itself.  Every pair
    // scans its neighbours in its own class (a handful), tests them exactly against the cell's global source cells and
    // keeps the (beam, rank) events; cells that rays of another class can reach too (on an axis or a diagonal through the
    // sensor) are finished by a second, dense pass with one lane per (cell, class).  The counter window is not in use yet:
    // the event lists live there.
    const int sat = sat_passes(v.cc);                                              // hits that saturate any cell: 20
    const int npair = 2 * G.bpad;
    uint32_t* const evn32 = cnt;                                                   // [npair] 16-bit event counts
    uint16_t* const evl = reinterpret_cast<uint16_t*>(cnt + npair / 2);            // [npair][ECAP] (beam << 3) | rank
    uint16_t* const spl = evl + npair * ECAP;                                      // [RSPEC] pairs that need the other classes
    auto sources = [&](uint32_t sc, FCell& f) { cell_sources(sc, C, gxb, gyb, fxl, fyl, f); };
    auto old_value = [&](const FCell& f) {
        const int a = a0 + (f.sx >= (a0 + 1) * v.dim ? 1 : 0) - (f.sx < a0 * v.dim ? 1 : 0);   // rays are shorter than a tile
        const int bb = b0 + (f.sy >= (b0 + 1) * v.dim ? 1 : 0) - (f.sy < b0 * v.dim ? 1 : 0);
        const int tile = s_need[a * v.L + bb] ? s_tab[a * v.L + bb] : -1;
        return tile >= 0 ? (int)v.pool[(size_t)tile * v.dim * v.dim + (size_t)(f.sx - a * v.dim) * v.dim + (f.sy - bb * v.dim)] : 0;
    };
    // does ray rb pass through the global cell at offset (ddx, ddy) from the start cell?  If so: the event's rank and
    // whether the NEARBY event follows (hybridmap.py:139-142).  Exact: the closed form of the reference's Bresenham.
    struct RayP { int ex, ey, dmaj, steep, smaj, smin, info; uint32_t fs; };
    auto load_ray = [&](int rb, RayP& r) {
        const int32_t re = r_end[rb];
        r.ex = (int)(int16_t)(re & 0xFFFF); r.ey = (int)(int16_t)((uint32_t)re >> 16);
        const int aex = r.ex < 0 ? -r.ex : r.ex, aey = r.ey < 0 ? -r.ey : r.ey;
        r.steep = aey > aex; r.dmaj = r.steep ? aey : aex;
        const int sx = r.ex > 0 ? 1 : -1, sy = r.ey > 0 ? 1 : -1;                    // hybridmap.py:282-283
        r.smaj = r.steep ? sy : sx; r.smin = r.steep ? sx : sy;
        r.fs = r_fstep[rb]; r.info = r_info[rb];
    };
    auto ray_hits = [&](const RayP& r, int ddx, int ddy, int& rank, bool& nearev) {
        const int j = (r.steep ? ddy : ddx) * r.smaj, c = (r.steep ? ddx : ddy) * r.smin;   // both must be >= 0
        if (j < 0 || c < 0 || j > r.dmaj) return false;
        if ((int)((r.fs * (uint32_t)j + (1u << (RFIX - 1))) >> RFIX) != c) return false;
        const int rem = r.dmaj - j;                                                  // steps left after this one
        rank = rem == 0 ? ((r.info & RI_OCC) ? EV_OCC : EV_E_LAST) : rem == 1 ? EV_E_2 : rem == 2 ? EV_E_3 : EV_E_FAR;
        nearev = rem == 1 && (r.info & RI_NEAR);
        return true;
    };
    // ---- the 16-bit block: steps 0 .. NEAR_R - 1 of every ray (it outlives the windows) ----
    auto walk_block = [&](bool collect, int* ncur, const int* nend, uint16_t* nev) {
        const int nw0 = (v.B + 63) >> 6;
        for (int q = wave; q < nw0; q += RB / 64) {
            const int b = lane * nw0 + q;                                          // the 64 rays of an instruction point in different directions
            if (b >= v.B || !(r_info[b] & RI_VALID)) continue;
            const uint32_t fs = r_fstep[b];
            const uint32_t cc = r_cc[b];
            const int cj = (int)(int16_t)(cc & 0xFFFFu), cm = (int)cc >> 16;
            const int dmaj = (int)r_dmaj[b];
            const int mj = cj == 1 || cj == -1 ? cj : (cj > 0 ? NEAR_W : -NEAR_W);   // the same steps in the 16-bit block
            const int mm = cm == 1 || cm == -1 ? cm : (cm > 0 ? NEAR_W : -NEAR_W);
            uint32_t facc = 1u << (RFIX - 1);
            int aj = NEAR_R * NEAR_W + NEAR_R;
            if (!collect) {
                aj += lds_addr(mini) >> 1;
#pragma unroll
                for (int u = 0; u < NEAR_R; ++u) {
                    fld16_add(aj + __mul24((int)(facc >> RFIX), mm), u <= dmaj ? 1u : 0u);   // (a step past the end stays inside the block: adds nothing)
                    facc += fs; aj += mj;
                }
            } else {
                const int info = r_info[b];
#pragma unroll
                for (int u = 0; u < NEAR_R; ++u) {
                    const int c = aj + __mul24((int)(facc >> RFIX), mm);
                    const int id = nid[c];
                    if (id != 0xFF && u <= dmaj) {                                     // rare: a source of a flagged cell
                        const int rem = dmaj - u;
                        const bool nearev = rem == 1 && (info & RI_NEAR);
                        const int rank = rem == 0 ? ((info & RI_OCC) ? EV_OCC : EV_E_LAST) : rem == 1 ? EV_E_2 : rem == 2 ? EV_E_3 : EV_E_FAR;
                        const int pos = atomicAdd(&ncur[id], nearev ? 2 : 1);
                        if (pos < nend[id]) nev[pos] = (uint16_t)(b << 3 | rank);
                        if (nearev && pos + 1 < nend[id]) nev[pos + 1] = (uint16_t)(b << 3 | EV_NEAR);
                    }
                    facc += fs; aj += mj;
                }
            }
        }
    };
    walk_block(false, nullptr, nullptr, nullptr);                                  // (no barrier: the waves go on to the bucket sort, whose threads mostly idle)
    {   // order the rays of every bucket by slope (ties by beam): the class is then sorted as a whole; rpos = inverse.
        // A regular scan has one or two rays per bucket (a thread sorts them in place); rays that end on a near surface
        // share end cells, hence slopes: buckets of a dozen or more are ranked by a wave.
        uint16_t* const bigb = evl + npair * ECAP;                                   // (the special list's place: not in use yet)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int key = 2 * tid + k, st = bkt_start(key), en = bkt_end(key);
            if (en - st > 256) s_fb = 1;
            else if (en - st > 6) { const int pos = atomicAdd(&s_nspec, 1); if (pos < RSPEC) bigb[pos] = (uint16_t)key; else s_fb = 1; }
            else for (int i = st + 1; i < en; ++i) {
                const int rb = brays[i];
                const uint32_t fbase = (uint32_t)(key % NBIN) << BIN_SHIFT;          // slopes of a bucket differ in their low 14 (15 in the last) bits
                const uint32_t kf = ((r_fstep[rb] - fbase) << 12) | (uint32_t)rb;
                int q = i - 1;
                while (q >= st) {
                    const int ro = brays[q];
                    if ((((r_fstep[ro] - fbase) << 12) | (uint32_t)ro) <= kf) break;
                    brays[q + 1] = (uint16_t)ro; --q;
                }
                brays[q + 1] = (uint16_t)rb;
            }
        }
        for (int i = tid; i < npair / 2; i += RB) evn32[i] = 0;
        for (int i = tid; i < npair / 4; i += RB) reinterpret_cast<uint32_t*>(pflag)[i] = 0;
        BAR_LDS();
        const int nbig = UNI(min(s_nspec, RSPEC));
        uint32_t* const kscr = reinterpret_cast<uint32_t*>(bigb + RSPEC) + wave * 256;   // the wave's keys (behind the list of big buckets: the ray records are not built yet)
        for (int k = wave; k < nbig; k += RB / 64) {
            const int key = bigb[k], st = bkt_start(key), n = bkt_end(key) - st;   // 7 .. 256 rays (more than 64: a wall right in front of the sensor)
            const uint32_t fbase = (uint32_t)(key % NBIN) << BIN_SHIFT;
            if (n <= 64) {
                const int rb = lane < n ? (int)brays[st + lane] : 0;
                const uint32_t kf = lane < n ? ((r_fstep[rb] - fbase) << 12) | (uint32_t)rb : 0xFFFFFFFFu;
                int rank = 0;
                for (int e = 0; e < n; ++e) rank += (uint32_t)__shfl((int)kf, e, 64) < kf;      // keys are distinct (the beam is part of them)
                if (lane < n) brays[st + rank] = (uint16_t)rb;                       // (every lane has read its own entry)
            } else {
                int rb[4]; uint32_t kf[4]; int rank[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int at = lane + 64 * i;
                    rb[i] = at < n ? (int)brays[st + at] : 0;
                    kf[i] = at < n ? ((r_fstep[rb[i]] - fbase) << 12) | (uint32_t)rb[i] : 0xFFFFFFFFu;
                    if (at < n) kscr[at] = kf[i];
                }
                for (int e = 0; e < n; ++e) {
                    const uint32_t ke = kscr[e];
#pragma unroll
                    for (int i = 0; i < 4; ++i) rank[i] += ke < kf[i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) if (lane + 64 * i < n) brays[st + rank[i]] = (uint16_t)rb[i];
            }
        }
        BAR_LDS();
        if (tid == 0) s_nspec = 0;
    }
    // the sorted order as packed records: one 8-byte read per candidate ray
    uint2* const srec = reinterpret_cast<uint2*>(spl + RSPEC);                     // [B] {slope | OCC << 24 | NEAR << 25, dmaj | beam << 16}
    uint16_t* const alist = reinterpret_cast<uint16_t*>(srec + G.bpad);            // [2 * B] pairs in play
    uint32_t* const poolkey = reinterpret_cast<uint32_t*>(alist + ((npair + 7) & ~7));   // [NPOOL] pair | events << 16 of a long list, ~0 = abandoned
    uint16_t* const pool = reinterpret_cast<uint16_t*>(poolkey + NPOOL);           // [NPOOL][PCAP]
    for (int q = tid; q < UNI(bkt_end(8 * NBIN - 1)); q += RB) {
        const int rb = brays[q];
        rpos[rb] = (uint16_t)q;
        const int info = r_info[rb];
        srec[q] = make_uint2(r_fstep[rb] | ((info & RI_OCC) ? 1u << 24 : 0u) | ((info & RI_NEAR) ? 1u << 25 : 0u),
                             (uint32_t)r_dmaj[rb] | ((uint32_t)rb << 16));
    }
    BAR_LDS();
    STAMP(2);
    // ---- pass 1: one lane per pair scans its beam's neighbours in slope order ----
    // In the frame of the beam's class a storage cell's global source cells are the major steps {j1, j2} x the minor
    // offsets {c1, c2} (the second of each only where the index map repeats a cell); a ray of the class crosses the cell
    // iff minor(j) is c1 or c2 for one of those j it reaches.
    // Pairs in play, listed in beam order: neighbouring beams end on the same surface at similar distances, so the lanes
    // of a wave scan windows of similar width and read neighbouring records.
    {
        for (int i0 = 0; i0 < v.B; i0 += RB) {                                     // wave-uniform trip count (ballot)
            const int i = i0 + tid;
            const int b = i < v.B ? i : -1;
            bool play[2] = {false, false};
            if (b >= 0 && (r_info[b] & (RI_VALID | RI_OCC)) == (RI_VALID | RI_OCC)) {
                // a smaller pair of the neighbouring beams on the same global cell: this one cannot be the owner (the other
                // duplicates show up in the scan)
                const uint32_t g0 = pair_gcell(2 * b), g1 = pair_gcell(2 * b + 1);
                const uint32_t p0 = b >= 1 ? pair_gcell(2 * b - 2) : 0xFFFFFFFFu, p1 = b >= 1 ? pair_gcell(2 * b - 1) : 0xFFFFFFFFu,
                               q0 = b >= 2 ? pair_gcell(2 * b - 4) : 0xFFFFFFFFu;
                if (g0 != p0 && g0 != p1 && g0 != q0) { play[0] = true; pflag[2 * b] = 3; }            // 3 = in play, not classified yet
                if (g1 != 0xFFFFFFFFu && g1 != g0 && g1 != p0 && g1 != p1 && g1 != q0) { play[1] = true; pflag[2 * b + 1] = 3; }
            }
            const unsigned long long m0 = __ballot(play[0]), m1 = __ballot(play[1]);
            int base = 0;
            if (lane == 0 && (m0 | m1)) base = atomicAdd(&s_nact, __popcll(m0) + __popcll(m1));
            base = __shfl(base, 0, 64);
            const unsigned long long lt = (1ull << lane) - 1ull;
            const int pos = base + __popcll(m0 & lt) + __popcll(m1 & lt);
            if (play[0]) alist[pos] = (uint16_t)(2 * b);
            if (play[1]) alist[pos + (play[0] ? 1 : 0)] = (uint16_t)(2 * b + 1);
        }
    }
    BAR_LDS();
    for (int it0 = 0; it0 < UNI(s_nact); it0 += RB) {                              // dense: (almost) every lane has a pair
        const int it = it0 + tid;
        const bool have = it < UNI(s_nact);
        const int mykey = have ? (int)alist[it] : 0;
        const int b = mykey >> 1;
        int nev = 0, oldv = 0, cap = ECAP, slot = -1;
        bool act = false;
        if (have) {
            const int32_t re_b = r_end[b];
            const int ex = (int)(int16_t)(re_b & 0xFFFF), ey = (int)(int16_t)((uint32_t)re_b >> 16);
            const int aex = ex < 0 ? -ex : ex, aey = ey < 0 ? -ey : ey;
            const int steep = aey > aex, dmaj_b = steep ? aey : aex;
            const int smaj = steep ? (ey > 0 ? 1 : -1) : (ex > 0 ? 1 : -1), smin = steep ? (ex > 0 ? 1 : -1) : (ey > 0 ? 1 : -1);
            const int cls = steep * 4 + (ex > 0 ? 2 : 0) + (ey > 0 ? 1 : 0);
            const int cst = bkt_start(cls * NBIN), cen = bkt_end(cls * NBIN + NBIN - 1);
            FCell f;
            sources(pair_cell(mykey), f);
            oldv = old_value(f);                                                   // in flight during the scan
            // sources along the major and the minor axis of the class frame
            const int gmaj0 = steep ? f.gy0 : f.gx0, gmaj1 = steep ? f.gy1 : f.gx1, nmaj = steep ? f.ngy : f.ngx;
            const int gmin0 = steep ? f.gx0 : f.gy0, gmin1 = steep ? f.gx1 : f.gy1, nmin = steep ? f.ngx : f.ngy;
            const int omaj = steep ? y0 : x0, omin = steep ? x0 : y0;
            const int cj1 = (gmaj0 - omaj) * smaj, cj2 = nmaj > 1 ? (gmaj1 - omaj) * smaj : -1;
            const int cc1 = (gmin0 - omin) * smin, cc2 = nmin > 1 ? (gmin1 - omin) * smin : -1;
            const int jmin = nmaj > 1 ? min(cj1, cj2) : cj1, jmax = nmaj > 1 ? max(cj1, cj2) : cj1;
            const int cmin = nmin > 1 ? min(cc1, cc2) : cc1, cmax = nmin > 1 ? max(cc1, cc2) : cc1;
            bool near_cell = false;
#pragma unroll
            for (int ix = 0; ix < 2; ++ix)
#pragma unroll
            for (int iy = 0; iy < 2; ++iy) {
                if (ix >= f.ngx || iy >= f.ngy) continue;
                const int sgx = ix ? f.gx1 : f.gx0, sgy = iy ? f.gy1 : f.gy0;
                const int ddx = sgx - x0, ddy = sgy - y0;
                if (max(ddx < 0 ? -ddx : ddx, ddy < 0 ? -ddy : ddy) < NEAR_R) near_cell = true;
            }
            const bool special = cmin <= 0 || cmax >= jmin;                         // an axis or a diagonal through the sensor: other classes reach it
            if (near_cell) {   // most rays cross it; claimed through bit 15 of the first source's 16-bit field
                const int mi = (f.gx0 - x0 + NEAR_R) * NEAR_W + (f.gy0 - y0 + NEAR_R), sh = (mi & 1) * 16;
                if (!((atomicOr(&mini[mi >> 1], 0x8000u << sh) >> sh) & 0x8000u)) {
                    // every source within the block's walk (steps 0 .. NEAR_R - 1): its events come from that walk;
                    // otherwise (a source on the block's rim) the scan over all beams
                    bool inside = true;
#pragma unroll
                    for (int ix = 0; ix < 2; ++ix)
#pragma unroll
                    for (int iy = 0; iy < 2; ++iy) {
                        if (ix >= f.ngx || iy >= f.ngy) continue;
                        const int ddx = (ix ? f.gx1 : f.gx0) - x0, ddy = (iy ? f.gy1 : f.gy0) - y0;
                        if (max(ddx < 0 ? -ddx : ddx, ddy < 0 ? -ddy : ddy) >= NEAR_R) inside = false;
                    }
                    int pos = inside ? atomicAdd(&s_nnear, 1) : NNEAR;
                    if (pos < NNEAR) {
                        nearl[pos] = (uint16_t)mykey;
#pragma unroll
                        for (int ix = 0; ix < 2; ++ix)
#pragma unroll
                        for (int iy = 0; iy < 2; ++iy) {
                            if (ix >= f.ngx || iy >= f.ngy) continue;
                            nid[((ix ? f.gx1 : f.gx0) - x0 + NEAR_R) * NEAR_W + ((iy ? f.gy1 : f.gy0) - y0 + NEAR_R)] = (uint8_t)pos;
                        }
                    } else {
                        pos = atomicAdd(&s_nslow, 1);
                        if (pos < RSLOW) slowl[pos] = (uint16_t)mykey; else s_fb = 1;
                    }
                }
                pflag[mykey] = 0;
            } else {
                act = true;
                // window on minor(dmaj_b) of a ray that can reach a source: minor() never decreases and moves by at most one
                // per major step, so minor(js) = cs needs minor(dmaj_b) in [cs, cs + (dmaj_b - js)] (js <= dmaj_b) or
                // [cs - (js - dmaj_b), cs] (js > dmaj_b)
                const int lo = cmin - max(0, jmax - dmaj_b), hi = cmax + max(0, dmaj_b - jmin);
                pflag[mykey] = special ? 2 : 1;
                if (special) {
                    const int pos = atomicAdd(&s_nspec, 1);
                    if (pos < RSPEC) spl[pos] = (uint16_t)mykey; else s_fb = 1;
                }
                uint16_t* myev = evl + mykey * ECAP;
                const int q0 = rpos[b];
                // one candidate record: past the window (-> that direction is finished), or tested against the cell's sources
                auto candidate = [&](const uint2 rr, const bool down, bool& finished) {
                    const uint32_t fs = rr.x & 0xFFFFFFu;
                    const int dmaj_r = (int)(rr.y & 0xFFFFu), rb = (int)(rr.y >> 16);
                    const int mg = (int)((fs * (uint32_t)dmaj_b + (1u << (RFIX - 1))) >> RFIX);
                    if (down ? mg < lo : mg > hi) { finished = true; return; }      // sorted by slope: nothing further can reach the cell
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const int jj = w ? cj2 : cj1;
                        if (jj < 0 || jj > dmaj_r) continue;
                        const int m = (int)((fs * (uint32_t)jj + (1u << (RFIX - 1))) >> RFIX);
                        if (m != cc1 && m != cc2) continue;
                        const int rem = dmaj_r - jj;
                        const bool occ_r = (rr.x >> 24) & 1u, nearev = rem == 1 && ((rr.x >> 25) & 1u);
                        const int rank = rem == 0 ? (occ_r ? EV_OCC : EV_E_LAST) : rem == 1 ? EV_E_2 : rem == 2 ? EV_E_3 : EV_E_FAR;
                        if ((rank == EV_OCC && (rb << 1) < mykey) || (nearev && (rb << 1 | 1) < mykey)) { act = false; return; }
                        if (nev + 2 > cap && cap == ECAP && !special) {                    // the list is full: move to a long one
                            slot = atomicAdd(&s_npool, 1);
                            if (slot < NPOOL) {
                                uint16_t* const pl = pool + slot * PCAP;
                                for (int i = 0; i < nev; ++i) pl[i] = myev[i];
                                myev = pl; cap = PCAP;
                            } else slot = -1;
                        }
                        if (nev < cap) myev[nev] = (uint16_t)(rb << 3 | rank);
                        ++nev;
                        if (nearev) { if (nev < cap) myev[nev] = (uint16_t)(rb << 3 | EV_NEAR); ++nev; }
                    }
                };
                // both directions at once - b and the steeper slopes upwards, the flatter ones downwards: two independent
                // record reads in flight per step, half the steps (the order of the events does not matter: they are sorted)
                int qu = q0, qd = q0 - 1;
                bool fu = qu >= cen, fd = qd < cst;
                while (act && !(fu && fd)) {
                    const uint2 ru = srec[fu ? q0 : qu], rd = srec[fd ? q0 : qd];
                    if (!fu) candidate(ru, false, fu);
                    if (act && !fd) candidate(rd, true, fd);
                    ++qu; --qd;
                    fu = fu || qu >= cen; fd = fd || qd < cst;
                }
                if (!act) pflag[mykey] = 0;
            }
        }
        // finalize: the network that fits the longest list of the wave
        bool fin = false;
        if (act) {
            oldv8[mykey] = (uint8_t)oldv;
            if (pflag[mykey] == 2) {                                               // the other classes add their events in pass 2
                atomicAdd(&evn32[mykey >> 1], (uint32_t)nev << ((mykey & 1) * 16));
            } else if (nev > cap) {
                const int pos = atomicAdd(&s_nslow, 1);
                if (pos < RSLOW) slowl[pos] = (uint16_t)mykey; else s_fb = 1;
            } else if (slot < 0) fin = true;
        }
        if (slot >= 0 && slot < NPOOL) poolkey[slot] = act && nev <= cap ? (uint32_t)mykey | ((uint32_t)nev << 16) : 0xFFFFFFFFu;
        const int nmax = wave_max(fin ? nev : 0);
        if (fin) {
            const uint16_t* myev = evl + mykey * ECAP;
            const int val = nmax <= 4 ? replay_sorted<4>(myev, nev, oldv, v.cc) : nmax <= 8 ? replay_sorted<8>(myev, nev, oldv, v.cc)
                                                                                            : replay_sorted<ECAP>(myev, nev, oldv, v.cc);
            oval[mykey] = (uint8_t)(val - v.cc.vmin);
        }
    }
    BAR_LDS();
    STAMP(3);
    {   // long lists (17 .. PCAP events): a wave sorts by counting and folds the clamped adds with a shuffle tree
        const int npool = UNI(min(s_npool, NPOOL));
        for (int k = wave; k < npool; k += RB / 64) {
            const uint32_t pk = poolkey[k];
            if (pk == 0xFFFFFFFFu) continue;
            const int key = (int)(pk & 0xFFFFu), m = (int)(pk >> 16);
            const uint32_t ekey = lane < m ? (uint32_t)pool[k * PCAP + lane] : 0xFFFFFFFFu;
            int rank = 0;
            for (int e = 0; e < m; ++e) {
                const uint32_t ke = (uint32_t)__shfl((int)ekey, e, 64);
                rank += (ke < ekey) || (ke == ekey && e < lane);
            }
            const uint32_t sorted = (uint32_t)__builtin_amdgcn_ds_permute((lane < m ? rank : lane) << 2, (int)ekey);
            const int BIG = 1000000;
            Caf fc = {0, -BIG, BIG};
            if (lane < m) {
                const int rk = (int)(sorted & 7u);
                fc = rk == EV_OCC ? Caf{v.cc.occ, -BIG, v.cc.vmax} : rk == EV_NEAR ? Caf{v.cc.nearby, -BIG, v.cc.vmax} : Caf{v.cc.emp, v.cc.vmin, BIG};
            }
            for (int off = 1; off < 64; off <<= 1) {
                Caf g;
                g.a = __shfl_down(fc.a, off, 64); g.lo = __shfl_down(fc.lo, off, 64); g.hi = __shfl_down(fc.hi, off, 64);
                if ((lane & (2 * off - 1)) == 0) fc = caf_then(fc, g);
            }
            if (lane == 0) { oval[key] = (uint8_t)(caf_apply(fc, (int)(int8_t)oldv8[key]) - v.cc.vmin); atomicAdd(&s_npoolf, 1); }
        }
    }
    // ---- pass 2b: cells other classes reach too; one lane per (cell, other class) ----
    {
        const int nspec = UNI(min(s_nspec, RSPEC));
        for (int it = tid; it < nspec * 8; it += RB) {
            const int pair = spl[it >> 3], cls = it & 7, b = pair >> 1;
            RayP me;
            load_ray(b, me);
            if (cls == me.steep * 4 + (me.ex > 0 ? 2 : 0) + (me.ey > 0 ? 1 : 0)) continue;      // done in pass 1
            FCell f;
            sources(pair_cell(pair), f);
            // slope buckets of this class that can hold a ray through one of the sources
            const int steep = cls >> 2, smaj = steep ? ((cls & 1) ? 1 : -1) : ((cls & 2) ? 1 : -1), smin = steep ? ((cls & 2) ? 1 : -1) : ((cls & 1) ? 1 : -1);
            int blo = NBIN, bhi = -1;
#pragma unroll
            for (int ix = 0; ix < 2; ++ix)
#pragma unroll
            for (int iy = 0; iy < 2; ++iy) {
                if (ix >= f.ngx || iy >= f.ngy) continue;
                const int sgx = ix ? f.gx1 : f.gx0, sgy = iy ? f.gy1 : f.gy0;
                const int ddx = sgx - x0, ddy = sgy - y0;
                const int j = (steep ? ddy : ddx) * smaj, c = (steep ? ddx : ddy) * smin;
                if (j <= 0 || c < 0 || c > j) continue;
                const float inv = (float)NBIN / (float)j;
                blo = min(blo, max(0, (int)(((float)c - 0.5f) * inv) - 1));
                bhi = max(bhi, min(NBIN - 1, (int)(((float)c + 0.5f) * inv) + 1));
            }
            if (bhi < blo) continue;
            const int psh = (pair & 1) * 16;
            for (int q = bkt_start(cls * NBIN + blo); q < bkt_end(cls * NBIN + bhi); ++q) {
                const int rb = brays[q];
                RayP r;
                load_ray(rb, r);
#pragma unroll
                for (int ix = 0; ix < 2; ++ix)
#pragma unroll
                for (int iy = 0; iy < 2; ++iy) {
                    if (ix >= f.ngx || iy >= f.ngy) continue;
                    const int sgx = ix ? f.gx1 : f.gx0, sgy = iy ? f.gy1 : f.gy0;
                    int rank; bool nearev;
                    if (!ray_hits(r, sgx - x0, sgy - y0, rank, nearev)) continue;
                    int pos = (int)((atomicAdd(&evn32[pair >> 1], 1u << psh) >> psh) & 0xFFFFu);
                    if (pos < ECAP) evl[pair * ECAP + pos] = (uint16_t)(rb << 3 | rank);
                    if (nearev) {
                        pos = (int)((atomicAdd(&evn32[pair >> 1], 1u << psh) >> psh) & 0xFFFFu);
                        if (pos < ECAP) evl[pair * ECAP + pos] = (uint16_t)(rb << 3 | EV_NEAR);
                    }
                }
            }
        }
    }
    BAR_LDS();
    // ---- pass 3: the cells of pass 2: owner check, sort, replay ----
    for (int it = tid; it < UNI(min(s_nspec, RSPEC)); it += RB) {
        const int pair = spl[it];
        if (pflag[pair] != 2) continue;                                          // abandoned in pass 1: a smaller pair owns the cell
        const int m = (int)((evn32[pair >> 1] >> ((pair & 1) * 16)) & 0xFFFFu);
        if (m > ECAP) {                                                          // (duplicates may both land here: same value twice)
            const int pos = atomicAdd(&s_nslow, 1);
            if (pos < RSLOW) slowl[pos] = (uint16_t)pair; else s_fb = 1;
            continue;
        }
        const uint16_t* evp = evl + pair * ECAP;
        bool owner = true;
        for (int k = 0; k < m; ++k) {
            const int key = evp[k], rank = key & 7, rp = (key >> 3) << 1;
            if ((rank == EV_OCC && rp < pair) || (rank == EV_NEAR && (rp | 1) < pair)) owner = false;
        }
        if (!owner) continue;
        const int val = m <= 8 ? replay_sorted<8>(evp, m, (int)(int8_t)oldv8[pair], v.cc) : replay_sorted<ECAP>(evp, m, (int)(int8_t)oldv8[pair], v.cc);
        oval[pair] = (uint8_t)(val - v.cc.vmin);
    }
    BAR_LDS();
    if (UNI(s_fb)) { GIVE_BACK(UNI(s_nslow) > RSLOW || UNI(s_nspec) > RSPEC ? 3 : 2); }
    // ---- flagged cells inside the block: their events come from a second walk of the block.  All unoccupied passes
    //      are the same clamped add, so only their NUMBER between consecutive occupied / nearby events (in beam order)
    //      matters: a wave per cell sorts those few events and counts the passes into the intervals they bound. ----
    {
        const int nnear = UNI(min(s_nnear, NNEAR));
        if (nnear > 0) {
            int* const ncur = reinterpret_cast<int*>(cnt);                         // [NNEAR] fill pointers (the event lists of the passes above are done with)
            int* const nend = ncur + NNEAR;                                        // [NNEAR] end of the cell's list
            int* const nbeg = nend + NNEAR;                                        // [NNEAR]
            uint16_t* const wsp = reinterpret_cast<uint16_t*>(nbeg + NNEAR);       // [waves][NSPC] sorted occupied / nearby events
            int* const wcnt = reinterpret_cast<int*>(wsp + (RB / 64) * NSPC);      // [waves][NSPC + 1] passes per interval
            uint16_t* const nev = reinterpret_cast<uint16_t*>(wcnt + (RB / 64) * (NSPC + 1));
            const int nev_cap = min((G.ncell - (int)((unsigned char*)nev - (unsigned char*)cnt)) / 2, 32767);
            if (wave == 0) {                                                       // list sizes: the passes counted by the first walk + room for nearby events
                int run = 0;
                for (int i0 = 0; i0 < nnear; i0 += 64) {
                    const int id = i0 + lane;
                    int need = 0;
                    if (id < nnear) {
                        FCell f;
                        sources(pair_cell(nearl[id]), f);
#pragma unroll
                        for (int ix = 0; ix < 2; ++ix)
#pragma unroll
                        for (int iy = 0; iy < 2; ++iy) {
                            if (ix >= f.ngx || iy >= f.ngy) continue;
                            const int mi = ((ix ? f.gx1 : f.gx0) - x0 + NEAR_R) * NEAR_W + ((iy ? f.gy1 : f.gy0) - y0 + NEAR_R);
                            need += (int)((mini[mi >> 1] >> ((mi & 1) * 16)) & 0x7FFFu);
                        }
                        need += NSPC;
                    }
                    const int ex = run + wave_excl_scan(need, lane);
                    if (id < nnear) {
                        const int beg = min(ex, nev_cap), end = min(ex + need, nev_cap);   // a list that does not fit: the scan over all beams
                        nbeg[id] = beg; ncur[id] = beg; nend[id] = end < ex + need ? beg : end;
                    }
                    run += wave_sum(need);
                }
            }
            BAR_LDS();
            walk_block(true, ncur, nend, nev);
            BAR_LDS();
            for (int id = wave; id < nnear; id += RB / 64) {
                const int key = nearl[id];
                const int beg = nbeg[id], m = ncur[id] - beg;
                uint16_t* const sp = wsp + wave * NSPC;
                int* const ic = wcnt + wave * (NSPC + 1);
                FCell f;
                sources(pair_cell(key), f);
                const int val0 = lane == 0 ? old_value(f) : 0;
                bool ok = beg + m <= nend[id] && nend[id] > beg;
                // the occupied / nearby events, sorted by (beam, rank)
                int k = 0;
                for (int i0 = 0; i0 < m && ok; i0 += 64) {
                    const int i = i0 + lane;
                    const uint32_t ev = i < m ? nev[beg + i] : 0u;
                    const bool spc = i < m && (ev & 7u) >= (uint32_t)EV_OCC;
                    const unsigned long long mk = __ballot(spc);
                    const int at = k + __popcll(mk & ((1ull << lane) - 1ull));
                    if (spc && at < NSPC) sp[at] = (uint16_t)ev;
                    k += __popcll(mk);
                }
                if (k > NSPC) ok = false;
                if (!ok) {                                                         // (uniform) too many events: the scan over all beams
                    if (lane == 0) { const int pos = atomicAdd(&s_nslow, 1); if (pos < RSLOW) slowl[pos] = (uint16_t)key; else s_fb = 1; }
                    continue;
                }
                {
                    const uint32_t mine = lane < k ? (uint32_t)sp[lane] : 0xFFFFFFFFu;
                    int rk = 0;
                    for (int e = 0; e < k; ++e) { const uint32_t o = (uint32_t)__shfl((int)mine, e, 64); rk += (o < mine) || (o == mine && e < lane); }
                    if (lane <= NSPC) ic[lane] = 0;
                    if (lane < k) sp[rk] = (uint16_t)mine;                         // (every lane has read its own entry)
                }
                // passes: interval = number of occupied / nearby events of smaller beams (a beam's own passes come first)
                for (int i0 = 0; i0 < m; i0 += 64) {
                    const int i = i0 + lane;
                    const uint32_t ev = i < m ? nev[beg + i] : 0xFFFFu;
                    if (i < m && (ev & 7u) < (uint32_t)EV_OCC) {
                        const uint32_t bm = ev >> 3;
                        int iv = 0;
                        for (int e = 0; e < k; ++e) iv += ((uint32_t)sp[e] >> 3) < bm;
                        atomicAdd(&ic[iv], 1);
                    }
                }
                {   // lane e <= k: the passes of interval e, then event e; folded in lane order by a shuffle tree
                    const int BIG = 1000000;
                    Caf fc = {0, -BIG, BIG};
                    if (lane <= k) {
                        const int n = min(ic[lane], sat);
                        fc = Caf{n * v.cc.emp, v.cc.vmin, BIG};                   // n clamped adds of emp (gridmap.py:97-101) = one with n * emp
                        if (lane < k) {
                            const int rk = (int)(sp[lane] & 7u);
                            fc = caf_then(fc, rk == EV_OCC ? Caf{v.cc.occ, -BIG, v.cc.vmax} : Caf{v.cc.nearby, -BIG, v.cc.vmax});
                        }
                    }
                    for (int off = 1; off < 64; off <<= 1) {
                        Caf g;
                        g.a = __shfl_down(fc.a, off, 64); g.lo = __shfl_down(fc.lo, off, 64); g.hi = __shfl_down(fc.hi, off, 64);
                        if ((lane & (2 * off - 1)) == 0) fc = caf_then(fc, g);
                    }
                    if (lane == 0) { oval[key] = (uint8_t)(caf_apply(fc, val0) - v.cc.vmin); atomicAdd(&s_nnearf, 1); }
                }
            }
            BAR_LDS();
            if (UNI(s_fb)) { GIVE_BACK(3); }                                       // (the list of cells for the scan over all beams is full)
        }
    }
    {   // cells near the sensor and cells with more than ECAP events: exact membership test over all beams, one cell at a
        // time by the whole workgroup.  A lane folds the events of its beam (the clamped adds compose associatively: Caf),
        // a wave folds its 64 consecutive beams with a shuffle tree, thread 0 folds the waves' results in beam order.
        const int nslow = UNI(s_nslow);
        int* const s_caf = reinterpret_cast<int*>(cnt);                            // [chunks of 64 beams][3] (the event lists are done with)
        const int BIG = 1000000;
        const Caf fE = {v.cc.emp, v.cc.vmin, BIG}, fO = {v.cc.occ, -BIG, v.cc.vmax}, fN = {v.cc.nearby, -BIG, v.cc.vmax};
        for (int k = 0; k < nslow; ++k) {
            const int key = UNI(slowl[k]);
            FCell f;
            sources(pair_cell(key), f);
            const int val0 = tid == 0 ? old_value(f) : 0;
            for (int base = 0; base < v.B; base += RB) {
                const int b = base + tid;
                Caf fb = {0, -BIG, BIG};
                if (b < v.B && (r_info[b] & RI_VALID)) {
                    RayP r;
                    load_ray(b, r);
                    bool occ_ev = false, near_ev = false;
#pragma unroll
                    for (int ix = 0; ix < 2; ++ix)
#pragma unroll
                    for (int iy = 0; iy < 2; ++iy) {
                        if (ix >= f.ngx || iy >= f.ngy) continue;
                        const int sgx = ix ? f.gx1 : f.gx0, sgy = iy ? f.gy1 : f.gy0;
                        int rank; bool ne;
                        if (!ray_hits(r, sgx - x0, sgy - y0, rank, ne)) continue;
                        if (rank == EV_OCC) occ_ev = true; else fb = caf_then(fb, fE);   // the beam's passes come before its last step
                        near_ev = near_ev || ne;
                    }
                    if (occ_ev) fb = caf_then(fb, fO);
                    if (near_ev) fb = caf_then(fb, fN);
                }
                if (base + 64 * wave < v.B) {                                      // (wave-uniform)
                    for (int off = 1; off < 64; off <<= 1) {
                        Caf g;
                        g.a = __shfl_down(fb.a, off, 64); g.lo = __shfl_down(fb.lo, off, 64); g.hi = __shfl_down(fb.hi, off, 64);
                        if ((lane & (2 * off - 1)) == 0) fb = caf_then(fb, g);
                    }
                    if (lane == 0) { int* o = s_caf + 3 * ((base >> 6) + wave); o[0] = fb.a; o[1] = fb.lo; o[2] = fb.hi; }
                }
            }
            BAR_LDS();
            if (tid == 0) {
                int val = val0;
                for (int c = 0; c < (v.B + 63) >> 6; ++c) { const Caf g = {s_caf[3 * c], s_caf[3 * c + 1], s_caf[3 * c + 2]}; val = caf_apply(g, val); }
                oval[key] = (uint8_t)(val - v.cc.vmin);
            }
            BAR_LDS();
        }
        if (tid == 0 && nslow) atomicAdd(&v.stats[ST_SLOW_CELLS], (unsigned long long)nslow);
        if (tid == 0 && s_npoolf) atomicAdd(&v.stats[ST_POOL_CELLS], (unsigned long long)s_npoolf);
        if (tid == 0 && s_nnearf) atomicAdd(&v.stats[ST_NEAR_CELLS], (unsigned long long)s_nnearf);
    }
    STAMP(3);

    // =============================================== windows ==============================================
    const WbConsts wbk = wb_consts(v.cc);
    int n_win = 0;
    for (int S0 = S_lo; S0 <= S_hi; S0 += rows_cap - 1, ++n_win) {
        const int S1 = min(S_hi, S0 + rows_cap - 2);                             // storage rows S0..S1
        const int gx_base = S0 - C, rows_w = S1 - S0 + 2;                        // global rows gx_base .. gx_base + rows_w - 1
        BAR_LDS();                                                               // the previous window is done with the counters
        for (int i = tid; i < (rows_w * stride + 15) >> 4; i += RB) reinterpret_cast<uint4*>(cnt)[i] = make_uint4(0, 0, 0, 0);
        BAR_LDS();
        STAMP(4);
        // ---- walk: lanes are rays, a work item is one 16-step chunk of 64 rays ----
        // Level k >= 1 = steps NEAR_R + 16 (k - 1) .. + 15.  The rays that own a whole k-th chunk are perm[0 .. N_k) (rays ordered by falling
        // chunk count), so every lane of an item runs all 16 steps: no predicates.  Lane l of the w-th wave of a level takes
        // ray l * (waves of the level) + w: the 64 rays of one instruction point in different directions and touch
        // different cells.  Step j of a ray is field base0 + j * cj + minor(j) * cm, minor(j) = (fstep * j + 2^21) >> 22:
        // five instructions and a fire-and-forget LDS add.  The first NEAR_R steps went into the 16-bit block (before the windows: it
        // outlives the windows); the last, partial chunk of every ray is a predicated item of its own.
        {
            const int rx0 = x0 - gx_base, ry0 = y0 - gy_base;
            const int base0 = rx0 * stride + ry0;
            const bool whole = S0 == S_lo && S1 == S_hi;                           // one window holds the fan: no row test
            const int cnt_lds = lds_addr(cnt);
            const int nlev = UNI(s_nlev);                                          // levels 1 .. nlev have whole chunks
            const int nitems = UNI(s_lp[nlev + 1]);                               // (levels above nlev have no waves: s_lp stays flat)
            // one whole chunk of a ray in a strip: every step tests its row
            auto strip_chunk = [&](int b, int k) {
                const uint32_t fs = r_fstep[b];
                const uint32_t cc = r_cc[b];
                const int cj = (int)(int16_t)(cc & 0xFFFFu), cm = (int)cc >> 16;
                const int j0 = NEAR_R + (k - 1) * LCH;
                uint32_t facc = (uint32_t)__umul24(fs, (uint32_t)j0) + (1u << (RFIX - 1));
                int aj = base0 + __mul24(j0, cj);
                // rows: row = rx0 + j * rj + m * rm, where (rj, rm) = (+-1, 0) for a ray along x and (0, +-1) along y
                const int rj = (cj == 1 || cj == -1) ? 0 : (cj > 0 ? 1 : -1), rm = (cm == 1 || cm == -1) ? 0 : (cm > 0 ? 1 : -1);
                int rowj = rx0 + j0 * rj;
#pragma unroll
                for (int u = 0; u < LCH; ++u) {
                    const int m = (int)(facc >> RFIX);
                    const bool in = (unsigned)(rowj + m * rm) < (unsigned)rows_w;
                    const int c = in ? aj + __mul24(m, cm) : 4 * lane;                     // outside the strip: nothing added, a word of the lane's own
                    atomicAdd(&cnt[c >> 2], in ? 1u << ((c & 3) * 8) : 0u);
                    facc += fs; aj += cj; rowj += rj;
                }
            };
            bool by_level = true;
            int nch_all = 0;                                                       // whole chunks of all rays (uniform)
            for (int kk = 1; kk <= nlev; ++kk) nch_all += UNI(s_nk[kk]);
            if (!whole && nch_all <= 65535) {                                      // (16-bit prefixes; decided per particle: the strips share perm's place)
                // A strip holds a part of every ray: the chunks of a ray that can reach the strip's rows are a run of levels
                // (exactly for a ray along x, from a single-precision bound with two steps of slack for a ray along y).  Their
                // counts are prefix-summed over the rays and a lane takes one (ray, chunk) item found by bisection, so that a
                // strip costs its own share of the walk and not the whole walk again.
                uint16_t* const cpre = perm;                                       // [B] first item of the ray (the level order is not needed in strips)
                uint8_t* const cka = pflag;                                        // [B] first level of the ray in this strip
                int nloc[4], tot = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int b = 4 * tid + i;
                    int n = 0;
                    if (b < v.B && (r_info[b] & RI_VALID)) {
                        const int nfull = ((int)r_dmaj[b] + 1 - NEAR_R) / LCH;
                        if (nfull >= 1) {
                            const uint32_t fs = r_fstep[b];
                            const uint32_t cc = r_cc[b];
                            const int cj = (int)(int16_t)(cc & 0xFFFFu), cm = (int)cc >> 16;
                            const int rj = (cj == 1 || cj == -1) ? 0 : (cj > 0 ? 1 : -1), rm = (cm == 1 || cm == -1) ? 0 : (cm > 0 ? 1 : -1);
                            int jlo = NEAR_R, jhi = NEAR_R + nfull * LCH - 1;
                            if (rj > 0) { jlo = max(jlo, -rx0); jhi = min(jhi, rows_w - 1 - rx0); }
                            else if (rj < 0) { jlo = max(jlo, rx0 - rows_w + 1); jhi = min(jhi, rx0); }
                            else {
                                const int mlo = max(rm > 0 ? -rx0 : rx0 - rows_w + 1, 0), mhi = rm > 0 ? rows_w - 1 - rx0 : rx0;
                                if (mhi < mlo) jhi = -1;
                                else if (fs == 0) { if (mlo > 0) jhi = -1; }                  // the minor offset stays 0
                                else {   // minor(j) = floor(j * fs / 2^22 + 1/2) in [mlo, mhi]
                                    const float inv = 4194304.0f / (float)fs;
                                    jlo = max(jlo, (int)(((float)mlo - 0.5f) * inv) - 2);
                                    const float ju = ((float)mhi + 0.5f) * inv;
                                    if (ju < 1.0e9f) jhi = min(jhi, (int)ju + 2);
                                }
                            }
                            if (jhi >= jlo) {
                                const int ka = 1 + (jlo - NEAR_R) / LCH, kb = 1 + (jhi - NEAR_R) / LCH;
                                n = kb - ka + 1;
                                cka[b] = (uint8_t)ka;
                            }
                        }
                    }
                    nloc[i] = n; tot += n;
                }
                int incl = tot;
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                if (lane == 63) s_wsum[wave] = incl;
                BAR_LDS();
                int run = incl - tot;
                for (int k = 0; k < wave; ++k) run += s_wsum[k];
                int total = 0;
                for (int k = 0; k < RB / 64; ++k) total += s_wsum[k];
                total = UNI(total);
                by_level = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) { const int b = 4 * tid + i; if (b < v.B) cpre[b] = (uint16_t)run; run += nloc[i]; }
                BAR_LDS();
                for (int q = wave * 64; q < total; q += RB) {
                    const int it = q + lane;
                    if (it >= total) continue;
                    int b = 0;
                    for (int st = 2048; st; st >>= 1) { const int cand = b + st; if (cand < v.B && (int)cpre[cand] <= it) b = cand; }
                    strip_chunk(b, (int)cka[b] + (it - (int)cpre[b]));
                }
            }
            if (by_level)
            for (int q = wave; q < nitems; q += RB / 64) {
                int k = 1;
                for (int kk = 2; kk <= nlev; ++kk) if (q >= UNI(s_lp[kk])) k = kk;
                const int nk = UNI(s_nk[k]), nwk = (nk + 63) >> 6, wslot = q - UNI(s_lp[k]);
                const int ii = lane * nwk + wslot;
                if (ii >= nk) continue;
                const int b = perm[ii];
                if (whole) {
                    const uint32_t fs = r_fstep[b];
                    const uint32_t cc = r_cc[b];
                    const int cj = (int)(int16_t)(cc & 0xFFFFu), cm = (int)cc >> 16;
                    const int j0 = NEAR_R + (k - 1) * LCH;
                    uint32_t facc = (uint32_t)__umul24(fs, (uint32_t)j0) + (1u << (RFIX - 1));
                    int aj = base0 + __mul24(j0, cj) + cnt_lds;
#pragma unroll
                    for (int u = 0; u < LCH; ++u) {
                        fld8_add(aj + __mul24((int)(facc >> RFIX), cm), 1u);
                        facc += fs; aj += cj;
                    }
                } else strip_chunk(b, k);
            }
            // the partial chunk at the end of every ray with at least NEAR_R + 1 steps
            for (int b = tid; b < v.B; b += RB) {
                const int dmaj = (int)r_dmaj[b];
                if (!(r_info[b] & RI_VALID) || dmaj < NEAR_R) continue;
                const int j0 = NEAR_R + ((dmaj + 1 - NEAR_R) / LCH) * LCH;         // first step after the whole chunks
                if (j0 > dmaj) continue;
                const uint32_t fs = r_fstep[b];
                const uint32_t cc = r_cc[b];
                const int cj = (int)(int16_t)(cc & 0xFFFFu), cm = (int)cc >> 16;
                const int rj = (cj == 1 || cj == -1) ? 0 : (cj > 0 ? 1 : -1), rm = (cm == 1 || cm == -1) ? 0 : (cm > 0 ? 1 : -1);
                uint32_t facc = (uint32_t)__umul24(fs, (uint32_t)j0) + (1u << (RFIX - 1));
                int aj = base0 + __mul24(j0, cj);
                int rowj = rx0 + j0 * rj;
                const int left = dmaj - j0;
                if (whole) {
                    aj += cnt_lds;
#pragma unroll
                    for (int u = 0; u < LCH - 1; ++u) {                            // branch-free: a dead step adds nothing to a word of the lane's own
                        const bool in = u <= left;
                        fld8_add(in ? aj + __mul24((int)(facc >> RFIX), cm) : cnt_lds + 4 * lane, in ? 1u : 0u);
                        facc += fs; aj += cj;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < LCH - 1; ++u) {
                        const int m = (int)(facc >> RFIX);
                        const bool in = u <= left && (unsigned)(rowj + m * rm) < (unsigned)rows_w;
                        const int c = in ? aj + __mul24(m, cm) : 4 * lane;
                        atomicAdd(&cnt[c >> 2], in ? 1u << ((c & 3) * 8) : 0u);
                        facc += fs; aj += cj; rowj += rj;
                    }
                }
            }
        }
        BAR_LDS();
        STAMP(5);
        // ---- the 16-bit block's counts go into the window (saturated: only min(n, sat) matters for an unflagged cell) ----
        for (int mi = tid; mi < NEAR_W * NEAR_W; mi += RB) {
            const int row = x0 + mi / NEAR_W - NEAR_R - gx_base, col = y0 + mi % NEAR_W - NEAR_R - gy_base;
            if ((unsigned)row >= (unsigned)rows_w || (unsigned)col >= (unsigned)stride) continue;
            const uint32_t f = (mini[mi >> 1] >> ((mi & 1) * 16)) & 0x7FFFu;       // bit 15: claim flag of a flagged cell
            if (f) cnt8[row * stride + col] = (uint8_t)min(f, (uint32_t)sat);
        }
        BAR_LDS();
        // ---- the owners put their cell's replayed value into the field of its first source, the other sources vanish ----
        for (int pr = tid; pr < 2 * v.B; pr += RB) {
            const uint32_t ov = oval[pr];
            if (ov == 0xFFu) continue;
            FCell f;
            sources(pair_cell(pr), f);
            if (f.sx < S0 || f.sx > S1) continue;
#pragma unroll
            for (int ix = 0; ix < 2; ++ix)
#pragma unroll
            for (int iy = 0; iy < 2; ++iy) {
                if (ix >= f.ngx || iy >= f.ngy) continue;
                const int sgx = ix ? f.gx1 : f.gx0, sgy = iy ? f.gy1 : f.gy0;
                cnt8[(sgx - gx_base) * stride + (sgy - gy_base)] = (ix | iy) ? (uint8_t)0 : (uint8_t)(0x80u | ov);
            }
        }
        if (tid == 0) s_wbq = 0;
        BAR_LDS();
        STAMP(6);
        // ---- write-back (rbpf_mapupdate.h) ----
        strip_write_back<FIELD_REPLAY_BIT7, false, false, true>(v, sg, S0, S1, gx_base, C, fxl, T_lo >> 5, wbk, cnt, gxb, gym, s_ggf, s_tab, s_need,
                                                                &s_wbq, &s_written, false, lane);
        BAR_LDS();
        STAMP(7);
    }
    BAR_LDS();
    if (tid == 0) {
        if (s_cells) atomicAdd(&v.stats[ST_RAY_CELLS], s_cells);
        if (s_written) atomicAdd(&v.stats[ST_CELLS_WRITTEN], (unsigned long long)s_written);
        atomicAdd(&v.stats[ST_MAP_WINDOWS], (unsigned long long)n_win);
        STAMP_FLUSH();
    }
}

void launch_map_update_ray(const DevView& v, const int32_t* only, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {   // t0 / t1: as launch_map_update_ev
    const RayGeom g = ray_geom(v.B, v.reach);
    static size_t lds_set[MAX_DEVICES] = {};
    ensure_dynamic_lds(reinterpret_cast<const void*>(map_update_ray_kernel), (size_t)g.bytes, lds_set);
    if (t0 && t1) hipExtLaunchKernelGGL(map_update_ray_kernel, dim3(v.P), dim3(RB), (size_t)g.bytes, s, t0, t1, 0, v, only);
    else hipLaunchKernelGGL(map_update_ray_kernel, dim3(v.P), dim3(RB), (size_t)g.bytes, s, v, only);
}

}  // namespace rbpf
