// rbpf_mapupdate.h -- what the three map-update kernels share (HybridMap.update, hybridmap.py:95-145): kernels_mapev.hip
// (event walk), kernels_mapray.hip (global-index counters with slope buckets), kernels_mapupdate.hip (128x128 LDS windows,
// also the fallback of the other two).  The particle preamble, the per-beam ray set-up, the tile allocation, the strip
// window geometry and the strip write-back live here once; each kernel keeps its own core.  gfx950 device code.
#pragma once
#include <limits.h>

#include "rbpf_internal.h"
#include "rbpf_device.h"

namespace rbpf {

// Workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() also drains vmcnt, i.e. every
// outstanding global load AND store; inside the window loop no thread reads or overwrites a global cell another
// thread of the workgroup wrote in the same kernel, so the HBM read-modify-writes may stay in flight across it.
#define BAR_LDS() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// a value every lane agrees on, moved to a scalar register (values read from LDS are not known to be uniform)
#define UNI(x) __builtin_amdgcn_readfirstlane((int)(x))

static const int CHUNK = 16;           // ray steps per work item of the walk (kernels_mapupdate.hip)

// Diagnostic build only (-DRBPF_STAMPS): thread 0 of every workgroup sums the cycles between phase boundaries (STAMP_DECL:
// the sums, STAMP_FLUSH: thread 0 adds them to the reserved counters); the kernel never reads them.
#ifdef RBPF_STAMPS
#define STAMP_DECL long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev = clock64()
#define STAMP(k) do { if (tid == 0) { long long t_ = clock64(); st_acc[k] += t_ - st_prev; st_prev = t_; } } while (0)
#define STAMP_FLUSH() do { for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&v.stats[8 + k_], (unsigned long long)st_acc[k_]); } while (0)
#else
#define STAMP_DECL do { } while (0)
#define STAMP(k) do { } while (0)
#define STAMP_FLUSH() do { } while (0)
#endif

// hand the particle to the window kernel (uniform over the workgroup; nothing has been written to the map yet);
// reason codes: 1 geometry / index map, 2 counter bound, 3 event tables (kernels_mapray.hip)
#define GIVE_BACK(reason) do { if (tid == 0) { v.mu_fallback[p] = (reason); atomicAdd(&v.stats[(reason) == 1 ? ST_FALLBACK_REASONS : (reason) == 2 ? ST_FB_BOUND : ST_FB_TABLES], 1ull); } return; } while (0)

// the event-walk and the global-index kernels (1024 threads, 8-bit fields in global cell-index space, strips of rows)
static const int NEAR_R = 16;                  // ray steps j < NEAR_R are counted in the 16-bit block round the start cell
static const int LCH = 16;                     // steps per chunk of the walk beyond it
static const int NEAR_W = 2 * NEAR_R + 1;      // cells with Chebyshev distance <= NEAR_R from the start cell (one spare ring)
static const int NBIN = 256;                   // slope buckets per direction class (counter bound)
static const int NB_WIN = NBIN / NEAR_R + 2;   // buckets that can hold the rays through one cell beyond the 16-bit block
static const int MAXLEV = 63;                  // whole 16-step chunks per ray (reach < 1000 cells)

__host__ __device__ inline int al16(int x) { return (x + 15) & ~15; }

// passes that saturate any cell (gridmap.py:97-101): 20
__host__ __device__ inline int sat_passes(const CellConsts& cc) { return (cc.vmax - cc.vmin + (-cc.emp) - 1) / (-cc.emp); }

// the cell constants the byte-wise write-back relies on: a cell biased by vmin fits 7 bits, and so do sat passes
inline bool lattice_fits_byte_fields(const CellConsts& cc) {
    if (cc.emp >= 0) return false;
    const int sat = sat_passes(cc);
    return sat <= 31 && cc.vmax - cc.vmin <= 127 && cc.vmin <= 0 && cc.vmax >= 0 && cc.vmin >= -127 && sat * -cc.emp <= 127 &&
           cc.thr >= cc.vmin && cc.thr < cc.vmax;
}

// LDS byte address of a pointer into shared memory
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ int lds_addr(const void* p) { return (int)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char*)p; }

// byte-wise min(x, sat) of four 7-bit counts
__device__ __forceinline__ uint32_t min4(uint32_t n7, uint32_t satb, uint32_t sadd) {
    const uint32_t ge = (n7 + sadd) & 0x80808080u;
    const uint32_t gem = ge | (ge - (ge >> 7));
    return (satb & gem) | (n7 & ~gem);
}
// the same for fields whose bit 7 marks a replayed value (kernels_mapray.hip): those bytes pass through
__device__ __forceinline__ uint32_t premin4(uint32_t x, uint32_t satb, uint32_t sadd) {
    const uint32_t m = min4(x & 0x7F7F7F7Fu, satb, sadd);
    const uint32_t fl = x & 0x80808080u;
    const uint32_t flm = fl | (fl - (fl >> 7));
    return (x & flm) | (m & ~flm);
}

// per-ray info byte
enum { RI_VALID = 1, RI_OCC = 2, RI_NEAR = 4 };   // bits 3-4: near dx + 1, bits 5-6: near dy + 1

// wave-level reductions (all 64 lanes take part): one LDS atomic per wave instead of one per lane
__device__ __forceinline__ int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64)); return v; }
__device__ __forceinline__ int wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64)); return v; }
__device__ __forceinline__ int wave_sum(int v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
__device__ __forceinline__ int wave_excl_scan(int v, int lane) {   // exclusive prefix sum over the wave
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { int n = __shfl_up(incl, o, 64); if (lane >= o) incl += n; }
    return incl - v;
}

// first j with minor offset >= m (m >= 1, dmin > 0), 32-bit (2*dmaj*m < 2^31 for rays shorter than a tile)
__device__ __forceinline__ int first_j_minor_ge(const Ray& r, int m) {
    int num = 2 * r.dmaj * m - r.dmaj, den = 2 * r.dmin;
    return (num + den - 1) / den;
}
__device__ __forceinline__ int last_j_minor_le(const Ray& r, int m) {
    int num = 2 * r.dmaj * (m + 1) - r.dmaj - 1;
    if (num < 0) return -1;
    int j = num / (2 * r.dmin);
    return j > r.dmaj ? r.dmaj : j;
}

// Clamped-add functions v -> min(max(v + a, lo), hi) are closed under composition, so the ordered sequence of
// a cell's events folds associatively: each lane folds the events of one beam, the wave folds 64 beams in
// beam order with a shuffle tree.
struct Caf { int a, lo, hi; };
__device__ __forceinline__ Caf caf_then(Caf f, Caf g) {          // g after f
    Caf r;
    r.a = f.a + g.a;
    int lo = f.lo + g.a; lo = lo < g.lo ? g.lo : lo; r.lo = lo > g.hi ? g.hi : lo;
    int hi = f.hi + g.a; hi = hi < g.lo ? g.lo : hi; r.hi = hi > g.hi ? g.hi : hi;
    return r;
}
__device__ __forceinline__ int caf_apply(Caf f, int x) { int t = x + f.a; t = t < f.lo ? f.lo : t; return t > f.hi ? f.hi : t; }

// One lane replays a bucket of up to N events: bitonic sorting network on registers (padded with 0xFFFF), then the
// clamped adds in ascending (beam, rank) order.
template <int N>
__device__ __forceinline__ int replay_sorted(const uint16_t* __restrict__ evp, int m, int val, const CellConsts& cc) {
    uint32_t ev[N];
#pragma unroll
    for (int e = 0; e < N; ++e) ev[e] = e < m ? (uint32_t)evp[e] : 0xFFFFu;
#pragma unroll
    for (int k = 2; k <= N; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t a = ev[i], b = ev[l];
                    const bool up = (i & k) == 0;
                    ev[i] = up ? min(a, b) : max(a, b);
                    ev[l] = up ? max(a, b) : min(a, b);
                }
            }
#pragma unroll
    for (int e = 0; e < N; ++e)
        if (e < m) val = cell_apply_rank(val, (int)(ev[e] & 7u), cc);
    return val;
}

__device__ inline int replay_cell_wave(const DevView& v, const uint8_t* r_info, const int32_t* r_end, int x0, int y0, const int* gxc, int ngx,
                                const int* gyc, int ngy, int val, int lane) {
    const int BIG = 1000000;
    const Caf fE = {v.cc.emp, v.cc.vmin, BIG}, fO = {v.cc.occ, -BIG, v.cc.vmax}, fN = {v.cc.nearby, -BIG, v.cc.vmax};
    for (int base = 0; base < v.B; base += 64) {
        const int b = base + lane;
        Caf f = {0, -BIG, BIG};
        bool has = false;
        if (b < v.B && (r_info[b] & RI_VALID)) {
            const int info = r_info[b];
            int x1, y1;
            unpack_end(r_end[b], x0, y0, x1, y1);
            Ray r = ray_make(x0, y0, x1, y1);
            const bool occ = info & RI_OCC;
            int js[4], nj = 0;
            for (int ix = 0; ix < ngx; ++ix)
                for (int iy = 0; iy < ngy; ++iy) {
                    int gx = gxc[ix], gy = gyc[iy];
                    int j = r.steep ? (gy - y0) * r.sy : (gx - x0) * r.sx;
                    if (j < 0 || j >= r.n) continue;
                    int qx, qy;
                    ray_point(r, j, qx, qy);
                    if (qx == gx && qy == gy) js[nj++] = j;
                }
            for (int a = 1; a < nj; ++a) {
                int key = js[a], c = a - 1;
                while (c >= 0 && js[c] > key) { js[c + 1] = js[c]; --c; }
                js[c + 1] = key;
            }
            bool near_here = false;
            for (int a = 0; a < nj; ++a) {
                int j = js[a];
                f = caf_then(f, (j == r.n - 1 && occ) ? fO : fE);
                if (j == r.n - 2 && (info & RI_NEAR)) near_here = true;
            }
            if (near_here) f = caf_then(f, fN);
            has = nj > 0;
        }
        if (__ballot(has) == 0ull) continue;
        for (int off = 1; off < 64; off <<= 1) {
            Caf g;
            g.a = __shfl_down(f.a, off, 64); g.lo = __shfl_down(f.lo, off, 64); g.hi = __shfl_down(f.hi, off, 64);
            if ((lane & (2 * off - 1)) == 0) f = caf_then(f, g);
        }
        val = caf_apply(f, val);        // lane 0 holds the fold of the whole chunk
        val = __shfl(val, 0, 64);
    }
    return val;
}


// ---- particle preamble ----------------------------------------------------------------------------------------------

// hybridmap.py:98-100: a tile holds the robot position (otherwise the update is a no-op)
__device__ __forceinline__ bool home_tile_ok(const DevView& v, const int32_t* tab, double px, double py) {
    int lx, ly;
    return tile_of_coord(px, v.tile_len, v.R, lx) && tile_of_coord(py, v.tile_len, v.R, ly) && tab[(lx + v.R) * v.L + (ly + v.R)] >= 0;
}
// the LUT covers every global index within `margin` of the start cell
__device__ __forceinline__ bool lut_covers(const DevView& v, int x0, int y0, int margin) {
    return lut_valid_g(v, x0 - margin) && lut_valid_g(v, x0 + margin) && lut_valid_g(v, y0 - margin) && lut_valid_g(v, y0 + margin);
}

// The start of a particle in the 1024-thread kernels: wave 0 takes the heading's sine and cosine into s_sincos (read after
// the caller's next barrier); the start cell (hybridmap.py:102); the home tile and LUT test (false: nothing to do, uniform);
// the index map over everything a ray can reach, with a margin of two columns (the sources of a storage cell are its own
// global index and the next one): ux[i] / uy[i] = U of global index x0 - reach - 2 + i / y0 - reach - 2 + i.
// fan_preamble_from: the same for a caller that has the heading's sine and cosine already (kernels_mapev.hip: a record of the
// particle's pose, sine, cosine and tile row is made while the particle before it is written back); tab may lie in LDS.
template <int NT>
__device__ __forceinline__ bool fan_preamble_from(const DevView& v, const int32_t* tab, int p, int tid, double px, double py, int lut_margin,
                                                  int fanw, uint16_t* ux, uint16_t* uy, int& x0, int& y0);
template <int NT>
__device__ __forceinline__ bool fan_preamble(const DevView& v, const int32_t* tab, int p, int tid, double px, double py, int lut_margin,
                                             int fanw, double* s_sincos, uint16_t* ux, uint16_t* uy, int& x0, int& y0) {
    if ((tid >> 6) == 0) {   // one wave takes the sine and cosine (a few hundred instructions); the others read them after the first barrier
        double sn, cs_;
        sincos(v.upd_pose[2 * v.P + p], &sn, &cs_);
        if (tid == 0) { s_sincos[0] = sn; s_sincos[1] = cs_; }
    }
    return fan_preamble_from<NT>(v, tab, p, tid, px, py, lut_margin, fanw, ux, uy, x0, y0);
}
template <int NT>
__device__ __forceinline__ bool fan_preamble_from(const DevView& v, const int32_t* tab, int p, int tid, double px, double py, int lut_margin,
                                                  int fanw, uint16_t* ux, uint16_t* uy, int& x0, int& y0) {
    x0 = UNI(trunc_to_int(px / v.cs)); y0 = UNI(trunc_to_int(py / v.cs));
    bool ok = home_tile_ok(v, tab, px, py);
    if (ok && !lut_covers(v, x0, y0, lut_margin)) { if (tid == 0) atomicCAS(v.err, 0, RBPF_ERANGE); ok = false; }
    if (tid == 0) v.mu_fallback[p] = 0;
    if (!UNI(ok)) return false;
    const int fxl = x0 - v.reach - 2, fyl = y0 - v.reach - 2;
    for (int i = tid; i < fanw; i += NT) {
        const int gxq = fxl + i, gyq = fyl + i;
        const uint32_t ex = lut_valid_g(v, gxq) ? lut_at(v, gxq) : LUT_INVALID, ey = lut_valid_g(v, gyq) ? lut_at(v, gyq) : LUT_INVALID;
        ux[i] = ex != LUT_INVALID ? (uint16_t)(lut_lat(ex) * v.dim + lut_cidx(ex)) : 0xFFFFu;
        uy[i] = ey != LUT_INVALID ? (uint16_t)(lut_lat(ey) * v.dim + lut_cidx(ey)) : 0xFFFFu;
    }
    return true;
}

// ---- per-beam ray set-up --------------------------------------------------------------------------------------------

// the fan's reach: its bounding box in global cell indices and its number of ray cells, per thread
struct FanBox { int x0, x1, y0, y1; unsigned long long cells; };

// One beam's ray (hybridmap.py:104-142): r.n == 0 is a degenerate ray (no points); info = RI_* bits, bits 3-6 the nearby
// cell's offset from the end cell.
struct BeamRay { Ray r; int x1, y1, info; };

// The end cell (lidar.py:123, hybridmap.py:106-113), the range check, the nearby cell and its same-tile test
// (hybridmap.py:139-142); the tiles the ray enters (staircase start -> [corner] -> end) are marked in need[] and the ray
// joins the fan's box.  lat_x / lat_y: lattice coordinate of a global index; scale(): the beam's BF_LONG factor.
template <class LatX, class LatY, class Scale>
__device__ __forceinline__ BeamRay beam_ray(const DevView& v, double x, double y, int bf, Scale scale, double sn, double cs_, double px,
                                            double py, int x0, int y0, int a0, int b0, LatX lat_x, LatY lat_y, int* need, FanBox& fan) {
    BeamRay o;
    const double gx = (cs_ * x + (-sn) * y) + px;                             // lidar.py:123
    const double gy = (sn * x + cs_ * y) + py;
    int x1 = trunc_to_int(gx / v.cs), y1 = trunc_to_int(gy / v.cs);        // hybridmap.py:106
    if (bf & BF_LONG) {                                                       // hybridmap.py:107-113
        const double sc = scale();
        x1 = trunc_to_int((double)x0 + sc * (double)(x1 - x0));
        y1 = trunc_to_int((double)y0 + sc * (double)(y1 - y0));
    }
    const int ddx = x1 - x0, ddy = y1 - y0;
    if (ddx < -v.reach || ddx > v.reach || ddy < -v.reach || ddy > v.reach) {
        atomicCAS(v.err, 0, RBPF_ERANGE);
        x1 = x0; y1 = y0 - 1;                                                 // degenerate: no points
    }
    o.x1 = x1; o.y1 = y1;
    const Ray r = ray_make(x0, y0, x1, y1);
    o.r = r;
    o.info = 0;
    if (r.n == 0) return o;
    o.info = RI_VALID | ((bf & BF_LONG) ? 0 : RI_OCC);
    fan.cells += (unsigned long long)r.n;
    fan.x0 = min(fan.x0, x1); fan.x1 = max(fan.x1, x1); fan.y0 = min(fan.y0, y1); fan.y1 = max(fan.y1, y1);
    const int a1 = lat_x(x1), b1 = lat_y(y1);
    if (r.n >= 2 && (o.info & RI_OCC)) {                                      // hybridmap.py:139-142
        int nx, ny;
        ray_point(r, r.n - 2, nx, ny);
        if (lat_x(nx) == a1 && lat_y(ny) == b1) o.info |= RI_NEAR;            // hybridmap.py:141 same tile as the end cell
        o.info |= ((nx - x1 + 1) & 3) << 3;
        o.info |= ((ny - y1 + 1) & 3) << 5;
    }
    need[a0 * v.L + b0] = 1;
    if (a1 != a0 || b1 != b0) {
        need[a1 * v.L + b1] = 1;
        if (a1 != a0 && b1 != b0) {
            // first global index on the far side of each boundary, in the ray's direction
            const int KW = (v.dim + WIN - 1) / WIN;
            const int gxb = r.sx > 0 ? v.gwin[a1 * (KW + 1)] : v.gwin[a0 * (KW + 1)] - 1;
            const int gyb = r.sy > 0 ? v.gwin[b1 * (KW + 1)] : v.gwin[b0 * (KW + 1)] - 1;
            int ox = gxb - x0; ox = ox < 0 ? -ox : ox;
            int oy = gyb - y0; oy = oy < 0 ? -oy : oy;
            const int jx = r.steep ? first_j_minor_ge(r, ox) : ox;
            const int jy = r.steep ? oy : first_j_minor_ge(r, oy);
            if (jx < jy) need[a1 * v.L + b0] = 1;
            else if (jy < jx) need[a0 * v.L + b1] = 1;
        }
    }
    return o;
}

// the workgroup's fan: every wave's box and cell count into s_fan (gx min, gx max, gy min, gy max) and s_cells
__device__ __forceinline__ void fan_box_join(FanBox f, int lane, int* s_fan, unsigned long long* s_cells) {
    const int ws = wave_sum((int)f.cells);                                    // < 64 * 16 rays * 2^16 steps
    f.x0 = wave_min(f.x0); f.x1 = wave_max(f.x1); f.y0 = wave_min(f.y0); f.y1 = wave_max(f.y1);
    if (lane == 0) {
        atomicAdd(s_cells, (unsigned long long)ws);
        atomicMin(&s_fan[0], f.x0); atomicMax(&s_fan[1], f.x1);
        atomicMin(&s_fan[2], f.y0); atomicMax(&s_fan[3], f.y1);
    }
}

// ---- tile allocation ------------------------------------------------------------------------------------------------

// The tiles the rays enter that the particle does not have yet come from the pool (free tiles are kept zero-filled: an
// old value read through either state of the table is 0).  An empty pool: RBPF_ENOMEM, and the tile is not needed.
__device__ __forceinline__ void alloc_missing_tiles(const DevView& v, int32_t* tab, int* s_need, int* s_tab, int tid) {
    if (tid >= v.L * v.L || !s_need[tid] || s_tab[tid] >= 0) return;
    const int idx = atomicSub(v.free_top, 1) - 1;
    if (idx < 0) {
        atomicAdd(v.free_top, 1);
        atomicCAS(v.err, 0, RBPF_ENOMEM);
        s_need[tid] = 0;
    } else {
        const int t = v.free_stack[idx];
        s_tab[tid] = t;
        tab[tid] = t;
        v.tile_bbox[4 * t + 0] = INT_MAX; v.tile_bbox[4 * t + 1] = -1;
        v.tile_bbox[4 * t + 2] = INT_MAX; v.tile_bbox[4 * t + 3] = -1;
    }
}

// ---- strip window geometry (event-walk and global-index kernels) ----------------------------------------------------

// The window: the fan's bounding box in global cell indices, strips of storage rows if it does not fit.
struct StripGeom {
    int S_lo, S_hi, T_lo, T_hi;   // storage rows / columns the fan can write
    int gy_base;                  // global column of window column 0
    int stride;                   // window columns per row
    int rows_cap;                 // global rows a window can hold
};
// Also checks the reference's index formula over the fan (one column more on either side): U(g) = g + C - G(g) with G in
// {0, 1}; gxb / gyb get G (s_fb = 1: it does not hold, or the LUT ends inside the fan).
template <int NT>
__device__ __forceinline__ StripGeom strip_geom(const uint16_t* ux, const uint16_t* uy, uint8_t* gxb, uint8_t* gyb, int fanw, int fxl,
                                                int fyl, int C, const int* s_fan, int* s_fb, int ncell, int tid) {
    const int bxl = UNI(s_fan[0]), bxh = UNI(s_fan[1]), byl = UNI(s_fan[2]), byh = UNI(s_fan[3]);
    for (int i = tid; i < fanw; i += NT) {
        const int dxg = (fxl + i + C) - (int)ux[i], dyg = (fyl + i + C) - (int)uy[i];
        if (fxl + i >= bxl - 1 && fxl + i <= bxh + 1 && (unsigned)dxg > 1u) *s_fb = 1;
        if (fyl + i >= byl - 1 && fyl + i <= byh + 1 && (unsigned)dyg > 1u) *s_fb = 1;
        gxb[i] = (uint8_t)(dxg & 1); gyb[i] = (uint8_t)(dyg & 1);
    }
    StripGeom g;
    g.S_lo = UNI(ux[bxl - fxl]); g.S_hi = UNI(ux[bxh - fxl]);
    g.T_lo = UNI(uy[byl - fyl]); g.T_hi = UNI(uy[byh - fyl]);
    g.gy_base = (g.T_lo - C) & ~3;                                            // (C is a multiple of 4)
    g.stride = (g.T_hi - C + 2 - g.gy_base + 3) & ~3;                         // columns gy_base .. T_hi - C + 1
    if (((g.stride >> 2) & 1) == 0) g.stride += 4;                            // rows an odd number of banks apart
    g.rows_cap = ncell / g.stride;
    return g;
}

// Wave 0: the levels of the walk from s_lcnt[k] = rays with exactly k whole chunks (k >= 1; level 0 is the 16-bit block).
// N_k = rays with at least k (suffix sums over the wave: MAXLEV = 63) -> s_nk, s_lfill (perm's fill pointer of the level:
// rays with more chunks come first), s_lp (the level's first work item: a wave per 64 rays), s_nlev (the highest level).
__device__ __forceinline__ void level_sums(int lane, const int* s_lcnt, int* s_lfill, int* s_nk, int* s_lp, int* s_nlev) {
    const int k = lane;
    const int ck = k >= 1 ? s_lcnt[k] : 0;
    int suf = ck;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(suf, o, 64); if (lane + o < 64) suf += t; }
    const int nwk = k >= 1 ? (suf + 63) >> 6 : 0;
    int pre = nwk;                                                            // inclusive prefix of the levels' wave counts
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(pre, o, 64); if (lane >= o) pre += t; }
    const unsigned long long live = __ballot(k >= 1 && suf > 0);
    if (k >= 1) { s_lfill[k] = suf - ck; s_nk[k] = suf; s_lp[k] = pre - nwk; }
    if (k == 63) s_lp[64] = pre;
    if (k == 0) { *s_nlev = live ? 63 - __clzll((long long)live) : 0; s_nk[MAXLEV + 1] = 0; }
}

// Column glitch mask in window coordinates (gym[lc]: 0 / 0xFF), and per 32-cell group of storage cells (index
// bt * gpt + gt - ggf_base over tile bt, group gt of its row; ggf_n entries) whether a glitched column is among the
// group's sources: its own 32 and, for a group's first four columns, the group before (gt = 0: the last one of the tile before).
template <int NT>
__device__ __forceinline__ void glitch_mask(const uint8_t* gyb, uint8_t* gym, uint8_t* s_ggf, int ggf_base, int ggf_n, const StripGeom& g,
                                            int fanw, int fyl, int nfx, int C, int dim, int gpt, int tid) {
    for (int lc = tid; lc < g.stride + 16 && lc < fanw + 16; lc += NT) {
        const int i = lc + g.gy_base - fyl;
        const bool gl = i >= 0 && i < nfx && gyb[i];
        gym[lc] = gl ? 0xFFu : 0u;
        if (gl) {
            const int sc = lc + g.gy_base + C, bt = sc / dim, t = sc - bt * dim;
            const int idx = bt * gpt + (t >> 5) - ggf_base;
            if ((unsigned)idx < (unsigned)ggf_n) s_ggf[idx] = 1;
            if ((t & 31) < 4 && (unsigned)(idx - 1) < (unsigned)ggf_n) s_ggf[idx - 1] = 1;
        }
    }
}

// ---- flagged cells (event-walk and global-index kernels) ------------------------------------------------------------

// The global cell flagged by pair (beam, e), relative to the start cell: the beam's end cell (e = 0) or the cell before it
// (e = 1, only when it lies in the end cell's tile); false = none.
__device__ __forceinline__ bool pair_offset(int pr, const uint8_t* r_info, const int32_t* r_end, int& dx, int& dy) {
    const int b = pr >> 1, info = r_info[b];
    if ((info & (RI_VALID | RI_OCC)) != (RI_VALID | RI_OCC) || ((pr & 1) && !(info & RI_NEAR))) return false;
    const int32_t re = r_end[b];
    dx = (int)(int16_t)(re & 0xFFFF); dy = (int)(int16_t)((uint32_t)re >> 16);
    if (pr & 1) { dx += ((info >> 3) & 3) - 1; dy += ((info >> 5) & 3) - 1; }
    return true;
}
// ... as a storage cell (U_x << 16 | U_y); ~0 = none
__device__ __forceinline__ uint32_t flagged_cell(int pr, const uint8_t* r_info, const int32_t* r_end, int x0, int y0, const uint16_t* ux,
                                                 const uint16_t* uy, int fxl, int fyl) {
    int dx, dy;
    if (!pair_offset(pr, r_info, r_end, dx, dy)) return 0xFFFFFFFFu;
    return ((uint32_t)ux[x0 + dx - fxl] << 16) | (uint32_t)uy[y0 + dy - fyl];
}

// A storage cell and its source global cells (scalars: no indexed arrays): per axis a = U - C if not glitched, a + 1 if glitched.
struct FCell { int sx, sy; int gx0, gx1, gy0, gy1; int ngx, ngy; };
__device__ __forceinline__ void cell_sources(uint32_t sc, int C, const uint8_t* gxb, const uint8_t* gyb, int fxl, int fyl, FCell& f) {
    f.sx = (int)(sc >> 16); f.sy = (int)(sc & 0xFFFFu);
    const int ax = f.sx - C, ay = f.sy - C;
    const bool xa = !gxb[ax - fxl], xb = gxb[ax + 1 - fxl], ya = !gyb[ay - fyl], yb = gyb[ay + 1 - fyl];
    f.ngx = (xa ? 1 : 0) + (xb ? 1 : 0); f.gx0 = xa ? ax : ax + 1; f.gx1 = ax + 1;
    f.ngy = (ya ? 1 : 0) + (yb ? 1 : 0); f.gy0 = ya ? ay : ay + 1; f.gy1 = ay + 1;
}

// ---- strip write-back (event-walk and global-index kernels) ---------------------------------------------------------

// Field formats of the 8-bit window: the event walk keeps the count in bits 1-7 and the flag in bit 0; the global-index
// kernel keeps the count in bits 0-6, and bit 7 marks a replayed value (value - vmin) that passes through.
enum { FIELD_COUNT_HI, FIELD_REPLAY_BIT7 };

struct WbConsts { uint32_t kb1, oadd, satb, sadd; int eabs; };
__device__ __forceinline__ WbConsts wb_consts(const CellConsts& cc) {
    const uint32_t sat = (uint32_t)sat_passes(cc);
    WbConsts k;
    k.kb1 = (uint32_t)(128 + cc.vmin) * 0x01010101u;                          // byte-wise: (cell ^ 0x80) - kb1 = cell - vmin
    k.oadd = (uint32_t)(127 - (cc.thr - cc.vmin)) * 0x01010101u;              // bit 7 of (R + oadd) = cell > thr
    k.satb = sat * 0x01010101u; k.sadd = (128u - sat) * 0x01010101u;
    k.eabs = -cc.emp;
    return k;
}

// One word of four cells through the write-back's arithmetic (gridmap.py:97-101, n times, byte-wise), branch-free: a word
// without hits passes through unchanged (dec = 0, nz = 0).  nw: the four counts (FIELD_REPLAY_BIT7: or replayed values).
// Returns the new word; touched4 / occ4 get the word's four bits (field not zero / cell > threshold).
template <int FIELD>
__device__ __forceinline__ uint32_t wb_word(const WbConsts& k, uint32_t pre, uint32_t nw, uint32_t& touched4, uint32_t& occ4) {
    const uint32_t Ob = (pre ^ 0x80808080u) - k.kb1;                          // cells biased to [0, vmax - vmin]
    const uint32_t n7 = FIELD == FIELD_REPLAY_BIT7 ? nw & 0x7F7F7F7Fu : nw;
    const uint32_t m = min4(n7, k.satb, k.sadd);                              // min(n, sat)
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const uint32_t dec = __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2, m) * (us2)(unsigned short)k.eabs);   // byte-wise: sat * |emp| < 128, no carries
    const uint32_t T1 = (Ob | 0x80808080u) - dec;
    const uint32_t pos = T1 & 0x80808080u;                                    // O - dec >= 0
    uint32_t R = T1 & 0x7F7F7F7Fu & (pos | (pos - (pos >> 7)));
    uint32_t nz = (n7 + 0x7F7F7F7Fu) & 0x80808080u;                           // fields that are not zero
    if (FIELD == FIELD_REPLAY_BIT7) {                                         // replayed cells: the field holds value - vmin
        const uint32_t fl = nw & 0x80808080u;
        const uint32_t flm = fl | (fl - (fl >> 7));
        R = (n7 & flm) | (R & ~flm);
        nz = ((n7 + 0x7F7F7F7Fu) | nw) & 0x80808080u;
    }
    touched4 = __builtin_amdgcn_udot4(nz >> 7, 0x08040201u, 0u, false);
    occ4 = __builtin_amdgcn_udot4(((R + k.oadd) & 0x80808080u) >> 7, 0x08040201u, 0u, false);   // cell > thr
    return (R + k.kb1) ^ 0x80808080u;
}

// Write-back of the strip of storage rows S0..S1 (window row 0 = global row gx_base): one read-modify-write per touched
// 32-cell group of storage cells, tile by tile.  Storage cell s receives global cell s - C where that one is not glitched
// plus global cell s - C + 1 where that one is (gxb from global index fxl; s_ggf as glitch_mask).  Template switches:
//   FIELD      the window's field format (above);
//   PARTIAL    dim need not be a multiple of 32: the last group of a tile row is partial;
//   THIN       a thin fan (`thin`, runtime) stores a group's one to three touched words alone;
//   NEED_ONLY  tiles whose s_need entry is clear are skipped.
// Waves draw batches of 64 items (32-cell groups) from a queue (*s_wbq = 0 before): the rows at the fan's rim hold few
// touched groups, and with a fixed share per wave the workgroup waited a quarter of the write-back's time for its slowest wave.
// Adds the cells written to *s_written.
template <int FIELD, bool PARTIAL, bool THIN, bool NEED_ONLY>
__device__ __forceinline__ void strip_write_back(const DevView& v, const StripGeom& s, int S0, int S1, int gx_base, int C, int fxl, int ggf_base,
                                                 const WbConsts& wbk, const uint32_t* cnt, const uint8_t* gxb, const uint8_t* gym,
                                                 const uint8_t* s_ggf, const int* s_tab, const int* s_need, int* s_wbq, int* s_written,
                                                 bool thin, int lane) {
    int my_written = 0;
    const int gpt = (v.dim + 31) >> 5;                                        // 32-cell groups per tile row
    auto next_batch = [&]() -> int { int g = 0; if (lane == 0) g = atomicAdd(s_wbq, 1); return UNI(g); };
    int batch = next_batch(), batch0 = 0;                                     // batch0: the first batch of the tile at hand
    for (int a = S0 / v.dim; a <= S1 / v.dim; ++a)
    for (int bt = s.T_lo / v.dim; bt <= s.T_hi / v.dim; ++bt) {
        if (a >= v.L || bt >= v.L || (NEED_ONLY && !s_need[a * v.L + bt])) continue;    // uniform
        const int tile = UNI(s_tab[a * v.L + bt]);
        if (tile < 0) continue;
        const int sr_lo = max(S0, a * v.dim), sr_hi = min(S1, (a + 1) * v.dim - 1);  // storage rows
        const int g_lo = max(s.T_lo - bt * v.dim, 0) >> 5, g_hi = min(s.T_hi - bt * v.dim, v.dim - 1) >> 5;   // groups of this tile's rows
        const int ngr = g_hi - g_lo + 1, items = (sr_hi - sr_lo + 1) * ngr;
        int8_t* __restrict__ tile_base = v.pool + (size_t)tile * v.dim * v.dim;
        int bx0 = INT_MAX, bx1 = -1, by0 = INT_MAX, by1 = -1;
        const int nbatch = (items + 63) >> 6;
        const float inv_ngr = 1.0f / (float)ngr;
        for (; batch < batch0 + nbatch; batch = next_batch()) {
            const int it = ((batch - batch0) << 6) + lane;
            if (it >= items) continue;
            const int rr = (int)(((float)it + 0.5f) * inv_ngr), gg = it - rr * ngr;   // it / ngr: (it + 0.5) / ngr is at least 0.5 / 192 from a whole number, the float product's error 1e-4 of that
            const int srow = sr_lo + rr, gt = g_lo + gg;
            const int ia = srow - C - fxl;                                 // source rows a (if not glitched), a + 1 (if glitched)
            const bool va = !gxb[ia], vb = gxb[ia + 1];
            if (!va && !vb) continue;                                          // no global row maps here
            const int lr = srow - C - gx_base;                             // window row of source a
            const int lc0 = bt * v.dim + 32 * gt - C - s.gy_base;            // window column of the group's first cell, multiple of 4
            const int nw = PARTIAL ? min(32, v.dim - 32 * gt) >> 2 : 8;         // words of this group (8; fewer in a tile's last group)
            auto field = [&](int i) { const uint32_t x = cnt[i]; return FIELD == FIELD_COUNT_HI ? (x >> 1) & 0x7F7F7F7Fu : x; };
            uint32_t n[8];
            uint32_t any = 0;
            if (!(va && vb) && !s_ggf[bt * gpt + gt - ggf_base]) {           // one source row, no glitched column: the fields are the group's counts
                const int rowo = (lr + (va ? 0 : 1)) * s.stride + lc0;
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    const int lc = lc0 + 4 * w;
                    n[w] = (lc >= 0 && lc < s.stride && w < nw) ? field((rowo + 4 * w) >> 2) : 0u;
                    any |= n[w];
                }
            } else {
                uint32_t gm[9];                                                // glitched columns in the group (its 32 cells and the one after)
#pragma unroll
                for (int w = 0; w < 9; ++w) {
                    const int lc = lc0 + 4 * w;
                    gm[w] = (lc >= 0 && lc < s.stride + 12) ? *reinterpret_cast<const uint32_t*>(gym + lc) : 0u;
                }
#pragma unroll
                for (int w = 0; w < 8; ++w) n[w] = 0;
                for (int src = 0; src < 2; ++src) {
                    if (src == 0 ? !va : !vb) continue;
                    const int row = lr + src;
                    uint32_t x[9];
#pragma unroll
                    for (int w = 0; w < 9; ++w) {
                        const int lc = lc0 + 4 * w;
                        x[w] = (lc >= 0 && lc < s.stride) ? field((row * s.stride + lc) >> 2) : 0u;
                    }
#pragma unroll
                    for (int w = 0; w < 9; ++w) x[w] = FIELD == FIELD_COUNT_HI ? min4(x[w], wbk.satb, wbk.sadd) : premin4(x[w], wbk.satb, wbk.sadd);
#pragma unroll
                    for (int w = 0; w < 8; ++w) {
                        const uint32_t keep = x[w] & ~gm[w];
                        const uint32_t mv = ((x[w] & gm[w]) >> 8) | ((x[w + 1] & gm[w + 1]) << 24);
                        n[w] += keep + mv;
                    }
                }
#pragma unroll
                for (int w = 0; w < 8; ++w) { if (w >= nw) n[w] = 0; any |= n[w]; }
            }
            if (!any) continue;
            const int row_t = srow - a * v.dim, col_t = 32 * gt;
            uint32_t* g_ptr = reinterpret_cast<uint32_t*>(tile_base + (size_t)row_t * v.dim + col_t);
            uint32_t pre[8];
            if (nw == 8) {
                const uint4 q0 = reinterpret_cast<const uint4*>(g_ptr)[0], q1 = reinterpret_cast<const uint4*>(g_ptr)[1];
                pre[0] = q0.x; pre[1] = q0.y; pre[2] = q0.z; pre[3] = q0.w; pre[4] = q1.x; pre[5] = q1.y; pre[6] = q1.z; pre[7] = q1.w;
            } else {
#pragma unroll
                for (int w = 0; w < 8; ++w) pre[w] = w < nw ? g_ptr[w] : 0u;
            }
            uint32_t occ = 0, touched = 0;
            bool stored = false;
            if (THIN && thin) {   // a thin fan (few beams on a fine grid): a group holds one or two touched words - the arithmetic and
                                  // the stores are theirs alone; the other words only give their occupancy bits (the group's 32 bytes are
                                  // one memory sector: read whole, written by the word)
                uint32_t nzm = 0;
#pragma unroll
                for (int w = 0; w < 8; ++w) nzm |= n[w] ? 1u << w : 0u;
                if (__popc(nzm) <= 3) {
#pragma unroll
                    for (int w = 0; w < 8; ++w)                                       // cell > thr of the cells as they are
                        occ |= __builtin_amdgcn_udot4(((((pre[w] ^ 0x80808080u) - wbk.kb1) + wbk.oadd) & 0x80808080u) >> 7, 0x08040201u, 0u, false) << (4 * w);
                    uint32_t mm = nzm;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const int wq = mm ? __ffs((int)mm) - 1 : -1;
                        mm &= mm - 1;
                        if (wq < 0) continue;
                        uint32_t pw = 0, nv = 0;
#pragma unroll
                        for (int w = 0; w < 8; ++w) { pw = w == wq ? pre[w] : pw; nv = w == wq ? n[w] : nv; }
                        uint32_t t4, o4;
                        g_ptr[wq] = wb_word<FIELD>(wbk, pw, nv, t4, o4);
                        touched |= t4 << (4 * wq);
                        occ = (occ & ~(0xFu << (4 * wq))) | (o4 << (4 * wq));
                    }
                    stored = true;
                }
            }
            if (!stored) {
                uint32_t out[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    uint32_t t4, o4;
                    out[w] = wb_word<FIELD>(wbk, pre[w], n[w], t4, o4);
                    touched |= t4 << (4 * w);
                    occ |= o4 << (4 * w);
                }
                if (nw == 8) {
                    reinterpret_cast<uint4*>(g_ptr)[0] = make_uint4(out[0], out[1], out[2], out[3]);
                    reinterpret_cast<uint4*>(g_ptr)[1] = make_uint4(out[4], out[5], out[6], out[7]);
                } else {
#pragma unroll
                    for (int w = 0; w < 8; ++w) if (w < nw) g_ptr[w] = out[w];
                }
            }
            if (nw < 8) occ &= (1u << (4 * nw)) - 1u;                          // (cells past the tile's last column are not cells)
            v.occ[((size_t)tile * v.dim + row_t) * v.ow + gt] = occ;
            my_written += __popc(touched);
            by0 = min(by0, col_t + __ffs(touched) - 1); by1 = max(by1, col_t + 31 - __clz(touched));
            bx0 = min(bx0, row_t); bx1 = max(bx1, row_t);
        }
        batch0 += nbatch;
        bx0 = wave_min(bx0); bx1 = wave_max(bx1); by0 = wave_min(by0); by1 = wave_max(by1);
        if (lane == 0 && bx1 >= 0) {                                           // this workgroup is the tile's only writer
            atomicMin(&v.tile_bbox[4 * tile + 0], bx0); atomicMax(&v.tile_bbox[4 * tile + 1], bx1);
            atomicMin(&v.tile_bbox[4 * tile + 2], by0); atomicMax(&v.tile_bbox[4 * tile + 3], by1);
        }
    }
    const int ww = wave_sum(my_written);
    if (lane == 0 && ww) atomicAdd(s_written, ww);
}

}  // namespace rbpf
