// rbpf_api.hip -- C ABI of librbpf_hip.so (see include/rbpf_hip.h).  Host orchestration only:
// configuration checks, LUT construction, device memory, stream ordering.  All per-particle work
// runs in the gfx950 kernels of kernels_*.hip; there is no CPU compute path.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <limits>

#include "rbpf_host.h"
#include "rbpf_scanbatch.h"
#include "rbpf_pathbatch.h"
#include "rbpf_rolloutbatch.h"
#include "rbpf_footbatch.h"
#include "rbpf_localbatch.h"

using namespace rbpf;

static thread_local std::string g_create_err;

#define HIP_TRY(h, call)                                                                           \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            return RBPF_EDEVICE;                                                                   \
        }                                                                                          \
    } while (0)

// Every entry point runs on the handle's device and leaves the caller's current device as it found it (a process may
// hold engines on several GPUs, and torch keeps its own notion of the current device).
struct DevGuard {
    int prev = -1; bool switched = false;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != dev) { if (hipSetDevice(dev) == hipSuccess) switched = prev >= 0; else (void)hipGetLastError(); }
    }
    ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard&) = delete; DevGuard& operator=(const DevGuard&) = delete;
};
#define ON_DEVICE_HELD(h) DevGuard dev_guard_((h)->cfg.device)
// ... and, first thing, launches the map update a preceding rbpf_scan_update held back (rbpf_resample alone takes it over
// instead, rbpf_destroy drops it): whatever the entry point reads or queues finds the stream as if nothing had been held back
static int flush_map_update(rbpf_handle* h);
#define ON_DEVICE(h) ON_DEVICE_HELD(h); do { const int flush_rc_ = flush_map_update(h); if (flush_rc_) return flush_rc_; } while (0)

static int fail(rbpf_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}

// the shared argument checks of rbpf_scanbatch.h return their message, or null
#define ARG_TRY(h, check) do { if (const char* msg_ = (check)) return fail(h, RBPF_EINVAL, msg_); } while (0)
// an entry point that reads or queues behind what a half-done scan update holds
#define MID_STEP_TRY(h, what) do { if ((h)->scan_begun) return fail(h, RBPF_ESTATE, mid_step_message(what)); } while (0)

// the host outputs of a call, copied out of its scratch block behind the launch (a null one is skipped), and the wait for them
struct Fetch { void* host; const void* dev; size_t bytes; };
static int fetch(rbpf_handle* h, std::initializer_list<Fetch> outs) {
    for (const Fetch& o : outs)
        if (o.host) HIP_TRY(h, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

template <typename T>
static int dev_alloc(rbpf_handle* h, T** out, size_t n) {
    h->allocs.emplace_back();
    hipError_t e = h->allocs.back().reserve(n * sizeof(T));
    if (e != hipSuccess) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return RBPF_ENOMEM; }
    *out = h->allocs.back().as<T>();
    return RBPF_OK;
}
#define ALLOC(h, ptr, n) do { int rc_ = dev_alloc(h, &(ptr), (n)); if (rc_) return rc_; } while (0)

static int check_device_error(rbpf_handle* h) {
    int32_t e = 0;
    HIP_TRY(h, hipMemcpyAsync(&e, h->v.err, sizeof(e), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (e != 0) {
        int32_t z = 0;
        hipMemcpyAsync(h->v.err, &z, sizeof(z), hipMemcpyHostToDevice, h->stream);
        hipStreamSynchronize(h->stream);
        const char* what = e == RBPF_ENOMEM ? "tile pool or work-item queue exhausted"
                         : e == RBPF_ERANGE ? "a pose or beam left the addressable tile lattice (raise lattice_radius)"
                         : "device-side error";
        return fail(h, e, what);
    }
    return RBPF_OK;
}

static bool env_is(const char* name, const char* value) { const char* e = getenv(name); return e && strcmp(e, value) == 0; }
// The scan step's front half runs as two parts on two streams from SCAN_HALVES_MIN_PER_CU particles per CU up to, not including,
// SCAN_HALVES_END_PER_CU.  Measured on 256 CUs: a gain of 1 to 2.5 % of the step at 3072, 3584, 4096 and 4608
// particles, nothing at 5120, a loss at 1024, 2048 and from 6144 on - the gain hangs on how the parts' rounds of workgroups
// fall over the CUs
static const long long SCAN_HALVES_MIN_PER_CU = 12, SCAN_HALVES_END_PER_CU = 20;

// ---- trajectory log (kernels_track.hip): the pieces the step entry points queue while tracking is on ------------
// one record from the current state, in stream order.  Log full: an implicit record (a step's own) is dropped and counted, an
// explicit one is RBPF_ENOMEM; the host knows the count, nothing is read back
// the two halves apart: the record's place is taken when the step is called (-1: dropped), the record is queued when the step's
// held-back map update is (the record holds the weights, which the NaN branch of that update changes)
static int track_take_place(rbpf_handle* h, bool implicit, int& t) {
    t = -1;
    if (h->track_n >= h->track_cap) {
        if (!implicit) return fail(h, RBPF_ENOMEM, "the trajectory log is full");
        h->track_dropped++;
        return RBPF_OK;
    }
    t = h->track_n++;
    return RBPF_OK;
}
static int track_queue(rbpf_handle* h, int t) {
    if (t < 0) return RBPF_OK;
    launch_track_record(h->v, h->track_log(), t, h->track_pending(h->track_cur), h->stream);
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}
static int track_record(rbpf_handle* h, bool implicit) {
    int t;
    const int rc = track_take_place(h, implicit, t);
    return rc ? rc : track_queue(h, t);
}

extern "C" {

int rbpf_default_config(rbpf_config* c) {
    if (!c) return RBPF_EINVAL;
    memset(c, 0, sizeof(*c));
    c->n_particles = 1;          // main.py:44
    c->n_samples = 30;           // robot.py:17
    c->max_beams = 1081;
    c->tile_len_m = 40;          // hybridmap.py:68
    c->cell_size = 0.05;         // hybridmap.py:67
    c->lattice_radius = 3;
    c->pool_tiles = 0;
    c->log_odds_occ = 0.80;      // gridmap.py:20-24
    c->log_odds_nearby = 0.20;
    c->max_odds_occ = 3.0;
    c->log_odds_emp = -0.30;
    c->min_odds_emp = -3.0;
    c->quantum = 0.1;
    c->occupied_threshold = 1.0; // hybridmap.py:18
    c->max_ray_m = 15.0;         // hybridmap.py:107
    c->weight_min_range = 0.01;  // robot.py:130
    c->weight_max_range = 25.0;
    c->match_min_range = 1e-3;   // hybridmap.py:218
    c->match_max_range = 11.0;   // hybridmap.py:20
    c->resample_spread = 200.0;  // main.py:50
    c->vel_noise[0] = 0.02; c->vel_noise[1] = 0.01; c->vel_noise[2] = 0.2; c->vel_noise[3] = 0.02;  // Freid101IMUData.py:51-55
    c->device = 0;
    c->ndt_refine = 1;           // matchScanCustom.m:32-50 runs its second stage on every valid grid match
    c->seed = 42;
    return RBPF_OK;
}

static bool to_quanta(double val, double q, int& out) {
    double r = val / q;
    long n = lround(r);
    if (fabs(r - (double)n) > 1e-9 || n < -127 || n > 127) return false;
    out = (int)n;
    return true;
}

int rbpf_create(const rbpf_config* cfg, rbpf_handle** out) {
    if (!cfg || !out) return fail(nullptr, RBPF_EINVAL, "null argument");
    *out = nullptr;
    const rbpf_config& c = *cfg;
    if (c.n_particles < 1) return fail(nullptr, RBPF_EINVAL, "n_particles must be >= 1");
    if (c.n_samples < 1 || c.n_samples > 32) return fail(nullptr, RBPF_EINVAL, "n_samples must be in 1..32");
    if (c.max_beams < 1 || c.max_beams > 4095) return fail(nullptr, RBPF_EINVAL, "max_beams must be in 1..4095");
    if (c.lattice_radius < 0 || c.lattice_radius > 3) return fail(nullptr, RBPF_EINVAL, "lattice_radius must be in 0..3");
    if (c.ndt_refine < 0 || c.ndt_refine > 2) return fail(nullptr, RBPF_EINVAL, "ndt_refine must be 0, 1 or 2");
    if (!(c.cell_size > 0) || c.tile_len_m < 1) return fail(nullptr, RBPF_EINVAL, "cell_size/tile_len_m");   // gridmap.py:29
    const int dim = (int)llround((double)c.tile_len_m / c.cell_size);                                        // gridmap.py:31
    if (dim < WIN || dim > 4096 || dim % 16 != 0) return fail(nullptr, RBPF_EINVAL, "tile dimension must be a multiple of 16 in 128..4096 cells");
    if (!(c.max_ray_m > 0) || c.max_ray_m / c.cell_size + 4 >= dim)
        return fail(nullptr, RBPF_EINVAL, "max_ray_m must be shorter than one tile");
    CellConsts cc;
    if (!(c.quantum > 0) || !to_quanta(c.log_odds_occ, c.quantum, cc.occ) || !to_quanta(c.log_odds_nearby, c.quantum, cc.nearby) ||
        !to_quanta(c.log_odds_emp, c.quantum, cc.emp) || !to_quanta(c.max_odds_occ, c.quantum, cc.vmax) ||
        !to_quanta(c.min_odds_emp, c.quantum, cc.vmin))
        return fail(nullptr, RBPF_EINVAL, "log-odds constants must be integer multiples of quantum within int8");
    if (cc.emp >= 0 || cc.occ <= 0 || cc.nearby < 0 || cc.vmin > 0 || cc.vmax < 0)
        return fail(nullptr, RBPF_EINVAL, "log-odds constants have the wrong sign");
    cc.thr = (int)floor(c.occupied_threshold / c.quantum + 1e-9);

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e == hipSuccess && (c.device < 0 || c.device >= n_dev)) e = hipErrorInvalidDevice;
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, RBPF_EDEVICE, std::string("device ") + std::to_string(c.device) + ": " + hipGetErrorString(e) +
                                     " (librbpf_hip needs an MI355X; there is no CPU path)"); }
    DevGuard dev_guard_(c.device);         // the caller's current device is restored on return

    rbpf_handle* h = new rbpf_handle();
    h->cfg = c;
    memset(&h->counters, 0, sizeof(h->counters));
    DevView& v = h->v;
    memset(&v, 0, sizeof(v));
    v.P = c.n_particles; v.K = c.n_samples; v.B = 0; v.dim = dim; v.R = c.lattice_radius; v.L = 2 * v.R + 1;
    v.pool_tiles = c.pool_tiles > 0 ? c.pool_tiles : 2 * c.n_particles;
    if (v.pool_tiles < v.P) { delete h; return fail(nullptr, RBPF_EINVAL, "pool_tiles must be >= n_particles"); }
    v.cs = c.cell_size; v.tile_len = (double)c.tile_len_m;
    v.quantum = c.quantum;
    double inv = 1.0 / c.quantum;
    v.inv_quantum = fabs(inv - round(inv)) < 1e-9 ? round(inv) : 0.0;
    v.cc = cc;
    v.w_min_range = c.weight_min_range; v.w_max_range = c.weight_max_range;
    v.reach = (int)(c.max_ray_m / c.cell_size) + 3;

    // ---- global-index LUT (hybridmap.py:123,136 + gridmap.py:93) -------------------------------
    {
        const int half = v.R * dim + dim / 2 + 2;
        std::vector<uint32_t>& lut = h->h_lut;
        int g_first = INT32_MAX;
        for (int g = -half; g <= half; ++g) {
            double pos = (double)g * v.cs;                       // hybridmap.py:123
            int lat;
            if (!tile_of_coord(pos, v.tile_len, v.R, lat)) { if (g_first != INT32_MAX) break; else continue; }
            double rel = pos - (double)lat * v.tile_len;         // hybridmap.py:136
            int cidx = trunc_to_int(rel / v.cs + (double)dim / 2.0);   // gridmap.py:93
            if (cidx < 0 || cidx >= dim) { delete h; return fail(nullptr, RBPF_EINVAL, "cell index formula leaves the tile for this cell_size (the reference would raise IndexError)"); }
            if (g_first == INT32_MAX) g_first = g;
            uint32_t ent = ((uint32_t)(lat + v.R) << 16) | (uint32_t)cidx;
            if (!lut.empty() && ent < lut.back()) { delete h; return fail(nullptr, RBPF_EINVAL, "cell index formula is not monotone for this cell_size"); }
            lut.push_back(ent);
        }
        v.g_min = g_first; v.n_lut = (int)lut.size();
    }

    int rc = RBPF_OK;
    auto build = [&]() -> int {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
        for (int k = 0; k < rbpf_handle::N_KERN; ++k)
            for (int e = 0; e < 2; ++e) {
                h->ring[k][e].resize(rbpf_handle::RING);
                // timing only: no system-scope fence when the event completes (it would flush the caches between the
                // kernels it brackets and slow the very thing it measures)
                for (auto& ev : h->ring[k][e]) HIP_TRY(h, h->events.create(&ev, hipEventDisableSystemFence));
                h->begin_used[k].assign(rbpf_handle::RING, nullptr);
            }
        for (int e = 0; e < 2; ++e) {
            h->rs_mid[e].resize(rbpf_handle::RING);
            for (auto& ev : h->rs_mid[e]) HIP_TRY(h, h->events.create(&ev, hipEventDisableSystemFence));
        }
        h->rs_split.assign(rbpf_handle::RING, 0);
        const size_t P = v.P, LL = (size_t)v.L * v.L, cells = (size_t)dim * dim;
        uint32_t* d_lut; ALLOC(h, d_lut, h->h_lut.size()); v.lut = d_lut;
        HIP_TRY(h, hipMemcpy(d_lut, h->h_lut.data(), h->h_lut.size() * 4, hipMemcpyHostToDevice));
        {   // inverse LUT: first global index of every 128-cell window of every lattice row
            const int KW = (dim + WIN - 1) / WIN;
            std::vector<int32_t> gw((size_t)v.L * (KW + 1));
            for (int a = 0; a < v.L; ++a)
                for (int k = 0; k <= KW; ++k) {
                    uint32_t key = k < KW ? (((uint32_t)a << 16) | (uint32_t)(k * WIN)) : ((uint32_t)(a + 1) << 16);
                    auto it = std::lower_bound(h->h_lut.begin(), h->h_lut.end(), key);
                    gw[(size_t)a * (KW + 1) + k] = v.g_min + (int32_t)(it - h->h_lut.begin());
                }
            int32_t* d_gw; ALLOC(h, d_gw, gw.size()); v.gwin = d_gw;
            HIP_TRY(h, hipMemcpy(d_gw, gw.data(), gw.size() * 4, hipMemcpyHostToDevice));
        }
        ALLOC(h, v.px, P); ALLOC(h, v.py, P); ALLOC(h, v.pth, P); ALLOC(h, v.cov, 9 * P); ALLOC(h, v.weight, P);
        ALLOC(h, v.slot, P); ALLOC(h, v.global_id, P);
        v.ow = (dim + 31) / 32;
        ALLOC(h, v.tile_tab, P * LL); ALLOC(h, v.pool, (size_t)v.pool_tiles * cells);
        ALLOC(h, v.occ, (size_t)v.pool_tiles * dim * v.ow + 4);       // (+4: the matcher's staging loads two / three words at a time)
        HIP_TRY(h, hipMemset(v.occ, 0, (size_t)v.pool_tiles * dim * v.ow * 4));
        ALLOC(h, v.tile_bbox, (size_t)v.pool_tiles * 4); ALLOC(h, v.free_stack, v.pool_tiles); ALLOC(h, v.free_top, 1);
        {   // the scan block: one device buffer, uploaded with one copy per scan (rbpf_set_scan)
            const size_t MB = (size_t)c.max_beams, MBP = (MB + 15) & ~(size_t)15;
            const size_t MBW = (MB + 63) & ~(size_t)63;           // the weighting's list is padded to whole passes of 64 beams
            h->scan_bytes = 3 * MBP * 8 + 4 * MBP * 4 + MBP + 2 * MBW * 4 + MBW * 2;
            ALLOC(h, h->d_scan, h->scan_bytes);
            unsigned char* d = h->d_scan;
            v.bx = reinterpret_cast<double*>(d); v.by = v.bx + MBP; v.bscale = v.by + MBP;
            v.msel_x = reinterpret_cast<float*>(d + 3 * MBP * 8); v.msel_y = v.msel_x + MBP; v.asel_x = v.msel_y + MBP; v.asel_y = v.asel_x + MBP;
            v.bflags = d + 3 * MBP * 8 + 4 * MBP * 4;
            v.wsel_x = reinterpret_cast<const float*>(d + 3 * MBP * 8 + 4 * MBP * 4 + MBP); v.wsel_y = v.wsel_x + MBW;
            v.wsel_idx = reinterpret_cast<const uint16_t*>(v.wsel_y + MBW);
            HIP_TRY(h, h->rings[R_SCAN].create(h->scan_bytes));
            HIP_TRY(h, h->rings[R_LAST].create(MB * 16));
            HIP_TRY(h, h->rings[R_IDX].create((size_t)P * 8));
        }
        ALLOC(h, v.upd_pose, 3 * P);
        ALLOC(h, v.prop_prep, 24 * P);
        ALLOC(h, v.prop_samp, 256 * P);
        ALLOC(h, v.stats, ST_COUNT); ALLOC(h, v.err, 1);
        ALLOC(h, v.mu_fallback, P); HIP_TRY(h, hipMemset(v.mu_fallback, 0, P * 4));
        ALLOC(h, v.ev_queue, 2); HIP_TRY(h, hipMemset(v.ev_queue, 0, 8));   // zeroed once: every launch leaves it zero (kernels_mapev.hip)
        ALLOC(h, h->d_did_early, 1);
        HIP_TRY(h, hipMemset(h->d_did_early, 0, 4));
        HIP_TRY(h, h->events.create(&h->ev_weights, hipEventDisableTiming | hipEventDisableSystemFence));   // device-side ordering only
        {   // RBPF_MAP_KERNEL=window keeps the 128x128-window map update for every particle, =ray / =ev run that first kernel (and
            // windows behind it); default: the event-walk kernel, windows for what it gives back (tests, comparisons)
            v.mu_mode = env_is("RBPF_MAP_KERNEL", "window") ? MU_WINDOW : env_is("RBPF_MAP_KERNEL", "ray") ? MU_RAY : env_is("RBPF_MAP_KERNEL", "ev") ? MU_EV : MU_DEFAULT;
            // the event walk's workgroups stay resident and draw particles from a queue; RBPF_EV_RESIDENT=0: one workgroup per
            // particle (A/B runs, tests), RBPF_EV_GRID=n: at most n resident workgroups (tests: several particles in a row)
            v.ev_resident = env_is("RBPF_EV_RESIDENT", "0") ? 0 : 1;
            const char* eg = getenv("RBPF_EV_GRID");
            v.ev_grid = eg ? std::max(0, atoi(eg)) : 0;
            v.match_stage_slow = env_is("RBPF_MATCH_STAGE", "slow") ? 1 : 0;    // the matcher's field is staged bit by bit (tests)
            const char* ws = getenv("RBPF_WSAFE");          // test knob: the weighting's guard band in cells (0 shows what the band is for)
            v.wsafe_override = ws ? (float)atof(ws) : -1.0f;
            v.weight_entry_f64 = env_is("RBPF_WEIGHT_ENTRY", "f64") ? 1 : 0;   // rbpf_weight_samples runs the float64 kernel (comparison)
            v.ndt_refine = h->cfg.ndt_refine;
            h->dedup_enabled = !env_is("RBPF_MATCH_DEDUP", "0");   // "0": every particle runs the matcher, duplicates included (tests)
            {   // rbpf_scan_update holds its map update back for the resample where that pays (rbpf_host.h: hold_back)
                int cus = 0;
                if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 1; }
                h->skip_discarded = !env_is("RBPF_SKIP_DISCARDED", "0");   // "0": the held-back map update leaves nobody out (A/B runs, tests)
                h->hold_back = getenv("RBPF_SKIP_DISCARDED") ? true : (long long)P > 4LL * cus;
                // the front half of the step as two staggered half-batches (rbpf_host.h: halves_first).  RBPF_SCAN_HALVES=1: always
                // (tests, A/B runs), =0: never; unset: the size rule measured in DESIGN.md 6
                const bool halves = env_is("RBPF_SCAN_HALVES", "0") ? false : getenv("RBPF_SCAN_HALVES") ? true : ((long long)P >= SCAN_HALVES_MIN_PER_CU * cus && (long long)P < SCAN_HALVES_END_PER_CU * cus);
                if (halves) {
                    int least = 0, greatest = 0;
                    HIP_TRY(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
                    HIP_TRY(h, hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, greatest));
                    // device-side ordering only; two of them ride on a kernel's dispatch, as the timing events do
                    HIP_TRY(h, h->events.create(&h->ev_fork, hipEventDisableTiming | hipEventDisableSystemFence));
                    HIP_TRY(h, h->events.create(&h->ev_half_match, hipEventDisableSystemFence));
                    HIP_TRY(h, h->events.create(&h->ev_half_weight, hipEventDisableSystemFence));
                    // the first part is the larger one: five eighths measured best at the flagship size; a filter of
                    // one particle has no second part
                    h->halves_first = (int)(P - std::max<size_t>(P > 1 ? 1 : 0, 3 * P / 8));
                }
            }
        }
        ALLOC(h, v.dup_of, P); v.dups_valid = 0;
        ALLOC(h, h->d_last_xy, 2 * (size_t)c.max_beams); ALLOC(h, h->d_tmp_sel, 2 * (size_t)c.max_beams);
        if (raycast_lds_bytes(c.max_beams, v.reach) > LDS_LIMIT) return fail(h, RBPF_EINVAL, "max_beams too large for the LDS window layout");
        match_geometry(c, c.cell_size, h->mN, h->mds, h->mmcs, h->md0, h->mncr);
        h->mlds = match_lds_bytes(h->mN, c.max_beams, match_max_coarse(h->mncr, 0.7, h->mmcs), match_per_rot(0.7, h->mmcs));
        if (h->mlds > LDS_LIMIT) return fail(h, RBPF_EINVAL, "matcher region does not fit in LDS for this cell_size");
        if (c.ndt_refine && ndt_cells(h->mmcs) >= 2) {         // the matcher hands its staged field to the NDT kernel
            if (ndt_lds_bytes(h->mN, c.max_beams) > LDS_LIMIT) return fail(h, RBPF_EINVAL, "NDT stage: matcher region does not fit in LDS");
            ALLOC(h, v.ndt_occ, P * (size_t)h->mN * (h->mN / 32)); ALLOC(h, v.ndt_aux, 5 * P);
        }
        ALLOC(h, h->d_match, 13 * P); ALLOC(h, h->d_bad, P); ALLOC(h, h->d_guess_full, P * (size_t)c.n_samples * 3);
        {
            ResampleBuffers& r = h->rs;
            ALLOC(h, r.T, P); ALLOC(h, r.idx, P); ALLOC(h, r.did, 1); ALLOC(h, r.slot2, P); ALLOC(h, r.dead_list, P);
            ALLOC(h, r.jobs, 2 * P); ALLOC(h, r.n_jobs, 2); ALLOC(h, r.pending_free, (size_t)v.pool_tiles); ALLOC(h, r.n_pending, 1);
            ALLOC(h, r.px2, P); ALLOC(h, r.py2, P); ALLOC(h, r.pth2, P); ALLOC(h, r.cov2, 9 * P); ALLOC(h, r.w2, P);
            ALLOC(h, r.skip, P); ALLOC(h, r.keep, P); ALLOC(h, r.plan, 2);
            HIP_TRY(h, hipMemset(r.n_pending, 0, 4)); HIP_TRY(h, hipMemset(r.n_jobs, 0, 8)); HIP_TRY(h, hipMemset(r.did, 0, 4));
            HIP_TRY(h, hipMemset(r.skip, 0, P)); HIP_TRY(h, hipMemset(r.plan, 0, 8));
        }
        HIP_TRY(h, hipMemset(v.pool, 0, (size_t)v.pool_tiles * cells));
        HIP_TRY(h, hipMemset(v.px, 0, P * 8)); HIP_TRY(h, hipMemset(v.py, 0, P * 8)); HIP_TRY(h, hipMemset(v.pth, 0, P * 8));
        HIP_TRY(h, hipMemset(v.cov, 0, 9 * P * 8));
        HIP_TRY(h, hipMemset(v.stats, 0, ST_COUNT * 8)); HIP_TRY(h, hipMemset(v.err, 0, 4));
        // robot.py:20-28 / hybridmap.py:70: weight 1.0, one empty tile centred (0,0) per particle
        std::vector<double> w(P, 1.0);
        HIP_TRY(h, hipMemcpy(v.weight, w.data(), P * 8, hipMemcpyHostToDevice));
        std::vector<int32_t> ids(P), tab(P * LL, -1), fs(v.pool_tiles), bb((size_t)v.pool_tiles * 4);
        for (size_t p = 0; p < P; ++p) { ids[p] = (int32_t)p; tab[p * LL + (size_t)v.R * v.L + v.R] = (int32_t)p; }
        for (int t = 0; t < v.pool_tiles; ++t) { bb[4 * t] = INT32_MAX; bb[4 * t + 1] = -1; bb[4 * t + 2] = INT32_MAX; bb[4 * t + 3] = -1; }
        int32_t top = v.pool_tiles - (int32_t)P;
        for (int i = 0; i < top; ++i) fs[i] = v.pool_tiles - 1 - i;   // pop order: P, P+1, ...
        HIP_TRY(h, hipMemcpy(v.slot, ids.data(), P * 4, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(v.global_id, ids.data(), P * 4, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(v.tile_tab, tab.data(), P * LL * 4, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(v.free_stack, fs.data(), (size_t)v.pool_tiles * 4, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(v.free_top, &top, 4, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(v.tile_bbox, bb.data(), bb.size() * 4, hipMemcpyHostToDevice));
        return RBPF_OK;
    };
    rc = build();
    if (rc != RBPF_OK) { g_create_err = h->err; rbpf_destroy(h); return rc; }
    *out = h;
    return RBPF_OK;
}

// Teardown order: (1) everything queued on the handle's stream has finished; (2) every event that guards host memory
// a kernel or a copy may still touch has completed (every Staging, the rings' slots included, and ev_weights) - the early
// read-back and the pinned rings can be in use by work on ANOTHER stream (rbpf_resample_indices_global_early takes one);
// (3) device memory (dev_alloc's, then every DevBuf), host staging memory, events, each kind in one loop; (4) the
// stream, only if the handle created it.  A borrowed stream (rbpf_set_stream) is synchronised once and otherwise left
// alone: it belongs to the caller and may already be gone when a late destructor runs.
int rbpf_destroy(rbpf_handle* h) {
    if (!h) return RBPF_OK;
    ON_DEVICE_HELD(h);
    h->mu_pending = false;                                                                // a held-back map update is dropped with the maps
    if (hipStreamSynchronize(h->stream) != hipSuccess) (void)hipGetLastError();          // nullptr: a borrowed null stream
    if (h->side && hipStreamSynchronize(h->side) != hipSuccess) (void)hipGetLastError();  // (joined into the stream by every step: idle unless a step failed half-way)
    h->each_staging([](Staging& s) { if (s.wait() != hipSuccess) (void)hipGetLastError(); });
    if (h->ev_weights_valid && hipEventSynchronize(h->ev_weights) != hipSuccess) (void)hipGetLastError();
    for (Block& b : h->allocs) b.release();
    for (Block& b : h->buf) b.release();
    for (Block& b : h->track_mem) b.release();
    h->each_staging([](Staging& s) { s.release(); });
    h->each_staging([](Staging& s) { s.destroy_event(); });
    h->events.destroy();
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    if (h->side) (void)hipStreamDestroy(h->side);
    (void)hipGetLastError();
    delete h;
    return RBPF_OK;
}

const char* rbpf_last_error(const rbpf_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rbpf_set_stream(rbpf_handle* h, void* s) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));        // nullptr = the default stream
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->own_stream = false;
    h->stream = static_cast<hipStream_t>(s);
    h->last_end = nullptr;
    return RBPF_OK;
}

// gives a borrowed stream back: everything queued on it by this handle has finished when the call returns, and the
// handle works on a stream of its own again (as after rbpf_create)
int rbpf_release_stream(rbpf_handle* h) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (h->own_stream) return RBPF_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->early_n > 0) HIP_TRY(h, h->stage[S_EARLY].wait());
    h->stream = nullptr;
    HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    h->last_end = nullptr;
    return RBPF_OK;
}

int rbpf_abi_struct_bytes(int32_t* config_bytes, int32_t* counters_bytes) {
    if (config_bytes) *config_bytes = (int32_t)sizeof(rbpf_config);
    if (counters_bytes) *counters_bytes = (int32_t)sizeof(rbpf_counters);
    return RBPF_OK;
}

int rbpf_synchronize(rbpf_handle* h) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    return check_device_error(h);
}

int rbpf_set_profiling_families(rbpf_handle* h, uint32_t mask) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    return rbpf_set_profiling(h, mask ? (int)(0x100u | (mask & 0x1Fu)) : 0);
}

int rbpf_set_profiling(rbpf_handle* h, int on) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    h->profiling = on != 0;
    h->prof_mask = !on ? 0u : (on & 0x100) ? ((unsigned)on & 0x1Fu) : 0x1Fu;
    for (int k = 0; k < rbpf_handle::N_KERN; ++k) h->ring_n[k] = 0;
    h->last_end = nullptr;
    HIP_TRY(h, hipMemsetAsync(h->v.stats, 0, ST_COUNT * sizeof(unsigned long long), h->stream));   // counters restart
    return RBPF_OK;
}

int rbpf_get_kernel_ms(rbpf_handle* h, int32_t which, double* out_ms, int32_t cap, int32_t* n_out) {
    if (!h || !n_out || which < 0 || which >= rbpf_handle::N_KERN) return RBPF_EINVAL;
    ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int n = std::min(h->ring_n[which], rbpf_handle::RING);
    int first = h->ring_n[which] - n;
    int m = 0;
    for (int i = 0; i < n && m < cap; ++i) {
        int slot = (first + i) % rbpf_handle::RING;
        float ms = 0;
        if (h->family_ms(which, slot, &ms) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (out_ms) out_ms[m] = ms;
        ++m;
    }
    *n_out = m;
    return RBPF_OK;
}

int rbpf_get_counters(rbpf_handle* h, rbpf_counters* out) {
    if (!h || !out) return RBPF_EINVAL;
    ON_DEVICE(h);
    unsigned long long st[ST_COUNT];
    int32_t top = 0;
    HIP_TRY(h, hipMemcpyAsync(st, h->v.stats, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&top, h->v.free_top, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    rbpf_counters& c = h->counters;
    c.scan_updates = h->scan_updates;
    c.ray_cells_visited = st[ST_RAY_CELLS]; c.cells_written = st[ST_CELLS_WRITTEN];
    c.cells_gathered = st[ST_GATHERS]; c.slow_cells = st[ST_SLOW_CELLS];
    c.resample_copies = st[ST_COPIES]; c.bytes_copied = st[ST_COPY_BYTES];
    c.tiles_in_use = (uint64_t)(h->v.pool_tiles - top);
    c.window_fallbacks = st[ST_WINDOW_FALLBACKS];
    c.ndt_runs = st[ST_NDT_RUNS]; c.ndt_evaluations = st[ST_NDT_EVALS]; c.ndt_accepted = st[ST_NDT_ACCEPTED];
    c.match_shared = st[ST_MATCH_SHARED];
    for (int k = 0; k < 7; ++k) c.reserved[k] = st[8 + k];
    c.stamp7 = st[15];
    {   // the packed form saturates per field; the exact tallies follow in their own fields
        auto sat16 = [](unsigned long long x) { return x > 65535ull ? 65535ull : x; };
        c.fallback_reasons = sat16(st[ST_FALLBACK_REASONS]) | (sat16(st[ST_FB_BOUND]) << 16) | (sat16(st[ST_FB_TABLES]) << 32);
        c.fallback_geometry = st[ST_FALLBACK_REASONS]; c.fallback_bound = st[ST_FB_BOUND]; c.fallback_tables = st[ST_FB_TABLES];
        c.map_events = st[ST_MAP_EVENTS]; c.map_event_overflows = st[ST_EV_OVERFLOWS];
    }
    c.map_windows = st[ST_MAP_WINDOWS];
    c.map_updates_skipped = st[ST_MU_SKIPPED];
    c.map_pool_cells = st[ST_POOL_CELLS]; c.map_near_cells = st[ST_NEAR_CELLS];
    if (h->profiling) {
        double* dst[5] = {&c.ms_raycast, &c.ms_weight, &c.ms_resample, &c.ms_match, &c.ms_ndt};
        for (int k = 0; k < 5; ++k) {
            if (h->ring_n[k] == 0) continue;
            int slot = (h->ring_n[k] - 1) % rbpf_handle::RING;
            float ms = 0;
            if (h->family_ms(k, slot, &ms) == hipSuccess) *dst[k] = ms;
        }
        (void)hipGetLastError();
    }
    *out = c;
    return RBPF_OK;
}

// ---- a1 ---------------------------------------------------------------------------------------------
// the scan block from sensor-frame end points: range classes, compacted matcher lists, one upload
static int upload_scan_points(rbpf_handle* h, const double* px, const double* py, int32_t B) {
    const rbpf_config& c = h->cfg;
    DevView& v = h->v;
    unsigned char* slot = static_cast<unsigned char*>(h->rings[R_SCAN].acquire());
    double *sx = h->in_slot(slot, v.bx), *sy = h->in_slot(slot, v.by), *sc = h->in_slot(slot, v.bscale);
    float *mx = h->in_slot(slot, v.msel_x), *my = h->in_slot(slot, v.msel_y);       // compacted beam lists for the matcher
    float *ax = h->in_slot(slot, v.asel_x), *ay = h->in_slot(slot, v.asel_y);       // (float32, sensor frame)
    uint8_t* fl = h->in_slot(slot, v.bflags);
    float *wx = h->in_slot(slot, v.wsel_x), *wy = h->in_slot(slot, v.wsel_y);       // the weighting's beams (kernels_propose.hip, weight_beams)
    uint16_t* wi = h->in_slot(slot, v.wsel_idx);
    const float w_inv_cs = (float)((double)h->v.dim / h->v.tile_len), w_lim = 1.5f * (float)h->v.dim;
    int nm = 0, na = 0, nw = 0;
    for (int i = 0; i < B; ++i) {
        const double x = px[i], y = py[i];
        double dist = sqrt(x * x + y * y);               // robot.py:129, hybridmap.py:105,217
        uint8_t f = 0;
        if (dist < c.weight_max_range && dist > c.weight_min_range) f |= BF_WEIGHT;   // robot.py:130
        if (dist < c.match_max_range && dist > c.match_min_range) f |= BF_MATCH;      // hybridmap.py:218
        if (dist < c.match_max_range) f |= BF_MATCH_ADJ;                              // hybridmap.py:172
        double s = 1.0;
        if (dist > c.max_ray_m) { f |= BF_LONG; s = c.max_ray_m / dist; }             // hybridmap.py:107-108
        sx[i] = x; sy[i] = y; sc[i] = s; fl[i] = f;
        if (f & BF_MATCH) { mx[nm] = (float)x; my[nm] = (float)y; ++nm; }
        if (f & BF_MATCH_ADJ) { ax[na] = (float)x; ay[na] = (float)y; ++na; }
        if (f & BF_WEIGHT) {
            const float x32 = (float)x, y32 = (float)y;
            const bool in_budget = h->v.dim <= 2048 && (fabsf(x32) + fabsf(y32)) * w_inv_cs <= w_lim;   // the error budget's premise
            wx[nw] = in_budget ? x32 : NAN; wy[nw] = y32; wi[nw] = (uint16_t)i; ++nw;
        }
    }
    for (int i = nw; i < ((nw + 63) & ~63); ++i) { wx[i] = NAN; wy[i] = 0.0f; wi[i] = 0; }
    v.n_msel = nm; v.n_asel = na; v.n_wsel = nw;
    HIP_TRY(h, h->rings[R_SCAN].upload(h->d_scan, h->scan_bytes, h->stream));
    v.B = B;
    h->have_scan = true;
    return RBPF_OK;
}

int rbpf_set_scan(rbpf_handle* h, const double* ranges, const double* angles, int32_t B) {
    if (!h || !ranges || !angles) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (B < 1 || B > h->cfg.max_beams) return fail(h, RBPF_EINVAL, "n_beams out of range");
    std::vector<double> x((size_t)B), y((size_t)B);
    for (int i = 0; i < B; ++i) {
        x[i] = ranges[i] * cos(angles[i]);               // lidar.py:78
        y[i] = ranges[i] * sin(angles[i]);               // lidar.py:79
    }
    return upload_scan_points(h, x.data(), y.data(), B);
}

// the same from a Scan object's own state: its sensor-frame end points x(), y() (lidar.py:76-87)
int rbpf_set_scan_xy(rbpf_handle* h, const double* x, const double* y, int32_t B) {
    if (!h || !x || !y) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (B < 1 || B > h->cfg.max_beams) return fail(h, RBPF_EINVAL, "n_beams out of range");
    return upload_scan_points(h, x, y, B);
}

// ---- a2 ---------------------------------------------------------------------------------------------
int rbpf_imu_update(rbpf_handle* h, int32_t model, const double* d, double dt_ticks) {
    if (!h || !d) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (model < 0 || model > 2) return fail(h, RBPF_EINVAL, "unknown motion model");
    launch_imu_update(h->v, model, d[0], d[1], d[2], dt_ticks, h->cfg.vel_noise, h->stream);
    HIP_TRY(h, hipGetLastError());
    if (h->track_on && (h->track_flags & RBPF_TRACK_IMU)) return track_record(h, true);
    return RBPF_OK;
}

// ---- a4 test entry --------------------------------------------------------------------------------------
int rbpf_weight_samples(rbpf_handle* h, const double* guesses, const double* prs, int32_t K, double* out_w) {
    if (!h || !guesses || !prs || !out_w) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->have_scan) return fail(h, RBPF_ESTATE, "rbpf_set_scan has not been called");
    if (K < 1 || K > 32) return fail(h, RBPF_EINVAL, "n_samples must be in 1..32");
    const size_t n = (size_t)h->v.P * K;
    HIP_TRY(h, h->reserve(B_SAMPLES, n * 5 * 8));
    double *d_guess = h->buf[B_SAMPLES].as<double>(), *d_prs = d_guess + 3 * n, *d_w = d_prs + n;
    HIP_TRY(h, hipMemcpyAsync(d_guess, guesses, n * 3 * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_prs, prs, n * 8, hipMemcpyHostToDevice, h->stream));
    h->prof_begin(1);
    if (h->v.weight_entry_f64) launch_weight_samples(h->v, d_guess, d_prs, K, d_w, h->stream);
    else launch_weight_samples_product(h->v, d_guess, d_prs, K, d_w, h->stream);   // the look-ups of every scan step (kernels_propose.hip)
    h->prof_end(1);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_w, d_w, n * 8, hipMemcpyDeviceToHost, h->stream));
    return check_device_error(h);
}

// ---- a5 test entry --------------------------------------------------------------------------------------
// the map-update chain on view v: the handle's own, or that with the list of the particles the coming resample keeps
static int run_map_update(rbpf_handle* h, const DevView& v, const uint8_t* d_bad = nullptr) {
    // The map update's timing events ride on the first kernel's dispatch (its own start and end: the dominant kernel, without
    // the follow-up launch that usually finds nothing to do) - two event records and their barriers less in the stream per step.
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (map_update_first_kernel(v) != 0 && h->prof_take(0, t0, t1)) h->ev_workgroups = launch_map_update_fused(v, d_bad, h->stream, t0, t1);
    else {
        h->prof_begin(0);
        h->ev_workgroups = launch_map_update_fused(v, d_bad, h->stream);
        h->prof_end(0);
    }
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}

// what rbpf_scan_update held back, with view v: the map update with the NaN-branch increments, then the step's trajectory record
static int launch_held_map_update(rbpf_handle* h, const DevView& v) {
    h->mu_pending = false;
    int rc = run_map_update(h, v, h->d_bad);
    if (rc) return rc;
    rc = track_queue(h, h->mu_pending_rec);
    h->mu_pending_rec = -1;
    return rc;
}
static int flush_map_update(rbpf_handle* h) { return h->mu_pending ? launch_held_map_update(h, h->v) : RBPF_OK; }

int rbpf_map_update(rbpf_handle* h, const double* poses) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    h->v.dups_valid = 0;
    if (!h->have_scan) return fail(h, RBPF_ESTATE, "rbpf_set_scan has not been called");
    DevView& v = h->v;
    const size_t P = v.P;
    if (poses) {
        std::vector<double> soa(3 * P);
        for (size_t p = 0; p < P; ++p) { soa[p] = poses[3 * p]; soa[P + p] = poses[3 * p + 1]; soa[2 * P + p] = poses[3 * p + 2]; }
        HIP_TRY(h, hipMemcpyAsync(v.upd_pose, soa.data(), 3 * P * 8, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {
        HIP_TRY(h, hipMemcpyAsync(v.upd_pose, v.px, P * 8, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(v.upd_pose + P, v.py, P * 8, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(v.upd_pose + 2 * P, v.pth, P * 8, hipMemcpyDeviceToDevice, h->stream));
    }
    int rc = run_map_update(h, h->v);
    if (rc) return rc;
    h->scan_updates++;
    return check_device_error(h);
}

// the previous scan of an adj = 1 step: the device-resident one (n_last: its size), or the caller's, uploaded on the stream
static int stage_last_scan(rbpf_handle* h, int32_t adj, const double* last_scan_xy, int32_t& n_last) {
    if (adj && !last_scan_xy) {                 // the device-resident previous scan (rbpf_refresh_last_scan / rbpf_import_last_scan)
        if (h->n_last_dev < 0) return fail(h, RBPF_ESTATE, "adj = 1 without last_scan_xy needs rbpf_refresh_last_scan first");
        n_last = h->n_last_dev;
    } else if (adj && (n_last < 0 || n_last > h->cfg.max_beams))
        return fail(h, RBPF_EINVAL, "adj = 1 needs last_scan_xy with at most max_beams points");
    if (adj && last_scan_xy) {
        void* slot = h->rings[R_LAST].acquire();
        memcpy(slot, last_scan_xy, (size_t)n_last * 16);
        HIP_TRY(h, hipMemcpyAsync(h->d_last_xy, slot, (size_t)n_last * 16, hipMemcpyHostToDevice, h->stream));
        h->rings[R_LAST].submitted(h->stream);
    }
    return RBPF_OK;
}

// one matcher stage (1: grid search, 2: NDT) for particles [p0, p0 + n) on stream s; stage 0: whether the NDT stage is active
static bool match_stage(rbpf_handle* h, int32_t adj, int32_t n_last, int stage, int p0, int n, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
    return launch_match_particles(h->v, adj ? 1 : 0, h->d_last_xy, adj ? n_last : 0, h->d_match, h->mN, h->mds, h->mmcs, h->md0,
                                  h->mncr, h->cfg.match_max_range, h->cfg.max_beams, h->mlds, stage, p0, n, s, t0, t1);
}

static int run_matcher(rbpf_handle* h, int32_t adj, int32_t n_last) {
    // both stages are one kernel each: their timing events ride on the dispatch and take the kernel's own start and end
    hipEvent_t t0 = nullptr, t1 = nullptr;
    h->prof_take(3, t0, t1);
    if (match_stage(h, adj, n_last, 1, 0, h->v.P, h->stream, t0, t1)) {
        h->prof_take(4, t0, t1);
        match_stage(h, adj, n_last, 2, 0, h->v.P, h->stream, t0, t1);
    }
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}

// The front half of the step as two staggered half-batches (rbpf_host.h: halves_first): particles [0, n0) on
// the side stream behind everything the step has queued so far, [n0, P) on the handle's stream.  Nothing couples one
// particle to another here but an exact duplicate's read of its representative's match row; the representative is the first
// copy, the lower index, so only the second half can read across the split: its frame kernel waits for the first half's
// last matcher kernel.  The stream continues behind both halves' weighting.
static int run_front_halves(rbpf_handle* h, int32_t adj, int32_t n_last, const int32_t* match_of, const double* d_g) {
    const DevView& v = h->v;
    const int n0 = std::min(h->halves_first, v.P), n1 = v.P - n0;
    const bool ndt = match_stage(h, adj, n_last, 0, 0, 0, h->stream);
    double* dbg = h->prop_capture ? h->d_prop_w : nullptr;
    HIP_TRY(h, hipEventRecord(h->ev_fork, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->side, h->ev_fork, 0));
    match_stage(h, adj, n_last, 1, 0, n0, h->side, nullptr, ndt || !n1 ? nullptr : h->ev_half_match);
    if (ndt) match_stage(h, adj, n_last, 2, 0, n0, h->side, nullptr, n1 ? h->ev_half_match : nullptr);
    launch_propose_weight(v, h->d_match, match_of, d_g, h->d_bad, h->cfg.seed, (uint32_t)h->scan_updates, dbg, 0, n0, h->side, h->ev_half_weight);
    HIP_TRY(h, hipGetLastError());
    if (n1) {
        match_stage(h, adj, n_last, 1, n0, n1, h->stream);
        if (ndt) match_stage(h, adj, n_last, 2, n0, n1, h->stream);
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_half_match, 0));
        launch_propose_weight(v, h->d_match, match_of, d_g, h->d_bad, h->cfg.seed, (uint32_t)h->scan_updates, dbg, n0, n1, h->stream);
    }
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_half_weight, 0));
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}

// ---- Robot.map_update for every particle (robot.py:59-115) -------------------------------------------------
int rbpf_scan_update(rbpf_handle* h, int32_t adj, const double* last_scan_xy, int32_t n_last,
                     const double* match_override, const double* guesses) {
    int rc = rbpf_scan_update_begin(h, adj, last_scan_xy, n_last, match_override, guesses);
    if (rc || !h->map_updates || !h->hold_back) return rc ? rc : rbpf_scan_update_end(h);
    // The second half waits for the next call.  The weights are final here (but for the NaN branch), and they decide whom a
    // resample that follows discards: that call launches the map update behind its plan, without those particles; any other
    // call launches it whole before it does anything else (ON_DEVICE).  What the host alone keeps of the step changes now.
    h->scan_begun = false;
    h->scan_updates++;
    h->mu_pending = true; h->mu_pending_rec = -1;
    if (h->track_on && (h->track_flags & RBPF_TRACK_SCAN)) return track_take_place(h, true, h->mu_pending_rec);
    return RBPF_OK;
}

// first half: scan matcher, proposal, weighting, moments (robot.py:62-114); the weights are final here unless a
// particle took the NaN branch
int rbpf_scan_update_begin(rbpf_handle* h, int32_t adj, const double* last_scan_xy, int32_t n_last,
                           const double* match_override, const double* guesses) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->have_scan) return fail(h, RBPF_ESTATE, "rbpf_set_scan has not been called");
    DevView& v = h->v;
    const size_t P = v.P;
    if (match_override) {
        h->match_rows = 0;
        HIP_TRY(h, hipMemcpyAsync(h->d_match, match_override, 13 * P * 8, hipMemcpyHostToDevice, h->stream));
    } else {
        const int rc = stage_last_scan(h, adj, last_scan_xy, n_last);
        if (rc) return rc;
        h->match_rows = v.dups_valid ? 2 : 1;
    }
    const double* d_g = nullptr;
    if (guesses) {
        HIP_TRY(h, hipMemcpyAsync(h->d_guess_full, guesses, P * (size_t)v.K * 3 * 8, hipMemcpyHostToDevice, h->stream));
        d_g = h->d_guess_full;
    }
    // the matcher ran once per group of exact duplicates (copies made by the last resample, untouched since): every
    // member reads its representative's row; the proposal below is what makes the copies differ, so the groups end here
    const int32_t* match_of = (!match_override && v.dups_valid) ? v.dup_of : nullptr;
    if (h->prop_capture && !h->d_prop_w) ALLOC(h, h->d_prop_w, P * (size_t)v.K);
    if (!match_override && h->halves_now()) {
        const int rc = run_front_halves(h, adj, n_last, match_of, d_g);
        if (rc) return rc;
    } else {
        if (!match_override) { const int rc = run_matcher(h, adj, n_last); if (rc) return rc; }
        if (!match_override && !guesses) h->prof_begin_chained(1); else h->prof_begin(1);     // right after the matcher's last kernel
        launch_propose_weight(v, h->d_match, match_of, d_g, h->d_bad, h->cfg.seed, (uint32_t)h->scan_updates, h->prop_capture ? h->d_prop_w : nullptr, 0, v.P, h->stream);
        h->prof_end(1);
    }
    h->prop_valid = true; h->prop_captured = h->prop_capture;
    v.dups_valid = 0;
    HIP_TRY(h, hipGetLastError());
    // the event orders an early weight export on ANOTHER stream behind the weighting; recorded only once such a caller exists
    h->ev_weights_valid = false;
    if (h->record_ev_weights) { HIP_TRY(h, hipEventRecord(h->ev_weights, h->stream)); h->ev_weights_valid = true; }
    h->scan_begun = true; h->begin_seen = true;
    return RBPF_OK;
}

// second half: the map update at the new mean pose and the NaN-covariance branch (robot.py:115, 73-78)
int rbpf_scan_update_end(rbpf_handle* h) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->scan_begun) return fail(h, RBPF_ESTATE, "rbpf_scan_update_begin has not been called");
    h->scan_begun = false;
    if (!h->map_updates) {
        // localization: the maps stay as they are; the NaN-branch increment (robot.py:73-78) on the unchanged map.  The
        // step still counts: scan_updates is the Philox stream of the next proposal
        launch_bad_weight(h->v, h->d_bad, h->stream);
        HIP_TRY(h, hipGetLastError());
        h->scan_updates++;
    } else {
        // HybridMap.update at the new mean pose (robot.py:115), then - in the same launch - the robot.py:73-78 weight
        // increment of the particles on the NaN-covariance branch, on their updated maps
        const int rc = run_map_update(h, h->v, h->d_bad);
        if (rc) return rc;
        h->scan_updates++;
    }
    if (h->track_on && (h->track_flags & RBPF_TRACK_SCAN)) return track_record(h, true);
    return RBPF_OK;
}

// ---- read-out of the last proposal (tests): the frame propose_prep_kernel left, the samples of propose_samples_kernel,
//      the raw weights of propose_weight_kernel (ProposeArgs::dbg_w) ------------------------------------------------------
int rbpf_set_proposal_capture(rbpf_handle* h, int32_t on) {
    if (!h) return RBPF_EINVAL;
    h->prop_capture = on != 0;
    return RBPF_OK;
}

int rbpf_get_proposal(rbpf_handle* h, int32_t particle, double* frame24, double* samples, float* frame_f32, double* raw_w) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (particle < 0 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle out of range");
    if (!h->prop_valid) return fail(h, RBPF_ESTATE, "no scan update has run yet");
    if (raw_w && !h->prop_captured) return fail(h, RBPF_ESTATE, "the last scan update ran without rbpf_set_proposal_capture");
    const int K = v.K;
    double prep[24], samp[256];                          // PREP_W, SAMP_W of kernels_propose.hip
    std::vector<double> w((size_t)K);
    HIP_TRY(h, hipMemcpyAsync(prep, v.prop_prep + (size_t)particle * 24, sizeof(prep), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(samp, v.prop_samp + (size_t)particle * 256, sizeof(samp), hipMemcpyDeviceToHost, h->stream));
    if (raw_w) HIP_TRY(h, hipMemcpyAsync(w.data(), h->d_prop_w + (size_t)particle * K, (size_t)K * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (frame24) memcpy(frame24, prep, sizeof(prep));
    for (int k = 0; k < K; ++k) {
        if (samples) {
            double* o = samples + 6 * k;
            o[0] = samp[64 + k]; o[1] = samp[96 + k]; o[2] = samp[128 + k]; o[3] = samp[k]; o[4] = samp[32 + k]; o[5] = samp[160 + k];
        }
        if (frame_f32) memcpy(frame_f32 + 4 * k, reinterpret_cast<const unsigned char*>(samp + 192) + 16 * k, 16);
        if (raw_w) raw_w[k] = w[k];
    }
    return RBPF_OK;
}

int rbpf_set_map_updates(rbpf_handle* h, int32_t on) {
    if (!h) return RBPF_EINVAL;
    h->map_updates = on != 0;
    return RBPF_OK;
}

int rbpf_get_map_update_workgroups(rbpf_handle* h, int32_t* n) {
    if (!h || !n) return RBPF_EINVAL;
    ON_DEVICE(h);                                   // (the number is known once the update is launched: a held-back one is, here)
    *n = h->ev_workgroups;
    return RBPF_OK;
}

int rbpf_get_map_updates(rbpf_handle* h, int32_t* on) {
    if (!h || !on) return RBPF_EINVAL;
    *on = h->map_updates ? 1 : 0;
    return RBPF_OK;
}

// matchScanCustom(curr, ref, guess, cells_per_m, pose_range) -> pose, cov, score  (hybridmap.py:244-251)
int rbpf_match_scan(rbpf_handle* h, const double* curr_xy, int32_t n_curr, const double* ref_xy, int32_t n_ref,
                    const double* guess3, int32_t cells_per_m, const double* pose_range3, double* pose_out3,
                    double* cov_out9, double* score_out) {
    if (!h || !curr_xy || !guess3 || !pose_range3 || !pose_out3 || !cov_out9 || !score_out) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (n_curr < 0 || n_curr > h->cfg.max_beams || n_ref < 0 || (n_ref > 0 && !ref_xy)) return fail(h, RBPF_EINVAL, "point counts out of range");
    if (cells_per_m < 1) return fail(h, RBPF_EINVAL, "cells_per_m must be >= 1");
    rbpf_config c = h->cfg;
    c.match_max_range = 15.0;                       // matchScanCustom.m:11 'MaxRange', 15
    int N, ds, ncr; double mcs, d0;
    match_geometry(c, 1.0 / (double)cells_per_m, N, ds, mcs, d0, ncr);
    ncr = (int)floor(fabs(pose_range3[2]) / (4 * d0));             // coarse rotation step = 4 * d0
    if (ncr * 4 * d0 >= fabs(pose_range3[2])) --ncr;
    if (ncr < 0) ncr = 0;
    size_t lds = match_lds_bytes(N, h->cfg.max_beams, match_max_coarse(ncr, std::max(pose_range3[0], pose_range3[1]), mcs),
                                 match_per_rot(std::max(pose_range3[0], pose_range3[1]), mcs));
    if (lds > LDS_LIMIT) return fail(h, RBPF_EINVAL, "matcher region does not fit in LDS for this resolution");
    std::vector<float> sel(2 * (size_t)h->cfg.max_beams, 0.f);
    for (int i = 0; i < n_curr; ++i) { sel[i] = (float)curr_xy[2 * i]; sel[h->cfg.max_beams + i] = (float)curr_xy[2 * i + 1]; }
    DevTemp d_ref, d_out, d_occ, d_aux;
    HIP_TRY(h, d_ref.reserve((size_t)n_ref * 16));
    HIP_TRY(h, d_out.reserve(13 * 8));
    if (c.ndt_refine && ndt_cells(mcs) >= 2 && ndt_lds_bytes(N, h->cfg.max_beams) <= LDS_LIMIT) {
        HIP_TRY(h, d_occ.reserve((size_t)N * (N / 32) * 4));
        HIP_TRY(h, d_aux.reserve(5 * 8));
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_tmp_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (n_ref) HIP_TRY(h, hipMemcpyAsync(d_ref.p, ref_xy, (size_t)n_ref * 16, hipMemcpyHostToDevice, h->stream));
    launch_match_single(h->v, d_ref.as<double>(), n_ref, guess3, pose_range3, h->d_tmp_sel, h->d_tmp_sel + h->cfg.max_beams, n_curr,
                        d_out.as<double>(), N, ds, mcs, d0, ncr, h->cfg.max_beams, lds, d_occ.as<uint32_t>(), d_aux.as<double>(), h->stream);
    double out[13];
    HIP_TRY(h, hipMemcpyAsync(out, d_out.p, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    int rc = check_device_error(h);
    if (rc) return rc;
    // matchScanCustom.m:19,52-57 validity gate
    const double PI = 3.141592653589793;
    double dth = fmod(out[2] - guess3[2] + PI, 2 * PI); if (dth < 0) dth += 2 * PI; dth -= PI;
    bool valid = fabs(out[0] - guess3[0]) < fabs(pose_range3[0]) && fabs(out[1] - guess3[1]) < fabs(pose_range3[1]) &&
                 fabs(dth) < fabs(pose_range3[2]) && !(out[3] != out[3]);
    for (int i = 0; i < 3; ++i) pose_out3[i] = out[i];
    for (int i = 0; i < 9; ++i) cov_out9[i] = valid ? out[3 + i] : std::numeric_limits<double>::quiet_NaN();
    *score_out = valid ? out[12] : 0.0;
    return RBPF_OK;
}
// HybridMap.get_scan_match up to the engine call (hybridmap.py:210-242) for one particle: the curr / ref point lists
int rbpf_match_inputs(rbpf_handle* h, int32_t particle, const double* guess3, double* curr_xy, int32_t* n_curr,
                      double* ref_xy, int32_t* n_ref, int32_t cap_ref) {
    if (!h || !guess3 || !curr_xy || !n_curr || !ref_xy || !n_ref || cap_ref < 0) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->have_scan) return fail(h, RBPF_ESTATE, "rbpf_set_scan has not been called");
    DevView& v = h->v;
    if (particle < 0 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    const size_t LL = (size_t)v.L * v.L, mask_words = LL * v.dim * v.ow, n_rows = (size_t)v.L * v.dim;
    DevTemp d_all, d_ref, d_curr, d_counts, d_mask, d_rows;
    HIP_TRY(h, d_all.reserve((size_t)v.B * 16)); HIP_TRY(h, d_curr.reserve((size_t)v.B * 16));
    HIP_TRY(h, d_ref.reserve((size_t)cap_ref * 16)); HIP_TRY(h, d_counts.reserve(16));
    HIP_TRY(h, d_mask.reserve(mask_words * 4)); HIP_TRY(h, d_rows.reserve(n_rows * 4));
    HIP_TRY(h, hipMemsetAsync(d_mask.p, 0, mask_words * 4, h->stream));
    HIP_TRY(h, hipMemsetAsync(d_counts.p, 0, 16, h->stream));
    const int win = (int)(1.8 / h->cfg.cell_size);                 // gridmap.py:143
    launch_match_inputs(v, particle, guess3, d_all.as<double>(), d_counts.as<int>(), d_mask.as<uint32_t>(), d_rows.as<int>(),
                        d_ref.as<double>(), cap_ref, d_curr.as<double>(), win, h->cfg.match_max_range, h->stream);
    int counts[3] = {0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(counts, d_counts.p, 12, hipMemcpyDeviceToHost, h->stream));
    int rc = check_device_error(h);
    if (rc == RBPF_OK) {
        *n_curr = counts[1]; *n_ref = counts[2];
        if (counts[1] > 0) HIP_TRY(h, hipMemcpy(curr_xy, d_curr.p, (size_t)counts[1] * 16, hipMemcpyDeviceToHost));
        int nr = std::min(counts[2], cap_ref);
        if (nr > 0) HIP_TRY(h, hipMemcpy(ref_xy, d_ref.p, (size_t)nr * 16, hipMemcpyDeviceToHost));
    }
    return rc;
}

// the rows the last built-in matcher wrote (pose, covariance, score per particle); a duplicate the matcher skipped gets its
// representative's row, the one the proposal read
int rbpf_match_results(rbpf_handle* h, double* out) {
    if (!h || !out) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (h->match_rows == 0) return fail(h, RBPF_ESTATE, "no built-in match since the last match_override / resample");
    const int P = h->v.P;
    std::vector<int32_t> dup(P);
    if (h->match_rows == 2) HIP_TRY(h, hipMemcpyAsync(dup.data(), h->v.dup_of, (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out, h->d_match, (size_t)P * 13 * 8, hipMemcpyDeviceToHost, h->stream));
    int rc = check_device_error(h);
    if (rc) return rc;
    if (h->match_rows == 2)
        for (int p = 0; p < P; ++p) if (dup[p] != p) memcpy(out + (size_t)p * 13, out + (size_t)dup[p] * 13, 13 * 8);
    return RBPF_OK;
}

// __sincosf on the device, as the grid stage of the matcher evaluates it
int rbpf_native_sincosf(rbpf_handle* h, const float* x, int32_t n, float* s, float* c) {
    if (!h || n < 0 || (n > 0 && (!x || !s || !c))) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (n == 0) return RBPF_OK;
    DevTemp tmp;
    HIP_TRY(h, tmp.reserve((size_t)n * 12));
    float* d = tmp.as<float>();
    HIP_TRY(h, hipMemcpyAsync(d, x, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    launch_native_sincosf(d, n, d + n, d + 2 * (size_t)n, h->stream);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(s, d + n, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(c, d + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    return check_device_error(h);
}

// ---- resample (main.py:46-79) -------------------------------------------------------------------------------
static double internal_uniform(rbpf_handle* h) {
    uint64_t z = h->cfg.seed + 0x9E3779B97F4A7C15ull * (++h->resample_draws);   // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

static void swap_state_buffers(rbpf_handle* h) {
    DevView& v = h->v; ResampleBuffers& r = h->rs;
    std::swap(v.px, r.px2); std::swap(v.py, r.py2); std::swap(v.pth, r.pth2);
    std::swap(v.cov, r.cov2); std::swap(v.weight, r.w2); std::swap(v.slot, r.slot2);
}

// the local resample of rbpf_resample (from the weights d_w) and rbpf_apply_resample_local (d_w == nullptr: from the
// sources in rs.idx), timed; the permuted state becomes current and the kernels wrote the groups of exact duplicates
// (identity if nothing was resampled; arrivals are their own representatives)
static int resample_local(rbpf_handle* h, const double* d_w, double u, double spread) {
    DevView& v = h->v;
    if (h->mu_pending) {
        // (rbpf_resample behind rbpf_scan_update) the plan, the held-back map update without the particles the plan discards, the
        // plan once more - it returns at once unless a particle on the NaN branch made the first one wait -, copies and release.
        // The update runs on the view from before the swap, with the three pointers that name the particles it leaves out.
        h->prof_begin(2);
        launch_resample_plan_early(v, h->rs, h->d_bad, h->skip_discarded ? 1 : 0, u, spread, h->stream);
        h->prof_pause(2);
        HIP_TRY(h, hipGetLastError());
        DevView mv = v;
        mv.mu_skip = h->rs.skip; mv.mu_keep = h->rs.keep; mv.mu_n_keep = h->rs.plan;
        const int rc = launch_held_map_update(h, mv);
        if (rc) return rc;
        h->prof_resume(2);
        launch_resample_plan_late(v, h->rs, u, spread, h->stream);
        launch_resample_copies(v, h->rs, h->stream);
        h->prof_end(2);
    } else {
        h->prof_begin(2);
        launch_resample_local(v, h->rs, d_w, u, spread, h->stream);
        h->prof_end(2);
    }
    HIP_TRY(h, hipGetLastError());
    swap_state_buffers(h);
    if (h->track_on) {                              // pending' = pending o ancestors where the device's flag says a resample happened
        launch_track_compose(v.P, h->rs.did, h->rs.idx, h->track_pending(h->track_cur), h->track_pending(h->track_cur ^ 1), h->stream);
        HIP_TRY(h, hipGetLastError());
        h->track_cur ^= 1;
    }
    v.dups_valid = h->dedup_enabled ? 1 : 0;
    if (h->match_rows == 2) h->match_rows = 0;      // the duplicate groups the matcher skipped are overwritten
    return RBPF_OK;
}

int rbpf_resample(rbpf_handle* h, double u, int32_t* idx_out, int32_t* did_resample) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE_HELD(h);                                  // a held-back map update goes between this call's own launches (resample_local)
    DevView& v = h->v;
    if (u != u) u = internal_uniform(h);
    if (!(u >= 0.0 && u < 1.0)) {
        const int rc = flush_map_update(h);
        return rc ? rc : fail(h, RBPF_EINVAL, "u must lie in [0, 1)");
    }
    int rc = resample_local(h, v.weight, u, h->cfg.resample_spread);
    if (rc) return rc;
    if (idx_out) HIP_TRY(h, hipMemcpyAsync(idx_out, h->rs.idx, (size_t)v.P * 4, hipMemcpyDeviceToHost, h->stream));
    if (did_resample) HIP_TRY(h, hipMemcpyAsync(did_resample, h->rs.did, 4, hipMemcpyDeviceToHost, h->stream));
    if (idx_out || did_resample) return check_device_error(h);
    return RBPF_OK;
}

// ---- multi-GPU pieces: one handle per rank, the collectives are the caller's (RCCL) ---------------------------------
int rbpf_set_global_ids(rbpf_handle* h, const int32_t* ids) {
    if (!h || !ids) return RBPF_EINVAL;
    ON_DEVICE(h);
    HIP_TRY(h, hipMemcpyAsync(h->v.global_id, ids, (size_t)h->v.P * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

int rbpf_export_weights(rbpf_handle* h, void* d_global, int32_t n_global) {
    if (!h || !d_global || n_global < h->v.P) return RBPF_EINVAL;
    ON_DEVICE(h);
    launch_export_weights(h->v, static_cast<double*>(d_global), n_global, nullptr, h->stream);
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;                                     // stream-ordered: see the header about collectives on other streams
}

int rbpf_export_weights_early(rbpf_handle* h, void* d_global, int32_t n_global, void* aux_stream) {
    if (!h || !d_global || n_global < h->v.P) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->begin_seen) return fail(h, RBPF_ESTATE, "rbpf_scan_update_begin has not been called");
    hipStream_t s = static_cast<hipStream_t>(aux_stream);
    if (s != h->stream) {                                 // same stream: stream order is the ordering
        if (!h->ev_weights_valid) {                       // first such call: order behind everything queued so far, record in time from now on
            HIP_TRY(h, hipEventRecord(h->ev_weights, h->stream));
            h->ev_weights_valid = true; h->record_ev_weights = true;
        }
        HIP_TRY(h, hipStreamWaitEvent(s, h->ev_weights, 0));
    }
    launch_export_weights(h->v, static_cast<double*>(d_global), n_global, h->d_bad, s);
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}

// queue the global ancestors of the n_global weights d_global (main.py:46-67) into B_GIDX on stream s; did -> d_did
static int queue_indices_global(rbpf_handle* h, const void* d_global, int32_t n_global, double u, int32_t* d_did, hipStream_t s) {
    if (!(u >= 0.0 && u < 1.0)) return fail(h, RBPF_EINVAL, "u must lie in [0, 1)");
    HIP_TRY(h, h->reserve(B_GT, (size_t)n_global * 4));
    HIP_TRY(h, h->reserve(B_GIDX, (size_t)n_global * 4));
    launch_resample_indices(n_global, static_cast<const double*>(d_global), u, h->cfg.resample_spread, h->buf[B_GT].as<int32_t>(),
                            h->buf[B_GIDX].as<int32_t>(), d_did, h->v.err, s);
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}

int rbpf_resample_indices_global_early(rbpf_handle* h, const void* d_global, int32_t n_global, double u, void* aux_stream) {
    if (!h || !d_global || n_global < 1) return RBPF_EINVAL;
    ON_DEVICE(h);
    hipStream_t s = static_cast<hipStream_t>(aux_stream);
    // the landing zone of the read-back: a kernel writes it through its device address, the host reads it after the
    // staging's event, which is created WITHOUT hipEventDisableSystemFence and so releases at system scope: plain pinned
    // memory is enough
    Staging& land = h->stage[S_EARLY];
    HIP_TRY(h, land.reserve((size_t)n_global * 4 + 16));
    int rc = queue_indices_global(h, d_global, n_global, u, h->d_did_early, s);
    if (rc) return rc;
    const int32_t* d_gidx = h->buf[B_GIDX].as<int32_t>();
    if (void* mapped = land.mapped()) {                  // one kernel writes the landing zone directly
        launch_readback(mapped, static_cast<const double*>(d_global) + n_global, h->d_did_early, d_gidx, n_global, s);
    } else {
        HIP_TRY(h, hipMemcpyAsync(land.p, static_cast<const double*>(d_global) + n_global, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(land.p + 8, h->d_did_early, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(land.p + 16, d_gidx, (size_t)n_global * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, land.submitted(s));
    h->early_n = n_global;
    return RBPF_OK;                                      // nothing waited for: what is queued behind it keeps the GPU busy
}

int rbpf_resample_indices_global_wait(rbpf_handle* h, int32_t* idx_out, int32_t* did_resample, double* nan_branch_ranks) {
    if (!h || !idx_out || !did_resample || !nan_branch_ranks) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (h->early_n <= 0) return fail(h, RBPF_ESTATE, "rbpf_resample_indices_global_early has not been called");
    HIP_TRY(h, h->stage[S_EARLY].wait());                // only up to the read-back, not the work queued after it
    const unsigned char* src = h->stage[S_EARLY].p;
    memcpy(nan_branch_ranks, src, 8);
    memcpy(did_resample, src + 8, 4);
    memcpy(idx_out, src + 16, (size_t)h->early_n * 4);
    h->early_n = 0;
    return RBPF_OK;
}

int rbpf_resample_indices_global(rbpf_handle* h, const void* d_global, int32_t n_global, double u, int32_t* idx_out,
                                 int32_t* did_resample) {
    if (!h || !d_global || !idx_out || !did_resample || n_global < 1) return RBPF_EINVAL;
    ON_DEVICE(h);
    int rc = queue_indices_global(h, d_global, n_global, u, h->rs.did, h->stream);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(idx_out, h->buf[B_GIDX].p, (size_t)n_global * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(did_resample, h->rs.did, 4, hipMemcpyDeviceToHost, h->stream));
    return check_device_error(h);
}

int rbpf_apply_resample_local(rbpf_handle* h, const int32_t* new_src, const int32_t* new_global_id) {
    if (!h || !new_src || !new_global_id) return RBPF_EINVAL;
    ON_DEVICE(h);
    DevView& v = h->v;
    if (h->track_on) return fail(h, RBPF_ESTATE, "the trajectory log does not follow lineages across ranks: rbpf_track_end first");
    // sources must be sorted ascending with the arrivals (-1) last: duplicates of one ancestor are then adjacent
    for (int j = 1; j < v.P; ++j) {
        bool ok = new_src[j] < 0 ? true : (new_src[j - 1] >= 0 && new_src[j - 1] <= new_src[j]);
        if (!ok) return fail(h, RBPF_EINVAL, "new_src must be sorted ascending with -1 entries last");
    }
    for (int j = 0; j < v.P; ++j) if (new_src[j] >= v.P) return fail(h, RBPF_EINVAL, "new_src out of range");
    int32_t* slot = static_cast<int32_t*>(h->rings[R_IDX].acquire());   // pinned: the caller's arrays are free on return
    memcpy(slot, new_src, (size_t)v.P * 4);
    memcpy(slot + v.P, new_global_id, (size_t)v.P * 4);
    // both index vectors go over in one kernel from the pinned, device-mapped slot (nothing below reads global_id:
    // only the weight export does, after this call)
    const int32_t* mapped = static_cast<const int32_t*>(h->rings[R_IDX].mapped());
    if (mapped) launch_ingest2(mapped, h->rs.idx, mapped + v.P, v.global_id, v.P, h->stream);
    else HIP_TRY(h, hipMemcpyAsync(h->rs.idx, slot, (size_t)v.P * 4, hipMemcpyHostToDevice, h->stream));
    int rc = resample_local(h, nullptr, 0.0, 0.0);
    if (rc) return rc;
    if (!mapped) HIP_TRY(h, hipMemcpyAsync(v.global_id, slot + v.P, (size_t)v.P * 4, hipMemcpyHostToDevice, h->stream));
    h->rings[R_IDX].submitted(h->stream);
    return RBPF_OK;                                     // no host synchronisation; device errors surface at the next check
}

// meta record of one particle: [0] tiles, [1] payload bytes / 16, then per lattice position (has, x0, x1, y0, y1, offset / 16):
// the written box itself, inclusive, which the receiver stores as it is; a held tile nothing was written to is
// (1, 0, -1, 0, -1, offset) and takes no bytes.  The payload holds the columns [ya, yb) of the rows x0..x1, ya = y0 & ~15,
// yb = min((y1 | 15) + 1, dim) - both sides derive them from y0, y1 -, then the rows' occupancy words, padded to 16 bytes.
// layout_packed (sizes, offsets, pack jobs) and unpack_kernel each compute ya, yb: the two derivations must stay identical, or the
// receiver reads other bytes than the sender wrote (tests/test_gpu_migrate.py holds both to the model's byte total).
int32_t rbpf_pack_meta_width(rbpf_handle* h) { return h ? 2 + 6 * h->v.L * h->v.L : -1; }

// job lists of the pack / unpack kernels go through one pinned buffer (S_JOBS -> B_JOBS): the copy is asynchronous and the
// std::vector may die on return; the staging's event tells when the buffer may be overwritten
static int stage_jobs(rbpf_handle* h, const void* src, size_t bytes) {
    Staging& st = h->stage[S_JOBS];
    HIP_TRY(h, st.begin(bytes));
    memcpy(st.p, src, bytes);
    HIP_TRY(h, h->reserve(B_JOBS, bytes));
    HIP_TRY(h, st.upload(h->buf[B_JOBS].p, bytes, h->stream));
    return RBPF_OK;
}

// Layout of n packed particles from their gathered tile boxes (g: per particle and lattice position 5 ints: tile index or
// -1, x0, x1, y0, y1 - the output of gather_meta_kernel).  Fills the receiver's meta rows (optional) and, for the sender
// (local_idx given), the pack jobs.  Returns the total payload bytes.  Host only.
static int64_t layout_packed(const DevView& v, const int32_t* g, int n, const int32_t* local_idx, int32_t* meta_out,
                             std::vector<PackJobHost>* jobs) {
    const int LL = v.L * v.L, W = 2 + 6 * LL;
    int64_t off = 0;
    for (int i = 0; i < n; ++i) {
        int32_t* m = meta_out ? meta_out + (size_t)i * W : nullptr;
        const int64_t start = off;
        if (jobs) jobs->push_back({local_idx[i], -1, 0, 0, 0, 0, (long long)off});
        off += 128;
        int nt = 0;
        for (int pos = 0; pos < LL; ++pos) {
            const int32_t* e = &g[((size_t)i * LL + pos) * 5];
            int32_t z[6] = {0, 0, 0, 0, 0, 0};
            int32_t* mm = m ? m + 2 + 6 * pos : z;
            mm[0] = mm[1] = mm[2] = mm[3] = mm[4] = mm[5] = 0;
            if (e[0] < 0) continue;
            ++nt;
            mm[0] = 1;
            int x0 = e[1], x1 = e[2], y0 = e[3], y1 = e[4];
            if (x0 > x1 || y0 > y1) { mm[1] = 0; mm[2] = -1; mm[3] = 0; mm[4] = -1; mm[5] = (int32_t)((off - start) / 16); continue; }   // empty tile
            int ya = y0 & ~15, yb = std::min((y1 | 15) + 1, v.dim);
            mm[1] = x0; mm[2] = x1; mm[3] = y0; mm[4] = y1; mm[5] = (int32_t)((off - start) / 16);
            if (jobs) jobs->push_back({local_idx[i], e[0], x0, x1, ya, yb, (long long)off});
            int64_t bytes = (int64_t)(x1 - x0 + 1) * (yb - ya) + (int64_t)(x1 - x0 + 1) * v.ow * 4;
            off += (bytes + 15) & ~(int64_t)15;
        }
        if (m) { m[0] = nt; m[1] = (int32_t)((off - start) / 16); }
    }
    return off;
}

// ---- the pack in three steps, with one host wait for a whole migration (thesis_amd/sharding.py) --------------------
// 1. rbpf_gather_pack_meta: the tile boxes of the departing particles, gathered into a device buffer (nothing waited
//    for) - the ranks exchange these records while they are still on the device and read their own and the incoming
//    ones back together;  2. rbpf_meta_from_raw: records -> the layout rows rbpf_unpack_particles takes (host only);
// 3. rbpf_pack_particles_raw: packs with the records already on the host (nothing waited for).
int32_t rbpf_pack_raw_width(rbpf_handle* h) { return h ? 5 * h->v.L * h->v.L : -1; }

int rbpf_gather_pack_meta(rbpf_handle* h, const int32_t* local_idx, int32_t n, void* d_raw) {
    if (!h || n < 0 || (n > 0 && (!local_idx || !d_raw))) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (n == 0) return RBPF_OK;
    DevView& v = h->v;
    if (n > v.P) return fail(h, RBPF_EINVAL, "more departing particles than particles");
    for (int i = 0; i < n; ++i) if (local_idx[i] < 0 || local_idx[i] >= v.P) return fail(h, RBPF_EINVAL, "local index out of range");
    HIP_TRY(h, h->reserve(B_I32, ((size_t)v.P + 4) * 4));
    int32_t* d_idx = h->buf[B_I32].as<int32_t>();
    memcpy(h->rings[R_IDX].acquire(), local_idx, (size_t)n * 4);           // pinned: the caller's array is free on return
    HIP_TRY(h, h->rings[R_IDX].upload(d_idx, (size_t)n * 4, h->stream));
    launch_gather_meta(v, d_idx, n, static_cast<int32_t*>(d_raw), h->stream);
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}

int rbpf_meta_from_raw(rbpf_handle* h, const int32_t* raw, int32_t n, int32_t* meta_out, int64_t* bytes_out) {
    if (!h || n < 0 || !bytes_out || (n > 0 && (!raw || !meta_out))) return RBPF_EINVAL;
    *bytes_out = n ? layout_packed(h->v, raw, n, nullptr, meta_out, nullptr) : 0;
    return RBPF_OK;
}

int rbpf_pack_particles_raw(rbpf_handle* h, const int32_t* local_idx, int32_t n, const int32_t* raw, void* d_buf,
                            int64_t cap_bytes, int64_t* bytes_out) {
    if (!h || n < 0 || !bytes_out || (n > 0 && (!local_idx || !raw || !d_buf))) return RBPF_EINVAL;
    ON_DEVICE(h);
    *bytes_out = 0;
    if (n == 0) return RBPF_OK;
    DevView& v = h->v;
    for (int i = 0; i < n; ++i) if (local_idx[i] < 0 || local_idx[i] >= v.P) return fail(h, RBPF_EINVAL, "local index out of range");
    std::vector<PackJobHost> jobs;
    const int64_t off = layout_packed(v, raw, n, local_idx, nullptr, &jobs);
    if (off > cap_bytes) return fail(h, RBPF_ENOMEM, "pack buffer too small");
    int rc = stage_jobs(h, jobs.data(), jobs.size() * sizeof(PackJobHost));
    if (rc) return rc;
    launch_pack(v, h->buf[B_JOBS].p, (int)jobs.size(), d_buf, h->stream);
    HIP_TRY(h, hipGetLastError());
    *bytes_out = off;
    return RBPF_OK;
}

// installs n received particles at the given local indices (after rbpf_apply_resample_local); weight <- 1.0 (main.py:77-78)
int rbpf_unpack_particles(rbpf_handle* h, const int32_t* local_idx, int32_t n, const void* d_buf, const int32_t* meta_in) {
    if (!h || n < 0 || (n > 0 && (!local_idx || !d_buf || !meta_in))) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (h->track_on) return fail(h, RBPF_ESTATE, "the trajectory log does not follow lineages across ranks: rbpf_track_end first");
    if (n == 0) return RBPF_OK;
    DevView& v = h->v;
    const int LL = v.L * v.L, W = 2 + 6 * LL;
    std::vector<UnpackJobHost> jobs;
    int64_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (local_idx[i] < 0 || local_idx[i] >= v.P) return fail(h, RBPF_EINVAL, "local index out of range");
        const int32_t* m = meta_in + (size_t)i * W;
        jobs.push_back({local_idx[i], -1, 1, 0, 0, 0, 0, 0, (long long)off});
        for (int pos = 0; pos < LL; ++pos) {
            const int32_t* mm = m + 2 + 6 * pos;
            jobs.push_back({local_idx[i], pos, mm[0], mm[1], mm[2], mm[3], mm[4], 0, (long long)(off + (int64_t)mm[5] * 16)});
        }
        off += (int64_t)m[1] * 16;
    }
    int rc = stage_jobs(h, jobs.data(), jobs.size() * sizeof(UnpackJobHost));
    if (rc) return rc;
    launch_unpack(v, h->rs, h->buf[B_JOBS].p, (int)jobs.size(), d_buf, h->stream);
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;                                     // no host synchronisation; device errors surface at the next check
}

// ---- state access -----------------------------------------------------------------------------------------
int rbpf_get_poses(rbpf_handle* h, double* out) {
    if (!h || !out) return RBPF_EINVAL;
    ON_DEVICE(h);
    const size_t P = h->v.P;
    std::vector<double> t(3 * P);
    HIP_TRY(h, hipMemcpyAsync(t.data(), h->v.px, P * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(t.data() + P, h->v.py, P * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(t.data() + 2 * P, h->v.pth, P * 8, hipMemcpyDeviceToHost, h->stream));
    int rc = check_device_error(h);
    for (size_t p = 0; p < P; ++p) { out[3 * p] = t[p]; out[3 * p + 1] = t[P + p]; out[3 * p + 2] = t[2 * P + p]; }
    return rc;
}

int rbpf_get_covs(rbpf_handle* h, double* out) {
    if (!h || !out) return RBPF_EINVAL;
    ON_DEVICE(h);
    const size_t P = h->v.P;
    std::vector<double> t(9 * P);
    HIP_TRY(h, hipMemcpyAsync(t.data(), h->v.cov, 9 * P * 8, hipMemcpyDeviceToHost, h->stream));
    int rc = check_device_error(h);
    for (size_t p = 0; p < P; ++p) for (int k = 0; k < 9; ++k) out[9 * p + k] = t[(size_t)k * P + p];
    return rc;
}

int rbpf_get_weights(rbpf_handle* h, double* out) {
    if (!h || !out) return RBPF_EINVAL;
    ON_DEVICE(h);
    HIP_TRY(h, hipMemcpyAsync(out, h->v.weight, (size_t)h->v.P * 8, hipMemcpyDeviceToHost, h->stream));
    return check_device_error(h);
}

int rbpf_set_state(rbpf_handle* h, const double* poses, const double* covs, const double* weights) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    h->v.dups_valid = 0;
    const size_t P = h->v.P;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (poses) {
        std::vector<double> t(3 * P);
        for (size_t p = 0; p < P; ++p) { t[p] = poses[3 * p]; t[P + p] = poses[3 * p + 1]; t[2 * P + p] = poses[3 * p + 2]; }
        HIP_TRY(h, hipMemcpy(h->v.px, t.data(), P * 8, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->v.py, t.data() + P, P * 8, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->v.pth, t.data() + 2 * P, P * 8, hipMemcpyHostToDevice));
    }
    if (covs) {
        std::vector<double> t(9 * P);
        for (size_t p = 0; p < P; ++p) for (int k = 0; k < 9; ++k) t[(size_t)k * P + p] = covs[9 * p + k];
        HIP_TRY(h, hipMemcpy(h->v.cov, t.data(), 9 * P * 8, hipMemcpyHostToDevice));
    }
    if (weights) HIP_TRY(h, hipMemcpy(h->v.weight, weights, P * 8, hipMemcpyHostToDevice));
    return RBPF_OK;
}

int rbpf_get_dim(rbpf_handle* h, int32_t* out) {
    if (!h || !out) return RBPF_EINVAL;
    *out = h->v.dim;
    return RBPF_OK;
}

static int fetch_tab(rbpf_handle* h, int32_t particle, std::vector<int32_t>& tab) {
    if (particle < 0 || particle >= h->v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    const size_t LL = (size_t)h->v.L * h->v.L;
    int32_t slot = 0;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(&slot, h->v.slot + particle, 4, hipMemcpyDeviceToHost));
    tab.resize(LL);
    HIP_TRY(h, hipMemcpy(tab.data(), h->v.tile_tab + (size_t)slot * LL, LL * 4, hipMemcpyDeviceToHost));
    return RBPF_OK;
}

int rbpf_refresh_last_scan(rbpf_handle* h, int32_t particle) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->have_scan) return fail(h, RBPF_ESTATE, "rbpf_set_scan has not been called");
    if (particle < 0 || particle >= h->v.P) return fail(h, RBPF_EINVAL, "particle out of range");
    launch_last_scan(h->v, particle, h->d_last_xy, h->stream);
    HIP_TRY(h, hipGetLastError());
    h->n_last_dev = h->v.B;
    return RBPF_OK;
}

int rbpf_export_last_scan(rbpf_handle* h, void* d_out_xy, int32_t* n_points) {
    if (!h || !d_out_xy || !n_points) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (h->n_last_dev < 0) return fail(h, RBPF_ESTATE, "no device-resident previous scan");
    HIP_TRY(h, hipMemcpyAsync(d_out_xy, h->d_last_xy, (size_t)h->n_last_dev * 16, hipMemcpyDeviceToDevice, h->stream));
    *n_points = h->n_last_dev;
    return RBPF_OK;
}

int rbpf_import_last_scan(rbpf_handle* h, const void* d_xy, int32_t n_points) {
    if (!h || !d_xy || n_points < 0 || n_points > h->cfg.max_beams) return RBPF_EINVAL;
    ON_DEVICE(h);
    HIP_TRY(h, hipMemcpyAsync(h->d_last_xy, d_xy, (size_t)n_points * 16, hipMemcpyDeviceToDevice, h->stream));
    h->n_last_dev = n_points;
    return RBPF_OK;
}

int rbpf_get_rng_state(rbpf_handle* h, uint64_t* scan_updates, uint64_t* resample_draws) {
    if (!h || !scan_updates || !resample_draws) return RBPF_EINVAL;
    *scan_updates = h->scan_updates; *resample_draws = h->resample_draws;
    return RBPF_OK;
}

int rbpf_set_rng_state(rbpf_handle* h, uint64_t scan_updates, uint64_t resample_draws) {
    if (!h) return RBPF_EINVAL;
    h->scan_updates = scan_updates; h->resample_draws = resample_draws;
    return RBPF_OK;
}

int rbpf_get_tile_count(rbpf_handle* h, int32_t particle, int32_t* out_n) {
    if (!h || !out_n) return RBPF_EINVAL;
    ON_DEVICE(h);
    std::vector<int32_t> tab;
    int rc = fetch_tab(h, particle, tab);
    if (rc) return rc;
    int n = 0;
    for (int32_t t : tab) n += t >= 0;
    *out_n = n;
    return RBPF_OK;
}

int rbpf_get_tile(rbpf_handle* h, int32_t particle, int32_t k, double* centre2, int8_t* cells) {
    if (!h || !centre2 || !cells) return RBPF_EINVAL;
    ON_DEVICE(h);
    std::vector<int32_t> tab;
    int rc = fetch_tab(h, particle, tab);
    if (rc) return rc;
    const DevView& v = h->v;
    int n = 0;
    for (int a = 0; a < v.L; ++a)
        for (int b = 0; b < v.L; ++b) {
            int32_t t = tab[(size_t)a * v.L + b];
            if (t < 0) continue;
            if (n++ == k) {
                centre2[0] = (double)(a - v.R) * v.tile_len;
                centre2[1] = (double)(b - v.R) * v.tile_len;
                HIP_TRY(h, hipMemcpy(cells, v.pool + (size_t)t * v.dim * v.dim, (size_t)v.dim * v.dim, hipMemcpyDeviceToHost));
                return RBPF_OK;
            }
        }
    return fail(h, RBPF_EINVAL, "tile index out of range");
}

int rbpf_set_tile(rbpf_handle* h, int32_t particle, double cx, double cy, const int8_t* cells) {
    if (!h || !cells) return RBPF_EINVAL;
    ON_DEVICE(h);
    h->v.dups_valid = 0;
    std::vector<int32_t> tab;
    int rc = fetch_tab(h, particle, tab);
    if (rc) return rc;
    DevView& v = h->v;
    double fa = cx / v.tile_len, fb = cy / v.tile_len;
    int a = (int)lround(fa), b = (int)lround(fb);
    if (fabs(fa - a) > 1e-9 || fabs(fb - b) > 1e-9 || abs(a) > v.R || abs(b) > v.R)
        return fail(h, RBPF_EINVAL, "tile centre must lie on the tile lattice inside lattice_radius");
    // the reference's cells never leave [min_odds_emp, max_odds_occ] (gridmap.py:86-117); the map kernels rely on it
    for (size_t i = 0, n = (size_t)v.dim * v.dim; i < n; ++i)
        if (cells[i] < v.cc.vmin || cells[i] > v.cc.vmax) return fail(h, RBPF_EINVAL, "cell value outside [min_odds_emp, max_odds_occ]");
    const size_t LL = (size_t)v.L * v.L, idx = (size_t)(a + v.R) * v.L + (b + v.R);
    int32_t t = tab[idx];
    if (t < 0) {   // pop a tile from the free stack on the host side
        int32_t top = 0;
        HIP_TRY(h, hipMemcpy(&top, v.free_top, 4, hipMemcpyDeviceToHost));
        if (top <= 0) return fail(h, RBPF_ENOMEM, "tile pool exhausted");
        --top;
        HIP_TRY(h, hipMemcpy(&t, v.free_stack + top, 4, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(v.free_top, &top, 4, hipMemcpyHostToDevice));
        int32_t slot = 0;
        HIP_TRY(h, hipMemcpy(&slot, v.slot + particle, 4, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(v.tile_tab + (size_t)slot * LL + idx, &t, 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(h, hipMemcpy(v.pool + (size_t)t * v.dim * v.dim, cells, (size_t)v.dim * v.dim, hipMemcpyHostToDevice));
    {   // occupancy bitmask of the uploaded cells (cell > threshold, gridmap.py:153)
        std::vector<uint32_t> occ((size_t)v.dim * v.ow, 0u);
        for (int x = 0; x < v.dim; ++x)
            for (int y = 0; y < v.dim; ++y)
                if ((int)cells[(size_t)x * v.dim + y] > v.cc.thr) occ[(size_t)x * v.ow + (y >> 5)] |= 1u << (y & 31);
        HIP_TRY(h, hipMemcpy(v.occ + (size_t)t * v.dim * v.ow, occ.data(), occ.size() * 4, hipMemcpyHostToDevice));
    }
    int32_t bb[4] = {0, v.dim - 1, 0, v.dim - 1};       // unknown content: the whole tile counts as written
    HIP_TRY(h, hipMemcpy(v.tile_bbox + 4 * (size_t)t, bb, sizeof(bb), hipMemcpyHostToDevice));
    return RBPF_OK;
}

int rbpf_get_odds_at(rbpf_handle* h, int32_t particle, const double* xy, int32_t n, double* out_vals, uint8_t* out_none) {
    if (!h || !xy || !out_vals || !out_none || n < 0) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (particle < 0 || particle >= h->v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    if (n == 0) return RBPF_OK;
    DevTemp d_xy, d_v, d_n;
    HIP_TRY(h, d_xy.reserve((size_t)n * 16));
    HIP_TRY(h, d_v.reserve((size_t)n * 8));
    HIP_TRY(h, d_n.reserve((size_t)n));
    HIP_TRY(h, hipMemcpyAsync(d_xy.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, h->stream));
    launch_get_odds(h->v, particle, d_xy.as<double>(), n, d_v.as<double>(), d_n.p, h->stream);
    HIP_TRY(h, hipMemcpyAsync(out_vals, d_v.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out_none, d_n.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    return check_device_error(h);
}

// ---- map read-out (kernels_render.hip) -----------------------------------------------------------------------------------
int rbpf_map_extent(rbpf_handle* h, int32_t particle, int32_t* box4) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!box4) return fail(h, RBPF_EINVAL, "box4 is NULL");
    if (particle < -1 || particle >= h->v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    MID_STEP_TRY(h, "map read-out");
    HIP_TRY(h, h->reserve(B_RENDER_OUT, 16));
    int32_t* d_box = h->buf[B_RENDER_OUT].as<int32_t>();
    const int32_t init[4] = {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};
    int32_t m[4];
    HIP_TRY(h, hipMemcpyAsync(d_box, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    launch_map_extent(h->v, particle, d_box, h->stream);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(m, d_box, sizeof(m), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (m[0] > m[1]) { box4[0] = box4[1] = box4[2] = box4[3] = 0; return RBPF_OK; }
    box4[0] = m[0]; box4[1] = m[1] + 1; box4[2] = m[2]; box4[3] = m[3] + 1;   // inclusive -> half-open
    return RBPF_OK;
}

// The box cut at tile seams into jobs: 16 rows at a time, columns in 256-cell blocks aligned to `align` (16, or 32 for the
// loader's occupancy words) inside the tile.
static void render_jobs(const DevView& v, const int32_t* box, std::vector<RenderJob>& jobs, long long align = 16) {
    const long long dim = v.dim, off = (long long)v.R * dim + dim / 2;          // mosaic X + off = a * dim + i
    auto fdiv = [dim](long long u) { return u >= 0 ? u / dim : -((-u + dim - 1) / dim); };
    struct Rows { long long a, i, n, ox; };
    struct Cols { long long b, j0, jlo, jhi, oy; };
    std::vector<Rows> rows;
    std::vector<Cols> cols;
    for (long long u = box[0] + off, e = box[1] + off; u < e;) {
        const long long a = fdiv(u), i = u - a * dim, n = std::min(std::min(16LL, dim - i), e - u);
        rows.push_back({a, i, n, u - off - box[0]});
        u += n;
    }
    for (long long u = box[2] + off, e = box[3] + off; u < e;) {
        const long long b = fdiv(u), jlo = u - b * dim, j0 = jlo & ~(align - 1), jhi = std::min(std::min(j0 + 256, dim), e - b * dim);
        cols.push_back({b, j0, jlo, jhi, b * dim + j0 - off - box[2]});
        u = b * dim + jhi;
    }
    jobs.clear();
    jobs.reserve(rows.size() * cols.size());
    for (const Rows& r : rows)
        for (const Cols& c : cols) {
            const bool in = r.a >= 0 && r.a < v.L && c.b >= 0 && c.b < v.L;
            jobs.push_back({in ? (int32_t)(r.a * v.L + c.b) : -1, (int32_t)r.i, (int32_t)c.j0, (int32_t)r.n, (int32_t)c.jlo,
                            (int32_t)c.jhi, (int32_t)r.ox, (int32_t)c.oy});
        }
}

int rbpf_render_map(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* weights, uint32_t flags,
                    int8_t* cells, float* prob, float* occ_frac) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!box4) return fail(h, RBPF_EINVAL, "box4 is NULL");
    if (flags & ~RBPF_RENDER_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    if (box4[1] < box4[0] || box4[3] < box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 >= x0 and y1 >= y0");
    const long long ny = (long long)box4[3] - box4[2], ncell = ((long long)box4[1] - box4[0]) * ny;
    if (ncell > (1LL << 31)) return fail(h, RBPF_EINVAL, "box holds more than 2^31 cells");
    if (particle >= 0 && (!cells || prob || occ_frac || weights))
        return fail(h, RBPF_EINVAL, "one particle: cells only (prob, occ_frac and weights must be NULL)");
    if (particle < 0 && (cells || (!prob && !occ_frac)))
        return fail(h, RBPF_EINVAL, "whole filter: prob and / or occ_frac (cells must be NULL)");
    MID_STEP_TRY(h, "map read-out");
    // particles are summed in groups of C (kernels_render.hip); the weight sum is formed in the same order
    const int P = v.P, C = std::max(8, (P + 63) / 64), ngroups = (P + C - 1) / C;
    double S = 0.0;
    if (particle < 0) {
        if (weights)
            for (int p = 0; p < P; ++p)
                if (!std::isfinite(weights[p]) || weights[p] < 0.0) return fail(h, RBPF_EINVAL, "weights must be finite and >= 0");
        for (int g = 0; g < ngroups; ++g) {
            double sg = 0.0;
            for (int p = g * C; p < std::min(P, (g + 1) * C); ++p) sg += weights ? weights[p] : 1.0;
            S += sg;
        }
        if (!(S > 0.0) || !std::isfinite(S)) return fail(h, RBPF_EINVAL, "weights must have a positive, finite sum");
    }
    if (ncell == 0) return RBPF_OK;
    std::vector<RenderJob> jobs;
    render_jobs(v, box4, jobs);
    if (jobs.size() > ((size_t)1 << 24)) return fail(h, RBPF_ENOMEM, "box too large to render in one call");
    const bool dev_out = (flags & RBPF_RENDER_DEVICE_OUT) != 0;
    const int n_out = (prob != nullptr) + (occ_frac != nullptr);
    const size_t lut_b = particle < 0 ? 256 * 8 : 0, w_b = particle < 0 ? (size_t)P * 8 : 0, job_b = jobs.size() * sizeof(RenderJob);
    const size_t out_b = particle >= 0 ? (size_t)ncell : (size_t)ncell * 4 * n_out;
    // a small box has too few jobs to fill the GPU: split the particle groups into G chunks along grid.y (RBPF_RENDER_SPLIT=G
    // forces a split, a test knob); the group sums then go through B_RENDER_PART
    int G = 1;
    if (particle < 0 && ngroups > 1) {
        const long long waves = 4LL * (long long)jobs.size();
        G = (int)std::min<long long>(ngroups, (2048 + waves - 1) / waves);
        if (const char* e = getenv("RBPF_RENDER_SPLIT")) G = std::max(1, std::min(ngroups, atoi(e)));
        if ((size_t)ngroups * ncell * n_out * 8 > ((size_t)256 << 20)) G = 1;
    }
    HIP_TRY(h, h->reserve(B_RENDER, lut_b + w_b + job_b));
    if (G > 1) HIP_TRY(h, h->reserve(B_RENDER_PART, (size_t)ngroups * ncell * n_out * 8));
    if (!dev_out) HIP_TRY(h, h->reserve(B_RENDER_OUT, out_b));
    HIP_TRY(h, h->stage[S_RENDER].begin(lut_b + w_b + job_b));              // the last upload may still read it
    unsigned char* st = h->stage[S_RENDER].p;
    if (particle < 0) {
        double* lut = reinterpret_cast<double*>(st);
        for (int k = 0; k < 256; ++k) {                 // get_pr_at, hybridmap.py:74-83
            const double e = exp((double)(int8_t)k * v.quantum);
            lut[k] = e / (1.0 + e);
        }
        double* w = lut + 256;
        for (int p = 0; p < P; ++p) w[p] = weights ? weights[p] : 1.0;
    }
    memcpy(st + lut_b + w_b, jobs.data(), job_b);
    const Block& d_in = h->buf[B_RENDER];
    HIP_TRY(h, h->stage[S_RENDER].upload(d_in.p, lut_b + w_b + job_b, h->stream));
    const RenderJob* d_jobs = d_in.as<const RenderJob>(lut_b + w_b);
    if (particle >= 0) {
        int8_t* out = dev_out ? cells : h->buf[B_RENDER_OUT].as<int8_t>();
        launch_render_cells(v, particle, d_jobs, (int)jobs.size(), ny, out, h->stream);
        HIP_TRY(h, hipGetLastError());
        if (!dev_out) HIP_TRY(h, hipMemcpyAsync(cells, out, (size_t)ncell, hipMemcpyDeviceToHost, h->stream));
    } else {
        RenderFilter f;
        f.jobs = d_jobs;
        f.lut = d_in.as<const double>();
        f.w = f.lut + 256;
        f.S = S; f.C = C; f.ngroups = ngroups; f.ny = ny; f.ncell = (size_t)ncell;
        float* o = h->buf[B_RENDER_OUT].as<float>();
        double* part = h->buf[B_RENDER_PART].as<double>();
        f.prob = !prob ? nullptr : dev_out ? prob : o;
        f.occ = !occ_frac ? nullptr : dev_out ? occ_frac : o + (prob ? ncell : 0);
        f.part_p = prob ? part : nullptr;
        f.part_o = occ_frac ? part + (prob ? (size_t)ngroups * ncell : 0) : nullptr;
        launch_render_filter(v, f, (int)jobs.size(), G, h->stream);
        HIP_TRY(h, hipGetLastError());
        if (!dev_out && prob) HIP_TRY(h, hipMemcpyAsync(prob, f.prob, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
        if (!dev_out && occ_frac) HIP_TRY(h, hipMemcpyAsync(occ_frac, f.occ, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (!dev_out) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

// ---- map loading (kernels_load.hip) and placement (kernels_place.hip) ---------------------------------------------------------
// What a call that writes a box into tiles works out before it queues anything: the lattice positions the box touches with
// (box n tile) in tile-local cells, the jobs of tile_write_kernel, and that the pool holds the tiles that are missing.
struct TileWritePlan { std::vector<LoadTile> tiles; std::vector<RenderJob> jobs; int p_lo = 0, p_hi = 0; };

static bool box_in_lattice(const DevView& v, const int32_t* box4) {
    const long long dim = v.dim, off = (long long)v.R * dim + dim / 2, edge = (long long)v.L * dim;   // mosaic X + off = a * dim + i
    return box4[0] + off >= 0 && box4[1] + off <= edge && box4[2] + off >= 0 && box4[3] + off <= edge;
}

static int plan_tile_write(rbpf_handle* h, int32_t particle, const int32_t* box4, const char* what, TileWritePlan& pl) {
    const DevView& v = h->v;
    const long long dim = v.dim, off = (long long)v.R * dim + dim / 2;
    {
        const long long a_lo = (box4[0] + off) / dim, a_hi = (box4[1] - 1 + off) / dim;
        const long long b_lo = (box4[2] + off) / dim, b_hi = (box4[3] - 1 + off) / dim;
        for (long long a = a_lo; a <= a_hi; ++a)
            for (long long b = b_lo; b <= b_hi; ++b)
                pl.tiles.push_back({(int32_t)(a * v.L + b), (int32_t)std::max(0LL, box4[0] + off - a * dim),
                                    (int32_t)std::min(dim - 1, box4[1] - 1 + off - a * dim), (int32_t)std::max(0LL, box4[2] + off - b * dim),
                                    (int32_t)std::min(dim - 1, box4[3] - 1 + off - b * dim)});
    }
    render_jobs(v, box4, pl.jobs, 32);
    if (pl.jobs.size() > ((size_t)1 << 24)) return fail(h, RBPF_ENOMEM, std::string("box too large for one ") + what);
    // count the missing tiles before anything is allocated: one read of free_top, the slots and their tile_tab rows
    pl.p_lo = particle < 0 ? 0 : particle; pl.p_hi = particle < 0 ? v.P : particle + 1;
    const int np = pl.p_hi - pl.p_lo;
    const size_t LL = (size_t)v.L * v.L;
    std::vector<int32_t> slot(np), tab((size_t)v.P * LL);
    int32_t top = 0;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(&top, v.free_top, 4, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(slot.data(), v.slot + pl.p_lo, (size_t)np * 4, hipMemcpyDeviceToHost));
    if (particle < 0) HIP_TRY(h, hipMemcpy(tab.data(), v.tile_tab, tab.size() * 4, hipMemcpyDeviceToHost));
    else HIP_TRY(h, hipMemcpy(tab.data() + (size_t)slot[0] * LL, v.tile_tab + (size_t)slot[0] * LL, LL * 4, hipMemcpyDeviceToHost));
    long long need = 0;
    for (int q = 0; q < np; ++q)
        for (const LoadTile& lt : pl.tiles) need += tab[(size_t)slot[q] * LL + lt.pos] < 0;
    if (need > top)
        return fail(h, RBPF_ENOMEM, std::string(what) + " needs " + std::to_string(need) + " free tiles, the pool has " + std::to_string(top));
    return RBPF_OK;
}

// Device staging of such a call in scratch buffer b through staging block st: [flag, padded to 16] [tiles] [jobs], then
// `extra` bytes of the caller's at byte meta_b, the first tail_b of them filled from `tail` (host memory, free again on return).
// One upload (the flag cleared); points `a` into it.
static int stage_tile_write(rbpf_handle* h, int b, int st_id, const TileWritePlan& pl, size_t extra, const void* tail, size_t tail_b,
                            LoadArgs& a, size_t& meta_b) {
    const size_t tiles_b = (pl.tiles.size() * sizeof(LoadTile) + 15) & ~(size_t)15, jobs_b = pl.jobs.size() * sizeof(RenderJob);
    meta_b = 16 + tiles_b + ((jobs_b + 15) & ~(size_t)15);
    HIP_TRY(h, h->reserve(b, meta_b + extra));
    const Block& d = h->buf[b];
    Staging& st = h->stage[st_id];
    HIP_TRY(h, st.begin(meta_b + tail_b));
    memset(st.p, 0, meta_b);
    memcpy(st.p + 16, pl.tiles.data(), pl.tiles.size() * sizeof(LoadTile));
    memcpy(st.p + 16 + tiles_b, pl.jobs.data(), jobs_b);
    if (tail_b) memcpy(st.p + meta_b, tail, tail_b);
    HIP_TRY(h, st.upload(d.p, meta_b + tail_b, h->stream));
    a.bad = d.as<int32_t>();
    a.tiles = d.as<const LoadTile>(16); a.n_tiles = (int)pl.tiles.size();
    a.jobs = d.as<const RenderJob>(16 + tiles_b);
    a.p_lo = pl.p_lo; a.p_hi = pl.p_hi;
    return RBPF_OK;
}

int rbpf_load_map(rbpf_handle* h, int32_t particle, const int32_t* box4, const int8_t* cells, uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    DevView& v = h->v;
    if (!box4 || !cells) return fail(h, RBPF_EINVAL, "box4 or cells is NULL");
    if (flags & ~RBPF_LOAD_DEVICE_IN) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    MID_STEP_TRY(h, "map load");
    if (box4[1] < box4[0] || box4[3] < box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 >= x0 and y1 >= y0");
    const long long ny = (long long)box4[3] - box4[2], ncell = ((long long)box4[1] - box4[0]) * ny;
    if (ncell > (1LL << 31)) return fail(h, RBPF_EINVAL, "box holds more than 2^31 cells");
    if (ncell > 0 && !box_in_lattice(v, box4)) return fail(h, RBPF_EINVAL, "box leaves the tile lattice (raise lattice_radius)");
    const bool dev_in = (flags & RBPF_LOAD_DEVICE_IN) != 0;
    if (!dev_in)   // the reference's cells never leave [min_odds_emp, max_odds_occ] (gridmap.py:86-117); the map kernels rely on it
        for (long long i = 0; i < ncell; ++i)
            if (cells[i] < v.cc.vmin || cells[i] > v.cc.vmax) return fail(h, RBPF_EINVAL, "cell value outside [min_odds_emp, max_odds_occ]");
    if (ncell == 0) return RBPF_OK;
    TileWritePlan pl;
    if (const int rc = plan_tile_write(h, particle, box4, "map load", pl)) return rc;
    // the raster (host input only) follows the staged lists
    LoadArgs a;
    size_t meta_b = 0;
    if (const int rc = stage_tile_write(h, B_LOAD, S_LOAD, pl, dev_in ? 0 : (size_t)ncell, nullptr, 0, a, meta_b)) return rc;
    const Block& d_load = h->buf[B_LOAD];
    if (!dev_in) HIP_TRY(h, hipMemcpyAsync(d_load.p + meta_b, cells, (size_t)ncell, hipMemcpyHostToDevice, h->stream));
    a.cells = dev_in ? cells : d_load.as<const int8_t>(meta_b);
    a.ny = ny; a.ncell = ncell;
    if (dev_in) launch_load_validate(v, a, h->stream);
    launch_load_map(v, a, (int)pl.jobs.size(), h->stream);
    HIP_TRY(h, hipGetLastError());
    int32_t bad = 0;
    HIP_TRY(h, hipMemcpyAsync(&bad, a.bad, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (bad) return fail(h, RBPF_EINVAL, "cell value outside [min_odds_emp, max_odds_occ]");
    v.dups_valid = 0;                   // a duplicate's map may differ from its representative's now
    return check_device_error(h);
}

int rbpf_place_map(rbpf_handle* h, int32_t particle, const int32_t* box4, const int8_t* src, int32_t nsx, int32_t nsy,
                   double src_cell, const double* src_pose3, int32_t samples, int32_t mode, uint32_t flags, int8_t* warped,
                   uint8_t* covered) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    DevView& v = h->v;
    if (!box4 || !src || !src_pose3) return fail(h, RBPF_EINVAL, "box4, src or src_pose3 is NULL");
    if (flags & ~(RBPF_PLACE_DEVICE_IN | RBPF_PLACE_DEVICE_OUT | RBPF_PLACE_DRY)) return fail(h, RBPF_EINVAL, "unknown flags");
    const bool dev_in = (flags & RBPF_PLACE_DEVICE_IN) != 0, dev_out = (flags & RBPF_PLACE_DEVICE_OUT) != 0, dry = (flags & RBPF_PLACE_DRY) != 0;
    if (mode != RBPF_PLACE_REPLACE && mode != RBPF_PLACE_KNOWN && mode != RBPF_PLACE_ADD) return fail(h, RBPF_EINVAL, "unknown mode");
    if (samples < 1 || samples > 8) return fail(h, RBPF_EINVAL, "1 <= samples <= 8 is required");
    if (nsx < 1 || nsy < 1 || (long long)nsx * nsy >= (1LL << 31)) return fail(h, RBPF_EINVAL, "nsx >= 1, nsy >= 1 and nsx * nsy < 2^31 are required");
    if (!std::isfinite(src_cell) || !(src_cell > 0.0)) return fail(h, RBPF_EINVAL, "src_cell must be finite and > 0");
    if (!std::isfinite(src_pose3[0]) || !std::isfinite(src_pose3[1]) || !std::isfinite(src_pose3[2])) return fail(h, RBPF_EINVAL, "src_pose3 must be finite");
    if (dry && !warped && !covered) return fail(h, RBPF_EINVAL, "a dry run needs warped and / or covered");
    if (!dry && (particle < -1 || particle >= v.P)) return fail(h, RBPF_EINVAL, "particle index out of range");
    MID_STEP_TRY(h, "map placement");
    if (box4[1] < box4[0] || box4[3] < box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 >= x0 and y1 >= y0");
    const long long ny = (long long)box4[3] - box4[2], ncell = ((long long)box4[1] - box4[0]) * ny;
    if (ncell > (1LL << 31)) return fail(h, RBPF_EINVAL, "box holds more than 2^31 cells");
    if (ncell > 0 && !box_in_lattice(v, box4)) return fail(h, RBPF_EINVAL, "box leaves the tile lattice (raise lattice_radius)");
    const size_t nsrc = (size_t)nsx * nsy;
    if (!dev_in)
        for (size_t i = 0; i < nsrc; ++i)
            if (src[i] < v.cc.vmin || src[i] > v.cc.vmax) return fail(h, RBPF_EINVAL, "source value outside [min_odds_emp, max_odds_occ]");
    if (ncell == 0) return RBPF_OK;
    TileWritePlan pl;
    if (!dry)
        if (const int rc = plan_tile_write(h, particle, box4, "map placement", pl)) return rc;
    // behind the staged lists: the source (host input only, uploaded with them), then the rasters for host outputs
    auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t src_b = dev_in ? 0 : pad(nsrc), out_b = dev_out ? 0 : pad((size_t)ncell);
    LoadArgs a;
    size_t meta_b = 0;
    if (const int rc = stage_tile_write(h, B_PLACE, S_PLACE, pl, src_b + 2 * out_b, src, dev_in ? 0 : nsrc, a, meta_b)) return rc;
    const Block& d = h->buf[B_PLACE];
    a.cells = dev_in ? src : d.as<const int8_t>(meta_b);
    a.ny = ny; a.ncell = (long long)nsrc;                                  // what the validation kernel walks
    PlaceArgs q;
    q.src = a.cells; q.nsx = nsx; q.nsy = nsy;
    q.c = cos(src_pose3[2]); q.s = sin(src_pose3[2]); q.ox = src_pose3[0]; q.oy = src_pose3[1];   // host libm: the device never sees the yaw
    q.src_cell = src_cell; q.cs = v.tile_len / (double)v.dim;
    q.S = samples; q.mode = mode; q.x0 = box4[0]; q.y0 = box4[2]; q.ny = ny; q.ncell = ncell;
    q.warped = !warped ? nullptr : dev_out ? warped : d.as<int8_t>(meta_b + src_b);
    q.covered = !covered ? nullptr : dev_out ? covered : d.as<uint8_t>(meta_b + src_b + out_b);
    q.bad = a.bad;
    if (dev_in) launch_load_validate(v, a, h->stream);
    if (warped || covered) launch_place_warp(q, h->stream);
    if (!dry) launch_place_map(v, a, q, (int)pl.jobs.size(), h->stream);
    HIP_TRY(h, hipGetLastError());
    if (dry && dev_out && !dev_in) return RBPF_OK;                         // nothing to wait for: the host checked the source
    int32_t bad = 0;
    HIP_TRY(h, hipMemcpyAsync(&bad, a.bad, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (bad) return fail(h, RBPF_EINVAL, "source value outside [min_odds_emp, max_odds_occ]");
    if (!dev_out) {
        if (warped) HIP_TRY(h, hipMemcpyAsync(warped, q.warped, (size_t)ncell, hipMemcpyDeviceToHost, h->stream));
        if (covered) HIP_TRY(h, hipMemcpyAsync(covered, q.covered, (size_t)ncell, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (dry) return RBPF_OK;
    v.dups_valid = 0;                   // a duplicate's map may differ from its representative's now
    return check_device_error(h);
}

// ---- scan casting (kernels_cast.hip) --------------------------------------------------------------------------------------
int rbpf_cast_scans(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* angles,
                    int32_t n_beams, double max_range, uint32_t flags, double* ranges, uint8_t* status) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!poses_n3 || !angles || !ranges) return fail(h, RBPF_EINVAL, "poses, angles or ranges is NULL");
    if (flags & ~RBPF_CAST_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    ARG_TRY(h, check_counts(n_poses, 0, n_beams, 0, "n_poses >= 0, n_beams >= 1 and n_poses * n_beams < 2^31 are required"));
    if (particle < 0 && n_poses != v.P) return fail(h, RBPF_EINVAL, "particle -1 casts pose n in particle n's map: n_poses must equal n_particles");
    ARG_TRY(h, check_max_range(max_range));
    ARG_TRY(h, check_poses(poses_n3, n_poses));
    ARG_TRY(h, check_angles(angles, n_beams));
    if (n_poses == 0) return RBPF_OK;
    const bool dev_out = (flags & RBPF_CAST_DEVICE_OUT) != 0;
    const size_t rays = (size_t)n_poses * n_beams;
    Carve c;                                                               // scratch: [poses] [beams] | host ranges, host status
    const size_t pose_at = c.pack((size_t)n_poses * 32), beam_at = c.pack((size_t)n_beams * 16), in_b = c.total();
    const size_t range_at = c.pack(dev_out ? 0 : rays * 8), status_at = c.pack(dev_out || !status ? 0 : rays);
    HIP_TRY(h, h->reserve(B_CAST, c.total()));
    const Block& d_cast = h->buf[B_CAST];
    HIP_TRY(h, h->stage[S_CAST].begin(in_b));                              // the last upload may still read it
    stage_beam2(stage_pose4(h->stage[S_CAST].as<double>(), poses_n3, n_poses), angles, n_beams);
    HIP_TRY(h, h->stage[S_CAST].upload(d_cast.p, in_b, h->stream));
    CastArgs a;
    a.pose4 = d_cast.as<const double>(pose_at);
    a.beam2 = d_cast.as<const double>(beam_at);
    a.n_poses = n_poses; a.B = n_beams; a.particle = particle;
    a.inv = (double)v.dim / v.tile_len;                                    // cells per metre, as lookup_cell_fast forms it
    a.tlim = max_range * a.inv; a.max_range = max_range;
    a.ranges = dev_out ? ranges : d_cast.as<double>(range_at);
    a.status = !status ? nullptr : dev_out ? status : d_cast.as<uint8_t>(status_at);
    launch_cast_scans(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{ranges, a.ranges, rays * 8}, {status, a.status, rays}});
}

// ---- global localization (kernels_locate.hip) -------------------------------------------------------------------------------
int rbpf_locate_scan(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* ranges, const double* angles,
                     int32_t n_beams, int32_t n_rot, uint32_t flags, int32_t* best, int32_t* rot) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!box4 || !ranges || !angles || !best) return fail(h, RBPF_EINVAL, "box4, ranges, angles or best is NULL");
    if (flags & ~RBPF_LOCATE_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < 0 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    if (n_beams < 1 || n_beams > 16384) return fail(h, RBPF_EINVAL, "1 <= n_beams <= 16384 is required");
    if (n_rot < 1 || n_rot > 4096) return fail(h, RBPF_EINVAL, "1 <= n_rot <= 4096 is required");
    if (box4[1] < box4[0] || box4[3] < box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 >= x0 and y1 >= y0");
    const long long nx = (long long)box4[1] - box4[0], ny = (long long)box4[3] - box4[2], ncell = nx * ny;
    if (ncell >= (1LL << 31)) return fail(h, RBPF_EINVAL, "box must hold fewer than 2^31 cells");
    const long long dim = v.dim, off = (long long)v.R * dim + dim / 2, edge = (long long)v.L * dim;   // mosaic X + off = a * dim + i
    if (ncell > 0 && (box4[0] + off < 0 || box4[1] + off > edge || box4[2] + off < 0 || box4[3] + off > edge))
        return fail(h, RBPF_EINVAL, "box leaves the tile lattice");
    for (int b = 0; b < n_beams; ++b)
        if (!std::isfinite(ranges[b]) || !std::isfinite(angles[b])) return fail(h, RBPF_EINVAL, "ranges and angles must be finite");
    MID_STEP_TRY(h, "scan search");
    if (ncell == 0) return RBPF_OK;
    const rbpf_config& c = h->cfg;
    LocateArgs a;
    a.inv = (double)v.dim / v.tile_len;                                    // cells per metre, as lookup_cell_fast forms it
    const double reach = ceil(c.match_max_range * a.inv) + 1.0;            // no used beam ends farther from its candidate cell
    if (!(reach >= 1.0) || reach > 32767.0) return fail(h, RBPF_EINVAL, "match_max_range is more than 32766 cells");
    int nb = 0;
    for (int b = 0; b < n_beams; ++b) nb += ranges[b] > c.match_min_range && ranges[b] < c.match_max_range;   // BF_MATCH, hybridmap.py:218
    a.particle = particle; a.x0 = box4[0]; a.y0 = box4[2]; a.nx = (int)nx; a.ny = (int)ny;
    a.nyw = (int)((ny + 31) / 32); a.M = (int)reach;
    a.rows = a.nx + 2 * a.M; a.W = a.nyw + ((2 * a.M) >> 5) + 2;
    a.n_rot = n_rot; a.nb = nb;
    // enough workgroups to fill the GPU: the rotations are cut into runs when the box has few candidate words
    const long long words = nx * a.nyw, word_waves = (words + 63) / 64;
    const long long runs = std::max(1LL, std::min<long long>(n_rot, (8192 + word_waves - 1) / word_waves));
    a.rpw = (int)((n_rot + runs - 1) / runs);
    const bool dev_out = (flags & RBPF_LOCATE_DEVICE_OUT) != 0;
    const size_t in_b = ((size_t)n_rot + nb) * 16, offs_b = pad256((size_t)n_rot * nb * 4), field_b = pad256((size_t)a.rows * a.W * 8);
    const size_t cand_b = pad256((size_t)words * 4), packed_b = pad256((size_t)ncell * 4), out_b = dev_out ? 0 : (size_t)ncell * 4 * (rot ? 2 : 1);
    const size_t total = pad256(in_b) + offs_b + field_b + 2 * cand_b + 256 + packed_b + out_b;
    if (total > ((size_t)2 << 30)) return fail(h, RBPF_ENOMEM, "box, beams and rotations need more than 2 GiB of scratch: search a smaller box");
    HIP_TRY(h, h->reserve(B_LOCATE, total));
    const Block& d = h->buf[B_LOCATE];
    HIP_TRY(h, h->stage[S_LOCATE].begin(in_b));                            // the last upload may still read it
    double* st = reinterpret_cast<double*>(h->stage[S_LOCATE].p);
    for (int r = 0; r < n_rot; ++r) {                                      // host libm: the device never sees an angle
        const double th = ((double)r * 6.283185307179586) / (double)n_rot;
        st[2 * r] = cos(th); st[2 * r + 1] = sin(th);
    }
    double* sb = st + 2 * (size_t)n_rot;
    for (int b = 0, k = 0; b < n_beams; ++b)
        if (ranges[b] > c.match_min_range && ranges[b] < c.match_max_range) {
            sb[2 * k] = ranges[b] * cos(angles[b]); sb[2 * k + 1] = ranges[b] * sin(angles[b]);   // as rbpf_set_scan forms them
            ++k;
        }
    HIP_TRY(h, h->stage[S_LOCATE].upload(d.p, in_b, h->stream));
    size_t at = pad256(in_b);
    a.cs = d.as<const double>(); a.bxy = a.cs + 2 * (size_t)n_rot;
    a.offs = d.as<int32_t>(at); at += offs_b;
    a.field = d.as<uint2>(at); at += field_b;
    a.cand = d.as<uint32_t>(at); at += cand_b;
    a.items = d.as<int32_t>(at); at += cand_b;
    a.n_items = d.as<int32_t>(at); at += 256;
    a.packed = d.as<uint32_t>(at);
    HIP_TRY(h, hipMemsetAsync(a.n_items, 0, 256 + packed_b, h->stream));   // the item count and the merge raster behind it
    at += packed_b;
    a.best = dev_out ? best : d.as<int32_t>(at);
    a.rot = !rot ? nullptr : dev_out ? rot : d.as<int32_t>(at + (size_t)ncell * 4);
    launch_locate_scan(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    if (dev_out) return RBPF_OK;
    HIP_TRY(h, hipMemcpyAsync(best, a.best, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
    if (rot) HIP_TRY(h, hipMemcpyAsync(rot, a.rot, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

// ---- alignment of a point set (kernels_align.hip) -------------------------------------------------------------------------------
int rbpf_align_points(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* occ_xy, int32_t n_occ,
                      const double* free_xy, int32_t n_free, int32_t n_rot, int32_t r_begin, int32_t r_count, uint32_t flags,
                      int32_t* best, int32_t* rot) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!box4 || !occ_xy || !best || !rot) return fail(h, RBPF_EINVAL, "box4, occ_xy, best or rot is NULL");
    if (flags & ~RBPF_ALIGN_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < 0 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    if (n_occ < 1 || n_free < 0 || (long long)n_occ + n_free > 32767) return fail(h, RBPF_EINVAL, "1 <= n_occ, 0 <= n_free and n_occ + n_free <= 32767 are required");
    if (n_free > 0 && !free_xy) return fail(h, RBPF_EINVAL, "free_xy is NULL with n_free > 0");
    if (n_rot < 1 || n_rot > 4096) return fail(h, RBPF_EINVAL, "1 <= n_rot <= 4096 is required");
    if (r_begin < 0 || r_count < 1 || (long long)r_begin + r_count > n_rot) return fail(h, RBPF_EINVAL, "0 <= r_begin, 1 <= r_count and r_begin + r_count <= n_rot are required");
    if (box4[1] < box4[0] || box4[3] < box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 >= x0 and y1 >= y0");
    const long long nx = (long long)box4[1] - box4[0], ny = (long long)box4[3] - box4[2], ncell = nx * ny;
    if (ncell >= (1LL << 31)) return fail(h, RBPF_EINVAL, "box must hold fewer than 2^31 cells");
    const long long dim = v.dim, off = (long long)v.R * dim + dim / 2, edge = (long long)v.L * dim;   // mosaic X + off = a * dim + i
    if (ncell > 0 && (box4[0] + off < 0 || box4[1] + off > edge || box4[2] + off < 0 || box4[3] + off > edge))
        return fail(h, RBPF_EINVAL, "box leaves the tile lattice");
    const int np = n_occ + n_free;
    const double inv = (double)v.dim / v.tile_len;                         // cells per metre, as lookup_cell_fast forms it
    double far = 0.0;
    for (int k = 0; k < np; ++k) {
        const double* q = k < n_occ ? occ_xy + 2 * (size_t)k : free_xy + 2 * (size_t)(k - n_occ);
        if (!std::isfinite(q[0]) || !std::isfinite(q[1])) return fail(h, RBPF_EINVAL, "point coordinates must be finite");
        far = std::max(far, hypot(q[0], q[1]));
    }
    const double reach = ceil(far * inv) + 1.0;                            // no point lands farther from its cell
    if (!(reach >= 1.0) || reach > 16384.0) return fail(h, RBPF_EINVAL, "the point set reaches more than 16383 cells from its origin");
    MID_STEP_TRY(h, "alignment");
    if (ncell == 0) return RBPF_OK;
    LocateArgs f;                                                          // the field: locate's, over the box grown by M
    AlignArgs a;
    f.particle = particle; a.x0 = f.x0 = box4[0]; a.y0 = f.y0 = box4[2]; a.nx = f.nx = (int)nx; a.ny = f.ny = (int)ny;
    a.nyw = f.nyw = (int)((ny + 31) / 32); a.M = f.M = (int)reach;
    f.rows = a.nx + 2 * a.M; a.W = f.W = a.nyw + ((2 * a.M) >> 5) + 2;
    a.n_rot = n_rot; a.r_begin = r_begin; a.r_count = r_count; a.n_occ = n_occ; a.np = np; a.inv = inv;
    // enough workgroups to fill the GPU: the window is cut into runs of rotations when the box has few words
    const long long words = nx * a.nyw, word_waves = (words + 63) / 64;
    const long long runs = std::max(1LL, std::min<long long>(r_count, (8192 + word_waves - 1) / word_waves));
    a.rpw = (int)((r_count + runs - 1) / runs);
    const bool dev_out = (flags & RBPF_ALIGN_DEVICE_OUT) != 0;
    const size_t in_b = ((size_t)r_count + np) * 16, offs_b = pad256((size_t)r_count * np * 4), field_b = pad256((size_t)f.rows * f.W * 8);
    const size_t packed_b = pad256((size_t)ncell * 4), out_b = dev_out ? 0 : (size_t)ncell * 8;
    const size_t total = pad256(in_b) + offs_b + field_b + packed_b + out_b;
    if (total > ((size_t)2 << 30)) return fail(h, RBPF_ENOMEM, "box, points and rotations need more than 2 GiB of scratch: search a smaller box or window");
    HIP_TRY(h, h->reserve(B_ALIGN, total));
    const Block& d = h->buf[B_ALIGN];
    HIP_TRY(h, h->stage[S_ALIGN].begin(in_b));                             // the last upload may still read it
    double* st = reinterpret_cast<double*>(h->stage[S_ALIGN].p);
    for (int q = 0; q < r_count; ++q) {                                    // host libm: the device never sees an angle
        const double th = ((double)(r_begin + q) * 6.283185307179586) / (double)n_rot;
        st[2 * q] = cos(th); st[2 * q + 1] = sin(th);
    }
    double* sp = st + 2 * (size_t)r_count;
    memcpy(sp, occ_xy, (size_t)n_occ * 16);
    if (n_free > 0) memcpy(sp + 2 * (size_t)n_occ, free_xy, (size_t)n_free * 16);
    HIP_TRY(h, h->stage[S_ALIGN].upload(d.p, in_b, h->stream));
    size_t at = pad256(in_b);
    a.cs = d.as<const double>(); a.pxy = a.cs + 2 * (size_t)r_count;
    a.offs = d.as<int32_t>(at); at += offs_b;
    a.field = f.field = d.as<uint2>(at); at += field_b;
    a.packed = d.as<uint32_t>(at);
    HIP_TRY(h, hipMemsetAsync(a.packed, 0, packed_b, h->stream));          // the merge raster
    at += packed_b;
    a.best = dev_out ? best : d.as<int32_t>(at);
    a.rot = dev_out ? rot : d.as<int32_t>(at + (size_t)ncell * 4);
    launch_align_points(v, f, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    if (dev_out) return RBPF_OK;
    HIP_TRY(h, hipMemcpyAsync(best, a.best, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(rot, a.rot, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

// ---- view gain (kernels_gain.hip) ---------------------------------------------------------------------------------------------
int rbpf_view_gain(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* angles,
                   int32_t n_beams, double max_range, const int32_t* value_tab, uint32_t flags, int64_t* gain, int32_t* seen,
                   int32_t* unknown) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!poses_n3 || !angles || !value_tab || !gain) return fail(h, RBPF_EINVAL, "poses, angles, value_tab or gain is NULL");
    if (flags & ~RBPF_GAIN_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    ARG_TRY(h, check_counts(n_poses, 1, n_beams, 0, "n_poses >= 1, n_beams >= 1 and n_poses * n_beams < 2^31 are required"));
    const long long results = (long long)(particle >= 0 ? 1 : v.P) * n_poses;
    if (results >= (1LL << 31)) return fail(h, RBPF_EINVAL, "n_particles * n_poses < 2^31 is required with particle -1");
    ARG_TRY(h, check_max_range(max_range));
    ARG_TRY(h, check_poses(poses_n3, n_poses));
    ARG_TRY(h, check_angles(angles, n_beams));
    const int nv = v.cc.vmax - v.cc.vmin + 1;                              // one entry per lattice value
    if (v.cc.vmin > 0 || v.cc.vmax < 0 || nv > 256) return fail(h, RBPF_EINVAL, "the lattice values must include 0");
    for (int k = 0; k < nv; ++k)
        if (value_tab[k] < 0 || value_tab[k] > (1 << 20)) return fail(h, RBPF_EINVAL, "value_tab entries must lie in 0 .. 2^20");
    GainArgs a;
    a.inv = (double)v.dim / v.tile_len;                                    // cells per metre, as rbpf_cast_scans forms it
    a.tlim = max_range * a.inv;
    const double reach = ceil(a.tlim) + 2.0;                               // no tested cell lies farther from the origin cell on either axis
    if (!(2.0 * reach + 1.0 <= 1024.0))
        return fail(h, RBPF_EINVAL, "max_range " + std::to_string(max_range) + " m needs a window of more than 1024 cells: the largest admissible "
                                    "max_range is " + std::to_string(509.0 / a.inv) + " m (ceil(max_range * cells per metre) <= 509)");
    MID_STEP_TRY(h, "view gain");
    a.M = (int)reach; a.W = (2 * a.M + 1 + 31) / 32 + 1;
    const bool dev_out = (flags & RBPF_GAIN_DEVICE_OUT) != 0;
    const size_t nres = (size_t)results;
    Carve c;                                                               // scratch: [poses] [beams] [table] | host gain, seen, unknown
    const size_t pose_at = c.pack((size_t)n_poses * 32), beam_at = c.pack((size_t)n_beams * 16), tab_at = c.pack((size_t)nv * 4), in_b = c.close();
    const size_t gain_at = c.pack(dev_out ? 0 : nres * 8), seen_at = c.pack(dev_out || !seen ? 0 : nres * 4);
    const size_t unknown_at = c.pack(dev_out || !unknown ? 0 : nres * 4);
    HIP_TRY(h, h->reserve(B_GAIN, c.total()));
    const Block& d = h->buf[B_GAIN];
    HIP_TRY(h, h->stage[S_GAIN].begin(in_b));                              // the last upload may still read it
    memcpy(stage_beam2(stage_pose4(h->stage[S_GAIN].as<double>(), poses_n3, n_poses), angles, n_beams), value_tab, (size_t)nv * 4);
    HIP_TRY(h, h->stage[S_GAIN].upload(d.p, in_b, h->stream));
    a.pose4 = d.as<const double>(pose_at);
    a.beam2 = d.as<const double>(beam_at);
    a.table = d.as<const int32_t>(tab_at);
    a.n_poses = n_poses; a.B = n_beams; a.nv = nv; a.particle = particle;
    a.gain = dev_out ? gain : d.as<int64_t>(gain_at);
    a.seen = !seen ? nullptr : dev_out ? seen : d.as<int32_t>(seen_at);
    a.unknown = !unknown ? nullptr : dev_out ? unknown : d.as<int32_t>(unknown_at);
    launch_view_gain(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{gain, a.gain, nres * 8}, {seen, a.seen, nres * 4}, {unknown, a.unknown, nres * 4}});
}

// ---- scan checks (kernels_scancheck.hip) ------------------------------------------------------------------------------------------
int rbpf_check_scans(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* ranges, int32_t n_scans,
                     const double* angles, int32_t n_beams, double max_range, double min_range, double tol, const int32_t* hit_tab,
                     int32_t half_bins, int32_t bins_per_cell, const int32_t* class_cost8, uint32_t flags, int64_t* cost, int32_t* counts,
                     uint8_t* classes, int32_t* votes) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!poses_n3 || !ranges || !angles || !hit_tab || !class_cost8 || !cost)
        return fail(h, RBPF_EINVAL, "poses, ranges, angles, hit_tab, class_cost8 or cost is NULL");
    if (flags & ~RBPF_SCANS_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    ARG_TRY(h, check_counts(n_poses, 1, n_beams, 0, "n_poses >= 1, n_beams >= 1 and n_poses * n_beams < 2^31 are required"));
    if (particle < 0 && n_poses != v.P) return fail(h, RBPF_EINVAL, "particle -1 checks pose n in particle n's map: n_poses must equal n_particles");
    ARG_TRY(h, check_scan_count(n_scans, n_poses));
    ARG_TRY(h, check_ranges(max_range, min_range));
    ARG_TRY(h, check_tol(tol));
    ARG_TRY(h, check_beam_tables(hit_tab, half_bins, bins_per_cell, class_cost8));
    ARG_TRY(h, check_poses(poses_n3, n_poses));
    ARG_TRY(h, check_angles(angles, n_beams));
    MID_STEP_TRY(h, "a scan check");
    const bool dev_out = (flags & RBPF_SCANS_DEVICE_OUT) != 0;
    const size_t N = (size_t)n_poses, B = (size_t)n_beams, rays = N * B, nz = (size_t)n_scans * B, ntab = 8 + 2 * (size_t)half_bins + 1;
    Carve c;                                                               // scratch: [poses] [beams] [ranges] [tables] | host cost, counts, votes, classes
    const size_t pose_at = c.pack(N * 32), beam_at = c.pack(B * 16), range_at = c.pack(nz * 8), tab_at = c.pack(ntab * 4), in_b = c.close();
    const size_t cost_at = c.take(dev_out ? 0 : N * 8), counts_at = c.take(dev_out || !counts ? 0 : N * 32);
    const size_t votes_at = c.take(dev_out || !votes ? 0 : B * 32), classes_at = c.take(dev_out || !classes ? 0 : rays);
    HIP_TRY(h, h->reserve(B_SCANCHECK, c.total()));
    const Block& d = h->buf[B_SCANCHECK];
    Staging& st = h->stage[S_SCANCHECK];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    double* zs = stage_beam2(stage_pose4(st.as<double>(), poses_n3, N), angles, B);
    memcpy(zs, ranges, nz * 8);
    stage_beam_tables(reinterpret_cast<int32_t*>(zs + nz), class_cost8, hit_tab, half_bins);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    ScanCheckArgs a;
    a.pose4 = d.as<const double>(pose_at); a.beam2 = d.as<const double>(beam_at); a.ranges = d.as<const double>(range_at);
    a.tabs = d.as<const int32_t>(tab_at);
    a.n_poses = n_poses; a.B = n_beams; a.scan_each = n_scans == n_poses; a.particle = particle; a.half_bins = half_bins;
    a.inv = (double)v.dim / v.tile_len;                                    // cells per metre, as rbpf_cast_scans forms it
    a.tmax = max_range * a.inv; a.ttol = tol * a.inv;
    a.max_range = max_range; a.min_range = min_range; a.bins_per_cell = (double)bins_per_cell;
    a.cost = reinterpret_cast<unsigned long long*>(dev_out ? cost : d.as<int64_t>(cost_at));
    a.counts = !counts ? nullptr : dev_out ? counts : d.as<int32_t>(counts_at);
    a.votes = !votes ? nullptr : dev_out ? votes : d.as<int32_t>(votes_at);
    a.classes = !classes ? nullptr : dev_out ? classes : d.as<uint8_t>(classes_at);
    HIP_TRY(h, hipMemsetAsync(a.cost, 0, N * 8, h->stream));               // the kernel adds to all three
    if (a.counts) HIP_TRY(h, hipMemsetAsync(a.counts, 0, N * 32, h->stream));
    if (a.votes) HIP_TRY(h, hipMemsetAsync(a.votes, 0, B * 32, h->stream));
    launch_check_scans(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{cost, a.cost, N * 8}, {counts, a.counts, N * 32}, {votes, a.votes, B * 32}, {classes, a.classes, rays}});
}

}  // extern "C"

// ---- block relaxation (rbpf_blockrelax.h): what rbpf_travel_cost and rbpf_frontier_regions share on the host ------------------
// relaxation rounds queued between two reads of their counters.  A read costs a host wait; a round after convergence costs one
// launch of workgroups that leave at once.  DESIGN.md 3.12 has the measurement behind the value.
static const int TRAVEL_ROUNDS_PER_READ = 8;
static const size_t RELAX_SCRATCH = (size_t)2 << 30;   // scratch of one batch of particles at the most

// particles per batch: `fixed` bytes once and `per` bytes for every particle of the batch fit RELAX_SCRATCH (the caller has
// checked that one particle does), a batch is one grid (gridDim.y), and the environment variable may cap it, for tests
static long long relax_batch(int np_all, size_t fixed, size_t per, const char* cap_env) {
    long long batch = std::min<long long>(std::min<long long>(np_all, 65535), (long long)((RELAX_SCRATCH - fixed) / per));
    if (const char* e = getenv(cap_env)) batch = std::max(1LL, std::min<long long>(batch, atoll(e)));
    return batch;
}

// The rounds of one batch, to the fixed point: queues per_read rounds, launch(r, counter of the round), reads their counters
// into the pinned stage `st` (256 bytes: 32 counts of changed blocks, 32 of block runs) and stops at the first batch that
// holds a round which changed no block.  Adds the rounds launched and the block runs to `launched` and `runs`.
template <class Launch>
static int relax_rounds(rbpf_handle* h, Staging& st, int32_t* d_count, long long round_limit, int per_read, const char* not_converged,
                        Launch launch, long long& launched, long long& runs) {
    const int32_t* h_count = reinterpret_cast<const int32_t*>(st.p);
    bool done = false;
    for (long long r = 0; !done; ) {
        if (r > round_limit) return fail(h, RBPF_EDEVICE, not_converged);
        HIP_TRY(h, hipMemsetAsync(d_count, 0, 256, h->stream));
        for (int q = 0; q < per_read; ++q, ++r) launch(r, d_count + q);
        HIP_TRY(h, hipGetLastError());
        launched += per_read;
        HIP_TRY(h, hipMemcpyAsync(st.p, d_count, 256, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int q = 0; q < per_read; ++q) {
            done = done || h_count[q] == 0;                                                // a round that changed no block: the fixed point
            runs += h_count[32 + q];
        }
    }
    return RBPF_OK;
}

static void relax_stats(uint64_t (&s)[3], long long launched, long long runs, long long pairs) { s[0] = (uint64_t)launched; s[1] = (uint64_t)runs; s[2] = (uint64_t)pairs; }

extern "C" {

// ---- travel cost (kernels_travel.hip) -----------------------------------------------------------------------------------------
int rbpf_travel_cost(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* start_xy, int32_t n_start,
                     const double* goal_xy, int32_t n_goals, int32_t inflate, int32_t clear_max, uint32_t flags, int32_t* cost,
                     uint16_t* clearance, int32_t* goal_cost, int32_t* rounds) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!box4 || !start_xy) return fail(h, RBPF_EINVAL, "box4 or start_xy is NULL");
    if (flags & ~(RBPF_TRAVEL_DEVICE_OUT | RBPF_TRAVEL_THROUGH_UNKNOWN)) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    const bool all = particle < 0;
    if (all && (cost || clearance)) return fail(h, RBPF_EINVAL, "cost and clearance must be NULL with particle -1");
    if (!cost && !clearance && !goal_cost) return fail(h, RBPF_EINVAL, "cost, clearance and goal_cost are all NULL");
    if (n_goals < 0 || (goal_cost && (n_goals < 1 || !goal_xy))) return fail(h, RBPF_EINVAL, "goal_cost needs goal_xy and n_goals >= 1");
    if (all ? (n_start != 1 && n_start != v.P) : n_start < 1)
        return fail(h, RBPF_EINVAL, "n_start >= 1 is required, and with particle -1 n_start must be 1 or the number of particles");
    if (inflate < 0 || clear_max <= inflate || clear_max > 320) return fail(h, RBPF_EINVAL, "0 <= inflate < clear_max <= 320 is required");
    if (box4[1] <= box4[0] || box4[3] <= box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 > x0 and y1 > y0");
    const long long nx = (long long)box4[1] - box4[0], ny = (long long)box4[3] - box4[2], ncell = nx * ny;
    if (ncell > (1LL << 27)) return fail(h, RBPF_EINVAL, "box must hold at most 2^27 cells");
    if (!box_in_lattice(v, box4)) return fail(h, RBPF_EINVAL, "box leaves the tile lattice");
    const int ng = goal_cost ? n_goals : 0;                                // goals are read only when their cost is asked for
    for (long long k = 0; k < 2LL * n_start; ++k)
        if (!std::isfinite(start_xy[k])) return fail(h, RBPF_EINVAL, "start coordinates must be finite");
    for (long long k = 0; k < 2LL * ng; ++k)
        if (!std::isfinite(goal_xy[k])) return fail(h, RBPF_EINVAL, "goal coordinates must be finite");
    MID_STEP_TRY(h, "travel cost");

    TravelArgs a;
    a.x0 = box4[0]; a.y0 = box4[2]; a.nx = (int)nx; a.ny = (int)ny;
    a.nbx = (int)((nx + 63) / 64); a.nby = (int)((ny + 63) / 64);
    a.m = (clear_max + 4) / 5; a.inflate = inflate; a.clear_max = clear_max;
    a.through_unknown = (flags & RBPF_TRAVEL_THROUGH_UNKNOWN) != 0;
    a.n_start = n_start; a.start_each = all && n_start == v.P && v.P > 1; a.n_goals = ng;
    const bool dev_out = (flags & RBPF_TRAVEL_DEVICE_OUT) != 0;
    const int np_all = all ? v.P : 1;
    const long long nblk = (long long)a.nbx * a.nby;
    a.cw = a.nby * 64 + 2;
    const size_t cost_b = pad256((size_t)(a.nbx * 64LL + 2) * a.cw * 4), t_b = pad256((size_t)nblk * 512), dirty_b = pad256((size_t)nblk);
    const size_t per = cost_b + t_b + 2 * dirty_b;
    const size_t in_b = pad256(((size_t)n_start + ng) * 8);
    const size_t out_b = dev_out ? 0 : pad256(cost ? (size_t)ncell * 4 : 0) + pad256(clearance ? (size_t)ncell * 2 : 0) + pad256((size_t)np_all * ng * 4);
    const size_t fixed = in_b + 256 + out_b;
    if (fixed + per > RELAX_SCRATCH) return fail(h, RBPF_ENOMEM, "one particle's travel cost over this box needs more than 2 GiB of scratch: use a smaller box");
    const long long batch = relax_batch(np_all, fixed, per, "RBPF_TRAVEL_BATCH");
    int per_read = TRAVEL_ROUNDS_PER_READ;
    if (const char* e = getenv("RBPF_TRAVEL_ROUNDS_PER_READ")) per_read = std::max(1, std::min(32, atoi(e)));   // measurement switch (tools/README.md)
    HIP_TRY(h, h->reserve(B_TRAVEL, fixed + (size_t)batch * per));
    const Block& d = h->buf[B_TRAVEL];
    Staging& st = h->stage[S_TRAVEL];
    HIP_TRY(h, st.begin(256 + in_b));                                      // the last upload may still read it
    const double inv = (double)v.dim / v.tile_len;                         // cells per metre, as rbpf_cast_scans forms it
    int32_t* cells = reinterpret_cast<int32_t*>(st.p + 256);
    for (long long k = 0; k < (long long)n_start + ng; ++k) {
        const double* q = k < n_start ? start_xy + 2 * k : goal_xy + 2 * (k - n_start);
        const double fx = floor(q[0] * inv) - (double)box4[0], fy = floor(q[1] * inv) - (double)box4[2];   // exact: integers in float64
        const bool in = fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny;
        cells[2 * k] = in ? (int32_t)fx : -1; cells[2 * k + 1] = in ? (int32_t)fy : -1;
    }
    HIP_TRY(h, hipMemcpyAsync(d.p, st.p + 256, in_b, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, st.submitted(h->stream));
    a.starts = d.as<const int32_t>(); a.goals = a.starts + 2 * (size_t)n_start;
    int32_t* d_count = d.as<int32_t>(in_b);
    size_t at = in_b + 256;
    int32_t* o_cost = nullptr; uint16_t* o_clear = nullptr; int32_t* o_goal = nullptr;
    if (!dev_out) {
        if (cost) { o_cost = d.as<int32_t>(at); at += pad256((size_t)ncell * 4); }
        if (clearance) { o_clear = d.as<uint16_t>(at); at += pad256((size_t)ncell * 2); }
        if (ng) { o_goal = d.as<int32_t>(at); at += pad256((size_t)np_all * ng * 4); }
    } else { o_cost = cost; o_clear = clearance; o_goal = goal_cost; }
    unsigned char* work = d.p + at;
    a.cost_out = o_cost; a.clearance = o_clear;
    long long launched = 0, runs = 0;
    for (long long p0 = 0; p0 < np_all; p0 += batch) {
        const long long nb = std::min<long long>(batch, np_all - p0);
        a.particle = all ? (int)p0 : particle; a.n_part = (int)nb;
        a.ras = reinterpret_cast<int32_t*>(work); a.ras_stride = (long long)(cost_b / 4);
        a.tbits = reinterpret_cast<uint16_t*>(work + (size_t)nb * cost_b); a.t_stride = (long long)(t_b / 2);
        a.dirty = work + (size_t)nb * (cost_b + t_b);
        a.goal_out = o_goal ? o_goal + (size_t)p0 * ng : nullptr;
        HIP_TRY(h, hipMemsetAsync(a.ras, 0x3f, (size_t)nb * cost_b, h->stream));          // TRAVEL_INF everywhere
        HIP_TRY(h, hipMemsetAsync(a.dirty, 0, 2 * (size_t)nb * dirty_b, h->stream));
        launch_travel_mask(v, a, h->stream);
        HIP_TRY(h, hipGetLastError());
        // dirty flags: [2][nb][nblk] packed without the padding of dirty_b (2 * nb * nblk <= 2 * nb * dirty_b)
        if (int rc = relax_rounds(h, st, d_count, ncell + 1, per_read, "internal error: the travel cost did not converge",
                                  [&](long long r, int32_t* c) { launch_travel_round(a, (int)(r & 1), c, h->stream); }, launched, runs)) return rc;
        launch_travel_output(a, h->stream);
        HIP_TRY(h, hipGetLastError());
        a.clearance = nullptr;
    }
    if (rounds) *rounds = (int32_t)std::min<long long>(launched, INT32_MAX);
    relax_stats(h->travel_stats, launched, runs, nblk * np_all);
    if (dev_out) return RBPF_OK;
    if (cost) HIP_TRY(h, hipMemcpyAsync(cost, o_cost, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
    if (clearance) HIP_TRY(h, hipMemcpyAsync(clearance, o_clear, (size_t)ncell * 2, hipMemcpyDeviceToHost, h->stream));
    if (ng) HIP_TRY(h, hipMemcpyAsync(goal_cost, o_goal, (size_t)np_all * ng * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

int rbpf_travel_stats(rbpf_handle* h, uint64_t* out3) {
    if (!h) return RBPF_EINVAL;
    if (!out3) return fail(h, RBPF_EINVAL, "out3 is NULL");
    for (int k = 0; k < 3; ++k) out3[k] = h->travel_stats[k];
    return RBPF_OK;
}

// ---- path checks (kernels_paths.hip; the host side is rbpf_pathbatch.h) ---------------------------------------------------------
static_assert(RBPF_PATHS_DEVICE_OUT == PATHS_DEVICE_OUT && RBPF_PATHS_THROUGH_UNKNOWN == PATHS_THROUGH_UNKNOWN &&
              RBPF_PATHS_START_EXEMPT == PATHS_START_EXEMPT && RBPF_PATHS_OWN == PATHS_OWN, "rbpf_pathbatch.h repeats the flags of rbpf_hip.h");
int rbpf_check_paths(rbpf_handle* h, int32_t particle, const double* xy, const int32_t* path_start, int32_t n_paths, int32_t inflate,
                     int32_t clear_max, uint32_t flags, int32_t* out, int32_t* steps) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    ARG_TRY(h, check_path_args(xy, path_start, out, particle, v.P, n_paths, inflate, clear_max, flags));
    ARG_TRY(h, check_path_results(particle, v.P, n_paths, flags));
    const long long off = (long long)v.R * v.dim + v.dim / 2;             // mosaic X + off counts from the lattice's first cell
    PathBatch pb;
    path_batch_build(pb, xy, path_start, n_paths, (double)v.dim / v.tile_len, -off, (long long)v.L * v.dim - off);
    ARG_TRY(h, pb.error());
    MID_STEP_TRY(h, "a path check");
    const bool dev_out = (flags & RBPF_PATHS_DEVICE_OUT) != 0;
    const size_t nw = pb.wstep.size(), nres = (size_t)path_results(particle, v.P, n_paths, flags);
    Carve c;                                                               // scratch: [cells] [steps of the waypoints] [offsets] | host out
    const size_t cell_at = c.pack(nw * 8), wstep_at = c.pack(nw * 4), start_at = c.pack(((size_t)n_paths + 1) * 4), in_b = c.close();
    const size_t out_at = c.take(dev_out ? 0 : nres * 16);
    HIP_TRY(h, h->reserve(B_PATHS, c.total()));
    const Block& d = h->buf[B_PATHS];
    Staging& st = h->stage[S_PATHS];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    memcpy(st.p + cell_at, pb.cells.data(), nw * 8);
    memcpy(st.p + wstep_at, pb.wstep.data(), nw * 4);
    memcpy(st.p + start_at, path_start, ((size_t)n_paths + 1) * 4);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    PathArgs a;
    a.cells = d.as<const int32_t>(cell_at); a.wstep = d.as<const int32_t>(wstep_at); a.path_start = d.as<const int32_t>(start_at);
    a.n_paths = n_paths; a.particle = particle >= 0 ? particle : 0;
    a.own_k = path_group_size(n_paths, v.P, flags);
    a.pairs = (long long)nres;
    a.inflate = inflate; a.clear_max = clear_max;
    a.through_unknown = (flags & RBPF_PATHS_THROUGH_UNKNOWN) != 0; a.start_exempt = (flags & RBPF_PATHS_START_EXEMPT) != 0;
    a.out = dev_out ? out : d.as<int32_t>(out_at);
    launch_check_paths(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    if (!dev_out)
        if (const int rc = fetch(h, {{out, a.out, nres * 16}})) return rc;
    if (steps) memcpy(steps, pb.steps.data(), (size_t)n_paths * 4);        // behind everything that can fail: nothing is written on an error
    return RBPF_OK;
}

// ---- rollout checks (kernels_paths.hip; the host side is rbpf_rolloutbatch.h) -----------------------------------------------------
int rbpf_check_rollouts(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* tmpl_xy,
                        const int32_t* tmpl_start, int32_t n_tmpl, int32_t inflate, int32_t clear_max, uint32_t flags, int32_t* out,
                        int32_t* steps) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    ARG_TRY(h, check_rollout_args(poses_n3, tmpl_xy, tmpl_start, out, particle, v.P, n_poses, n_tmpl, inflate, clear_max, flags));
    ARG_TRY(h, check_rollout_results(n_poses, n_tmpl));
    const long long off = (long long)v.R * v.dim + v.dim / 2;             // mosaic X + off counts from the lattice's first cell
    const double inv = (double)v.dim / v.tile_len;                         // cells per metre, as rbpf_check_paths forms it
    RolloutBatch rb;
    rollout_templates(rb, tmpl_xy, tmpl_start, n_tmpl, inv);
    ARG_TRY(h, rb.error());
    rollout_poses(rb, poses_n3, n_poses, inv, -off, (long long)v.L * v.dim - off);
    ARG_TRY(h, rb.error());
    MID_STEP_TRY(h, "a rollout check");
    const bool dev_out = (flags & RBPF_PATHS_DEVICE_OUT) != 0;
    const size_t N = (size_t)n_poses, nw = (size_t)tmpl_start[n_tmpl], nres = (size_t)rollout_results(n_poses, n_tmpl);
    Carve c;                                                               // scratch: [poses] [template waypoints] [offsets] | host out, host steps
    const size_t pose_at = c.pack(N * 32), xy_at = c.pack(nw * 16), start_at = c.pack(((size_t)n_tmpl + 1) * 4), in_b = c.close();
    const size_t out_at = c.take(dev_out ? 0 : nres * 16), steps_at = c.take(dev_out || !steps ? 0 : nres * 4);
    HIP_TRY(h, h->reserve(B_ROLLOUTS, c.total()));
    const Block& d = h->buf[B_ROLLOUTS];
    Staging& st = h->stage[S_ROLLOUTS];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    double* txy = stage_pose4(st.as<double>(pose_at), poses_n3, N);
    memcpy(txy, tmpl_xy, nw * 16);
    memcpy(st.p + start_at, tmpl_start, ((size_t)n_tmpl + 1) * 4);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    RolloutArgs a;
    a.pose4 = d.as<const double>(pose_at); a.tmpl_xy = d.as<const double>(xy_at); a.tmpl_start = d.as<const int32_t>(start_at);
    a.n_tmpl = n_tmpl; a.particle = particle; a.off = (int)off; a.inv = inv;
    a.pairs = (long long)nres;
    a.inflate = inflate; a.clear_max = clear_max;
    a.through_unknown = (flags & RBPF_PATHS_THROUGH_UNKNOWN) != 0; a.start_exempt = (flags & RBPF_PATHS_START_EXEMPT) != 0;
    a.out = dev_out ? out : d.as<int32_t>(out_at);
    a.steps = !steps ? nullptr : dev_out ? steps : d.as<int32_t>(steps_at);
    launch_check_rollouts(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{out, a.out, nres * 16}, {steps, a.steps, nres * 4}});
}

// ---- footprint checks (kernels_footprint.hip; the host side is rbpf_footbatch.h) ------------------------------------------------
int rbpf_check_footprints(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* tmpl_xy,
                          const int32_t* tmpl_bin, const int32_t* tmpl_start, int32_t n_tmpl, const int32_t* fp_span, const int32_t* fp_start,
                          int32_t n_bins, int32_t inflate, int32_t clear_max, int32_t exempt, uint32_t flags, int32_t* out, int32_t* steps) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    ARG_TRY(h, check_footprint_args(poses_n3, tmpl_xy, tmpl_bin, tmpl_start, fp_span, fp_start, out, particle, v.P, n_poses, n_tmpl, n_bins,
                                    inflate, clear_max, exempt, flags));
    ARG_TRY(h, check_footprint_results(particle, v.P, n_poses, n_tmpl));
    const long long off = (long long)v.R * v.dim + v.dim / 2;             // mosaic X + off counts from the lattice's first cell
    const double inv = (double)v.dim / v.tile_len;                         // cells per metre, as rbpf_check_paths forms it
    RolloutBatch rb;
    rollout_templates(rb, tmpl_xy, tmpl_start, n_tmpl, inv);
    ARG_TRY(h, rb.error());
    rollout_poses(rb, poses_n3, n_poses, inv, -off, (long long)v.L * v.dim - off);
    ARG_TRY(h, rb.error());
    FootTable ft;
    footprint_table(ft, fp_span, fp_start, n_bins);
    ARG_TRY(h, ft.error());
    footprint_template_bins(ft, tmpl_bin, tmpl_start, n_tmpl, n_bins);
    ARG_TRY(h, ft.error());
    std::vector<int32_t> pb((size_t)n_poses);
    footprint_pose_bins(ft, pb.data(), poses_n3, n_poses, n_bins);
    ARG_TRY(h, ft.error());
    MID_STEP_TRY(h, "a footprint check");
    const bool dev_out = (flags & RBPF_PATHS_DEVICE_OUT) != 0;
    const size_t N = (size_t)n_poses, nw = (size_t)tmpl_start[n_tmpl], ns = (size_t)fp_start[n_bins];
    const size_t nres = (size_t)footprint_results(particle, v.P, n_poses, n_tmpl);
    Carve c;            // scratch: [poses] [template waypoints] [pose bins] [template bins] [offsets] [span offsets] [spans] | host out, host steps
    const size_t pose_at = c.pack(N * 32), xy_at = c.pack(nw * 16), pbin_at = c.pack(N * 4), tbin_at = c.pack(nw * 4);
    const size_t start_at = c.pack(((size_t)n_tmpl + 1) * 4), fstart_at = c.pack(((size_t)n_bins + 1) * 4), span_at = c.pack(ns * 4), in_b = c.close();
    const size_t out_at = c.take(dev_out ? 0 : nres * 16), steps_at = c.take(dev_out || !steps ? 0 : nres * 4);
    HIP_TRY(h, h->reserve(B_FOOTPRINTS, c.total()));
    const Block& d = h->buf[B_FOOTPRINTS];
    Staging& st = h->stage[S_FOOTPRINTS];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    double* txy = stage_pose4(st.as<double>(pose_at), poses_n3, N);
    memcpy(txy, tmpl_xy, nw * 16);
    memcpy(st.p + pbin_at, pb.data(), N * 4);
    memcpy(st.p + tbin_at, tmpl_bin, nw * 4);
    memcpy(st.p + start_at, tmpl_start, ((size_t)n_tmpl + 1) * 4);
    memcpy(st.p + fstart_at, fp_start, ((size_t)n_bins + 1) * 4);
    int32_t* spans = st.as<int32_t>(span_at);
    for (size_t k = 0; k < ns; ++k) spans[k] = footprint_pack(fp_span + 3 * k);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    FootArgs a;
    a.pose4 = d.as<const double>(pose_at); a.pose_bin = d.as<const int32_t>(pbin_at);
    a.tmpl_xy = d.as<const double>(xy_at); a.tmpl_bin = d.as<const int32_t>(tbin_at); a.tmpl_start = d.as<const int32_t>(start_at);
    a.fp_start = d.as<const int32_t>(fstart_at); a.fp_span = d.as<const int32_t>(span_at);
    a.n_tmpl = n_tmpl; a.n_bins = n_bins; a.particle = particle; a.one_pose = particle < 0 && n_poses == 1;
    a.off = (int)off; a.inv = inv;
    a.pairs = (long long)nres;
    a.inflate = inflate; a.clear_max = clear_max;
    a.through_unknown = (flags & RBPF_PATHS_THROUGH_UNKNOWN) != 0; a.exempt = exempt;
    a.out = dev_out ? out : d.as<int32_t>(out_at);
    a.steps = !steps ? nullptr : dev_out ? steps : d.as<int32_t>(steps_at);
    launch_check_footprints(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{out, a.out, nres * 16}, {steps, a.steps, nres * 4}});
}

// ---- local map (kernels_local.hip; the host side is rbpf_localbatch.h) ----------------------------------------------------------
static_assert(RBPF_LOCAL_DEVICE_OUT == LOCAL_DEVICE_OUT && RBPF_LOCAL_MAX_SIDE == LOCAL_MAX_SIDE && LOCAL_GROUP == LOCAL_GROUP_POSES &&
              LOCAL_LDS == LDS_LIMIT, "rbpf_localbatch.h repeats constants of rbpf_hip.h, rbpf_internal.h and rbpf_host.h");
int rbpf_local_map(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const uint32_t* wq, int32_t n,
                   double cell_out, int32_t samples, const double* offset2, uint32_t flags, int64_t* fused, int8_t* crops) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    ARG_TRY(h, check_local_args(poses_n3, fused, crops, particle, v.P, n_poses, n, cell_out, samples, offset2, flags));
    const double inv = (double)v.dim / v.tile_len;                         // cells per metre, as rbpf_check_rollouts forms it
    LocalPlan lp;
    local_plan(lp, n, cell_out, samples, offset2, inv);
    ARG_TRY(h, lp.error());
    local_poses(lp, poses_n3, n_poses, inv);
    ARG_TRY(h, lp.error());
    local_weights(lp, wq, n_poses);
    ARG_TRY(h, lp.error());
    MID_STEP_TRY(h, "a local map");
    const bool dev_out = (flags & RBPF_LOCAL_DEVICE_OUT) != 0, fuse = fused != nullptr, scratch_crops = !crops;
    const size_t N = (size_t)n_poses, ncell = (size_t)n * n, nq = (size_t)lp.nq;
    if (local_batch_bytes(1, n, scratch_crops, fuse) > LOCAL_SCRATCH)
        return fail(h, RBPF_ENOMEM, "one pose's window needs more than 256 MiB of scratch: use a smaller n");
    long long cap = 0;
    if (const char* e = getenv("RBPF_LOCAL_BATCH")) cap = std::max(1LL, atoll(e));
    const long long batch = local_batch(n_poses, n, scratch_crops, fuse, cap);
    Carve c;                                                               // scratch: [poses] [gx] [gy] [wq] | host fused, host crops, batch crops, group sums
    const size_t pose_at = c.pack(N * 32), gx_at = c.pack(nq * 8), gy_at = c.pack(nq * 8), wq_at = c.pack(N * 4), in_b = c.close();
    const size_t fused_at = c.take(dev_out || !fuse ? 0 : ncell * 32), crops_at = c.take(dev_out || !crops ? 0 : N * ncell);
    const size_t bcrops_at = c.take(scratch_crops ? (size_t)batch * local_crop_stride(n, false) : 0);
    const size_t ncellp = local_cells_padded(n), groups = (size_t)local_groups(batch);
    const size_t pw_at = c.take(fuse ? groups * ncellp * 12 : 0), pv_at = c.take(fuse ? groups * ncellp * 8 : 0);
    HIP_TRY(h, h->reserve(B_LOCAL, c.total()));
    const Block& d = h->buf[B_LOCAL];
    Staging& st = h->stage[S_LOCAL];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    stage_pose4(st.as<double>(pose_at), poses_n3, N);
    memcpy(st.p + gx_at, lp.gx.data(), nq * 8);
    memcpy(st.p + gy_at, lp.gy.data(), nq * 8);
    uint32_t* w = st.as<uint32_t>(wq_at);
    for (size_t k = 0; k < N; ++k) w[k] = wq ? wq[k] : 1u;
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    LocalArgs a;
    a.pose4 = d.as<const double>(pose_at); a.gx = d.as<const double>(gx_at); a.gy = d.as<const double>(gy_at); a.wq = d.as<const uint32_t>(wq_at);
    a.n = n; a.S = samples; a.nq = lp.nq;
    a.reach = (int)lp.reach; a.side = lp.side; a.row_bytes = local_row_bytes(lp.side); a.tab_lds = local_tables_fit(lp.side, lp.nq);
    a.particle = particle; a.off = v.R * v.dim + v.dim / 2; a.inv = inv;
    int8_t* all_crops = !crops ? nullptr : dev_out ? crops : d.as<int8_t>(crops_at);   // [n_poses][n][n], dense
    a.cstride = local_crop_stride(n, !scratch_crops);
    a.ncellp = ncellp;
    a.part_w = d.as<uint32_t>(pw_at); a.part_v = d.as<long long>(pv_at);
    a.fused = !fuse ? nullptr : dev_out ? reinterpret_cast<long long*>(fused) : d.as<long long>(fused_at);
    if (fuse) HIP_TRY(h, hipMemsetAsync(a.fused, 0, ncell * 32, h->stream));
    for (long long p0 = 0; p0 < n_poses; p0 += batch) {
        a.p0 = (int)p0; a.nb = (int)std::min<long long>(batch, n_poses - p0);
        a.crops = all_crops ? all_crops + (size_t)p0 * ncell : d.as<int8_t>(bcrops_at);
        a.wide = a.cstride % 16 == 0 && reinterpret_cast<uintptr_t>(a.crops) % 16 == 0;
        a.ngroups = (int)local_groups(a.nb);
        launch_local_crop(v, a, h->stream);
        HIP_TRY(h, hipGetLastError());
        if (fuse) {
            launch_local_fuse(v, a, h->stream);
            HIP_TRY(h, hipGetLastError());
        }
    }
    return dev_out ? RBPF_OK : fetch(h, {{fused, a.fused, ncell * 32}, {crops, all_crops, N * ncell}});
}

// ---- frontier regions (kernels_frontier.hip) ----------------------------------------------------------------------------------
int rbpf_frontier_regions(rbpf_handle* h, int32_t particle, const int32_t* box4, int32_t clear, int32_t min_size, int32_t max_regions,
                          uint32_t flags, int32_t* label, int64_t* regions, int32_t* counts) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!box4) return fail(h, RBPF_EINVAL, "box4 is NULL");
    if (flags & ~RBPF_FRONTIER_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    const bool all = particle < 0;
    if (all && label) return fail(h, RBPF_EINVAL, "label must be NULL with particle -1");
    if (!label && !regions && !counts) return fail(h, RBPF_EINVAL, "label, regions and counts are all NULL");
    if (clear < 0 || clear > 16) return fail(h, RBPF_EINVAL, "0 <= clear <= 16 is required");
    if (min_size < 1 || max_regions < 1 || max_regions > 1024) return fail(h, RBPF_EINVAL, "min_size >= 1 and 1 <= max_regions <= 1024 are required");
    if (box4[1] <= box4[0] || box4[3] <= box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 > x0 and y1 > y0");
    const long long nx = (long long)box4[1] - box4[0], ny = (long long)box4[3] - box4[2], ncell = nx * ny;
    if (nx > 32768 || ny > 32768 || ncell > (1LL << 27)) return fail(h, RBPF_EINVAL, "box must be at most 32768 cells on a side and hold at most 2^27 cells");
    if (!box_in_lattice(v, box4)) return fail(h, RBPF_EINVAL, "box leaves the tile lattice");
    MID_STEP_TRY(h, "frontier regions");

    FrontierArgs a;
    a.x0 = box4[0]; a.y0 = box4[2]; a.nx = (int)nx; a.ny = (int)ny;
    a.nbx = (int)((nx + 63) / 64); a.nby = (int)((ny + 63) / 64);
    a.clear = clear; a.min_size = min_size; a.max_regions = max_regions;
    const bool dev_out = (flags & RBPF_FRONTIER_DEVICE_OUT) != 0, table = regions || counts;
    const int np_all = all ? v.P : 1;
    const long long nblk = (long long)a.nbx * a.nby;
    a.cw = a.nby * 64 + 2;
    const size_t lab_b = pad256((size_t)(a.nbx * 64LL + 2) * a.cw * 4), dirty_b = pad256((size_t)nblk);
    const size_t per = lab_b * (table ? 2 : 1) + 2 * dirty_b;
    const size_t counts_b = pad256((size_t)np_all * 12), table_b = table ? pad256((size_t)np_all * max_regions * 80) : 0;
    const size_t label_b = label && !dev_out ? pad256((size_t)ncell * 4) : 0;
    const size_t fixed = 256 + counts_b + table_b + label_b;
    if (fixed + per > RELAX_SCRATCH) return fail(h, RBPF_ENOMEM, "one particle's frontier regions over this box need more than 2 GiB of scratch: use a smaller box");
    const long long batch = relax_batch(np_all, fixed, per, "RBPF_FRONTIER_BATCH");
    HIP_TRY(h, h->reserve(B_FRONTIER, fixed + (size_t)batch * per));
    const Block& d = h->buf[B_FRONTIER];
    Staging& st = h->stage[S_FRONTIER];
    HIP_TRY(h, st.begin(256));
    int32_t* d_count = d.as<int32_t>();
    // the counts and the table are written where they are wanted when that is device memory, else into scratch and copied
    int32_t* o_counts = dev_out && counts ? counts : d.as<int32_t>(256);
    unsigned long long* o_table = !table ? nullptr : dev_out && regions ? reinterpret_cast<unsigned long long*>(regions) : d.as<unsigned long long>(256 + counts_b);
    a.label_out = !label ? nullptr : dev_out ? label : d.as<int32_t>(256 + counts_b + table_b);
    unsigned char* work = d.p + fixed;
    HIP_TRY(h, hipMemsetAsync(o_counts, 0, (size_t)np_all * 12, h->stream));
    long long launched = 0, runs = 0;
    for (long long p0 = 0; p0 < np_all; p0 += batch) {
        const long long nb = std::min<long long>(batch, np_all - p0);
        a.particle = all ? (int)p0 : particle; a.n_part = (int)nb;
        a.ras = reinterpret_cast<int32_t*>(work); a.ras_stride = (long long)(lab_b / 4);
        a.aux = table ? reinterpret_cast<int32_t*>(work + (size_t)nb * lab_b) : nullptr;
        a.dirty = work + (size_t)nb * lab_b * (table ? 2 : 1);
        a.counts = o_counts + 3 * (size_t)p0;
        a.table = table ? o_table + (size_t)p0 * max_regions * 10 : nullptr;
        HIP_TRY(h, hipMemsetAsync(a.ras, 0x7f, (size_t)nb * lab_b, h->stream));           // FRONTIER_NONE everywhere
        HIP_TRY(h, hipMemsetAsync(work + (size_t)nb * lab_b, 0, (size_t)nb * (per - lab_b), h->stream));   // sizes and dirty flags
        launch_frontier_mask(v, a, h->stream);
        HIP_TRY(h, hipGetLastError());
        // dirty flags: [2][nb][nblk] packed without the padding of dirty_b
        if (int rc = relax_rounds(h, st, d_count, ncell + 1, TRAVEL_ROUNDS_PER_READ, "internal error: the frontier labels did not converge",
                                  [&](long long r, int32_t* c) { launch_frontier_round(a, (int)(r & 1), c, h->stream); }, launched, runs)) return rc;
        launch_frontier_output(a, h->stream);
        HIP_TRY(h, hipGetLastError());
    }
    relax_stats(h->frontier_stats, launched, runs, nblk * np_all);
    if (dev_out) return RBPF_OK;
    if (label) HIP_TRY(h, hipMemcpyAsync(label, a.label_out, (size_t)ncell * 4, hipMemcpyDeviceToHost, h->stream));
    if (regions) HIP_TRY(h, hipMemcpyAsync(regions, o_table, (size_t)np_all * max_regions * 80, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIP_TRY(h, hipMemcpyAsync(counts, o_counts, (size_t)np_all * 12, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

int rbpf_frontier_stats(rbpf_handle* h, uint64_t* out3) {
    if (!h) return RBPF_EINVAL;
    if (!out3) return fail(h, RBPF_EINVAL, "out3 is NULL");
    for (int k = 0; k < 3; ++k) out3[k] = h->frontier_stats[k];
    return RBPF_OK;
}

// ---- map scores (kernels_score.hip) -------------------------------------------------------------------------------------------
int rbpf_score_maps(rbpf_handle* h, int32_t particle, const int32_t* box4, const int8_t* ref, int32_t tol, const int32_t* value_tab,
                    uint32_t flags, int64_t* scores) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!box4 || !ref || !scores) return fail(h, RBPF_EINVAL, "box4, ref or scores is NULL");
    if (flags & ~(RBPF_SCORE_DEVICE_IN | RBPF_SCORE_DEVICE_OUT)) return fail(h, RBPF_EINVAL, "unknown flags");
    if (particle < -1 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    if (tol < 0 || tol > 16) return fail(h, RBPF_EINVAL, "0 <= tol <= 16 is required");
    if (box4[1] <= box4[0] || box4[3] <= box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 > x0 and y1 > y0");
    const long long nx = (long long)box4[1] - box4[0], ny = (long long)box4[3] - box4[2], ncell = nx * ny;
    if (ncell > (1LL << 27)) return fail(h, RBPF_EINVAL, "box must hold at most 2^27 cells");
    if (!box_in_lattice(v, box4)) return fail(h, RBPF_EINVAL, "box leaves the tile lattice");
    const int nv = v.cc.vmax - v.cc.vmin + 1;                              // one entry per lattice value
    if (v.cc.vmin > 0 || v.cc.vmax < 0 || nv > 256) return fail(h, RBPF_EINVAL, "the lattice values must include 0");
    if (value_tab)
        for (int k = 0; k < nv; ++k)
            if (value_tab[k] < 0 || value_tab[k] > (1 << 20)) return fail(h, RBPF_EINVAL, "value_tab entries must lie in 0 .. 2^20");
    const bool dev_in = (flags & RBPF_SCORE_DEVICE_IN) != 0, dev_out = (flags & RBPF_SCORE_DEVICE_OUT) != 0;
    if (!dev_in)
        for (long long i = 0; i < ncell; ++i)
            if (ref[i] < v.cc.vmin || ref[i] > v.cc.vmax) return fail(h, RBPF_EINVAL, "reference value outside [min_odds_emp, max_odds_occ]");
    MID_STEP_TRY(h, "map scores");

    ScoreArgs a;
    a.x0 = box4[0]; a.y0 = box4[2]; a.nx = (int)nx; a.ny = (int)ny;
    a.nbx = (int)((nx + 63) / 64); a.nby = (int)((ny + 63) / 64);
    a.tol = tol; a.validate = dev_in;
    const int np_all = particle < 0 ? v.P : 1;
    const size_t nblk = (size_t)a.nbx * a.nby;
    // scratch: [flag] [table] [host reference] | [near rows] [block sums] [host scores]; the first three are one upload
    const size_t tab_b = pad256((size_t)nv * 4), ref_b = dev_in ? 0 : pad256((size_t)ncell), in_b = 256 + tab_b + ref_b;
    const size_t near_b = pad256(nblk * BR_EDGE * 8), sums_b = pad256(nblk * 16), out_n = (size_t)np_all * SCORE_FIELDS * 8;
    HIP_TRY(h, h->reserve(B_SCORE, in_b + near_b + sums_b + (dev_out ? 0 : pad256(out_n))));
    const Block& d = h->buf[B_SCORE];
    Staging& st = h->stage[S_SCORE];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    memset(st.p, 0, 256 + tab_b);
    if (value_tab) memcpy(st.p + 256, value_tab, (size_t)nv * 4);
    if (!dev_in) memcpy(st.p + 256 + tab_b, ref, (size_t)ncell);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    a.bad = d.as<int32_t>();
    a.table = value_tab ? d.as<const int32_t>(256) : nullptr;
    a.ref = dev_in ? ref : d.as<const int8_t>(256 + tab_b);
    a.near_r = d.as<unsigned long long>(in_b);
    a.ref_sums = d.as<int32_t>(in_b + near_b);
    long long* o_scores = dev_out ? reinterpret_cast<long long*>(scores) : d.as<long long>(in_b + near_b + sums_b);
    launch_score_ref(v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    if (dev_in) {                                                          // the verdict, before anything is written
        int32_t bad = 0;
        HIP_TRY(h, hipMemcpyAsync(&bad, a.bad, 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (bad) return fail(h, RBPF_EINVAL, "reference value outside [min_odds_emp, max_odds_occ]");
    }
    HIP_TRY(h, hipMemsetAsync(o_scores, 0, out_n, h->stream));
    for (int p0 = 0; p0 < np_all; p0 += 65535) {                           // gridDim.y
        a.particle = particle < 0 ? p0 : particle; a.n_part = std::min(65535, np_all - p0);
        a.scores = o_scores + (size_t)p0 * SCORE_FIELDS;
        launch_score_maps(v, a, h->stream);
    }
    HIP_TRY(h, hipGetLastError());
    if (dev_out) return RBPF_OK;
    HIP_TRY(h, hipMemcpyAsync(scores, o_scores, out_n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

}  // extern "C"

// ---- pose estimate and trajectory log (kernels_track.hip) -------------------------------------------------------
static int check_weights_mode(rbpf_handle* h, int32_t mode, const double* weights) {
    if (mode != RBPF_W_UNIFORM && mode != RBPF_W_RESAMPLE && mode != RBPF_W_GIVEN) return fail(h, RBPF_EINVAL, "unknown weights_mode");
    if ((mode == RBPF_W_GIVEN) != (weights != nullptr)) return fail(h, RBPF_EINVAL, "weights go with RBPF_W_GIVEN, and only with it");
    if (weights)
        for (int j = 0; j < h->v.P; ++j)
            if (weights[j] < 0) return fail(h, RBPF_EINVAL, "a given weight is negative");
    return RBPF_OK;
}

static int track_state_and_range(rbpf_handle* h, int32_t t0, int32_t t1) {
    if (!h->track_on) return fail(h, RBPF_ESTATE, "tracking is off: rbpf_track_begin first");
    if (t0 < 0 || t0 >= t1 || t1 > h->track_n) return fail(h, RBPF_EINVAL, "0 <= t0 < t1 <= n_records is required");
    return RBPF_OK;
}

// scratch of a walk over [t0, n_records): comp and start, rows counted from the chunk of t0
static size_t track_walk_bytes(const rbpf_handle* h, int t0, int n) {
    const size_t chunks = (size_t)((h->track_n - 1) / RBPF_TRACK_CHUNK - t0 / RBPF_TRACK_CHUNK + 1);
    return pad256(chunks * h->v.P * 4) + pad256(chunks * (size_t)n * 4);
}

// queues the three stages; the scratch of track_walk_bytes starts at B_TRACK + off
static int track_walk(rbpf_handle* h, int t0, int t1, const int32_t* d_particles, int n, size_t off, int32_t* d_idx, double* d_pose) {
    TrackWalk q;
    q.g = h->track_log();
    q.t0 = t0; q.t1 = t1; q.N = h->track_n;
    q.c0 = t0 / RBPF_TRACK_CHUNK; q.c1 = (h->track_n - 1) / RBPF_TRACK_CHUNK;
    q.n = n; q.particles = d_particles; q.pending = h->track_pending(h->track_cur);
    q.comp = h->buf[B_TRACK].as<int32_t>(off);
    q.start = h->buf[B_TRACK].as<int32_t>(off + pad256((size_t)(q.c1 - q.c0 + 1) * h->v.P * 4));
    q.out_idx = d_idx; q.out_pose = d_pose;
    launch_track_walk(q, h->stream);
    HIP_TRY(h, hipGetLastError());
    return RBPF_OK;
}

extern "C" {

int rbpf_estimate(rbpf_handle* h, int32_t mode, const double* weights, double* out16, int32_t* out4) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!out16 || !out4) return fail(h, RBPF_EINVAL, "out16 or out4 is NULL");
    int rc = check_weights_mode(h, mode, weights);
    if (rc) return rc;
    const size_t w_b = pad256((size_t)h->v.P * 8);
    HIP_TRY(h, h->reserve(B_TRACK, w_b + 256));
    const Block& d = h->buf[B_TRACK];
    if (weights) {
        Staging& st = h->stage[S_TRACK];
        HIP_TRY(h, st.begin(w_b));
        memcpy(st.p, weights, (size_t)h->v.P * 8);
        HIP_TRY(h, st.upload(d.p, (size_t)h->v.P * 8, h->stream));
    }
    launch_estimate(h->v, weights ? d.as<const double>() : nullptr, mode, d.as<double>(w_b), d.as<int32_t>(w_b + RBPF_EST_F64 * 8), h->stream);
    HIP_TRY(h, hipGetLastError());
    unsigned char row[RBPF_EST_F64 * 8 + RBPF_EST_I32 * 4];
    HIP_TRY(h, hipMemcpyAsync(row, d.p + w_b, sizeof(row), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memcpy(out16, row, RBPF_EST_F64 * 8);
    memcpy(out4, row + RBPF_EST_F64 * 8, RBPF_EST_I32 * 4);
    return RBPF_OK;
}

int rbpf_track_begin(rbpf_handle* h, int32_t capacity, uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (h->track_on) return fail(h, RBPF_ESTATE, "tracking is already on");
    if (capacity < 1 || capacity > 65535 * RBPF_TRACK_CHUNK) return fail(h, RBPF_EINVAL, "1 <= capacity <= 65535 * RBPF_TRACK_CHUNK is required");
    if (flags & ~(RBPF_TRACK_IMU | RBPF_TRACK_SCAN)) return fail(h, RBPF_EINVAL, "unknown flags");
    const size_t P = h->v.P, stride = track_record_stride(h->v.P);
    if (h->track_mem[rbpf_handle::T_LOG].reserve((size_t)capacity * stride) != hipSuccess ||
        h->track_mem[rbpf_handle::T_PENDING].reserve(2 * P * 4) != hipSuccess) {
        (void)hipGetLastError();
        for (Block& b : h->track_mem) b.release();
        return fail(h, RBPF_ENOMEM, "no device memory for " + std::to_string(capacity) + " records of " + std::to_string(stride) + " bytes");
    }
    std::vector<int32_t> id(P);
    for (size_t j = 0; j < P; ++j) id[j] = (int32_t)j;
    HIP_TRY(h, hipMemcpyAsync(h->track_pending(0), id.data(), P * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));           // id dies on return
    h->track_on = true; h->track_flags = flags; h->track_cap = capacity; h->track_n = 0; h->track_dropped = 0; h->track_cur = 0;
    return track_record(h, false);
}

int rbpf_track_end(rbpf_handle* h) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->track_on) return fail(h, RBPF_ESTATE, "tracking is off: rbpf_track_begin first");
    HIP_TRY(h, hipStreamSynchronize(h->stream));           // queued records and walks still use the log
    for (Block& b : h->track_mem) b.release();
    h->track_on = false; h->track_flags = 0; h->track_cap = h->track_n = h->track_dropped = h->track_cur = 0;
    return RBPF_OK;
}

int rbpf_track_record(rbpf_handle* h) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->track_on) return fail(h, RBPF_ESTATE, "tracking is off: rbpf_track_begin first");
    return track_record(h, false);
}

int rbpf_track_info(rbpf_handle* h, int32_t* n_records, int32_t* capacity, int32_t* dropped, uint32_t* flags) {
    if (!h) return RBPF_EINVAL;
    if (!h->track_on) return fail(h, RBPF_ESTATE, "tracking is off: rbpf_track_begin first");
    if (n_records) *n_records = h->track_n;
    if (capacity) *capacity = h->track_cap;
    if (dropped) *dropped = h->track_dropped;
    if (flags) *flags = h->track_flags;
    return RBPF_OK;
}

int rbpf_track_lineage(rbpf_handle* h, int32_t t0, int32_t t1, const int32_t* particles, int32_t n, void* out_idx, void* out_pose,
                       uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    int rc = track_state_and_range(h, t0, t1);
    if (rc) return rc;
    const int P = h->v.P;
    if (flags & ~RBPF_TRACK_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    if (!out_idx && !out_pose) return fail(h, RBPF_EINVAL, "out_idx and out_pose are both NULL");
    if (particles ? n < 1 : n != 0) return fail(h, RBPF_EINVAL, "particles needs n >= 1; NULL goes with n = 0 (all particles)");
    for (int k = 0; k < n; ++k)
        if (particles[k] < 0 || particles[k] >= P) return fail(h, RBPF_EINVAL, "particle index out of range");
    if (!particles) n = P;
    const bool dev_out = (flags & RBPF_TRACK_DEVICE_OUT) != 0;
    const size_t T = (size_t)(t1 - t0), list_b = particles ? pad256((size_t)n * 4) : 0, walk_b = track_walk_bytes(h, t0, n);
    const size_t idx_n = T * n * 4, pose_n = T * n * 24;
    const size_t idx_b = (out_idx && !dev_out) ? pad256(idx_n) : 0, pose_b = (out_pose && !dev_out) ? pad256(pose_n) : 0;
    HIP_TRY(h, h->reserve(B_TRACK, list_b + walk_b + idx_b + pose_b));
    const Block& d = h->buf[B_TRACK];
    if (particles) {
        Staging& st = h->stage[S_TRACK];
        HIP_TRY(h, st.begin(list_b));
        memcpy(st.p, particles, (size_t)n * 4);
        HIP_TRY(h, st.upload(d.p, (size_t)n * 4, h->stream));
    }
    int32_t* d_idx = !out_idx ? nullptr : dev_out ? static_cast<int32_t*>(out_idx) : d.as<int32_t>(list_b + walk_b);
    double* d_pose = !out_pose ? nullptr : dev_out ? static_cast<double*>(out_pose) : d.as<double>(list_b + walk_b + idx_b);
    rc = track_walk(h, t0, t1, particles ? d.as<const int32_t>() : nullptr, n, list_b, d_idx, d_pose);
    if (rc || dev_out) return rc;
    if (out_idx) HIP_TRY(h, hipMemcpyAsync(out_idx, d_idx, idx_n, hipMemcpyDeviceToHost, h->stream));
    if (out_pose) HIP_TRY(h, hipMemcpyAsync(out_pose, d_pose, pose_n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

int rbpf_track_summary(rbpf_handle* h, int32_t t0, int32_t t1, int32_t mode, const double* weights, double* out_f64, int32_t* out_i32) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    int rc = track_state_and_range(h, t0, t1);
    if (rc) return rc;
    const int P = h->v.P;
    if (P > TRACK_SUMMARY_MAX_P) return fail(h, RBPF_EINVAL, "rbpf_track_summary needs P <= 65536");
    if ((rc = check_weights_mode(h, mode, weights))) return rc;
    const size_t T = (size_t)(t1 - t0), w_b = weights ? pad256((size_t)P * 8) : 0, walk_b = track_walk_bytes(h, t0, P);
    const size_t lin_b = pad256(T * P * 4), f_n = T * RBPF_EST_F64 * 8, i_n = T * RBPF_EST_I32 * 4;
    HIP_TRY(h, h->reserve(B_TRACK, w_b + walk_b + lin_b + pad256(f_n) + i_n));
    const Block& d = h->buf[B_TRACK];
    if (weights) {
        Staging& st = h->stage[S_TRACK];
        HIP_TRY(h, st.begin(w_b));
        memcpy(st.p, weights, (size_t)P * 8);
        HIP_TRY(h, st.upload(d.p, (size_t)P * 8, h->stream));
    }
    int32_t* d_lin = d.as<int32_t>(w_b + walk_b);
    double* d_f = d.as<double>(w_b + walk_b + lin_b);
    int32_t* d_i = d.as<int32_t>(w_b + walk_b + lin_b + pad256(f_n));
    if ((rc = track_walk(h, t0, t1, nullptr, P, w_b, d_lin, nullptr))) return rc;
    launch_track_summary(h->track_log(), t0, t1, d_lin, h->v.weight, weights ? d.as<const double>() : nullptr, mode, d_f, d_i, h->stream);
    HIP_TRY(h, hipGetLastError());
    if (out_f64) HIP_TRY(h, hipMemcpyAsync(out_f64, d_f, f_n, hipMemcpyDeviceToHost, h->stream));
    if (out_i32) HIP_TRY(h, hipMemcpyAsync(out_i32, d_i, i_n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

}  // extern "C"

// ---- pose modes (kernels_modes.hip) ------------------------------------------------------------------------------
static const size_t MODES_SLAB_BYTES = (size_t)256 << 20;    // lineage rows and tables of the records rbpf_track_modes has in flight

// the checks the two entry points share, in the order of the header; fills what the kernel needs but the pointers
static int modes_args(rbpf_handle* h, int32_t mode, const double* weights, double bin_xy, int32_t n_th, int32_t max_modes, ModesArgs& a) {
    if (h->v.P > MODES_MAX_P) return fail(h, RBPF_EINVAL, "pose modes need P <= 65536");
    const int rc = check_weights_mode(h, mode, weights);
    if (rc) return rc;
    if (weights)
        for (int j = 0; j < h->v.P; ++j)
            if (!std::isfinite(weights[j])) return fail(h, RBPF_EINVAL, "a given weight is not finite");
    if (!std::isfinite(bin_xy) || !(bin_xy > 0)) return fail(h, RBPF_EINVAL, "bin_xy must be finite and > 0");
    if (n_th < 1 || n_th > 4096) return fail(h, RBPF_EINVAL, "1 <= n_th <= 4096 is required");
    if (max_modes < 1 || max_modes > RBPF_MODES_MAX) return fail(h, RBPF_EINVAL, "1 <= max_modes <= RBPF_MODES_MAX is required");
    a.P = h->v.P; a.S = modes_slots(a.P);
    a.n_th = n_th; a.K = max_modes; a.mode = mode;
    a.inv = 1.0 / bin_xy; a.kth = (double)n_th / 6.283185307179586;
    a.w_raw = h->v.weight; a.w_given = nullptr; a.label = nullptr;
    return RBPF_OK;
}

static int modes_upload_weights(rbpf_handle* h, const double* weights) {
    Staging& st = h->stage[S_TRACK];
    HIP_TRY(h, st.begin((size_t)h->v.P * 8));
    memcpy(st.p, weights, (size_t)h->v.P * 8);
    HIP_TRY(h, st.upload(h->buf[B_TRACK].p, (size_t)h->v.P * 8, h->stream));
    return RBPF_OK;
}

extern "C" {

int rbpf_pose_modes(rbpf_handle* h, int32_t mode, const double* weights, double bin_xy, int32_t n_th, int32_t max_modes, uint32_t flags,
                    int64_t* info4, double* rows_f64, int32_t* rows_i32, int32_t* label) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!info4) return fail(h, RBPF_EINVAL, "info4 is NULL");
    if (!rows_f64 != !rows_i32) return fail(h, RBPF_EINVAL, "rows_f64 and rows_i32 are both given or both NULL");
    if (flags & ~RBPF_MODES_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    ModesArgs a;
    int rc = modes_args(h, mode, weights, bin_xy, n_th, max_modes, a);
    if (rc) return rc;
    const bool dev_out = (flags & RBPF_MODES_DEVICE_OUT) != 0;
    const size_t P = (size_t)a.P, K = (size_t)a.K;
    const size_t w_b = weights ? pad256(P * 8) : 0, tab_b = modes_set_bytes(a.P, a.S);
    const size_t f_n = K * RBPF_EST_F64 * 8, i_n = K * RBPF_EST_I32 * 4;
    const size_t out_b = dev_out ? 0 : 256 + pad256(f_n) + pad256(i_n);
    HIP_TRY(h, h->reserve(B_TRACK, w_b + tab_b + out_b));
    const Block& d = h->buf[B_TRACK];
    if (weights && (rc = modes_upload_weights(h, weights))) return rc;
    a.w_given = weights ? d.as<const double>() : nullptr;
    a.tables = d.p + w_b;
    const size_t at = w_b + tab_b;
    a.info = dev_out ? reinterpret_cast<long long*>(info4) : d.as<long long>(at);
    a.rows_f = !rows_f64 ? nullptr : dev_out ? rows_f64 : d.as<double>(at + 256);
    a.rows_i = !rows_i32 ? nullptr : dev_out ? rows_i32 : d.as<int32_t>(at + 256 + pad256(f_n));
    a.label = dev_out ? label : nullptr;
    launch_pose_modes(h->v, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    if (dev_out) return RBPF_OK;
    return fetch(h, {{info4, a.info, 32}, {rows_f64, a.rows_f, f_n}, {rows_i32, a.rows_i, i_n},
                     {label, a.tables + modes_label_offset(a.P, a.S), P * 4}});
}

int rbpf_track_modes(rbpf_handle* h, int32_t t0, int32_t t1, int32_t mode, const double* weights, double bin_xy, int32_t n_th,
                     int32_t max_modes, int64_t* info, double* rows_f64, int32_t* rows_i32) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    int rc = track_state_and_range(h, t0, t1);
    if (rc) return rc;
    if (!info && !rows_f64 && !rows_i32) return fail(h, RBPF_EINVAL, "info, rows_f64 and rows_i32 are all NULL");
    ModesArgs a;
    if ((rc = modes_args(h, mode, weights, bin_xy, n_th, max_modes, a))) return rc;
    const size_t P = (size_t)a.P, K = (size_t)a.K, T = (size_t)(t1 - t0);
    const size_t tab_b = modes_set_bytes(a.P, a.S), lin_row = P * 4;
    size_t budget = MODES_SLAB_BYTES;
    if (const char* env = getenv("RBPF_MODES_SLAB_BYTES")) {                                     // tests: several slabs on a short log
        const long long v = atoll(env);
        if (v > 0) budget = std::min(budget, (size_t)v);
    }
    const size_t slab = std::max<size_t>(1, std::min(T, budget / (tab_b + lin_row)));            // records in flight
    const size_t w_b = weights ? pad256(P * 8) : 0, walk_b = track_walk_bytes(h, t0, a.P), lin_b = pad256(slab * lin_row);
    const size_t info_b = pad256(slab * 32), f_b = pad256(slab * K * RBPF_EST_F64 * 8), i_b = pad256(slab * K * RBPF_EST_I32 * 4);
    HIP_TRY(h, h->reserve(B_TRACK, w_b + walk_b + lin_b + slab * tab_b + info_b + f_b + i_b));
    const Block& d = h->buf[B_TRACK];
    if (weights && (rc = modes_upload_weights(h, weights))) return rc;
    a.w_given = weights ? d.as<const double>() : nullptr;
    int32_t* d_lin = d.as<int32_t>(w_b + walk_b);
    size_t at = w_b + walk_b + lin_b;
    a.tables = d.p + at; at += slab * tab_b;
    a.info = d.as<long long>(at); at += info_b;
    a.rows_f = d.as<double>(at); at += f_b;
    a.rows_i = d.as<int32_t>(at);
    for (size_t r0 = 0; r0 < T; r0 += slab) {              // a slab's outputs leave in stream order before the next slab overwrites them
        const size_t n = std::min(slab, T - r0);
        const int a0 = t0 + (int)r0;
        if ((rc = track_walk(h, a0, a0 + (int)n, nullptr, a.P, w_b, d_lin, nullptr))) return rc;
        launch_track_modes(h->track_log(), a0, (int)n, d_lin, a, h->stream);
        HIP_TRY(h, hipGetLastError());
        if (info) HIP_TRY(h, hipMemcpyAsync(info + r0 * 4, a.info, n * 32, hipMemcpyDeviceToHost, h->stream));
        if (rows_f64) HIP_TRY(h, hipMemcpyAsync(rows_f64 + r0 * K * RBPF_EST_F64, a.rows_f, n * K * RBPF_EST_F64 * 8, hipMemcpyDeviceToHost, h->stream));
        if (rows_i32) HIP_TRY(h, hipMemcpyAsync(rows_i32 + r0 * K * RBPF_EST_I32, a.rows_i, n * K * RBPF_EST_I32 * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

int rbpf_track_filtered(rbpf_handle* h, int32_t t0, int32_t t1, double* out_f64, int32_t* out_i32) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const int rc = track_state_and_range(h, t0, t1);
    if (rc) return rc;
    const TrackLog g = h->track_log();
    const unsigned char* first = g.base + (size_t)t0 * g.stride;
    const size_t T = (size_t)(t1 - t0), fw = RBPF_EST_F64 * 8, iw = RBPF_EST_I32 * 4;
    if (out_f64) HIP_TRY(h, hipMemcpy2DAsync(out_f64, fw, first + (size_t)g.P * 24, g.stride, fw, T, hipMemcpyDeviceToHost, h->stream));
    if (out_i32) HIP_TRY(h, hipMemcpy2DAsync(out_i32, iw, first + track_parent_offset(g.P) + (size_t)g.P * 4, g.stride, iw, T, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

int64_t rbpf_track_record_bytes(rbpf_handle* h) { return h ? (int64_t)track_record_stride(h->v.P) : -1; }

int rbpf_track_export(rbpf_handle* h, int32_t t0, int32_t t1, void* records) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->track_on) return fail(h, RBPF_ESTATE, "tracking is off: rbpf_track_begin first");
    if (!records || t0 < 0 || t0 > t1 || t1 > h->track_n) return fail(h, RBPF_EINVAL, "records is NULL, or not 0 <= t0 <= t1 <= n_records");
    const TrackLog g = h->track_log();
    const size_t bytes = (size_t)(t1 - t0) * g.stride;
    if (bytes) HIP_TRY(h, hipMemcpyAsync(records, g.base + (size_t)t0 * g.stride, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(static_cast<unsigned char*>(records) + bytes, h->track_pending(h->track_cur), (size_t)g.P * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RBPF_OK;
}

int rbpf_track_import(rbpf_handle* h, int32_t n, const void* records) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!h->track_on) return fail(h, RBPF_ESTATE, "tracking is off: rbpf_track_begin first");
    if (!records || n < 1 || n > h->track_cap) return fail(h, RBPF_EINVAL, "records is NULL, or not 1 <= n <= capacity");
    const TrackLog g = h->track_log();
    const unsigned char* src = static_cast<const unsigned char*>(records);
    const size_t bytes = (size_t)n * g.stride, P = (size_t)g.P;
    for (int t = 0; t <= n; ++t) {                         // the parents of every record, then the pending map: the walk gathers through them
        int32_t k[64];
        const unsigned char* row = t < n ? src + (size_t)t * g.stride + track_parent_offset(g.P) : src + bytes;
        for (size_t j = 0; j < P; j += 64) {
            const size_t m = std::min<size_t>(64, P - j);
            memcpy(k, row + j * 4, m * 4);
            for (size_t i = 0; i < m; ++i)
                if (k[i] < 0 || k[i] >= g.P) return fail(h, RBPF_EINVAL, "a parent or pending index lies outside 0 .. P-1");
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(g.base, src, bytes, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->track_pending(h->track_cur), src + bytes, P * 4, hipMemcpyHostToDevice));
    h->track_n = n;
    return RBPF_OK;
}

// ---- map building (kernels_build.hip) -----------------------------------------------------------------------------
int rbpf_build_map(rbpf_handle* h, const double* poses_n3, int32_t n_scans, const double* ranges, const double* angles,
                   int32_t n_beams, double cells_per_m, const int32_t* box4, double min_range, double max_range,
                   uint32_t flags, int32_t* hits, int32_t* seen) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!poses_n3 || !ranges || !angles || !box4) return fail(h, RBPF_EINVAL, "poses, ranges, angles or box4 is NULL");
    if (!hits && !seen) return fail(h, RBPF_EINVAL, "hits and seen are both NULL");
    if (flags & ~(RBPF_BUILD_DEVICE_OUT | RBPF_BUILD_ACCUMULATE)) return fail(h, RBPF_EINVAL, "unknown flags");
    ARG_TRY(h, check_counts(n_scans, 1, n_beams, 0, "n_scans >= 1, n_beams >= 1 and n_scans * n_beams < 2^31 are required"));
    if (box4[1] <= box4[0] || box4[3] <= box4[2]) return fail(h, RBPF_EINVAL, "box must have x1 > x0 and y1 > y0");
    const long long nx = (long long)box4[1] - box4[0], ny = (long long)box4[3] - box4[2];
    if (nx > INT32_MAX || ny > INT32_MAX || nx > (1LL << 31) / ny)
        return fail(h, RBPF_EINVAL, "box must hold at most 2^31 cells, in fewer than 2^31 rows and columns");
    const long long ncell = nx * ny;
    if (!std::isfinite(cells_per_m) || !(cells_per_m > 0.0)) return fail(h, RBPF_EINVAL, "cells_per_m must be finite and > 0");
    ARG_TRY(h, check_ranges(max_range, min_range));
    ARG_TRY(h, check_poses(poses_n3, n_scans));
    ARG_TRY(h, check_angles(angles, n_beams));
    BuildArgs a;
    a.inv = cells_per_m;
    a.tlim = max_range * a.inv;
    const double reach = ceil(a.tlim) + 2.0;                               // no cell of a scan lies farther from the origin cell on either axis
    if (!(2.0 * reach + 1.0 <= 1024.0))
        return fail(h, RBPF_EINVAL, "max_range " + std::to_string(max_range) + " m needs a window of more than 1024 cells: the largest admissible "
                                    "max_range is " + std::to_string(509.0 / a.inv) + " m (ceil(max_range * cells per metre) <= 509)");
    MID_STEP_TRY(h, "map building");
    a.M = (int)reach; a.W = (2 * a.M + 1 + 31) / 32 + 1;
    a.x0 = box4[0]; a.y0 = box4[2]; a.nx = (int)nx; a.ny = (int)ny;
    a.min_range = min_range; a.max_range = max_range;
    a.n_scans = n_scans; a.B = n_beams;
    const bool dev_out = (flags & RBPF_BUILD_DEVICE_OUT) != 0, accumulate = (flags & RBPF_BUILD_ACCUMULATE) != 0;
    const size_t nray = (size_t)n_scans * n_beams, out_b = (size_t)ncell * 4;
    Carve c;                                                               // scratch: [poses] [beams] [ranges] | [end cells] [host hits] [host seen]
    const size_t pose_at = c.pack((size_t)n_scans * 32), beam_at = c.pack((size_t)n_beams * 16), range_at = c.pack(nray * 8), in_b = c.close();
    const size_t ends_at = c.take(nray * 4), hits_at = c.take(dev_out || !hits ? 0 : out_b), seen_at = c.take(dev_out || !seen ? 0 : out_b);
    if (c.total() > ((size_t)4 << 30)) return fail(h, RBPF_ENOMEM, "scans and box need more than 4 GiB of scratch: build fewer scans per call (RBPF_BUILD_ACCUMULATE) or a smaller box");
    HIP_TRY(h, h->reserve(B_BUILD, c.total()));
    const Block& d = h->buf[B_BUILD];
    Staging& st = h->stage[S_BUILD];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    memcpy(stage_beam2(stage_pose4(st.as<double>(), poses_n3, n_scans), angles, n_beams), ranges, nray * 8);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    a.pose4 = d.as<const double>(pose_at);
    a.beam2 = d.as<const double>(beam_at);
    a.ranges = d.as<const double>(range_at);
    a.ends = d.as<uint32_t>(ends_at);
    a.hits = !hits ? nullptr : dev_out ? hits : d.as<int32_t>(hits_at);
    a.seen = !seen ? nullptr : dev_out ? seen : d.as<int32_t>(seen_at);
    int32_t* const host_out[2] = {hits, seen};
    int32_t* const dev[2] = {a.hits, a.seen};
    for (int k = 0; k < 2; ++k) {
        if (!dev[k]) continue;
        if (!accumulate) HIP_TRY(h, hipMemsetAsync(dev[k], 0, (size_t)ncell * 4, h->stream));
        else if (!dev_out) HIP_TRY(h, hipMemcpyAsync(dev[k], host_out[k], (size_t)ncell * 4, hipMemcpyHostToDevice, h->stream));   // read before the return below
    }
    launch_build_map(a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{hits, a.hits, out_b}, {seen, a.seen, out_b}});
}

// ---- scan-to-map refinement (kernels_refine.hip) -------------------------------------------------------------------
static const size_t REFINE_LDS_LIMIT = 160 * 1024 - 64;                    // dynamic LDS of the search kernel: 160 KiB less its statics
// rotations whose tasks fit one workgroup: its lanes over the tasks of one rotation (search_kpw)
static int refine_fit(int substeps, int n_trans) { const int nw = 2 * n_trans + 1; return REFINE_BLOCK / (nw * refine_runs(nw, search_shift(substeps))); }

int32_t rbpf_refine_max_reach(int32_t substeps, int32_t n_trans) {
    if (!search_substeps_ok(substeps) || n_trans < 0 || n_trans > 32) return -1;
    const int extra = (n_trans + substeps - 1) / substeps + 2;
    int reach = -1;                                                        // the LDS need grows with Mw: the first failure ends the search
    for (int c = 0; refine_lds_bytes(c + extra, refine_row_words(c + extra)) <= REFINE_LDS_LIMIT; ++c) reach = c;
    return reach;
}

// the window limit's message: the largest max_range with ceil(max_range * inv) <= max_reach
static std::string refine_window_message(double max_range, double inv, int max_reach) {
    double most = (double)max_reach / inv;
    if (ceil(most * inv) > (double)max_reach) most = nextafter(most, 0.0);
    char num[32];
    snprintf(num, sizeof num, "%.17g", most);
    return "max_range " + std::to_string(max_range) + " m needs a window that does not fit one workgroup's LDS: the largest "
           "admissible max_range is " + num + " m (ceil(max_range * cells per metre) <= " + std::to_string(max_reach) + ")";
}

int rbpf_refine_poses(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_scans, const double* ranges,
                      const double* angles, int32_t n_beams, double min_range, double max_range, int32_t substeps, int32_t n_trans,
                      int32_t n_rot, double rot_step, double* out_pose_n3, int32_t* out_n6, int32_t* scores, uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    const DevView& v = h->v;
    if (!poses_n3 || !ranges || !angles) return fail(h, RBPF_EINVAL, "poses, ranges or angles is NULL");
    if (!out_pose_n3 && !out_n6) return fail(h, RBPF_EINVAL, "out_pose_n3 and out_n6 are both NULL");
    if (flags & ~RBPF_REFINE_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    ARG_TRY(h, check_counts(n_scans, 1, n_beams, 16384, "n_scans >= 1, 1 <= n_beams <= 16384 and n_scans * n_beams < 2^31 are required"));
    if (particle < 0 || particle >= v.P) return fail(h, RBPF_EINVAL, "particle index out of range");
    ARG_TRY(h, check_search(substeps, n_trans, n_rot));
    ARG_TRY(h, check_rot_step(rot_step));
    ARG_TRY(h, check_ranges(max_range, min_range));
    ARG_TRY(h, check_poses(poses_n3, n_scans));
    ARG_TRY(h, check_angles(angles, n_beams));
    const double inv = (double)v.dim / v.tile_len;                         // cells per metre, as lookup_cell_fast forms it
    const double invS = inv * (double)substeps;                            // exact: a power of two
    for (int n = 0; n < n_scans; ++n)
        for (int c = 0; c < 2; ++c)
            if (!((fabs(poses_n3[3 * (size_t)n + c]) + max_range) * invS + (double)n_trans < 1073741824.0))
                return fail(h, RBPF_EINVAL, "(|pose| + max_range) * cells per metre * substeps + n_trans < 2^30 is required");
    RefineArgs a;
    const int max_reach = rbpf_refine_max_reach(substeps, n_trans), nw = 2 * n_trans + 1;
    if (!search_setup(a, n_scans, n_beams, substeps, n_trans, n_rot, inv, min_range, max_range, max_reach, refine_fit(substeps, n_trans), "RBPF_REFINE_KPW"))
        return fail(h, RBPF_EINVAL, refine_window_message(max_range, inv, max_reach));
    MID_STEP_TRY(h, "pose refinement");
    // the field: the union of the windows, cut to the lattice grown by 2 (F = 0 farther out)
    const long long dim = v.dim, off = (long long)v.R * dim + dim / 2, edge = (long long)v.L * dim;   // mosaic X + off = a * dim + i
    long long lo[2] = {INT64_MAX, INT64_MAX}, hi[2] = {INT64_MIN, INT64_MIN};
    for (int n = 0; n < n_scans; ++n)
        for (int c = 0; c < 2; ++c) {
            const long long cell = (long long)floor(poses_n3[3 * (size_t)n + c] * inv);
            lo[c] = std::min(lo[c], cell); hi[c] = std::max(hi[c], cell);
        }
    LocateArgs f;
    long long ext[2];
    for (int c = 0; c < 2; ++c) {
        lo[c] = std::max(lo[c] - a.Mw, -off - 2); hi[c] = std::min(hi[c] + a.Mw + 1, edge - off + 2);
        ext[c] = std::max(0LL, hi[c] - lo[c]);
    }
    const bool any_field = ext[0] > 0 && ext[1] > 0;
    f.particle = particle; f.M = 0; f.x0 = a.fx0 = any_field ? (int)lo[0] : 0; f.y0 = a.fy0 = any_field ? (int)lo[1] : 0;
    f.rows = a.frows = any_field ? (int)ext[0] : 0; f.W = a.fW = any_field ? (int)((ext[1] + 31) / 32) : 0;
    const bool dev_out = (flags & RBPF_REFINE_DEVICE_OUT) != 0;
    // scratch: [guesses] [rotations] [beams] [ranges] [centre cells] | [field] [merge words] [guess scores] [n_used] | host outputs
    const size_t N = (size_t)n_scans, nray = N * n_beams, vol = N * a.nk * nw * nw;
    Carve c;
    const size_t guess_at = c.pack(N * 16), rot_at = c.pack(N * a.nk * 32), beam_at = c.pack((size_t)n_beams * 16), range_at = c.pack(nray * 8);
    const size_t cell_at = c.pack(N * 8), in_b = c.close(), field_at = c.take((size_t)a.frows * a.fW * 8);
    const size_t packed_at = c.take(N * 8), gscore_at = c.take(N * 4), used_at = c.take(N * 4), merge_b = c.total() - packed_at;
    const size_t pose_at = c.take(dev_out || !out_pose_n3 ? 0 : N * 24), n6_at = c.take(dev_out || !out_n6 ? 0 : N * 24);
    const size_t score_at = c.take(dev_out || !scores ? 0 : vol * 4);
    if (c.total() + (scores && dev_out ? vol * 4 : 0) > ((size_t)4 << 30))
        return fail(h, RBPF_ENOMEM, "scans, field and score volume need more than 4 GiB: refine fewer scans per call");
    HIP_TRY(h, h->reserve(B_REFINE, c.total()));
    const Block& d = h->buf[B_REFINE];
    Staging& st = h->stage[S_REFINE];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    double* sg = st.as<double>(guess_at);
    int32_t* sc = st.as<int32_t>(cell_at);
    for (size_t n = 0; n < N; ++n) {
        const double* g = poses_n3 + 3 * n;
        sg[2 * n] = g[0]; sg[2 * n + 1] = g[1];
        sc[2 * n] = (int32_t)floor(g[0] * inv); sc[2 * n + 1] = (int32_t)floor(g[1] * inv);
        stage_rotations(st.as<double>(rot_at) + n * a.nk * 4, g[2], n_rot, rot_step);
    }
    memcpy(stage_beam2(st.as<double>(beam_at), angles, n_beams), ranges, nray * 8);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    a.guess = d.as<const double>(guess_at); a.rot = d.as<const double>(rot_at); a.beam2 = d.as<const double>(beam_at);
    a.ranges = d.as<const double>(range_at); a.cell0 = d.as<const int32_t>(cell_at);
    a.field = f.field = d.as<uint2>(field_at);
    a.packed = d.as<unsigned long long>(packed_at); a.guess_score = d.as<int32_t>(gscore_at); a.n_used = d.as<int32_t>(used_at);
    HIP_TRY(h, hipMemsetAsync(a.packed, 0, merge_b, h->stream));
    a.out_pose = !out_pose_n3 ? nullptr : dev_out ? out_pose_n3 : d.as<double>(pose_at);
    a.out_n6 = !out_n6 ? nullptr : dev_out ? out_n6 : d.as<int32_t>(n6_at);
    a.scores = !scores ? nullptr : dev_out ? scores : d.as<int32_t>(score_at);
    launch_refine_poses(v, f, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{out_pose_n3, a.out_pose, N * 24}, {out_n6, a.out_n6, N * 24}, {scores, a.scores, vol * 4}});
}

// ---- scan-to-submap matching (kernels_pairs.hip) -------------------------------------------------------------------
int rbpf_match_pairs(rbpf_handle* h, const double* poses_n3, int32_t n_scans, const double* ranges, const double* angles,
                     int32_t n_beams, const int32_t* pairs_m3, int32_t n_pairs, const double* guess_m3, double cells_per_m,
                     double min_range, double max_range, int32_t substeps, int32_t n_trans, int32_t n_rot, double rot_step,
                     double* out_pose_m3, int32_t* out_m8, int32_t* scores, uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!poses_n3 || !ranges || !angles || !pairs_m3) return fail(h, RBPF_EINVAL, "poses, ranges, angles or pairs is NULL");
    if (!out_pose_m3 && !out_m8) return fail(h, RBPF_EINVAL, "out_pose_m3 and out_m8 are both NULL");
    if (flags & ~RBPF_PAIRS_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    const char* const counts = "n_scans >= 1, n_pairs >= 1, 1 <= n_beams <= 16384 and n_scans * n_beams < 2^31 are required";
    ARG_TRY(h, n_pairs < 1 ? counts : check_counts(n_scans, 1, n_beams, 16384, counts));
    ARG_TRY(h, check_search(substeps, n_trans, n_rot));
    const int nk = 2 * n_rot + 1, nw = 2 * n_trans + 1;
    if ((long long)n_pairs * nk >= (1LL << 31)) return fail(h, RBPF_EINVAL, "n_pairs * (2 n_rot + 1) < 2^31 is required");
    ARG_TRY(h, check_rot_step(rot_step));
    if (!std::isfinite(cells_per_m) || !(cells_per_m > 0.0)) return fail(h, RBPF_EINVAL, "cells_per_m must be finite and > 0");
    ARG_TRY(h, check_ranges(max_range, min_range));
    ARG_TRY(h, check_poses(poses_n3, n_scans));
    if (guess_m3) ARG_TRY(h, check_finite(guess_m3, 3LL * n_pairs, "guesses must be finite"));
    ARG_TRY(h, check_angles(angles, n_beams));
    for (int m = 0; m < n_pairs; ++m) {
        const int32_t* p = pairs_m3 + 3 * (size_t)m;
        if (p[0] < 0 || p[0] >= n_scans || p[1] < 0 || p[1] >= p[2] || p[2] > n_scans)
            return fail(h, RBPF_EINVAL, "a pair {q, r0, r1} needs 0 <= q < n_scans and 0 <= r0 < r1 <= n_scans");
    }
    const double inv = cells_per_m, invS = inv * (double)substeps;         // exact: a power of two
    auto in_reach = [&](double c) { return (fabs(c) + max_range) * invS + (double)n_trans < 1073741824.0; };
    for (int m = 0; m < n_pairs; ++m) {                                    // the guesses and the poses of the runs' scans
        const int32_t* p = pairs_m3 + 3 * (size_t)m;
        const double* g = guess_m3 ? guess_m3 + 3 * (size_t)m : poses_n3 + 3 * (size_t)p[0];
        bool ok = in_reach(g[0]) && in_reach(g[1]);
        for (int n = p[1]; ok && n < p[2]; ++n) ok = in_reach(poses_n3[3 * (size_t)n]) && in_reach(poses_n3[3 * (size_t)n + 1]);
        if (!ok) return fail(h, RBPF_EINVAL, "(|coordinate| + max_range) * cells per metre * substeps + n_trans < 2^30 is required of every guess and reference pose");
    }
    RefineArgs a;
    const int max_reach = rbpf_refine_max_reach(substeps, n_trans);
    if (!search_setup(a, n_pairs, n_beams, substeps, n_trans, n_rot, inv, min_range, max_range, max_reach, refine_fit(substeps, n_trans), "RBPF_PAIRS_KPW"))
        return fail(h, RBPF_EINVAL, refine_window_message(max_range, inv, max_reach));
    MID_STEP_TRY(h, "pair matching");
    a.fx0 = a.fy0 = a.frows = a.fW = 0; a.field = nullptr;                 // every pair stages its own field
    const bool dev_out = (flags & RBPF_PAIRS_DEVICE_OUT) != 0;
    // scratch: [guesses] [rotations] [scan poses] [beams] [ranges] [centre cells] [runs] [queries] | [fields] [merge words] [guess
    // scores] [n_used] [n_ref] | host outputs
    const size_t M = (size_t)n_pairs, N = (size_t)n_scans, nray = N * n_beams, vol = M * nk * nw * nw;
    Carve c;
    const size_t guess_at = c.pack(M * 16), rot_at = c.pack(M * nk * 32), pose_at = c.pack(N * 32), beam_at = c.pack((size_t)n_beams * 16);
    const size_t range_at = c.pack(nray * 8), cell_at = c.pack(M * 8), run_at = c.pack(M * 8), query_at = c.pack(M * 4), in_b = c.close();
    const size_t field_at = c.take(M * (2 * (size_t)a.Mw + 1) * a.WW * 8);
    const size_t packed_at = c.take(M * 8), gscore_at = c.take(M * 4), used_at = c.take(M * 4), ref_at = c.take(M * 4), merge_b = c.total() - packed_at;
    const size_t out_pose_at = c.take(dev_out || !out_pose_m3 ? 0 : M * 24), m8_at = c.take(dev_out || !out_m8 ? 0 : M * 32);
    const size_t score_at = c.take(dev_out || !scores ? 0 : vol * 4);
    if (c.total() + (scores && dev_out ? vol * 4 : 0) > ((size_t)4 << 30))
        return fail(h, RBPF_ENOMEM, "pairs, fields and score volume need more than 4 GiB: match fewer pairs per call");
    HIP_TRY(h, h->reserve(B_PAIRS, c.total()));
    const Block& d = h->buf[B_PAIRS];
    Staging& st = h->stage[S_PAIRS];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    double* sg = st.as<double>(guess_at);
    int32_t *sc = st.as<int32_t>(cell_at), *sn = st.as<int32_t>(run_at), *sq = st.as<int32_t>(query_at);
    for (size_t m = 0; m < M; ++m) {
        const int32_t* p = pairs_m3 + 3 * m;
        const double* g = guess_m3 ? guess_m3 + 3 * m : poses_n3 + 3 * (size_t)p[0];
        sg[2 * m] = g[0]; sg[2 * m + 1] = g[1];
        sc[2 * m] = (int32_t)floor(g[0] * inv); sc[2 * m + 1] = (int32_t)floor(g[1] * inv);
        sn[2 * m] = p[1]; sn[2 * m + 1] = p[2]; sq[m] = p[0];
        stage_rotations(st.as<double>(rot_at) + m * nk * 4, g[2], n_rot, rot_step);
    }
    stage_pose4(st.as<double>(pose_at), poses_n3, N);
    memcpy(stage_beam2(st.as<double>(beam_at), angles, n_beams), ranges, nray * 8);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    a.guess = d.as<const double>(guess_at); a.rot = d.as<const double>(rot_at); a.beam2 = d.as<const double>(beam_at);
    a.ranges = d.as<const double>(range_at); a.cell0 = d.as<const int32_t>(cell_at);
    PairsArgs f;
    f.M = n_pairs; f.B = n_beams; f.Mw = a.Mw; f.WW = a.WW; f.inv = inv; f.min_range = min_range; f.max_range = max_range;
    f.pose4 = d.as<const double>(pose_at); f.beam2 = a.beam2; f.ranges = a.ranges; f.cell0 = a.cell0;
    f.runs = d.as<const int32_t>(run_at); f.query = d.as<const int32_t>(query_at);
    f.fields = d.as<uint2>(field_at);
    a.packed = d.as<unsigned long long>(packed_at); a.guess_score = d.as<int32_t>(gscore_at); a.n_used = d.as<int32_t>(used_at);
    f.n_ref = d.as<int32_t>(ref_at);
    HIP_TRY(h, hipMemsetAsync(a.packed, 0, merge_b, h->stream));
    a.out_pose = nullptr; a.out_n6 = nullptr;                              // pairs_final_kernel writes the pair outputs
    f.out_pose = !out_pose_m3 ? nullptr : dev_out ? out_pose_m3 : d.as<double>(out_pose_at);
    f.out_m8 = !out_m8 ? nullptr : dev_out ? out_m8 : d.as<int32_t>(m8_at);
    a.scores = !scores ? nullptr : dev_out ? scores : d.as<int32_t>(score_at);
    launch_match_pairs(f, a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{out_pose_m3, f.out_pose, M * 24}, {out_m8, f.out_m8, M * 32}, {scores, a.scores, vol * 4}});
}

// ---- places by appearance (kernels_places.hip) -------------------------------------------------------------------
int rbpf_describe_scans(rbpf_handle* h, const double* ranges, int32_t n_scans, const double* angles, int32_t n_beams,
                        double min_range, double max_range, int32_t n_rings, uint64_t* desc, int32_t* info_n2, uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!ranges || !angles) return fail(h, RBPF_EINVAL, "ranges or angles is NULL");
    if (!desc && !info_n2) return fail(h, RBPF_EINVAL, "desc and info_n2 are both NULL");
    if (flags & ~RBPF_PLACES_DEVICE_OUT) return fail(h, RBPF_EINVAL, "unknown flags");
    ARG_TRY(h, check_counts(n_scans, 1, n_beams, 16384, "n_scans >= 1, 1 <= n_beams <= 16384 and n_scans * n_beams < 2^31 are required"));
    if (n_rings < 1 || n_rings > RBPF_PLACES_MAX_RINGS) return fail(h, RBPF_EINVAL, "1 <= n_rings <= 32 is required");
    ARG_TRY(h, check_ranges(max_range, min_range));
    ARG_TRY(h, check_angles(angles, n_beams));
    MID_STEP_TRY(h, "scan description");
    const bool dev_out = (flags & RBPF_PLACES_DEVICE_OUT) != 0;
    const size_t N = (size_t)n_scans, R = (size_t)n_rings, nray = N * n_beams;
    Carve c;                                                               // scratch: [sectors] [ranges] | host outputs
    const size_t sector_at = c.take((size_t)n_beams * 4), range_at = c.pack(nray * 8), in_b = c.close();
    const size_t desc_at = c.take(dev_out || !desc ? 0 : N * R * 8), info_at = c.take(dev_out || !info_n2 ? 0 : N * 8);
    if (c.total() > ((size_t)4 << 30)) return fail(h, RBPF_ENOMEM, "the scans need more than 4 GiB: describe fewer scans per call");
    HIP_TRY(h, h->reserve(B_PLACES, c.total()));
    const Block& d = h->buf[B_PLACES];
    Staging& st = h->stage[S_PLACES];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    int32_t* ss = st.as<int32_t>(sector_at);
    const double per_rad = 32.0 / M_PI;
    for (int b = 0; b < n_beams; ++b)                                      // host floating point: the device never sees an angle.  fmod is exact:
        ss[b] = (int32_t)((long long)fmod(floor(angles[b] * per_rad), 64.0) & 63);   // ((int64)floor) & 63, also where the floor exceeds an int64
    memcpy(st.p + range_at, ranges, nray * 8);
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    unsigned long long* o_desc = !desc ? nullptr : dev_out ? reinterpret_cast<unsigned long long*>(desc) : d.as<unsigned long long>(desc_at);
    int32_t* o_info = !info_n2 ? nullptr : dev_out ? info_n2 : d.as<int32_t>(info_at);
    launch_describe_scans(d.as<const double>(range_at), d.as<const int32_t>(sector_at), n_scans, n_beams, n_rings, min_range, max_range,
                          (double)n_rings / max_range, o_desc, o_info, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{desc, o_desc, N * R * 8}, {info_n2, o_info, N * 8}});
}

int rbpf_match_places(rbpf_handle* h, const uint64_t* query_desc, int32_t n_queries, const uint64_t* ref_desc, int32_t n_refs,
                      int32_t n_rings, const int32_t* ref_limit, int32_t k, int32_t* out_qk4, int32_t* out_q2, uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!query_desc || !ref_desc) return fail(h, RBPF_EINVAL, "query_desc or ref_desc is NULL");
    if (!out_qk4 && !out_q2) return fail(h, RBPF_EINVAL, "out_qk4 and out_q2 are both NULL");
    if (flags & ~(RBPF_PLACES_DEVICE_OUT | RBPF_PLACES_DEVICE_IN)) return fail(h, RBPF_EINVAL, "unknown flags");
    if (n_queries < 1 || n_refs < 1) return fail(h, RBPF_EINVAL, "n_queries >= 1 and n_refs >= 1 are required");
    if (n_rings < 1 || n_rings > RBPF_PLACES_MAX_RINGS) return fail(h, RBPF_EINVAL, "1 <= n_rings <= 32 is required");
    if (k < 1 || k > RBPF_PLACES_MAX_K) return fail(h, RBPF_EINVAL, "1 <= k <= 16 is required");
    if ((long long)n_queries * k >= (1LL << 31)) return fail(h, RBPF_EINVAL, "n_queries * k < 2^31 is required");
    for (int q = 0; ref_limit && q < n_queries; ++q)
        if (ref_limit[q] < 0 || ref_limit[q] > n_refs) return fail(h, RBPF_EINVAL, "0 <= ref_limit[q] <= n_refs is required");
    MID_STEP_TRY(h, "place search");
    PlacesArgs a;
    a.nq = n_queries; a.nr = n_refs; a.R = n_rings; a.k = k;
    a.chunk = std::min(256, n_refs);
    if (const char* e = getenv("RBPF_PLACES_CHUNK")) a.chunk = std::max(1, std::min(n_refs, atoi(e)));   // for tests
    a.nch = (n_refs + a.chunk - 1) / a.chunk;
    const bool dev_out = (flags & RBPF_PLACES_DEVICE_OUT) != 0, dev_in = (flags & RBPF_PLACES_DEVICE_IN) != 0;
    // scratch: [limits] [host query table] [host reference table] | [dilated references] [weights] [chunk lists] | host outputs
    const size_t Q = (size_t)n_queries, N = (size_t)n_refs, R = (size_t)n_rings;
    Carve c;
    const size_t limit_at = c.take(Q * 4), qd_at = c.take(dev_in ? 0 : Q * R * 8), rd_at = c.take(dev_in ? 0 : N * R * 8), in_b = c.total();
    const size_t dil_at = c.take(N * R * 8), w_at = c.take(N * 4), part_at = c.take(Q * a.nch * k * 16);
    const size_t qk4_at = c.take(dev_out || !out_qk4 ? 0 : Q * k * 16), q2_at = c.take(dev_out || !out_q2 ? 0 : Q * 8);
    if (c.total() > ((size_t)4 << 30) || (Q + 3) / 4 * a.nch >= ((size_t)1 << 31))
        return fail(h, RBPF_ENOMEM, "tables and chunk lists need more than 4 GiB: match fewer queries per call");
    HIP_TRY(h, h->reserve(B_PLACES, c.total()));
    const Block& d = h->buf[B_PLACES];
    Staging& st = h->stage[S_PLACES];
    HIP_TRY(h, st.begin(in_b));                                            // the last upload may still read it
    int32_t* sl = st.as<int32_t>(limit_at);
    for (size_t q = 0; q < Q; ++q) sl[q] = ref_limit ? ref_limit[q] : n_refs;
    if (!dev_in) { memcpy(st.p + qd_at, query_desc, Q * R * 8); memcpy(st.p + rd_at, ref_desc, N * R * 8); }
    HIP_TRY(h, st.upload(d.p, in_b, h->stream));
    a.limit = d.as<const int32_t>(limit_at);
    a.qd = dev_in ? reinterpret_cast<const unsigned long long*>(query_desc) : d.as<const unsigned long long>(qd_at);
    a.rd = dev_in ? reinterpret_cast<const unsigned long long*>(ref_desc) : d.as<const unsigned long long>(rd_at);
    a.dil = d.as<unsigned long long>(dil_at); a.w = d.as<int32_t>(w_at); a.partial = d.as<int4>(part_at);
    a.out_qk4 = !out_qk4 ? nullptr : dev_out ? out_qk4 : d.as<int32_t>(qk4_at);
    a.out_q2 = !out_q2 ? nullptr : dev_out ? out_q2 : d.as<int32_t>(q2_at);
    launch_match_places(a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{out_qk4, a.out_qk4, Q * k * 16}, {out_q2, a.out_q2, Q * 8}});
}

// ---- peaks and moments of score volumes (kernels_surface.hip) -----------------------------------------------------
int rbpf_score_surface(rbpf_handle* h, const int32_t* scores, int32_t n_items, int32_t n_rot, int32_t n_trans,
                       const int32_t* drop_n, int32_t ex_trans, int32_t ex_rot, int32_t n_peaks,
                       int64_t* out_nk16, int32_t* out_count, uint32_t flags) {
    if (!h) return RBPF_EINVAL;
    ON_DEVICE(h);
    if (!scores || !out_nk16) return fail(h, RBPF_EINVAL, "scores or out_nk16 is NULL");
    if (flags & ~(RBPF_SURFACE_DEVICE_IN | RBPF_SURFACE_DEVICE_OUT)) return fail(h, RBPF_EINVAL, "unknown flags");
    if (n_items < 1) return fail(h, RBPF_EINVAL, "n_items >= 1 is required");
    if (n_trans < 0 || n_trans > 32) return fail(h, RBPF_EINVAL, "0 <= n_trans <= 32 is required");
    if (n_rot < 0 || n_rot > 100) return fail(h, RBPF_EINVAL, "0 <= n_rot <= 100 is required");
    if (ex_trans < 0 || ex_trans > 64 || ex_rot < 0 || ex_rot > 200) return fail(h, RBPF_EINVAL, "0 <= ex_trans <= 64 and 0 <= ex_rot <= 200 are required");
    if (n_peaks < 1 || n_peaks > SURFACE_MAX_PEAKS) return fail(h, RBPF_EINVAL, "1 <= n_peaks <= 8 is required");
    const size_t N = (size_t)n_items, K = (size_t)n_peaks, per = (size_t)(2 * n_rot + 1) * (2 * n_trans + 1) * (2 * n_trans + 1), vol = N * per;
    if (vol >= ((size_t)1 << 31)) return fail(h, RBPF_EINVAL, "n_items * (2 n_rot + 1) * (2 n_trans + 1)^2 < 2^31 is required");
    const bool dev_in = (flags & RBPF_SURFACE_DEVICE_IN) != 0, dev_out = (flags & RBPF_SURFACE_DEVICE_OUT) != 0;
    if (!dev_in) {
        for (size_t n = 0; drop_n && n < N; ++n)
            if (drop_n[n] < 0 || drop_n[n] > 32768) return fail(h, RBPF_EINVAL, "0 <= drop_n[n] <= 32768 is required");
        for (size_t t = 0; t < vol; ++t)
            if ((uint32_t)scores[t] > 32768u) return fail(h, RBPF_EINVAL, "a score outside 0 .. 32768");
    }
    MID_STEP_TRY(h, "score surface");
    Carve c;                                                               // scratch: [host volume] [host drops] | host outputs
    const size_t vol_at = c.take(dev_in ? 0 : vol * 4), drop_at = c.pack(dev_in || !drop_n ? 0 : N * 4), in_b = c.close();
    const size_t rec_at = c.take(dev_out ? 0 : N * K * 128), cnt_at = c.take(dev_out ? 0 : N * 4), total = c.total();
    if (total > ((size_t)4 << 30)) return fail(h, RBPF_ENOMEM, "the volume and the records need more than 4 GiB: fewer items per call");
    SurfaceArgs a;
    a.N = n_items; a.R = n_rot; a.W = n_trans; a.ex_t = ex_trans; a.ex_r = ex_rot; a.K = n_peaks;
    a.scores = scores; a.drop = drop_n;
    a.out = reinterpret_cast<long long*>(out_nk16); a.count = out_count;
    if (total) {
        HIP_TRY(h, h->reserve(B_SURFACE, total));
        const Block& d = h->buf[B_SURFACE];
        if (!dev_in) {
            Staging& st = h->stage[S_SURFACE];
            HIP_TRY(h, st.begin(in_b));                                    // the last upload may still read it
            memcpy(st.p + vol_at, scores, vol * 4);
            if (drop_n) memcpy(st.p + drop_at, drop_n, N * 4);
            HIP_TRY(h, st.upload(d.p, in_b, h->stream));
            a.scores = d.as<const int32_t>(vol_at);
            a.drop = drop_n ? d.as<const int32_t>(drop_at) : nullptr;
        }
        if (!dev_out) { a.out = d.as<long long>(rec_at); a.count = d.as<int32_t>(cnt_at); }
    }
    launch_score_surface(a, h->stream);
    HIP_TRY(h, hipGetLastError());
    return dev_out ? RBPF_OK : fetch(h, {{out_nk16, a.out, N * K * 128}, {out_count, a.count, N * 4}});
}

}  // extern "C"
