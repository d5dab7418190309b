/*
 * rbpf_hip.h -- C ABI of librbpf_hip.so, the MI355X (gfx950) RBPF-SLAM particle-update engine.
 *
 * This is the drop-in boundary for the reference's per-particle hot path (reference =
 * amansanghvi/Thesis, cited file:line).  The reference has no FFI; its seams are Python
 * methods called once per particle from list comprehensions (main.py:144,157-160).  Each
 * entry point below replaces one of those per-particle methods by ONE batched call over all
 * particles of a handle.  The Python mirror of the reference's classes (thesis_amd/) binds
 * these symbols with ctypes; INTEGRATION.md shows the stub a maintainer of the reference
 * would add.
 *
 * Conventions
 *   - every function returns 0 (RBPF_OK) or a negative RBPF_E* code; the message is
 *     available from rbpf_last_error();
 *   - the caller owns every host buffer passed in or out (C-contiguous, float64 / int32 /
 *     int8); the library owns all device memory behind the opaque handle; no pointer is
 *     retained after a call returns; device pointers handed over explicitly (the rbpf_export_* /
 *     rbpf_resample_indices_global* / rbpf_pack_* calls) are used in stream order by the work that call queues;
 *   - calls on one handle are not re-entrant; one HIP stream per handle (rbpf_set_stream);
 *   - every call runs on the handle's device (rbpf_config.device) and leaves the caller's current
 *     HIP device as it found it;
 *   - a soft scan-matcher failure is not an error: it is reported per particle as NaN
 *     covariance and the engine takes the reference's fallback branch (robot.py:73-78).
 *
 * Map cells are stored as int8 multiples of `quantum` (0.1 for the reference's constants
 * +0.8/+0.2/-0.3 clamped to [-3,3], gridmap.py:20-24): in exact arithmetic every reachable
 * log-odds value is such a multiple, the reference's float64 cells deviate from it only by
 * accumulated rounding noise (< 1e-12).  rbpf_create() fails with RBPF_EINVAL if a constant
 * is not an integer multiple of `quantum` or does not fit in int8.
 */
#ifndef RBPF_HIP_H
#define RBPF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBPF_OK 0
#define RBPF_EINVAL (-1)    /* bad argument / configuration */
#define RBPF_ENOMEM (-2)    /* device or tile-pool exhaustion */
#define RBPF_EDEVICE (-3)   /* HIP runtime error (message has the HIP string) */
#define RBPF_ESTATE (-4)    /* call order violated (e.g. no scan set) */
#define RBPF_ERANGE (-5)    /* a pose left the addressable tile lattice */

/* motion-model families (IMUData.py:9-40 callbacks; a2 of SURVEY.md section 8) */
#define RBPF_IMU_UNICYCLE 0          /* DefaultIMUData.py:26-54: data = (speed, omega)          */
#define RBPF_IMU_ABSOLUTE 1          /* IntelIMUData.py:23-36:   data = (x, y, theta) passthrough */
#define RBPF_IMU_VELOCITY 2          /* Freid101IMUData.py:34-55: data = (vx, vy, omega)         */

typedef struct rbpf_handle rbpf_handle;

typedef struct rbpf_config {
    int32_t n_particles;      /* P: particles held by this handle (main.py:44 NUM_PARTICLES)      */
    int32_t n_samples;        /* K: proposal samples per particle (robot.py:17, 30)               */
    int32_t max_beams;        /* upper bound on beams per scan (<= 4095)                          */
    int32_t tile_len_m;       /* tile edge in metres (hybridmap.py:68, 40)                        */
    double  cell_size;        /* metres per cell (hybridmap.py:67, 0.05)                          */
    int32_t lattice_radius;   /* tiles addressable per axis: -R..R (default 3 => +-140 m)         */
    int32_t pool_tiles;       /* tile-pool capacity, 0 => 2*P                                     */
    double  log_odds_occ;     /* gridmap.py:20  +0.80                                             */
    double  log_odds_nearby;  /* gridmap.py:21  +0.20                                             */
    double  max_odds_occ;     /* gridmap.py:22  +3.0                                              */
    double  log_odds_emp;     /* gridmap.py:23  -0.30                                             */
    double  min_odds_emp;     /* gridmap.py:24  -3.0                                              */
    double  quantum;          /* cell unit; the five constants above must be multiples (0.1)      */
    double  occupied_threshold; /* gridmap.py:17 / hybridmap.py:18  1.0 (strict >)                */
    double  max_ray_m;        /* hybridmap.py:107 rays longer than this are shortened (15.0)      */
    double  weight_min_range; /* robot.py:130  0.01                                               */
    double  weight_max_range; /* robot.py:130  25.0                                               */
    double  match_min_range;  /* hybridmap.py:218  1e-3                                           */
    double  match_max_range;  /* hybridmap.py:20,218  11.0                                        */
    double  resample_spread;  /* main.py:50  200.0                                                */
    double  vel_noise[4];     /* RBPF_IMU_VELOCITY Q: (a0 + a1|v|dt)^2, (b0 deg + b1|w|dt)^2;
                                 Freid101IMUData.py:51-55 => {0.02, 0.01, 0.2, 0.02}             */
    int32_t device;           /* HIP device ordinal                                               */
    int32_t ndt_refine;       /* second matcher stage, matchScanCustom.m:32-50 (NDT, CellSize 0.1 m, 500 iterations):
                                 0 off; 1 (default) on, accepted by the reference's rule (valid pose and
                                 2*ndtScore > gridScore);
                                 2 on, every valid NDT pose is taken (diagnostic).  Inactive when the matcher cell
                                 is 0.1 m or coarser (no NDT cell can hold the 3 points a Gaussian needs).          */
    uint64_t seed;            /* Philox seed for on-device proposal sampling                      */
} rbpf_config;

typedef struct rbpf_counters {
    /* cumulative since rbpf_create or the last rbpf_set_profiling call: */
    uint64_t scan_updates;        /* rbpf_scan_update/rbpf_map_update calls                       */
    uint64_t ray_cells_visited;   /* sum of Bresenham points over all rays                        */
    uint64_t cells_written;       /* unique cells written per update, summed (|W| over particles) */
    uint64_t cells_gathered;      /* map cells read by the weighting kernels (K*B gathers per particle-update) */
    uint64_t tiles_in_use;        /* tiles allocated from the pool (current)                      */
    uint64_t resample_copies;     /* tile copies made by resampling                               */
    uint64_t bytes_copied;        /* bytes moved by those copies (read + write)                   */
    double   ms_raycast;          /* HIP-event time of the last ray-cast kernel                   */
    double   ms_weight;           /* ... of the last weighting kernel                             */
    double   ms_match;            /* ... of the last scan-match kernels                           */
    double   ms_resample;         /* ... of the last resample (plan + copies)                     */
    uint64_t slow_cells;          /* flagged cells replayed by the exact membership scan          */
    uint64_t reserved[7];         /* phase cycle sums of a -DRBPF_STAMPS diagnostic build, else 0 */
    uint64_t window_fallbacks;    /* particles the first map-update kernel handed to the 128x128-window kernel */
    uint64_t ndt_runs;            /* matches that entered the NDT stage                           */
    uint64_t ndt_evaluations;     /* NDT score/gradient/Hessian evaluations, summed over runs     */
    uint64_t ndt_accepted;        /* runs whose pose replaced the grid pose (matchScanCustom.m:39-41) */
    uint64_t match_shared;        /* particles that took the match result of an exact duplicate (a copy made by the
                                     last resample: same pose, covariance and map) instead of repeating the search */
    uint64_t fallback_reasons;    /* why particles left the first map-update kernel, packed: three 16-bit tallies
                                     (geometry / index map, counter bound, event tables), each SATURATING at 65535;
                                     the exact tallies are fallback_geometry / _bound / _tables below             */
    double   ms_ndt;              /* HIP-event time of the last NDT-stage kernel                  */
    uint64_t stamp7;              /* eighth phase stamp of a -DRBPF_STAMPS diagnostic build, else 0 */
    uint64_t map_windows;         /* LDS windows the map update processed, summed over particles (1 per particle when
                                     the whole ray fan fits one window)                                            */
    uint64_t fallback_geometry;   /* particles handed to the 128x128-window kernel: fan / index-map form / LDS rows  */
    uint64_t fallback_bound;      /* ... the 8-bit hit fields could overflow (slope-bucket bound)                   */
    uint64_t fallback_tables;     /* ... event tables full (global-index kernel)                                    */
    uint64_t map_events;          /* event-walk kernel: passes over cells that also got an occupied / nearby hit in
                                     the same scan, found by the walk's returning adds, summed over particles       */
    uint64_t map_event_overflows; /* ... particles whose list of such passes was full (every flagged cell of theirs
                                     was then replayed by the exact membership test)                               */
    uint64_t map_updates_skipped; /* particles a map update left out because the resample that followed discarded them
                                     (rbpf_resample right behind rbpf_scan_update); ray_cells_visited, cells_written and
                                     the other map-update tallies do not count them                                */
    uint64_t map_pool_cells;      /* flagged cells folded by a wave from a fixed-capacity list: global-index kernel, cells
                                     whose list outgrew the 16-event per-pair list and moved to a pool list of 64 (a list
                                     moves when two more events would not fit, so cells that end with 15 or 16 events
                                     can count); 128x128-window kernel, buckets of 17 .. cap events.  Longer lists
                                     count in slow_cells                                                             */
    uint64_t map_near_cells;      /* global-index kernel: flagged cells within 16 steps of the sensor folded from the
                                     second walk of the block round the start cell (not those handed to slow_cells)  */
} rbpf_counters;

/* ---- lifecycle ------------------------------------------------------------------------- */
int  rbpf_default_config(rbpf_config* cfg);
/* Robot.__init__ x P (robot.py:20-28): pose 0, cov 0, weight 1, one empty tile centred (0,0). */
int  rbpf_create(const rbpf_config* cfg, rbpf_handle** out);
int  rbpf_destroy(rbpf_handle* h);
const char* rbpf_last_error(const rbpf_handle* h);   /* h may be NULL (create failures)      */
int  rbpf_set_stream(rbpf_handle* h, void* hip_stream); /* e.g. torch's current stream (borrowed: the handle
                                                           never destroys it)                       */
/* gives a borrowed stream back (waits for what this handle queued on it); the handle then works on a stream of its
 * own again.  Call it before the owner of the stream goes away, or simply before rbpf_destroy. */
int  rbpf_release_stream(rbpf_handle* h);
/* sizeof(rbpf_config), sizeof(rbpf_counters) as this library was built: a binding checks its struct layouts */
int  rbpf_abi_struct_bytes(int32_t* config_bytes, int32_t* counters_bytes);
int  rbpf_synchronize(rbpf_handle* h);
int  rbpf_get_counters(rbpf_handle* h, rbpf_counters* out);
int  rbpf_set_profiling(rbpf_handle* h, int on);     /* per-kernel HIP events; resets the rings */
/* the same for a subset of the kernel families (bit k = family k of rbpf_get_kernel_ms): every record costs a few
 * microseconds of stream time, a benchmark brackets only what it needs inside its timed region */
int  rbpf_set_profiling_families(rbpf_handle* h, uint32_t mask);
/* durations (ms) of the launches recorded since rbpf_set_profiling, HIP events on the handle's stream;
 * which: 0 ray-cast map-update kernel, 1 proposal/weighting kernel, 2 resample kernels, 3 scan-match grid stage,
 * 4 scan-match NDT stage.  Synchronises the stream. */
int  rbpf_get_kernel_ms(rbpf_handle* h, int32_t which, double* out_ms, int32_t cap, int32_t* n_out);

/* ---- a1: scan geometry (Scan.__init__, lidar.py:76-80) ------------------------------------ */
/* ranges[B], angles[B] -> sensor-frame endpoints (host libm cos/sin, as the reference), the
 * per-beam range classes (robot.py:130, hybridmap.py:107,218) and the upload. */
int  rbpf_set_scan(rbpf_handle* h, const double* ranges, const double* angles, int32_t n_beams);
/* the same from the end points a reference Scan object holds (Scan.x(), Scan.y(), lidar.py:82-87): what the per-object
 * facade (thesis_amd/dropin.py) has in hand when main.py:157 passes it a Scan */
int  rbpf_set_scan_xy(rbpf_handle* h, const double* x, const double* y, int32_t n_beams);

/* ---- a2: Robot.imu_update (robot.py:45-57) for every particle ------------------------------ */
int  rbpf_imu_update(rbpf_handle* h, int32_t model, const double* data3, double dt_ticks);

/* ---- a4: Robot._generate_sample_weight (robot.py:118-139), test entry ------------------------ */
/* guesses[P*K*3], motion_prs[P*K] -> out_w[P*K] against each particle's own map. */
int  rbpf_weight_samples(rbpf_handle* h, const double* guesses, const double* motion_prs,
                         int32_t n_samples, double* out_w);

/* ---- a5: HybridMap.update (hybridmap.py:95-145), test entry ----------------------------------- */
/* poses[P*3] or NULL (= each particle's latest pose). */
int  rbpf_map_update(rbpf_handle* h, const double* poses);

/* ---- a3+a4+a5(+a6/a7): Robot.map_update (robot.py:59-115) for every particle ------------------ */
/* adj            : main.py:156-159 (0 = match against own map, 1 = against last_scan_xy)
 * last_scan_xy   : [n_last*2] global endpoints of the reference scan (adj=1), else NULL
 * match_override : NULL => built-in correlative matcher; else [P*13] = pose(3), cov(9), score(1)
 *                  per particle, as returned by Map.get_scan_match (engine-seam double)
 * guesses        : NULL => on-device Philox proposal; else [P*K*3] explicit samples
 *                  (replaces np.random.multivariate_normal, robot.py:81)
 * The map update waits for the next call in filters of more than four particles per compute unit of the device (below
 * that, leaving particles out saves no round of the map kernel and the step is as ever).  There, with map updates on,
 * rbpf_scan_update queues the matcher, the proposal and
 * the weighting and holds back what rbpf_scan_update_end does (the map update, the NaN-branch weight increments, the
 * step's trajectory record).  rbpf_resample as the next call launches its plan first, then the held-back update WITHOUT
 * the particles the plan discards - their maps are overwritten by the copies that follow -, then copies and release; if a
 * particle is on the NaN-covariance branch its weight still changes, the plan is made behind the update and nobody is left
 * out.  Every other entry point that touches the device launches the held-back update whole before anything else
 * (rbpf_set_stream and rbpf_release_stream on the old stream; rbpf_destroy drops it), so results, counters and the order
 * of work in the stream are those of rbpf_scan_update_begin + _end for every sequence of calls; only
 * counters.map_updates_skipped and the map update's tallies tell a left-out particle.  What the host alone keeps
 * (scan_updates, the random streams' position, the trajectory log's record count) changes at the call.
 * RBPF_SKIP_DISCARDED in the environment of rbpf_create (tests, A/B runs): 1 holds back whatever the filter's size;
 * 0 does too and leaves nobody out - the same order of launches.                                                  */
int  rbpf_scan_update(rbpf_handle* h, int32_t adj, const double* last_scan_xy, int32_t n_last,
                      const double* match_override, const double* guesses);
/* main.py:167-168: last_scan = scan.from_global_reference(particles[0].get_latest_pose()).  Computed on the device
 * from the current scan and the pose of `particle`, and kept there: a later rbpf_scan_update with adj = 1 and
 * last_scan_xy = NULL uses it, so the driver loop never has to read a pose back.  rbpf_export_last_scan /
 * rbpf_import_last_scan copy it to / from a device buffer of max_beams * 2 doubles (stream-ordered), for the rank
 * that owns particle 0 to broadcast it in a multi-GPU job. */
int  rbpf_refresh_last_scan(rbpf_handle* h, int32_t particle);
int  rbpf_export_last_scan(rbpf_handle* h, void* d_out_xy, int32_t* n_points);
int  rbpf_import_last_scan(rbpf_handle* h, const void* d_xy, int32_t n_points);
/* The same in two halves, for a driver that wants the weights as early as possible (multi-GPU resampling):
 * _begin = scan matcher, proposal, weighting, moments (robot.py:62-114): the weights are final here unless a particle
 * took the NaN-covariance branch; _end = the map update at the new mean pose and that branch (robot.py:115, 73-78). */
int  rbpf_scan_update_begin(rbpf_handle* h, int32_t adj, const double* last_scan_xy, int32_t n_last,
                            const double* match_override, const double* guesses);
int  rbpf_scan_update_end(rbpf_handle* h);
/* Read-out of the proposal of the last rbpf_scan_update_begin / rbpf_scan_update (test / inspection entry).
 * rbpf_set_proposal_capture(on != 0): the following scan updates also keep every sample's raw weight w_k (robot.py:138,
 * before the shift of robot.py:96) in a [P][K] buffer allocated on first use.  Off by default, and then the launches are
 * exactly those of a handle that never heard of it.
 * rbpf_get_proposal copies out, for one particle (any output may be NULL):
 *   frame24    [24]   U[9] (row-major, pseudo-inverse square root: maha = |(g - mean) U|^2), A[9] (row-major sampling
 *                     matrix: g = mean + A z), mean[3], log c, bad flag (1 = NaN / indefinite covariance: no proposal, the
 *                     rest of the read-out is then whatever an earlier step left), one unused
 *   samples    [K][6] x, y, theta, cos theta, sin theta, motion probability (pdf * 10)
 *   frame_f32  [K][4] the single-precision look-up frame: cos / cell, sin / cell, x / cell + off_x, y / cell + off_y
 *   raw_w      [K]    the captured w_k; RBPF_ESTATE unless capture was on during that scan update
 * RBPF_ESTATE before the first scan update. */
int  rbpf_set_proposal_capture(rbpf_handle* h, int32_t on);
int  rbpf_get_proposal(rbpf_handle* h, int32_t particle, double* frame24, double* samples, float* frame_f32, double* raw_w);

/* ---- a6/a7: scan matcher, stateless twin of the engine seam (hybridmap.py:244-251) ------------ */
int  rbpf_match_scan(rbpf_handle* h, const double* curr_xy, int32_t n_curr, const double* ref_xy,
                     int32_t n_ref, const double* guess3, int32_t cells_per_m,
                     const double* pose_range3, double* pose_out3, double* cov_out9,
                     double* score_out);
/* matcher inputs built from particle p's map (hybridmap.py:210-242), test/inspection entry */
int  rbpf_match_inputs(rbpf_handle* h, int32_t particle, const double* guess3, double* curr_xy,
                       int32_t* n_curr, double* ref_xy, int32_t* n_ref, int32_t cap_ref);
/* out[P][13]: pose, 3x3 covariance, score of every particle as the last built-in matcher of rbpf_scan_update(_begin)
 * wrote them; a duplicate particle the matcher skipped gets its representative's row (the row the proposal read).
 * RBPF_ESTATE if no built-in match ran, or if match_override or a resample came after it.  Test/inspection entry. */
int  rbpf_match_results(rbpf_handle* h, double* out);
/* s[i], c[i] = __sincosf(x[i]) on the device, compiled with the matcher's grid stage: the sines and cosines it rotates the
 * beams by.  Test/inspection entry. */
int  rbpf_native_sincosf(rbpf_handle* h, const float* x, int32_t n, float* s, float* c);

/* ---- a8+a9: resample (main.py:46-79) ---------------------------------------------------------- */
/* u in [0,1) replaces np.random.random() (main.py:59); NaN => internal Philox draw.
 * idx_out[P] (may be NULL) receives the ancestor index of every new particle.
 * Tile pool: a copy takes a tile from the free pool for every lattice position its ancestor holds and its destination
 * does not; the tiles the destinations give up go back to the pool only after all copies.  A resample therefore needs as
 * many FREE tiles as it allocates, not the net number: one that releases a tile and allocates another with no free tile
 * fails.  Exhaustion is RBPF_ENOMEM (here with idx_out or did_resample, else at the next call that checks the device's
 * error word, e.g. rbpf_synchronize); the maps are then incomplete and the handle should be destroyed.  The same holds for
 * rbpf_apply_resample_local.
 * Right behind rbpf_scan_update the call also launches that step's map update, between its plan and its copies (see
 * there); ms_resample and the "resample" timings stay plan plus copies.  An invalid u launches the update whole, then
 * fails as ever. */
int  rbpf_resample(rbpf_handle* h, double u, int32_t* idx_out, int32_t* did_resample);

/* multi-GPU pieces (one handle per rank; the collectives themselves are the caller's, over RCCL).
 * Every particle carries a global id (0 .. n_global-1, its index in the reference's particle list); the
 * Philox proposal streams are keyed by it, so results do not depend on which rank holds a particle. */
int  rbpf_set_global_ids(rbpf_handle* h, const int32_t* ids_p);
/* zero a device vector of n_global doubles and scatter the local weights into it at the global ids, so that
 * an all-reduce(sum) yields the full weight vector on every rank.  Stream-ordered on the handle's stream, no host
 * synchronisation: run the collective on the same stream (rbpf_set_stream with the communicator's stream, e.g.
 * torch's current stream) or call rbpf_synchronize() first ...                                                 */
int  rbpf_export_weights(rbpf_handle* h, void* d_global_weights, int32_t n_global);
/* ... then compute the global systematic-resampling ancestors from it (main.py:46-67), identically on every
 * rank; idx_out[n_global] on the host. */
int  rbpf_resample_indices_global(rbpf_handle* h, const void* d_global_weights, int32_t n_global,
                                  double u, int32_t* idx_out, int32_t* did_resample);
/* The early variants, for overlapping the global resample with rbpf_scan_update_end.  Queue, between
 * rbpf_scan_update_begin and rbpf_scan_update_end and on `stream` (the handle's own stream, or another one: the calls
 * wait for the weighting kernel through an event):
 *   rbpf_export_weights_early            the vector has n_global + 1 elements; the last one is 1 on a rank with a
 *                                        particle on the NaN-covariance branch (robot.py:73-78)
 *   (the caller's all-reduce(sum) on that stream)
 *   rbpf_resample_indices_global_early   ancestors + read-back into pinned memory; returns at once
 * then rbpf_scan_update_end, and finally
 *   rbpf_resample_indices_global_wait    waits for the read-back only (an event), not for the map update queued
 *                                        behind it.  *nan_branch_ranks != 0: weights of NaN-branch particles change in
 *                                        rbpf_scan_update_end - discard the result and use the late calls above. */
int  rbpf_export_weights_early(rbpf_handle* h, void* d_global_weights_n_plus_1, int32_t n_global, void* stream);
int  rbpf_resample_indices_global_early(rbpf_handle* h, const void* d_global_weights_n_plus_1, int32_t n_global, double u,
                                        void* stream);
int  rbpf_resample_indices_global_wait(rbpf_handle* h, int32_t* idx_out, int32_t* did_resample, double* nan_branch_ranks);
/* local part of a global resample: new local particle j continues local particle new_src[j] (sorted ascending)
 * or, for new_src[j] = -1 (last), arrives from another rank and is installed by rbpf_unpack_particles; weights
 * restart at 1.0 (main.py:77-78) */
int  rbpf_apply_resample_local(rbpf_handle* h, const int32_t* new_src, const int32_t* new_global_id);
int  rbpf_unpack_particles(rbpf_handle* h, const int32_t* local_idx, int32_t n, const void* d_buf,
                           const int32_t* meta_in);
/* The migration with ONE host wait (thesis_amd/sharding.py): (1) the tile boxes of the departing particles are gathered
 * into d_raw ([n][rbpf_pack_raw_width()] int32, device) without waiting; the ranks exchange these records while they
 * are on the device and read their own and the incoming ones back in one copy; (2) records -> the layout rows of
 * rbpf_unpack_particles and the payload size (host only, no device work); (3) the pack with the records already on
 * the host (nothing waited for): the particles' state, the written boxes of their tiles and their occupancy masks,
 * serialised into d_buf. */
int32_t rbpf_pack_raw_width(rbpf_handle* h);
/* meta_out of rbpf_meta_from_raw, meta_in of rbpf_unpack_particles: [n][rbpf_pack_meta_width()] host ints that
 * describe the payload layout for the receiver.  A row: tile count, payload bytes / 16, then per lattice position
 * (lx + R) * L + (ly + R) six ints (has, x0, x1, y0, y1, offset / 16): the tile's written box, inclusive, which the
 * receiver's tile gets exactly, and where its bytes start in the particle's payload; a held tile nothing was written to
 * is (1, 0, -1, 0, -1, offset) and takes no bytes.  A particle's payload: 128 bytes of state (13 doubles x, y, theta,
 * cov[9], weight), then per written tile the rows x0..x1 of the columns [y0 & ~15, min((y1 | 15) + 1, dim)) as int8 and
 * (x1 - x0 + 1) * ceil(dim / 32) occupancy words, each tile padded to a multiple of 16 bytes. */
int32_t rbpf_pack_meta_width(rbpf_handle* h);
int  rbpf_gather_pack_meta(rbpf_handle* h, const int32_t* local_idx, int32_t n, void* d_raw);
int  rbpf_meta_from_raw(rbpf_handle* h, const int32_t* raw, int32_t n, int32_t* meta_out, int64_t* bytes_out);
int  rbpf_pack_particles_raw(rbpf_handle* h, const int32_t* local_idx, int32_t n, const int32_t* raw, void* d_buf,
                             int64_t cap_bytes, int64_t* bytes_out);

/* ---- state access (Robot.get_latest_pose/weight, HybridMap readback; main.py:152,170-176) ----- */
int  rbpf_get_poses(rbpf_handle* h, double* out_p3);
int  rbpf_get_covs(rbpf_handle* h, double* out_p9);
int  rbpf_get_weights(rbpf_handle* h, double* out_p);
int  rbpf_set_state(rbpf_handle* h, const double* poses_p3, const double* covs_p9,
                    const double* weights_p);             /* any pointer may be NULL           */
/* position of the two internal random streams (sample draws: one per scan update; resample uniforms), for checkpoints
   that continue a run bit-identically; replaces the `np.random` state the reference pickles (main.py:183-210) */
int  rbpf_get_rng_state(rbpf_handle* h, uint64_t* scan_updates, uint64_t* resample_draws);
int  rbpf_set_rng_state(rbpf_handle* h, uint64_t scan_updates, uint64_t resample_draws);
int  rbpf_get_tile_count(rbpf_handle* h, int32_t particle, int32_t* out_n);
/* k-th tile of a particle in lattice order: centre (metres) and dim*dim cells, cell[x*dim+y] */
int  rbpf_get_tile(rbpf_handle* h, int32_t particle, int32_t k, double* centre2, int8_t* cells);
/* cells must lie in [min_odds_emp, max_odds_occ] / quantum, as every map of the reference does (RBPF_EINVAL) */
int  rbpf_set_tile(rbpf_handle* h, int32_t particle, double cx, double cy, const int8_t* cells);
int  rbpf_get_dim(rbpf_handle* h, int32_t* out_dim);
/* HybridMap.get_odds_at (hybridmap.py:85-93) for n points against particle p's map;
 * out_none[i] = 1 where the reference returns None */
int  rbpf_get_odds_at(rbpf_handle* h, int32_t particle, const double* xy, int32_t n,
                      double* out_vals, uint8_t* out_none);

/* ---- map read-out: dense rasters of one particle's map or of the whole filter ------------------------------------------
 * Rasters are indexed in mosaic cells.  Tile (a, b) of the lattice (centre ((a-R) tile_len, (b-R) tile_len), as
 * rbpf_get_tile) holds mosaic cells X = (a-R) dim + i - dim/2, Y = (b-R) dim + j - dim/2 in its storage cell (i, j)
 * (dim/2 in integer division).  For even dim, (X, Y) is the "cell units" point of get_occupied_points
 * (hybridmap.py:303-313).  A box is int32 box4 = {x0, x1, y0, y1}, half-open; an output is row-major
 * [x1-x0][y1-y0], indexed [X-x0][Y-y0] (as cell[x*dim + y]).  Cells outside every tile of a particle, or outside the
 * lattice, hold log-odds 0 (a fresh tile, gridmap.py:26-35).  Neither call changes any engine state; both return
 * RBPF_ESTATE between rbpf_scan_update_begin and rbpf_scan_update_end. */
#define RBPF_RENDER_DEVICE_OUT 1u  /* outputs are device pointers, written in stream order, no host wait */
/* smallest box holding the written cells (tile_bbox) of every tile of `particle`, or of all particles (-1);
 * {0, 0, 0, 0} when there is none */
int  rbpf_map_extent(rbpf_handle* h, int32_t particle, int32_t* box4);
/* particle >= 0: cells = its int8 lattice values (units of quantum); prob, occ_frac and weights NULL.
 * particle == -1: cells NULL, prob and / or occ_frac; weights NULL (uniform) or P host float64, finite, >= 0, with a
 * positive sum:   prob[c]     = sum_p w_p sigma(v_p(c) quantum) / sum_p w_p,   sigma(o) = e^o / (1 + e^o) (get_pr_at,
 *                               hybridmap.py:74-83; 0.5 where no particle has a tile),
 *                 occ_frac[c] = sum_p w_p [v_p(c) > occupied_threshold / quantum] / sum_p w_p   (gridmap.py:153),
 * summed in float64 in a fixed order and rounded to float32 once: bit-identical from call to call.  A box of more than
 * 2^31 cells or a wrong NULL pattern is RBPF_EINVAL, and nothing is written.  Without RBPF_RENDER_DEVICE_OUT the outputs
 * are host arrays, complete on return. */
int  rbpf_render_map(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* weights,
                     uint32_t flags, int8_t* cells, float* prob, float* occ_frac);

/* ---- map loading: a dense raster into the particles' tiles; localization with the maps held fixed ---------------------
 * rbpf_load_map writes the int8 lattice values `cells` (units of quantum, in [min_odds_emp, max_odds_occ] / quantum) of
 * the box box4 = {x0, x1, y0, y1} into `particle` (>= 0) or into every particle (-1).  box4 and the raster layout are
 * those of rbpf_render_map: mosaic cells, half-open, [x1-x0][y1-y0] row-major.  Cells inside the box are replaced; cells
 * outside it keep their values.  Missing lattice tiles come from the free pool (zero-filled); every touched tile's
 * written box grows to hold (box n tile), and its occupancy bits are recomputed.  Groups of exact duplicates made by the
 * last resample are dissolved (the next matcher runs once per particle).  All or nothing: a value out of range, a box
 * that leaves the lattice or holds more than 2^31 cells is RBPF_EINVAL; too few free tiles for the whole request is
 * RBPF_ENOMEM (the message gives the number needed); a call between rbpf_scan_update_begin and _end is RBPF_ESTATE.  In
 * each case nothing is written.  Complete on return. */
#define RBPF_LOAD_DEVICE_IN 1u     /* cells is a device pointer, read in stream order (validated on the device) */
int  rbpf_load_map(rbpf_handle* h, int32_t particle, const int32_t* box4, const int8_t* cells, uint32_t flags);
/* ---- map placement: a map with its own cell size and its own pose in the world, resampled into the particles' tiles ----
 * src[nsx][nsy] (row-major int8, units of quantum, every value in [min_odds_emp, max_odds_occ] / quantum) is a raster whose
 * cell (i, j) covers [i, i+1) x [j, j+1) times src_cell in the frame with origin (ox, oy) rotated by yaw;
 * src_pose3 = (ox, oy, yaw) is the world pose of the corner of cell (0, 0) (the origin of the common PGM + YAML map format).
 * box4 = {x0, x1, y0, y1} and the mosaic cells are those of rbpf_render_map / rbpf_load_map.  In float64, every operation
 * rounded on its own, c = cos(yaw), s = sin(yaw) (host libm), cs = tile_len / dim, S = samples (1 .. 8); for the mosaic cell
 * (X, Y) of the box and a, b = 0 .. S-1:
 *   fa = (a + 0.5) / S                      fb = (b + 0.5) / S
 *   wx = (X + fa) * cs                      wy = (Y + fb) * cs
 *   dx = wx - ox                            dy = wy - oy
 *   u  = (c*dx + s*dy) / src_cell           w  = (c*dy - s*dx) / src_cell
 *   inside iff 0 <= floor(u) < nsx and 0 <= floor(w) < nsy;   sample = src[floor(u)][floor(w)]
 *   covered[X-x0][Y-y0] = any sample inside
 *   warped [X-x0][Y-y0] = max of the inside samples (0 when none)
 * The maximum keeps a wall that crosses any part of the cell; a cell is free only if all of it is; S = 1 is nearest
 * neighbour.  DESIGN.md 3.9 has the kernels.
 * Without RBPF_PLACE_DRY the covered cells of the box are merged under `mode` into `particle` (>= 0) or into every particle
 * (-1), each with its own old cells; cells of the box that are not covered keep their values.  Everything else is as
 * rbpf_load_map: missing lattice tiles of the box come from the free pool, every touched tile's written box grows to hold
 * (box n tile), its occupancy bits are recomputed, duplicate groups are dissolved, and the call is complete on return.
 * warped and covered ([x1-x0][y1-y0]) may each be NULL.  With RBPF_PLACE_DRY at least one must be given, `particle` is
 * ignored and no engine state changes (maps, tiles, counters, random streams, duplicate grouping); with RBPF_PLACE_DEVICE_OUT
 * and a host source such a call does not wait for the device.
 * All or nothing, checked before anything is written: a NULL box4, src or src_pose3, nsx or nsy < 1, nsx * nsy >= 2^31, a box
 * of more than 2^31 cells or one that leaves the lattice, a non-finite pose, src_cell not finite or not > 0, samples outside
 * 1 .. 8, an unknown mode or flag, a bad particle or a source value out of range (a device source is checked on the device,
 * and the call then waits for the verdict) is RBPF_EINVAL; too few free tiles is RBPF_ENOMEM (the message gives the number
 * needed); a call between rbpf_scan_update_begin and _end is RBPF_ESTATE. */
#define RBPF_PLACE_DEVICE_IN  1u   /* src is a device pointer, read in stream order, validated on the device */
#define RBPF_PLACE_DEVICE_OUT 2u   /* warped / covered are device pointers, written in stream order, no host wait */
#define RBPF_PLACE_DRY        4u   /* compute warped / covered only: no map, tile, counter or duplicate grouping changes */
#define RBPF_PLACE_REPLACE 0       /* covered cells take the warped value                                  */
#define RBPF_PLACE_KNOWN   1       /* ... only where the warped value is not 0 (the source knows something) */
#define RBPF_PLACE_ADD     2       /* covered cells become clamp(old + warped, vmin, vmax): log-odds fusion  */
int  rbpf_place_map(rbpf_handle* h, int32_t particle, const int32_t* box4, const int8_t* src, int32_t nsx, int32_t nsy,
                    double src_cell, const double* src_pose3, int32_t samples, int32_t mode, uint32_t flags, int8_t* warped,
                    uint8_t* covered);
/* Map updates on (1, the default) or off (0).  Off, rbpf_scan_update(_end) leaves every map unchanged: the NaN-branch
 * weight increment (robot.py:73-78) is taken on the unchanged map, and the proposal's random stream still advances one
 * step per scan update (rbpf_get_rng_state).  This is localization in a known map.  An explicit rbpf_map_update writes
 * in either mode. */
int  rbpf_set_map_updates(rbpf_handle* h, int32_t on);
int  rbpf_get_map_updates(rbpf_handle* h, int32_t* on);
/* Workgroups the event-walk map kernel was launched with in the last map update: min(P, CUs, RBPF_EV_GRID) resident ones, P with
 * RBPF_EV_RESIDENT=0, 0 if that kernel did not run (tests of the launch shape; no device access). */
int  rbpf_get_map_update_workgroups(rbpf_handle* h, int32_t* n);

/* ---- scan casting: what a lidar at a pose would see in a particle's map ------------------------------------------------
 * particle >= 0: all n_poses poses (x, y, theta) are cast in that particle's map.  particle == -1: n_poses must equal P
 * and pose n is cast in particle n's map.  Beam b of pose n leaves (x, y) in direction theta + angles[b] (sensor frame, x
 * forward, as rbpf_set_scan) and walks the supercover (4-connected) sequence of mosaic cells it crosses, in float64 (the
 * walk is spelled out in DESIGN.md 3.7): the first cell with cell * quantum > occupied_threshold ends it.
 *   ranges[n_poses][n_beams]  metres from the origin to the point where the ray ENTERS the hit cell (0 when it starts in
 *                             an occupied cell); max_range where status is not 1
 *   status[n_poses][n_beams]  1 hit; 0 nothing occupied within max_range; 2 the ray (or its origin) left the tile lattice
 *                             before either.  May be NULL.
 * A lattice position without a tile and a cell outside its tile's written box are free.  Independent of rbpf_set_scan: any
 * n_beams >= 1, n_poses * n_beams < 2^31, no scan needs to be set.  cos and sin of theta and of the angles are host libm
 * values.  A NULL poses_n3, angles or ranges, a non-finite pose or angle, max_range not finite or not > 0, a bad particle,
 * n_poses != P with particle == -1 or an unknown flag is RBPF_EINVAL, checked before anything is queued: nothing is
 * written.  The call changes no engine state (maps, particles, random streams, counters).  It runs on the handle's
 * stream; without RBPF_CAST_DEVICE_OUT the outputs are host arrays, complete on return. */
#define RBPF_CAST_DEVICE_OUT 1u    /* ranges / status are device pointers, written in stream order, no host wait */
int  rbpf_cast_scans(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* angles,
                     int32_t n_beams, double max_range, uint32_t flags, double* ranges, uint8_t* status);

/* ---- global localization: where in a particle's map does this scan fit? -------------------------------------------------
 * Scores the scan at every candidate pose (X, Y, r) of the box box4 = {x0, x1, y0, y1} (mosaic cells, half-open, the layout of
 * rbpf_render_map) in the map of `particle` (>= 0), the robot standing at the centre of cell (X, Y) with heading theta_r.
 * With v(X, Y) the lattice value rbpf_render_map gives (0 without a tile, outside a tile's written box, outside the lattice):
 *   occ(X, Y)  = v * quantum > occupied_threshold            dil(X, Y) = OR of occ over the 3 x 3 cells round (X, Y)
 *   F(X, Y)    = occ + dil  in {0, 1, 2}                     cand(X, Y) = v < 0   (observed free)
 * Beam b is used iff match_min_range < ranges[b] < match_max_range (n_used of them); bx = ranges[b] cos(angles[b]),
 * by = ranges[b] sin(angles[b]) (host libm, as rbpf_set_scan).  theta_r = (r * 6.283185307179586) / n_rot, r = 0 .. n_rot-1,
 * c_r = cos(theta_r), s_r = sin(theta_r) (host libm).  In float64, every operation rounded on its own, inv = dim / tile_len:
 *   u[r,b] = floor(0.5 + (c_r bx - s_r by) inv)              w[r,b] = floor(0.5 + (s_r bx + c_r by) inv)
 *   score(X, Y, r) = sum over used b of F(X + u[r,b], Y + w[r,b])        (end points anywhere in the map, not only in the box)
 *   best[X-x0][Y-y0] = max_r score(X, Y, r)      rot[X-x0][Y-y0] = the smallest r that attains it       where cand(X, Y),
 *   both -1 elsewhere.  best <= 2 n_used; with no used beam best = rot = 0 on candidates.  rot may be NULL.
 * Independent of rbpf_set_scan: 1 <= n_beams <= 16384, 1 <= n_rot <= 4096.  The box must lie in the tile lattice and hold
 * fewer than 2^31 cells.  A NULL box4, ranges, angles or best, a non-finite range or angle, a bad particle, n_beams, n_rot or
 * box, or an unknown flag is RBPF_EINVAL; a call between rbpf_scan_update_begin and _end is RBPF_ESTATE; both are checked
 * before anything is queued, and nothing is written.  A box whose scratch would pass 2 GiB is RBPF_ENOMEM.  The call changes
 * no engine state (maps, particles, random streams, counters, duplicate grouping).  It runs on the handle's stream; without
 * RBPF_LOCATE_DEVICE_OUT the outputs are host arrays, complete on return. */
#define RBPF_LOCATE_DEVICE_OUT 1u  /* best / rot are device pointers, written in stream order, no host wait */
int  rbpf_locate_scan(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* ranges, const double* angles,
                      int32_t n_beams, int32_t n_rot, uint32_t flags, int32_t* best, int32_t* rot);

/* ---- alignment: where in a particle's map does this point set (a map of unknown pose) fit? ------------------------------
 * Scores a set of occupied points occ_xy[n_occ][2] and free points free_xy[n_free][2] (metres, in a frame of their own) at
 * every pose (X, Y, r) of the box box4 = {x0, x1, y0, y1} and the rotation window r = r_begin .. r_begin + r_count - 1 in the
 * map of `particle` (>= 0): the origin of the points' frame stands at the centre of cell (X, Y), turned by theta_r.  v, occ,
 * dil, F, inv, theta_r, c_r, s_r (host libm), the mosaic cells and box4 are those of rbpf_locate_scan.  In float64, every
 * operation rounded on its own, for occupied and free points (px, py) alike:
 *   u[r,k] = floor(0.5 + (c_r px_k - s_r py_k) inv)          w[r,k] = floor(0.5 + (s_r px_k + c_r py_k) inv)
 *   hits (X, Y, r) = sum over occupied points of F(X + u, Y + w)                        in 0 .. 2 n_occ
 *   clash(X, Y, r) = number of free points with occ(X + u, Y + w)                       in 0 .. n_free
 *   score(X, Y, r) = hits - 2 clash                                                     in -2 n_free .. 2 n_occ
 *   best[X-x0][Y-y0] = max over the window of score      rot[X-x0][Y-y0] = the smallest r of the window that attains it
 * Every cell of the box is a candidate: there is no gate and no -1.  (The kernels sum hits + 2 (n_free - clash) >= 0 and
 * subtract 2 n_free at the end.)  Limits: 1 <= n_occ, 0 <= n_free (free_xy may then be NULL), n_occ + n_free <= 32767;
 * 1 <= n_rot <= 4096, 0 <= r_begin, 1 <= r_count, r_begin + r_count <= n_rot; the box must lie in the tile lattice and hold
 * fewer than 2^31 cells; M = ceil(max_k hypot(px_k, py_k) inv) + 1 (host libm) must not pass 16384.  A NULL box4, occ_xy,
 * best or rot, a non-finite coordinate, a bad particle, box, count, window or M, or an unknown flag is RBPF_EINVAL; a call
 * between rbpf_scan_update_begin and _end is RBPF_ESTATE; scratch beyond 2 GiB is RBPF_ENOMEM; all are checked before
 * anything is queued, and nothing is written.  The call changes no engine state (maps, particles, random streams,
 * counters, duplicate grouping).  It runs on the handle's stream; without RBPF_ALIGN_DEVICE_OUT the outputs are host
 * arrays, complete on return. */
#define RBPF_ALIGN_DEVICE_OUT 1u   /* best / rot are device pointers, written in stream order, no host wait */
int  rbpf_align_points(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* occ_xy, int32_t n_occ,
                       const double* free_xy, int32_t n_free, int32_t n_rot, int32_t r_begin, int32_t r_count, uint32_t flags,
                       int32_t* best, int32_t* rot);

/* ---- view gain: which map cells would a scan taken at a pose observe? ----------------------------------------------------
 * For each pose (x, y, theta) the rays are exactly those of rbpf_cast_scans (same host libm cos / sin of theta and of each angle,
 * same float64 walk, inv and tlim = max_range * inv, same tie rule and the same strict "occupied" test).  The
 * visited set V of a pose in a map is the set of DISTINCT mosaic cells that the walk of any of its beams tests while inside the
 * lattice: the origin cell, every cell entered with t <= tlim, and the hit cell that ends a ray (an occupied cell that is seen
 * is observed); nothing behind a hit, nothing outside the lattice; V is empty when the origin cell lies outside the lattice.
 * With v(c) the lattice value rbpf_render_map gives for cell c and vmin = min_odds_emp / quantum:
 *   seen    = |V|
 *   unknown = #{c in V : v(c) == 0}
 *   gain    = sum over c in V of value_tab[v(c) - vmin]
 * value_tab has (max_odds_occ - min_odds_emp) / quantum + 1 entries (61 with the defaults), each in 0 .. 2^20.  All three are
 * exact integers: the result does not depend on any summation order and is bit-identical from call to call.  DESIGN.md 3.11
 * has the kernel.
 * particle >= 0: outputs are [n_poses], every pose in that particle's map.  particle == -1: outputs are [P][n_poses], EVERY
 * pose in EVERY particle's map (what an expectation over the posterior needs) - unlike rbpf_cast_scans, which pairs pose n
 * with particle n.  seen and unknown may each be NULL.
 * Window limit: with M = ceil(max_range * inv) + 2 every visited cell lies within M cells of the origin cell on each axis, and
 * the kernel keeps the (2M + 1)^2 window as a bitmap in one workgroup's LDS: 2M + 1 <= 1024 is required (max_range up to about
 * 25.4 m at 0.05 m cells, 12.7 m at 0.025 m, 50.9 m at 0.1 m), otherwise RBPF_EINVAL; the message gives the largest admissible
 * max_range.
 * A NULL poses_n3, angles, value_tab or gain, a non-finite pose or angle, max_range not finite or not > 0, n_beams < 1,
 * n_poses < 1, n_poses * n_beams >= 2^31, a table entry out of range, a bad particle or an unknown flag is RBPF_EINVAL; a call
 * between rbpf_scan_update_begin and _end is RBPF_ESTATE; both are checked before anything is queued, and nothing is written.
 * The call changes no engine state (maps, particles, random streams, counters, duplicate grouping).  It runs on the handle's
 * stream; without RBPF_GAIN_DEVICE_OUT the outputs are host arrays, complete on return. */
#define RBPF_GAIN_DEVICE_OUT 1u    /* gain / seen / unknown are device pointers, written in stream order, no host wait */
int  rbpf_view_gain(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* angles,
                    int32_t n_beams, double max_range, const int32_t* value_tab, uint32_t flags, int64_t* gain, int32_t* seen,
                    int32_t* unknown);

/* ---- travel cost: can the robot get there, how far is it, and which way? ---------------------------------------------------
 * Clearance, traversable set and shortest-path cost from a set of start points to every cell of the box box4 = {x0, x1, y0, y1}
 * (mosaic cells, half-open, raster layout [x1-x0][y1-y0] and v(X, Y) of rbpf_render_map / rbpf_locate_scan: v is 0 without a tile,
 * outside a tile's written box and outside the lattice) in the map of `particle`.  occ(c) = v(c) * quantum > occupied_threshold,
 * strict.  A point (x, y) in metres lies in cell (floor(x * inv), floor(y * inv)), inv = dim / tile_len, in float64 as
 * rbpf_cast_scans forms its origin cell.  All results are integers in chamfer units: an axial step costs 5, a diagonal step 7, so
 * cost * (tile_len / dim) / 5 is metres.
 *   d(c)         = min over ALL occupied cells o of the map (outside the box too) of 5 max(|dx|, |dy|) + 2 min(|dx|, |dy|)
 *   clearance[c] = min(d(c), clear_max).  Only occupied cells count, unknown ones do not.  0 <= inflate < clear_max <= 320; the
 *                  map is read over the box grown by ceil(clear_max / 5) cells (v = 0 outside the lattice), which is exact.
 *   blocked(c)   = v(c) >= 0: only known-free cells carry the robot; with RBPF_TRAVEL_THROUGH_UNKNOWN blocked(c) = occ(c)
 *   T            = {c in box : !blocked(c) and d(c) > inflate}, plus every start cell that lies in the box (the robot is where it
 *                  is).  Start points outside the box are ignored; if none lies inside, every cost is -1 and the call succeeds.
 *   cost[c]      = length of the shortest path from any start cell to c over cells of T by steps to the 8 neighbours (5 axial, 7
 *                  diagonal); the diagonal step (X, Y) -> (X+sx, Y+sy) needs both (X+sx, Y) and (X, Y+sy) in T (no corner is
 *                  cut).  0 on start cells, -1 where there is no path, so on every cell outside T.  It is the unique least fixed
 *                  point of the relaxation: independent of evaluation order, identical from call to call.
 *   goal_cost[g] = cost at the cell of goal g, -1 for a goal outside the box.
 * The box must hold at least one and at most 2^27 cells (7 * 2^27 fits an int32) and lie in the tile lattice.
 * particle >= 0: all n_start >= 1 starts are sources in that particle's map; cost (int32 [nx][ny]), clearance (uint16 [nx][ny]) and
 * goal_cost ([n_goals]) may each be NULL, but not all; goal_cost needs goal_xy and n_goals >= 1 (goal_xy is read only then).
 * particle == -1: cost and clearance must be NULL; goal_cost is [P][n_goals], EVERY goal in EVERY particle's map (as
 * rbpf_view_gain); n_start is 1 (the same start in every map) or P (start n in particle n's map, the pairing of rbpf_cast_scans).
 * The particles are worked on in batches whose scratch stays under 2 GiB; the environment variable RBPF_TRAVEL_BATCH=<n>, read per
 * call, caps a batch at n particles (for tests).  One particle whose scratch would pass 2 GiB is RBPF_ENOMEM.
 * rounds (may be NULL) receives the number of relaxation rounds launched, summed over the batches: a diagnostic.  Rounds are
 * queued several at a time between two reads of their counters, so it is a multiple of that number.  DESIGN.md 3.12 has the kernels.
 * A NULL box4 or start_xy, a wrong NULL pattern, a non-finite coordinate, a bad particle, count, box, inflate or clear_max, a box
 * that leaves the lattice or holds more than 2^27 cells, or an unknown flag is RBPF_EINVAL; a call between rbpf_scan_update_begin
 * and _end is RBPF_ESTATE; all are checked before anything is queued, and nothing is written.  The call changes no engine state
 * (maps, particles, random streams, counters, duplicate grouping).  It runs on the handle's stream; without
 * RBPF_TRAVEL_DEVICE_OUT the outputs are host arrays, complete on return; with it the call still waits for its own convergence
 * reads but not for the outputs.  rounds is complete on return either way. */
#define RBPF_TRAVEL_DEVICE_OUT      1u   /* cost / clearance / goal_cost are device pointers, stream order, no host wait for them */
#define RBPF_TRAVEL_THROUGH_UNKNOWN 2u   /* cells that are not known free may be crossed unless occupied */
int  rbpf_travel_cost(rbpf_handle* h, int32_t particle, const int32_t* box4, const double* start_xy, int32_t n_start,
                      const double* goal_xy, int32_t n_goals, int32_t inflate, int32_t clear_max, uint32_t flags, int32_t* cost,
                      uint16_t* clearance, int32_t* goal_cost, int32_t* rounds);
/* How the last successful rbpf_travel_cost of this handle went (test / inspection entry): out3 = {relaxation rounds launched,
 * block runs: (particle, block, round) triples whose workgroup did not leave at once, (particle, block) pairs}.  A sweep of
 * every block in every round would be out3[0] * out3[2] block runs. */
int  rbpf_travel_stats(rbpf_handle* h, uint64_t* out3);

/* ---- path checks: is this path free, in which share of the posterior, and which of these rollouts keeps clear of the walls? ----
 * n_paths polylines walked cell by cell through the map of `particle` and every step's cell tested.  xy is [path_start[n_paths]][2]
 * waypoints in metres, path_start [n_paths + 1] their CSR offsets, strictly increasing from 0: every path has at least one
 * waypoint.  v(X, Y), occ(c) (strict), inv, the cell of a point (floor(x * inv), float64, on the host), d(c) over ALL occupied cells
 * of the map, the chamfer units, 0 <= inflate < clear_max <= 320 and blocked(c) with or without the through-unknown flag are those
 * of rbpf_travel_cost.
 * The walk, in exact integers and in closed form (no step depends on the step before it): step 0 of a path is the cell of waypoint
 * 0.  A segment from cell A to cell B with ax = |XB - XA|, ay = |YB - YA|, n = max(ax, ay) and signs sx, sy adds the steps
 * t = 1 .. n: if ax >= ay, X = XA + sx t and Y = YA + sy floor((2 t ay + n) / (2 n)); otherwise with the roles of x and y swapped.
 * n = 0 adds nothing.  Consecutive cells are 8-neighbours, step n stands on B, and steps[k] = 1 + the sum of n over path k.
 *   ok(c)         = !blocked(c) and d(c) > inflate; with RBPF_PATHS_START_EXEMPT ok(cell of step 0) is true wherever that cell is tested
 *   blocked step  = its cell is not ok, or it is diagonal (both coordinates differ from the cell (Xp, Yp) of the step before) and
 *                   (X, Yp) or (Xp, Y) is not ok: T and the no-corner-cut rule of rbpf_travel_cost, so a path that plan.path_to walks
 *                   down a cost field checks clear in the same map with the same inflate and RBPF_PATHS_START_EXEMPT
 *   out[..][4]    = {first_blocked: the least blocked step, -1 if none;  first_unknown: the least step whose cell has v == 0, -1 if
 *                   none;  min_clearance: min over the path's cells (side cells not included) of min(d, clear_max);  n_unknown: the
 *                   number of steps whose cell has v == 0, a cell visited again counted again}                       (int32)
 * All four are order-free reductions of exact integers: bit-identical from call to call.
 * particle >= 0: out is [n_paths][4].  particle == -1: out is [P][n_paths][4], EVERY path in EVERY particle's map (as
 * rbpf_view_gain).  particle == -1 with RBPF_PATHS_OWN: n_paths = P * K, the paths [p K, (p + 1) K) are checked in the map of
 * particle p alone (rollouts from each particle's own pose), and out is [P][K][4].
 * steps (may be NULL) is a host array [n_paths], computed on the host and complete on return whatever the flags.
 * A waypoint whose cell lies outside the tile lattice is RBPF_EINVAL (the message names the path and the waypoint), so every walked
 * cell lies in the lattice and only the clearance margin can leave it, where v = 0.  Also RBPF_EINVAL: a NULL xy, path_start or out, a
 * non-finite coordinate, an offset table that does not start at 0 or does not increase strictly, n_paths < 1, a bad particle,
 * inflate, clear_max or flag, RBPF_PATHS_OWN without particle == -1 or with n_paths % P != 0, a path of more than 2^20 steps, and
 * 2^29 or more results (P * n_paths with particle == -1 without RBPF_PATHS_OWN, n_paths otherwise).  A call between
 * rbpf_scan_update_begin and _end is RBPF_ESTATE.  Everything is checked before anything is queued, and nothing is written on an
 * error.  The call changes no engine state (maps, particles, random streams, counters, duplicate grouping).  It runs on the
 * handle's stream, in one launch over (particle, path) with no per-particle scratch; without RBPF_PATHS_DEVICE_OUT out is a host
 * array, complete on return.  DESIGN.md 3.22 has the kernel. */
#define RBPF_PATHS_DEVICE_OUT      1u  /* out is a device pointer, written in stream order, no host wait */
#define RBPF_PATHS_THROUGH_UNKNOWN 2u  /* as RBPF_TRAVEL_THROUGH_UNKNOWN */
#define RBPF_PATHS_START_EXEMPT    4u  /* the cell of a path's first waypoint counts as traversable (the robot is where it is) */
#define RBPF_PATHS_OWN             8u  /* particle == -1 only: path group p belongs to particle p */
int  rbpf_check_paths(rbpf_handle* h, int32_t particle, const double* xy, const int32_t* path_start, int32_t n_paths,
                      int32_t inflate, int32_t clear_max, uint32_t flags, int32_t* out, int32_t* steps);

/* ---- rollout checks: the same K motion templates from every pose, placed on the GPU ------------------------------------------
 * What a local planner asks every control cycle: a fan of arcs in the robot's frame, driven from each of n_poses poses, each rollout
 * walked and tested as a path of rbpf_check_paths.  tmpl_xy is [tmpl_start[n_tmpl]][2] waypoints (lx, ly) in metres in the robot's
 * frame, tmpl_start [n_tmpl + 1] their CSR offsets, strictly increasing from 0; every template has 1 .. 128 waypoints.  poses_n3
 * is [n_poses][3] = x, y, theta.  particle >= 0: every pose is checked in that particle's map; particle == -1: n_poses must equal
 * P and pose p is checked in particle p's map, the pairing of rbpf_check_scans.  (Every template in every map is
 * rbpf_check_paths's, with particle == -1.)
 * The placement.  The host turns each pose into x, y, c = cos(theta), s = sin(theta) with its libm: the device never sees an
 * angle.  Waypoint j of template k at pose n is, every operation a float64 operation rounded on its own and in this order,
 *   wx = x + (c * lx - s * ly)          wy = y + (s * lx + c * ly)
 *   cell = (floor(wx * inv), floor(wy * inv)),  inv = dim / tile_len as for rbpf_check_paths.
 * The walk.  With the waypoint cells so placed, wstep[0] = 0, wstep[j] = wstep[j - 1] + max(|dX|, |dY|) of the cells of waypoints
 * j - 1 and j, and steps = wstep[m - 1] + 1 for a template of m waypoints.  The closed-form walk, ok(c), the blocked step, the
 * exemption of the cell of step 0 and the four outputs are those of rbpf_check_paths, applied to these cells.
 *   out[n_poses][n_tmpl][4]   int32, the four results of rbpf_check_paths.  Required.
 *   steps[n_poses][n_tmpl]    int32, computed on the device.  May be NULL.  It lives where out lives: a host array complete on
 *                             return, or with RBPF_PATHS_DEVICE_OUT a device pointer written in stream order.
 * flags: RBPF_PATHS_DEVICE_OUT, RBPF_PATHS_THROUGH_UNKNOWN and RBPF_PATHS_START_EXEMPT as for rbpf_check_paths; RBPF_PATHS_OWN and
 * any other bit are RBPF_EINVAL.
 * What is checked instead of N * K * M waypoints: with rmax the largest |lx| + |ly| over all template waypoints (it bounds both
 * rotated coordinates whatever the heading, |c|, |s| <= 1) and reach = ceil(rmax * inv) + 2 cells, a pose is RBPF_EINVAL (the
 * message names it) if the square of half-side reach round its own cell (floor(x * inv), floor(y * inv)) leaves the tile lattice,
 * and the call is RBPF_EINVAL if (m_max - 1) * 2 * reach >= 2^20, m_max the waypoints of the longest template.  So every placed
 * waypoint's cell lies in the lattice and no rollout has more than 2^20 steps (DESIGN.md 3.24 has the argument for the two cells).
 * Also RBPF_EINVAL: a NULL poses_n3, tmpl_xy, tmpl_start or out, a non-finite pose or template coordinate or a non-finite
 * rmax * inv, an offset table that does not start at 0 or does not increase strictly, a template of more than 128 waypoints,
 * n_poses < 1 or n_tmpl < 1, a bad particle, particle == -1 with n_poses != P, a bad inflate or clear_max (the bounds of
 * rbpf_check_paths), and n_poses * n_tmpl >= 2^29.  A call between rbpf_scan_update_begin and _end is RBPF_ESTATE.  Everything is
 * checked before anything is queued, and nothing is written on an error.  The call changes no engine state (maps, particles,
 * random streams, counters, duplicate grouping).  It runs on the handle's stream in one launch over (pose, template); what is
 * uploaded is 32 bytes a pose and 16 a template waypoint.  DESIGN.md 3.24 has the kernel. */
int  rbpf_check_rollouts(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* tmpl_xy,
                         const int32_t* tmpl_start, int32_t n_tmpl, int32_t inflate, int32_t clear_max, uint32_t flags, int32_t* out,
                         int32_t* steps);

/* ---- footprint checks: the rollouts of rbpf_check_rollouts, driven by a robot that is no disc ----------------------------------
 * A disc's clearance does not depend on heading; a 0.8 m x 0.5 m base's does.  Every step of every rollout tests, besides the
 * inscribed-radius test at its centre, the cells an oriented footprint covers there, and a turn on the spot sweeps the corners.
 * Templates, poses, placement and walk are those of rbpf_check_rollouts, unchanged: tmpl_xy / tmpl_start in CSR with 1 .. 128
 * waypoints a template, c = cos(theta) and s = sin(theta) from the host's libm, wx = x + (c * lx - s * ly) in float64 with every
 * operation rounded on its own, cell = floor(w * inv), wstep from max(|dX|, |dY|), the closed-form walk, steps = wstep[m - 1] + 1,
 * the reach check on the poses and the bound of 2^20 steps.
 * The footprint table.  n_bins = H heading bins, 1 <= H <= 256; bin b stands for the heading 2 pi b / H.  fp_start [H + 1] is a
 * CSR offset table from 0, every bin holds 1 .. 256 spans, fp_span is [fp_start[H]][3] = (dx, y0, y1) with |dx| <= 127,
 * -127 <= y0 <= y1 <= 127 and y1 - y0 <= 63.  A robot whose centre stands on the cell (X, Y) in bin b covers the cells
 * (X + dx, Y + y), y0 <= y <= y1, of bin b's spans: spans run along y, the contiguous axis of a tile row.  A covered cell outside
 * the tile lattice has v = 0, as the clearance margin of rbpf_check_paths.
 * Heading bins: the device never sees an angle.  The entry point forms, on the host in float64 and in this order,
 *   pb[n] = floor(theta_n * (H / (2 pi)) + 0.5) mod H      (pi = M_PI; reduced into 0 .. H - 1 for negative headings)
 * and |theta * H / (2 pi)| >= 2^31 is RBPF_EINVAL.  tmpl_bin [tmpl_start[n_tmpl]] holds, per template waypoint, a bin in [0, H):
 * the same formula applied to the waypoint's heading in the robot's frame.  Waypoint j tests bin (pb[n] + tmpl_bin[j]) mod H.  The
 * two roundings come to one bin at the most; the table is the caller's to pad for it (plan.footprint_table does).
 * Which bins a step tests.  A step s that stands on waypoints (s = wstep[j]) tests the bin of every such j: repeated waypoints
 * test every heading they carry, and a turn on the spot is one step with m bins.  A step strictly between the waypoints j - 1 and
 * j, t = 1 .. n - 1 of a segment of n steps, tests the bin of j - 1 if 2 t < n, else that of j.
 * The rules.  v, occ, blocked(c) with and without RBPF_PATHS_THROUGH_UNKNOWN, d(c), the chamfer units and
 * 0 <= inflate < clear_max <= 320 are those of rbpf_travel_cost.  exempt(c) holds when exempt >= 0 and c lies within Chebyshev
 * distance `exempt` of the cell of step 0 (the robot is where it is); exempt = -1 turns it off, exempt > 255 is RBPF_EINVAL.
 *   blocked step  = its centre cell c0 is not exempt and (blocked(c0) or d(c0) <= inflate), or some covered cell c of a tested
 *                   bin is not exempt and blocked(c).  The centre test is the inscribed-radius test; there is no corner-cut
 *                   rule, the footprint has area.
 *   out[..][4]    = {first_blocked: the least blocked step, -1 if none;  first_unknown: the least step at which the centre or a
 *                   tested covered cell has v == 0, -1 if none;  min_clearance: min over the centre cells of min(d, clear_max),
 *                   exactly that of rbpf_check_rollouts;  n_unknown: the number of such steps, each counted once; the exemption
 *                   does not touch it}                                                                              (int32)
 * All four are order-free reductions of exact integers.  steps is as for rbpf_check_rollouts: may be NULL, lives where out lives.
 * particle >= 0: every pose in that map, out [n_poses][n_tmpl][4].  particle == -1 with n_poses == P: pose p in particle p's map;
 * with n_poses == 1: that pose in EVERY particle's map; out [P][n_tmpl][4] both times.  A world path across the posterior is a
 * template at the pose (0, 0, 0), where the placement is the identity bit for bit.
 * flags: RBPF_PATHS_DEVICE_OUT and RBPF_PATHS_THROUGH_UNKNOWN; any other bit is RBPF_EINVAL.
 * RBPF_EINVAL, raised before anything is queued, with nothing written and a message that names the offender: everything
 * rbpf_check_rollouts rejects, a NULL tmpl_bin, fp_span or fp_start, a bin outside [0, H), a bad n_bins, an offset table that
 * does not start at 0, has an empty bin or more than 256 spans in a bin, a span outside its bounds, a bad exempt, particle == -1
 * with n_poses neither 1 nor P, and 2^29 or more results.  A call between rbpf_scan_update_begin and _end is RBPF_ESTATE.  The
 * call changes no engine state.  It runs on the handle's stream in one launch; what is uploaded is 36 bytes a pose, 20 a template
 * waypoint and 4 a span.  DESIGN.md 3.25 has the kernel. */
int  rbpf_check_footprints(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* tmpl_xy,
                           const int32_t* tmpl_bin, const int32_t* tmpl_start, int32_t n_tmpl, const int32_t* fp_span,
                           const int32_t* fp_start, int32_t n_bins, int32_t inflate, int32_t clear_max, int32_t exempt, uint32_t flags,
                           int32_t* out, int32_t* steps);

/* ---- local map: what is around the robot, in the robot's frame, fused over the particles ------------------------------------------
 * The raster a local planner, a controller or an obstacle layer asks for every cycle: a window of n x n cells of cell_out metres
 * with the robot at a fixed place in it.  Particles whose trajectories have drifted apart hold the same room at different world
 * positions, so the world-frame sum of rbpf_render_map doubles every wall; relative to each particle's own pose they agree.
 * poses_n3 is [n_poses][3] = x, y, theta.  particle >= 0: every pose is read in that particle's map; particle == -1: n_poses must
 * equal P and pose p is read in particle p's map, the pairing of rbpf_check_rollouts and rbpf_check_scans.
 * The host turns each pose into x, y, c = cos(theta), s = sin(theta) with its libm: the device never sees an angle.
 * Sample tables.  With S = samples (1 .. 8) and n >= 1, the host forms in float64, for q = 0 .. n S - 1,
 *   gx[q] = ((q / S) + ((q % S) + 0.5) / S - 0.5 n) * cell_out + fx        (q / S and q % S in integers)
 *   gy[q] the same with fy,
 * every operation rounded on its own, in the written order; offset2 = (fx, fy), NULL for (0, 0), is the window's centre in the
 * robot's frame in metres (a look-ahead window).  The device does not recompute the tables.
 * Placement of the sample (qa, qb) at a pose, exactly that of rbpf_check_rollouts, every operation a float64 operation rounded on
 * its own and in this order:
 *   wx = x + (c * gx[qa] - s * gy[qb])          wy = y + (s * gx[qa] + c * gy[qb])
 *   X = floor(wx * inv), Y = floor(wy * inv),   inv = dim / tile_len.
 * v(X, Y) is the lattice value of rbpf_render_map in the pose's map: 0 without a tile, outside a tile's written box and outside
 * the lattice.  A pose near or beyond the lattice's edge is legal; its window reads 0 there.
 * Per pose and output cell (i, j), i along the robot's x (forward), j along its y (left), row-major [n][n]:
 *   m = max of v over the samples qa in [i S, i S + S), qb in [j S, j S + S)
 * the rule of rbpf_place_map: a wall that crosses any part of the cell keeps it, a cell is free only if all of it is.  S = 1 is
 * nearest neighbour.
 *   crops[n_poses][n][n]   int8, m.  May be NULL.
 *   fused[n][n][4]         int64, may be NULL (not both).  With thr = occupied_threshold / quantum (strict, as everywhere) and k
 *                          over the poses: {occ_w = sum wq_k [m_k > thr], free_w = sum wq_k [m_k < 0], unknown_w = sum wq_k [m_k == 0],
 *                          sum_wv = sum wq_k m_k}.
 * wq is host uint32 [n_poses]; NULL: every weight is 1.  A pose with wq = 0 adds nothing to fused and still gets its crop.  All
 * four sums are sums of exact integers: order-free, bit-identical from call to call whatever the grouping.
 * Without RBPF_LOCAL_DEVICE_OUT fused and crops are host arrays, complete on return; with it they are device pointers written in
 * stream order, with no host wait.
 * The window in LDS.  With h = 0.5 n cell_out, reach = ceil(hypot(|fx| + h, |fy| + h) * inv) + 2 cells: every sample of a pose
 * lies in the square of half-side reach round the pose's own cell (floor(x inv), floor(y inv)), since |c a - s b| <=
 * hypot(a, b) hypot(c, s) and the two spare cells cover the rounding of c, s and of the six operations (DESIGN.md 3.26 has the
 * argument).  One workgroup stages that square as bytes; 2 reach + 1 > RBPF_LOCAL_MAX_SIDE is RBPF_EINVAL, and the message gives
 * the side and the limit.
 * RBPF_EINVAL, checked before anything is queued, with nothing written: a NULL poses_n3, fused and crops both NULL; a non-finite
 * pose, cell_out or offset; cell_out <= 0, n < 1, samples outside 1 .. 8, n_poses < 1; a bad particle, particle == -1 with
 * n_poses != P; |x inv| or |y inv| >= 2^30 (the message names the pose); sum wq equal to 0 or above 2^31 - 1;
 * n_poses * n * n >= 2^31; an unknown flag; the window limit.  A window whose single crop and sums exceed the scratch cap of
 * 256 MiB is RBPF_ENOMEM.  A call between rbpf_scan_update_begin and _end is RBPF_ESTATE.
 * The call changes no engine state (maps, particles, random streams, counters, duplicate grouping) and runs on the handle's
 * stream.  Poses are worked on in batches whose scratch (crops not asked for, group sums) stays under 256 MiB; the environment
 * variable RBPF_LOCAL_BATCH=<k>, read per call, caps a batch at k poses (tests).  Batches add into fused; the sums are integers,
 * so the result does not depend on k.  DESIGN.md 3.26 has the kernels. */
#define RBPF_LOCAL_DEVICE_OUT 1u   /* fused / crops are device pointers, written in stream order, no host wait */
#define RBPF_LOCAL_MAX_SIDE   384  /* largest LDS window side in map cells */
int  rbpf_local_map(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const uint32_t* wq, int32_t n,
                    double cell_out, int32_t samples, const double* offset2, uint32_t flags, int64_t* fused, int8_t* crops);

/* ---- scan checks: how well does the scan the robot took agree with a particle's map? ----------------------------------------
 * ranges is [n_scans][n_beams] in metres, n_scans 1 (one scan, checked at every pose) or n_poses (scan n at pose n); non-finite
 * and non-positive ranges are data and are classified below.  particle >= 0: every pose (x, y, theta) is checked in that particle's
 * map; particle == -1: n_poses must equal P and pose n is checked in particle n's map, the pairing of rbpf_cast_scans.
 * Beam b of pose n is the ray of rbpf_cast_scans (same host libm cos / sin of theta and of the angles, same float64 supercover walk
 * with every operation rounded on its own, same tie rule, strict "occupied" test and lattice test); only the limit
 * differs.  With inv = dim / tile_len, z the beam's measured range, tz = z * inv, ttol = tol * inv and tmax = max_range * inv, each
 * beam gets a class (uint8):
 *   0 RBPF_SCAN_SKIP     !(z > 0) - NaN, -inf, 0 and negatives - or z < min_range.  No walk.
 *   a returned beam, z < max_range, is walked with tlim = min(tz + ttol, tmax):
 *   1 RBPF_SCAN_MATCH    the walk hits (status 1) at entry parameter t, and d = t - tz >= -ttol
 *   2 RBPF_SCAN_LONG     the walk hits and d < -ttol: the map holds a wall well in front of the measured end
 *   3 RBPF_SCAN_SHORT    no hit within tlim (status 0) and v(E) < 0, E the last cell the walk tested whose entry parameter is <= tz
 *                        (the origin cell is entered at 0) and v the lattice value of rbpf_render_map (0 without a tile and outside a
 *                        tile's written box): the beam ended in observed-free space, on something the map does not hold
 *   4 RBPF_SCAN_NEW      status 0 and v(E) >= 0: the end lies in unknown space, or on a cell not yet over the threshold
 *   5 RBPF_SCAN_OFF      the ray or its origin left the tile lattice (status 2), for returned and no-return beams alike
 *   a no-return beam, z >= max_range (+inf included), is walked with tlim = tmax:
 *   6 RBPF_SCAN_MISSING  the walk hits: the map holds a wall within max_range that the sensor did not report
 *   7 RBPF_SCAN_CLEAR    no hit
 * Cost, in exact integers: a MATCH or LONG beam has the bin q = clamp(floor(d * bins_per_cell + 0.5), -half_bins, half_bins), the
 * clamp applied to the float64 before the conversion, and costs class_cost8[class] + hit_tab[q + half_bins]; every other beam costs
 * class_cost8[class].  hit_tab has 2 * half_bins + 1 entries; 1 <= half_bins <= 4096, 1 <= bins_per_cell <= 64; every entry of both
 * tables lies in 0 .. 2^20 (thesis_amd/sensor.py builds them from a beam model: cost / 65536 then reads as bits).
 *   cost[n_poses]             int64: the sum over the pose's beams.  Required.
 *   counts[n_poses][8]        int32: beams per class.  May be NULL.
 *   classes[n_poses][n_beams] uint8.  May be NULL.
 *   votes[n_beams][8]         int32: in how many of the n_poses poses the beam fell into each class.  May be NULL.
 * All are order-free reductions of exact integers: bit-identical from call to call.  DESIGN.md 3.23 has the kernel.
 * A NULL poses_n3, ranges, angles, hit_tab, class_cost8 or cost, a non-finite pose or angle, max_range not finite or not > 0,
 * min_range or tol not finite or < 0, a bad half_bins or bins_per_cell, a table entry out of range, n_scans neither 1 nor n_poses,
 * n_poses < 1, n_beams < 1, n_poses * n_beams >= 2^31, a bad particle, n_poses != P with particle == -1 or an unknown flag is
 * RBPF_EINVAL; a call between rbpf_scan_update_begin and _end is RBPF_ESTATE; everything is checked before anything is queued, and
 * nothing is written on an error.  The call changes no engine state (maps, particles, random streams, counters, duplicate
 * grouping).  It runs on the handle's stream; without RBPF_SCANS_DEVICE_OUT the outputs are host arrays, complete on return. */
#define RBPF_SCANS_DEVICE_OUT 1u   /* cost / counts / classes / votes are device pointers, written in stream order, no host wait */
enum { RBPF_SCAN_SKIP = 0, RBPF_SCAN_MATCH = 1, RBPF_SCAN_LONG = 2, RBPF_SCAN_SHORT = 3, RBPF_SCAN_NEW = 4, RBPF_SCAN_OFF = 5,
       RBPF_SCAN_MISSING = 6, RBPF_SCAN_CLEAR = 7 };
int  rbpf_check_scans(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_poses, const double* ranges,
                      int32_t n_scans, const double* angles, int32_t n_beams, double max_range, double min_range, double tol,
                      const int32_t* hit_tab, int32_t half_bins, int32_t bins_per_cell, const int32_t* class_cost8, uint32_t flags,
                      int64_t* cost, int32_t* counts, uint8_t* classes, int32_t* votes);

/* ---- frontier regions: where does the known map end, and how large is each opening? ---------------------------------------
 * The frontier cells of the box box4 (cells, raster layout and v(X, Y) as for rbpf_travel_cost; occ(c) = v(c) * quantum >
 * occupied_threshold, strict) in the map of `particle`, their connected components, and a table of the largest.  With nx = x1-x0,
 * ny = y1-y0, dx = X-x0, dy = Y-y0 and L(c) = dx * ny + dy:
 *   front(c)  = v(c) < 0 and some 4-neighbour n of c has v(n) == 0 and no cell o with occ(o) lies within Chebyshev distance
 *               `clear` of c.  The REAL map decides: neighbours and occupied cells outside the box count (the map is read over
 *               the box grown by max(clear, 1) cells, v = 0 outside the lattice); 0 <= clear <= 16.
 *   F         = {c in box : front(c)}
 *   region    = a connected component of F under 8-connectivity, members inside the box only (the box clips regions)
 *   label[c]  = min of L over the region of c; -1 for c not in F                                       (int32 [nx][ny])
 *   size, sum_dx, sum_dy, x_min, x_max, y_min, y_max of a region: over its members (sums of dx, dy; the bounds in absolute X, Y)
 *   cx        = floor((2 sum_dx + size) / (2 size)), cy likewise      (the centroid, rounded half up; it need not be a member)
 *   rep       = the member that minimises (dx - cx)^2 + (dy - cy)^2, ties to the smaller L    (a cell the robot can be sent to)
 *   kept      = the regions with size >= min_size, by size descending, ties to the smaller label, the first max_regions of them
 *   regions[k][10] (int64) = {label, size, sum_dx, sum_dy, x_min, x_max, y_min, y_max, rep_X, rep_Y} of kept region k; all -1 for
 *               k >= n_kept
 *   counts[3] = {|F|, number of regions before the size filter, n_kept}
 * Everything is an exact integer, a least fixed point (the labels) or an order-free reduction: the result does not depend on any
 * evaluation order and is bit-identical from call to call.  Limits: 1 <= nx, ny <= 32768, nx * ny <= 2^27, the box lies in the
 * tile lattice, min_size >= 1, 1 <= max_regions <= 1024.
 * particle >= 0: label, regions and counts may each be NULL, but not all three.  particle == -1: label must be NULL, regions is
 * [P][max_regions][10] and counts [P][3], every particle in its own map; regions and counts may each be NULL, not both.  The
 * particles are worked on in batches whose scratch stays under 2 GiB; the environment variable RBPF_FRONTIER_BATCH=<n>, read per
 * call, caps a batch at n particles (for tests).  One particle whose scratch would pass 2 GiB is RBPF_ENOMEM.  DESIGN.md 3.13 has
 * the kernels.
 * A NULL box4, a wrong NULL pattern, a bad particle, box, clear, min_size or max_regions, or an unknown flag is RBPF_EINVAL; a call
 * between rbpf_scan_update_begin and _end is RBPF_ESTATE; all are checked before anything is queued, and nothing is written.  The
 * call changes no engine state (maps, particles, random streams, counters, duplicate grouping).  It runs on the handle's stream;
 * without RBPF_FRONTIER_DEVICE_OUT the outputs are host arrays, complete on return; with it the call still waits for its own
 * convergence reads but not for the outputs. */
#define RBPF_FRONTIER_DEVICE_OUT 1u   /* label / regions / counts are device pointers, stream order, no host wait for them */
int  rbpf_frontier_regions(rbpf_handle* h, int32_t particle, const int32_t* box4, int32_t clear, int32_t min_size,
                           int32_t max_regions, uint32_t flags, int32_t* label, int64_t* regions, int32_t* counts);
/* How the last successful rbpf_frontier_regions of this handle went: out3 = {labelling rounds launched, block runs, (particle,
 * block) pairs}, as rbpf_travel_stats. */
int  rbpf_frontier_stats(rbpf_handle* h, uint64_t* out3);

/* ---- map scores: how close is a particle's map to a reference map? ----------------------------------------------------------
 * The box box4 (cells, raster layout and v(X, Y) as for rbpf_travel_cost) of the map of `particle`, v_p, compared cell by cell
 * with the reference raster `ref`: int8 [x1-x0][y1-y0] in units of quantum as rbpf_load_map takes it, every value in
 * [min_odds_emp, max_odds_occ] / quantum; r(c) is its value at cell c of the box, and there is no reference outside the box.
 * occ(x) = x * quantum > occupied_threshold, strict, the test of the tiles' occupancy bits.  A value x has the class F = 0 if
 * x < 0, O = 2 if occ(x), U = 1 otherwise (unknown cells, and cells that lean occupied but are not past the threshold).
 *   n[a][b]   = #{c in box : class(v_p(c)) == a and class(r(c)) == b}
 *   near_m(c) = some cell o with occ(v_p(o)) lies within Chebyshev distance tol of c.  The REAL map decides: o may lie outside
 *               the box (the map is read over the box grown by tol cells, v = 0 outside the lattice)
 *   near_r(c) = some cell o IN THE BOX with occ(r(o)) lies within Chebyshev distance tol of c
 *   hit_m     = #{c in box : occ(v_p(c)) and near_r(c)}        the particle's walls the reference confirms
 *   hit_r     = #{c in box : occ(r(c)) and near_m(c)}          the reference's walls the particle has found
 *   l1        = sum over the box of |v_p(c) - r(c)|
 *   tab       = sum over the box of value_tab[v_p(c) - vmin], vmin = min_odds_emp / quantum; 0 when value_tab is NULL
 *   scores[13] = {n[F][F], n[F][U], n[F][O], n[U][F], n[U][U], n[U][O], n[O][F], n[O][U], n[O][O], hit_m, hit_r, l1, tab}
 * particle >= 0: scores is [13].  particle == -1: scores is [P][13], every particle in its own map against the same reference;
 * exact duplicates left by a resample are computed again.  0 <= tol <= 16.  value_tab is rbpf_view_gain's table (same length,
 * entries in 0 .. 2^20) or NULL.  The box must hold at least one and at most 2^27 cells and lie in the tile lattice.  Every value
 * is an exact integer and an order-free sum: bit-identical from call to call.  DESIGN.md 3.14 has the kernels.
 * A NULL box4, ref or scores, a bad particle, box, tol, table entry or flag, or a reference value out of range is RBPF_EINVAL (a
 * device reference is checked on the device, and the call waits for the verdict, as rbpf_place_map does); a call between
 * rbpf_scan_update_begin and _end is RBPF_ESTATE; everything is checked before anything is written.  The call changes no engine
 * state (maps, tile pool, particles, random streams, counters, duplicate grouping).  It runs on the handle's stream; without
 * RBPF_SCORE_DEVICE_OUT scores is a host array, complete on return. */
#define RBPF_SCORE_DEVICE_IN  1u   /* ref is a device pointer, read in stream order, validated on the device */
#define RBPF_SCORE_DEVICE_OUT 2u   /* scores is a device pointer, written in stream order, no host wait */
#define RBPF_SCORE_FIELDS 13
int  rbpf_score_maps(rbpf_handle* h, int32_t particle, const int32_t* box4, const int8_t* ref, int32_t tol,
                     const int32_t* value_tab, uint32_t flags, int64_t* scores);

/* ---- pose estimate and trajectory log: where is the robot, and where has every particle been? ----------------------------------
 * The estimate row of a set of poses (x_j, y_j, th_j) with weights w_j >= 0.  weights_mode:
 *   RBPF_W_UNIFORM   w_j = 1
 *   RBPF_W_RESAMPLE  the distribution the resample draws from (main.py:52-56) of the filter's current weights: -inf -> 0, then,
 *                    if the smallest value is negative, its magnitude is added to every non-zero value
 *   RBPF_W_GIVEN     `weights`: P host float64, none negative (RBPF_EINVAL)
 * A particle with w_j = 0, or with a non-finite pose or weight, contributes nothing.  Over the others, in float64:
 *   W = sum w    mx = sum w x / W    my = sum w y / W    S = sum w sin th    C = sum w cos th    mth = atan2(S, C)    R = hypot(S, C) / W
 *   d_j = (x_j - mx, y_j - my, wrap(th_j - mth)),  wrap(a) = remainder(a, 6.283185307179586) moved from -pi to pi: into (-pi, pi]
 *   c   = sum w d d^T / W        n_eff = W^2 / sum w^2
 *   f64 row [RBPF_EST_F64] = {mx, my, mth, cxx, cxy, cxth, cyy, cyth, cthth, R, W, n_eff, 0, 0, 0, 0}; with W = 0 the twelve values
 *                            are NaN
 *   i32 row [RBPF_EST_I32] = {best, n_used, n_alive, 0}: best = the first argmax of the filter's current raw weights whatever the
 *                            mode (a NaN counts as the largest, as np.argmax), n_used = contributing particles, n_alive = -1
 *                            wherever no lineage table is involved
 * The sums run in a fixed order: two calls on the same state return identical bits.
 * rbpf_estimate: the row of the current poses; needs no tracking, changes no engine state, complete on return. */
#define RBPF_W_UNIFORM  0
#define RBPF_W_RESAMPLE 1
#define RBPF_W_GIVEN    2
#define RBPF_EST_F64 16
#define RBPF_EST_I32 4
int  rbpf_estimate(rbpf_handle* h, int32_t weights_mode, const double* weights, double* out16, int32_t* out4);
/* The log.  rbpf_track_begin allocates `capacity` (1 .. 65535 * RBPF_TRACK_CHUNK) records in device memory, 28 bytes per particle
 * and record (rbpf_track_record_bytes), and writes record 0 from the current state.  A record holds bit copies of every particle's
 * pose, parent[j] = the index in the record before of the particle that j continues (record 0: the identity), and the estimate row
 * of that moment (RBPF_W_RESAMPLE, n_alive = -1).  Between records every local resample composes its ancestors onto a pending
 * map on the device (it reads the device's did-resample flag; the host reads nothing, rbpf_resample without outputs stays
 * asynchronous); a record takes parent = pending and resets it.  Records are written
 *   by rbpf_track_begin (record 0) and rbpf_track_record;
 *   at the end of rbpf_imu_update with RBPF_TRACK_IMU;
 *   at the end of rbpf_scan_update / rbpf_scan_update_end with RBPF_TRACK_SCAN (never by rbpf_map_update or rbpf_weight_samples),
 * all in stream order, nothing waits.  With the log full an implicit record is dropped and counted in `dropped` (the call it
 * belongs to still succeeds and pending keeps composing); rbpf_track_record returns RBPF_ENOMEM.
 * Off by default, and then the launches are exactly those of a handle that never heard of it; the same again after
 * rbpf_track_end, which frees the log.  Lineages across ranks are not followed: while tracking is on,
 * rbpf_apply_resample_local and rbpf_unpack_particles return RBPF_ESTATE.
 * RBPF_ESTATE: any rbpf_track_* call but _begin and _record_bytes while tracking is off, and _begin while it is on.  RBPF_EINVAL: a
 * bad capacity, flag, mode, NULL pattern, a range that is not 0 <= t0 < t1 <= n_records, a particle outside 0 .. P-1; checked
 * before anything is queued, and nothing is written. */
#define RBPF_TRACK_IMU   1u        /* rbpf_imu_update records */
#define RBPF_TRACK_SCAN  2u        /* rbpf_scan_update / rbpf_scan_update_end record */
#define RBPF_TRACK_CHUNK 64        /* records per chunk of the walk back */
#define RBPF_TRACK_DEVICE_OUT 1u   /* out_idx / out_pose are device pointers, written in stream order, no host wait */
int  rbpf_track_begin(rbpf_handle* h, int32_t capacity, uint32_t flags);
int  rbpf_track_end(rbpf_handle* h);
int  rbpf_track_record(rbpf_handle* h);
/* any output may be NULL */
int  rbpf_track_info(rbpf_handle* h, int32_t* n_records, int32_t* capacity, int32_t* dropped, uint32_t* flags);
/* The lineage of the CURRENT particles `particles`[n] (NULL, 0: all P, n = P): out_idx[t - t0][k] (int32) = the index in record t
 * of the ancestor of current particle particles[k], through every resample since, those after the last record included;
 * out_pose[t - t0][k][3] (float64) = that ancestor's recorded pose.  Either output may be NULL, not both.  Without
 * RBPF_TRACK_DEVICE_OUT the outputs are host arrays, complete on return. */
int  rbpf_track_lineage(rbpf_handle* h, int32_t t0, int32_t t1, const int32_t* particles, int32_t n, void* out_idx, void* out_pose,
                        uint32_t flags);
/* The smoothed trajectory: out_f64[t - t0][RBPF_EST_F64], out_i32[t - t0][RBPF_EST_I32] = the estimate row over the poses at
 * record t of the current particles' ancestors, with the FINAL weights (weights_mode / weights as rbpf_estimate); n_alive = the
 * number of distinct ancestors at record t.  P <= 65536 (RBPF_EINVAL).  Host outputs, either may be NULL, complete on return. */
int  rbpf_track_summary(rbpf_handle* h, int32_t t0, int32_t t1, int32_t weights_mode, const double* weights, double* out_f64,
                        int32_t* out_i32);
/* the rows stored at record time (the filtered trajectory); host outputs, either may be NULL, complete on return */
int  rbpf_track_filtered(rbpf_handle* h, int32_t t0, int32_t t1, double* out_f64, int32_t* out_i32);
/* Checkpoints.  rbpf_track_export copies the raw records [t0, t1) (0 <= t0 <= t1 <= n_records), rbpf_track_record_bytes(h) bytes
 * each (a function of P alone, no tracking needed; -1 for a NULL handle), followed by the pending map (P int32) into host memory.
 * rbpf_track_import replaces the log of a tracking handle by n such records (1 <= n <= capacity) followed by a pending map;
 * n_records becomes n.  A parent or pending index outside 0 .. P-1 is RBPF_EINVAL and nothing is replaced. */
int64_t rbpf_track_record_bytes(rbpf_handle* h);
int  rbpf_track_export(rbpf_handle* h, int32_t t0, int32_t t1, void* records);
int  rbpf_track_import(rbpf_handle* h, int32_t n, const void* records);

/* ---- pose modes: which hypotheses are alive, how heavy is each, and where? ---------------------------------------------------
 * A set is P poses (x_j, y_j, th_j) with the effective weights w_j of weights_mode / weights (as rbpf_estimate; the RBPF_W_RESAMPLE
 * shift is taken over all P).  Parameters: bin_xy (metres, finite, > 0), n_th (heading bins, 1 .. 4096), max_modes K
 * (1 .. RBPF_MODES_MAX).  The host computes inv = 1.0 / bin_xy and kth = (double)n_th / 6.283185307179586 once, in float64.
 *   bin of a particle     ix = floor(x * inv), iy = floor(y * inv), it = floor(th * kth) mod n_th taken non-negative: one IEEE
 *                         multiplication and a floor each; any finite th is accepted, nothing is wrapped beforehand
 *   contributing          finite w > 0 and a finite pose (the rule of the estimate row), and |x * inv| < 2^23, |y * inv| < 2^23,
 *                         |th * kth| < 2^40.  Everyone else contributes nothing and has label -1
 *   adjacency             two occupied bins with |dix| <= 1, |diy| <= 1 and cyclic distance of `it` modulo n_th <= 1: the
 *                         26-neighbourhood; n_th <= 3 makes all heading bins adjacent, n_th = 1 ignores the heading
 *   mode                  a connected component of occupied bins; its root = the smallest index of its contributing particles,
 *                         its members = the contributing particles in its bins
 *   order                 wmax = the largest effective weight of a contributing particle;
 *                         q_j = (uint64) floor((w_j / wmax) * 4294967296.0), 0 .. 2^32; Q_c = sum of q_j over the members (< 2^49);
 *                         Q_total = sum of Q_c.  Modes are ordered by Q_c descending, ties by root ascending: integers only.
 *                         The first min(n_modes, K) get rows
 *   info  int64 [4]       {n_modes, n_bins, n_used, Q_total}; n_modes counts all modes, also those beyond K, n_bins all occupied bins
 *   rows_f64 [K][16]      the estimate row over the mode's members with the effective weights: the bits of the estimate row of the
 *                         set with everyone else's weight 0 (same sums, same order).  Slot 12 = (double)Q_c, slot 13 =
 *                         (double)Q_c / (double)Q_total (the mode's share), slots 14, 15 = 0
 *   rows_i32 [K][4]       {best, n_used, n_bins, root} of the mode; best = the first argmax of the RAW weights among the members
 *   rows past min(n_modes, K): NaN in slots 0 .. 11, 0 in slots 12 .. 15, {-1, 0, 0, -1}
 *   label int32 [P]       the root of particle j's mode, or -1
 * With no contributing particle info is all zeros and every row is the unused row.  Two calls on the same state return identical
 * bits.  DESIGN.md 3.21 has the kernel.
 * rbpf_pose_modes: the set of the filter's current poses.  Needs no tracking, changes no engine state, runs on the handle's stream,
 * and stands towards a held-back map update and a half-done scan update as rbpf_estimate does.  info4 is required; rows_f64 and
 * rows_i32 are both given or both NULL; label may be NULL.  Without RBPF_MODES_DEVICE_OUT the outputs are host arrays, complete on
 * return.
 * rbpf_track_modes: the smoothed form, the companion of rbpf_track_summary.  For every record t of [t0, t1) the set holds the poses
 * at t of the current particles' ancestors, with the FINAL weights; member indices (root, best) are the current particles'.  info
 * [T][4], rows_f64 [T][K][16], rows_i32 [T][K][4] are host arrays, complete on return; any may be NULL, not all.  The records are
 * worked through in slabs whose tables stay within 256 MiB (RBPF_MODES_SLAB_BYTES in the environment lowers that: tests).
 * RBPF_ESTATE while tracking is off.
 * Both: P <= 65536.  RBPF_EINVAL, checked before anything is queued and with no output touched: a NULL pattern, a bad mode, a
 * negative or non-finite given weight, a bin_xy that is not finite or not > 0, n_th or max_modes out of range, an unknown flag, a
 * bad record range. */
#define RBPF_MODES_DEVICE_OUT 1u   /* the four outputs are device pointers, written in stream order, no host wait */
#define RBPF_MODES_MAX 64
int  rbpf_pose_modes(rbpf_handle* h, int32_t weights_mode, const double* weights, double bin_xy, int32_t n_th, int32_t max_modes,
                     uint32_t flags, int64_t* info4, double* rows_f64, int32_t* rows_i32, int32_t* label);
int  rbpf_track_modes(rbpf_handle* h, int32_t t0, int32_t t1, int32_t weights_mode, const double* weights, double bin_xy, int32_t n_th,
                      int32_t max_modes, int64_t* info /* [T][4] */, double* rows_f64 /* [T][K][16] */, int32_t* rows_i32 /* [T][K][4] */);

/* ---- map building: what map do these scans draw from these poses? ----------------------------------------------------------
 * Hit and visit counts of n_scans scans (ranges [n_scans][n_beams], metres; angles [n_beams], sensor frame, as rbpf_set_scan) taken
 * at the sensor poses poses_n3 [n_scans][3], rasterised at ANY cell size: inv = cells_per_m (finite, > 0), cell (X, Y) is the world
 * square [X, X+1) x [Y, Y+1) / inv, and box4 = {x0, x1, y0, y1} is half-open in those cells.  With inv = dim / tile_len they are the
 * mosaic cells of rbpf_render_map.  hits and seen are int32 [x1-x0][y1-y0], laid out like every raster here.  The call reads no
 * particle map and changes no engine state (maps, particles, random streams, counters, duplicate grouping); the handle supplies
 * the stream, scratch and staging.
 * The ray of beam b of scan n is the ray of rbpf_cast_scans without a map to test: float64, no contraction, host
 * libm cos / sin of theta and of each angle, the same ox, oy, dx, dy, X, Y, sx, sy, tdx, tdy, fx, fy, the same crossing parameters
 * (n + f) * td and the same tie rule (a tie steps in y).  The walk visits cells C0, C1, ... entered at 0 = t0 < t1 <= t2 ...  With
 * r = ranges[n][b]:
 *   r is NaN, or r < min_range      the beam is skipped: it contributes nothing
 *   r > max_range (+inf included)   a free beam:   tend = max_range * inv
 *   otherwise                       a return beam: tend = r * inv
 * Let k be the largest index with tk <= tend.  The beam PASSES C0 .. C(k-1) and ENDS in Ck; a return beam HITS Ck, a free beam only
 * passes it.  Counts are per scan, not per beam (the set semantics of rbpf_view_gain: near the sensor hundreds of beams cross the
 * same cells): H_n = the set of cells hit by any return beam of scan n, V_n = the set of cells passed or ended in by any of its
 * beams that is not skipped, and for every cell c of the box
 *   hits[c] = #{n : c in H_n}          seen[c] = #{n : c in V_n}
 * Cells outside the box are dropped; the walk is not clipped, so a ray may start outside the box and enter it.  A cell one scan
 * both passes and hits counts once in each: 0 <= hits <= seen <= n_scans everywhere.  Both are exact integers and integer adds
 * commute: the result is bit-identical from call to call whatever the schedule.  Either output may be NULL, not both.
 * Window limit: with M = ceil(max_range * inv) + 2 every cell of V_n lies within M cells of the pose's cell on each axis, and the
 * kernel keeps a scan's (2M + 1)^2 window as a bitmap in one workgroup's LDS: ceil(max_range * inv) <= 509 is required, otherwise
 * RBPF_EINVAL; the message gives the largest admissible max_range.
 * A NULL poses_n3, ranges, angles or box4, hits and seen both NULL, n_scans < 1, n_beams < 1, n_scans * n_beams >= 2^31, an empty
 * box, one of more than 2^31 cells or of 2^31 rows or columns, a non-finite pose or angle, cells_per_m, min_range or max_range not
 * finite, cells_per_m <= 0, max_range <= 0, min_range < 0, an unknown flag or the window limit is RBPF_EINVAL; a call between
 * rbpf_scan_update_begin and _end is RBPF_ESTATE; both are checked before anything is queued, and nothing is written.  A NaN or
 * infinite RANGE is data, not an error.  More than 4 GiB of scratch (12 bytes per beam, and 4 per cell and host output) is
 * RBPF_ENOMEM: build fewer scans per call.  It runs on the handle's stream; without RBPF_BUILD_DEVICE_OUT the outputs are host
 * arrays, complete on return.  DESIGN.md 3.16 has the kernel. */
#define RBPF_BUILD_DEVICE_OUT 1u   /* hits / seen are device pointers, written in stream order, no host wait */
#define RBPF_BUILD_ACCUMULATE 2u   /* the outputs are added to, not zeroed first: the two halves of a log give exactly the whole */
int  rbpf_build_map(rbpf_handle* h, const double* poses_n3, int32_t n_scans, const double* ranges, const double* angles,
                    int32_t n_beams, double cells_per_m, const int32_t* box4, double min_range, double max_range,
                    uint32_t flags, int32_t* hits, int32_t* seen);

/* ---- pose refinement: which pose near each guess fits the map best? ----------------------------------------------------------
 * n_scans scans (ranges [n_scans][n_beams], metres; angles [n_beams], sensor frame, as rbpf_set_scan) with n_scans guessed sensor
 * poses poses_n3 [n_scans][3] = (gx, gy, gtheta) are matched against `particle`'s map: every candidate of a window of sub-cell
 * translations and rotations round each guess is scored, and the best one is returned per scan.  The call reads one particle's
 * map and changes no engine state (maps, particles, random streams, counters, duplicate grouping).
 * Field: F(X, Y) = occ + dil in {0, 1, 2} of rbpf_locate_scan: 0 where there is no tile, outside a tile's written
 * box and outside the lattice.
 * Beams: beam b of scan n is used iff min_range < ranges[n][b] < max_range (NaN, +-inf, 0 and negative ranges are data and are not
 * used); n_used[n] counts them.  ca = cos(angles[b]), sa = sin(angles[b]) from host libm, bx = r * ca, by = r * sa.
 * Candidates: S = substeps in {1, 2, 4, 8, 16}, s = log2 S; W = n_trans in 0 .. 32; R = n_rot in 0 .. 100; candidate (i, j, k) has
 * i, j in [-W, W], k in [-R, R].  inv = dim / tile_len, invS = inv * S (exact).  float64, every + - * rounded on its own:
 *   theta_k = gtheta + (double)k * rot_step      ck = cos(theta_k), sk = sin(theta_k)       (host libm)
 *   PX[k][b] = floor((gx + (ck * bx - sk * by)) * invS)      PY[k][b] = floor((gy + (sk * bx + ck * by)) * invS)
 *   EX = (PX + i) >> s     EY = (PY + j) >> s                (arithmetic shift: floor division by S)
 *   score(n, i, j, k) = sum over the used beams of F(EX, EY)      (duplicates count; 0 <= score <= 2 n_used)
 * Candidate (i, j, k) stands for the pose (gx + i / invS, gy + j / invS, theta_k).
 * Best: per scan the candidate of maximal score; ties go to the smallest |k|, then the smallest i^2 + j^2, then the
 * lexicographically smallest (k, i, j).  A guess that attains the maximum is returned as it is: (0, 0, 0), the pose bit for bit
 * (a coordinate of -0.0 comes back as +0.0).
 * Outputs: out_pose_n3[n] = (gx + (double)i / invS, gy + (double)j / invS, theta_k) of the best candidate; out_n6[n] = {i, j, k,
 * best score, score(0, 0, 0), n_used}; scores, if not NULL, the whole volume int32 [n_scans][2R+1][2W+1][2W+1], indexed
 * [n][k + R][i + W][j + W].  One of out_pose_n3 and out_n6 may be NULL.
 * Window limit: with Mw = ceil(max_range * inv) + ceil(W / S) + 2 every (EX, EY) of scan n lies within Mw cells of
 * (floor(gx * inv), floor(gy * inv)) on each axis, and the kernel keeps that window of F in one workgroup's LDS, 2 Mw + 1 rows of
 * WW = (((2 Mw + 32) >> 5) + 2) | 1 pairs of occ and dil words, beside a beam table of 16 KiB:
 *   16384 + (2 Mw + 1) * WW * 8 <= 163776 bytes,  that is  Mw <= 367,
 * is required, otherwise RBPF_EINVAL; the message gives the largest admissible max_range.  rbpf_refine_max_reach(S, W) is the
 * largest admissible ceil(max_range * inv), 367 - ceil(W / S) - 2 (-1 for an S or W out of range): 18.1 m at 0.05 m cells and
 * 9.05 m at 0.025 m with W / S = 3.
 * A NULL poses_n3, ranges or angles, out_pose_n3 and out_n6 both NULL, n_scans < 1, n_beams < 1 or > 16384, n_scans * n_beams >=
 * 2^31, a bad particle, substeps not one of the five values, n_trans or n_rot out of range, rot_step not finite or < 0, a non-finite
 * pose or angle, min_range < 0, max_range <= 0 or either not finite, (|g| + max_range) * invS + W >= 2^30 on either axis, an unknown
 * flag or the window limit is RBPF_EINVAL; a call between rbpf_scan_update_begin and _end is RBPF_ESTATE; both are checked before
 * anything is queued, and nothing is written.  More than 4 GiB of scratch (32 bytes per scan and rotation, 8 per beam, the field
 * of the windows' union, and a requested score volume, wherever it goes) is RBPF_ENOMEM: refine fewer scans per call.  It runs on
 * the handle's stream; without RBPF_REFINE_DEVICE_OUT the outputs are host arrays, complete on return.  Each scan is matched
 * against the map as it is: a map that holds the scan itself is not corrected for that.  DESIGN.md 3.17 has the kernel. */
#define RBPF_REFINE_DEVICE_OUT 1u   /* out_pose_n3 / out_n6 / scores are device pointers, written in stream order, no host wait */
int32_t rbpf_refine_max_reach(int32_t substeps, int32_t n_trans);
int  rbpf_refine_poses(rbpf_handle* h, int32_t particle, const double* poses_n3, int32_t n_scans, const double* ranges,
                       const double* angles, int32_t n_beams, double min_range, double max_range, int32_t substeps, int32_t n_trans,
                       int32_t n_rot, double rot_step, double* out_pose_n3, int32_t* out_n6, int32_t* scores, uint32_t flags);

/* ---- pair matching: where does a scan sit among earlier scans? --------------------------------------------------------------
 * n_pairs pairs over n_scans scans (ranges [n_scans][n_beams], angles [n_beams], as rbpf_refine_poses) whose current sensor poses
 * are poses_n3 [n_scans][3] = (px, py, ptheta).  pairs_m3[m] = {q, r0, r1}: the query scan q is matched against the reference
 * scans r0 .. r1 - 1 at their poses; 0 <= q < n_scans and 0 <= r0 < r1 <= n_scans.  q may lie inside its run (a self-match; the
 * caller avoids it).  guess_m3[m] = (gx, gy, gtheta) is the guessed world pose of the query's sensor; NULL: poses_n3[q].  No
 * particle's map is read and no engine state changes: the handle supplies the stream, scratch and staging.
 * Everything is float64, every + - * rounded on its own; every cos and sin comes from host libm.
 * Beams: a beam is used iff min_range < r < max_range (NaN, +-inf, 0 and negative ranges are data and are not used);
 * ca = cos(angles[b]), sa = sin(angles[b]), bx = r * ca, by = r * sa.
 * Field of pair m: inv = cells_per_m, any finite value > 0 as in rbpf_build_map.  Every used beam of every reference scan n of the
 * run, with c = cos(ptheta), s = sin(ptheta), hits the cell
 *   HX = floor((px + (c * bx - s * by)) * inv)      HY = floor((py + (s * bx + c * by)) * inv)
 * occ(X, Y) = 1 iff some (HX, HY) equals (X, Y); dil is the OR of occ over the 3 x 3 cells round (X, Y);
 * F = occ + dil in {0, 1, 2}, defined on the whole plane.  n_ref is the number of used reference beams of the run: beams, not
 * cells.
 * Candidates, score, best and pose are rbpf_refine_poses's with this inv, invS = inv * S (exact), and the query's used beams:
 *   theta_k = gtheta + (double)k * rot_step      PX = floor((gx + (ck * bx - sk * by)) * invS)      PY alike
 *   EX = (PX + i) >> s     EY = (PY + j) >> s     score(m, i, j, k) = sum over the query's used beams of F(EX, EY)
 * with S = substeps in {1, 2, 4, 8, 16}, W = n_trans in 0 .. 32, R = n_rot in 0 .. 100; ties go to the smallest |k|, then the
 * smallest i^2 + j^2, then the lexicographically smallest (k, i, j): a guess that attains the maximum comes back bit for bit.
 * Outputs: out_pose_m3[m] = (gx + (double)i / invS, gy + (double)j / invS, theta_k); out_m8[m] = {i, j, k, best score,
 * score(0, 0, 0), n_used of the query, n_ref, 0}; scores, if not NULL, int32 [n_pairs][2R+1][2W+1][2W+1].  One of out_pose_m3 and
 * out_m8 may be NULL.
 * Self-match: with q in its own run and a NULL guess, floor(floor(v * inv * S) / S) = floor(v * inv) for every v (inv * S is
 * exact), so every used beam of q ends in a cell it drew itself: score(0, 0, 0) = 2 n_used, the result is (0, 0, 0) and the pose
 * comes back bit for bit, for any S, W and R.
 * Window limit: rbpf_refine_poses's, unchanged: Mw = ceil(max_range * inv) + ceil(W / S) + 2 <= 367 round the guess's cell
 * (rbpf_refine_max_reach(S, W) is the largest admissible ceil(max_range * inv)), otherwise RBPF_EINVAL; the message gives the
 * largest admissible max_range.  No candidate reads F outside that window, so reference points outside it change nothing.
 * A NULL poses_n3, ranges, angles or pairs_m3, out_pose_m3 and out_m8 both NULL, n_scans, n_pairs or n_beams < 1, n_beams >
 * 16384, n_scans * n_beams or n_pairs * (2R+1) >= 2^31, a bad pair, a non-finite pose, guess or angle, a bad substeps, n_trans,
 * n_rot, rot_step, min_range, max_range or cells_per_m, (|coordinate| + max_range) * invS + W >= 2^30 for a guess or for the pose
 * of a scan of a run, an unknown flag or the window limit is RBPF_EINVAL; a call between rbpf_scan_update_begin and _end is
 * RBPF_ESTATE; both are checked before anything is queued, and nothing is written.  More than 4 GiB of scratch is RBPF_ENOMEM:
 * match fewer pairs per call.  Scratch: per pair 56 bytes, 32 per rotation and the field, (2 Mw + 1) * WW * 8 with WW =
 * (((2 Mw + 32) >> 5) + 2) | 1 (31 KiB at Mw = 150, 144 KiB at 367); per scan 32 bytes and 8 per beam; 16 per beam angle; host
 * outputs 56 per pair; a requested score volume wherever it goes.  It runs on the handle's stream; without RBPF_PAIRS_DEVICE_OUT
 * the outputs are host arrays, complete on return.  DESIGN.md 3.18 has the kernels. */
#define RBPF_PAIRS_DEVICE_OUT 1u    /* out_pose_m3 / out_m8 / scores are device pointers, written in stream order, no host wait */
int  rbpf_match_pairs(rbpf_handle* h, const double* poses_n3, int32_t n_scans, const double* ranges, const double* angles,
                      int32_t n_beams, const int32_t* pairs_m3, int32_t n_pairs, const double* guess_m3, double cells_per_m,
                      double min_range, double max_range, int32_t substeps, int32_t n_trans, int32_t n_rot, double rot_step,
                      double* out_pose_m3, int32_t* out_m8, int32_t* scores, uint32_t flags);

/* ---- places by appearance: which earlier scan looks like this one, and how is it turned? ----------------------------------------
 * rbpf_describe_scans turns n_scans scans (ranges [n_scans][n_beams], angles [n_beams], as rbpf_refine_poses) into descriptors:
 * polar occupancy images in the sensor frame of R = n_rings rings (1 <= R <= RBPF_PLACES_MAX_RINGS) and 64 sectors of 5.625
 * degrees, one 64-bit word a ring, bit j of the word sector j.
 * Beams: a beam is used iff min_range < r < max_range (NaN, +-inf, 0 and negative ranges are data and are not used).
 * Sector (host, float64, every * and / rounded on its own, once per call): sector[b] = ((int64)floor(angles[b] * (32.0 / M_PI)))
 * & 63; any finite angle is accepted.  Ring: min((int)floor(r * rings_per_m), R - 1) with rings_per_m = (double)R / max_range, one
 * host division.  Bit sector of desc[n][ring] is set iff some used beam of scan n lands there.
 * Outputs: desc [n_scans][R]; info_n2[n] = {n_used, n_bits}, n_bits the popcount over the R words.  Either may be NULL, not both.
 * A NULL ranges or angles, both outputs NULL, n_scans < 1, n_beams < 1 or > 16384, n_scans * n_beams >= 2^31, R out of range, a
 * non-finite angle, min_range < 0 or not finite, max_range <= 0 or not finite, or an unknown flag is RBPF_EINVAL; a call between
 * rbpf_scan_update_begin and _end is RBPF_ESTATE; both are checked before anything is queued, and nothing is written.  More than
 * 4 GiB of scratch (8 bytes per range, 4 per beam, the host outputs) is RBPF_ENOMEM.  No engine state changes.
 *
 * rbpf_match_places compares two descriptor tables, query_desc [n_queries][R] and ref_desc [n_refs][R] (they may be the same).
 * Field of a reference with words D: D'[g] = OR over g' in {g - 1, g, g + 1} within [0, R) of (D[g'] | rotl(D[g'], 1) |
 * rotr(D[g'], 1)), the 3 x 3 dilation with circular sectors and clipped rings; w_r = popcount(D) + popcount(D').
 * Score of query q (words Q) against reference r turned by s sectors, s in 0 .. 63, rotl moving bit j to bit (j + s) & 63:
 *   score(q, r, s) = sum over g of popcount(Q[g] & rotl(D[g], s)) + popcount(Q[g] & rotl(D'[g], s))   <= min(2 n_bits_q, w_r) <= 4096
 * Best turn of a pair: the s of maximal score; ties go to the smaller min(s, 64 - s), then to the smaller s; v_r is that score.
 * The query's heading is the reference's minus s sectors.
 * Eligible: r < ref_limit[q] (NULL: every reference; an entry outside 0 .. n_refs is RBPF_EINVAL), w_r > 0 and v_r > 0.
 * Rank per query: a is better than b iff v_a^2 * w_b > v_b^2 * w_a in uint64 (both sides below 2^37), ties to the smaller r:
 * v^2 / w, a cosine-like similarity, without a division.
 * Outputs: the k best, 1 <= k <= RBPF_PLACES_MAX_K: out_qk4[q][j] = {r, s, v_r, w_r} best first, unused slots {-1, 0, 0, 0};
 * out_q2[q] = {n_bits_q, slots filled}.  Either may be NULL, not both.
 * NULL tables, both outputs NULL, n_queries or n_refs < 1, n_queries * k >= 2^31, R or k out of range, a bad ref_limit entry or an
 * unknown flag is RBPF_EINVAL; RBPF_ESTATE and RBPF_ENOMEM (8 bytes per word of a host table and per word of the reference table, 16
 * k per query and chunk of references) as above.  ref_limit is a host array.  The environment variable RBPF_PLACES_CHUNK sets the
 * references per chunk (default 256); the result does not depend on it.  DESIGN.md 3.19 has the kernels. */
#define RBPF_PLACES_MAX_RINGS 32
#define RBPF_PLACES_MAX_K 16
#define RBPF_PLACES_DEVICE_OUT 1u   /* the outputs are device pointers, written in stream order, no host wait */
#define RBPF_PLACES_DEVICE_IN 2u    /* rbpf_match_places: both descriptor tables are device pointers, read in stream order */
int  rbpf_describe_scans(rbpf_handle* h, const double* ranges, int32_t n_scans, const double* angles, int32_t n_beams,
                         double min_range, double max_range, int32_t n_rings, uint64_t* desc, int32_t* info_n2, uint32_t flags);
int  rbpf_match_places(rbpf_handle* h, const uint64_t* query_desc, int32_t n_queries, const uint64_t* ref_desc, int32_t n_refs,
                       int32_t n_rings, const int32_t* ref_limit, int32_t k, int32_t* out_qk4, int32_t* out_q2, uint32_t flags);

/* ---- score surface: how sharp is a match, and is there another one? ------------------------------------------------------------
 * Reduces n_items score volumes, int32 [n_items][nk][nw][nw] with nk = 2R+1, nw = 2W+1, R = n_rot in 0 .. 100 and W = n_trans in
 * 0 .. 32, indexed [n][k+R][i+W][j+W] with values in 0 .. 32768: exactly what rbpf_refine_poses and rbpf_match_pairs write into
 * `scores`.  Everything is exact integer arithmetic.
 * Parameters: drop_n[n] in 0 .. 32768 per item (NULL: 0 for every item); ex_trans in 0 .. 64; ex_rot in 0 .. 200; K = n_peaks in
 * 1 .. 8.
 * Order: candidate c = (i, j, k) with score V(c) comes before another iff its V is larger, then its |k| smaller, then its
 * i^2 + j^2 smaller, then its (k, i, j) lexicographically smaller: the tie order of rbpf_refine_poses.
 * Peaks, greedy: free_0 is every candidate.  For p = 0, 1, .. < K while free_p is not empty: peak_p = (i_p, j_p, k_p) is the
 * first candidate of free_p in that order, s_p its score; box_p = {c : |i - i_p| <= ex_trans, |j - j_p| <= ex_trans, |k - k_p| <=
 * ex_rot}; free_{p+1} = free_p \ box_p.  out_count[n] is the number of peaks found, at least 1.  Peak 0 is the best candidate
 * rbpf_refine_poses or rbpf_match_pairs reports for that volume.
 * Plateau of peak p: T_p = {c in free_p and box_p : V(c) >= s_p - drop}; it always holds the peak.  Weight w(c) = V(c) -
 * (s_p - drop) + 1 in 1 .. drop + 1; offsets d = (di, dj, dk) = (i - i_p, j - j_p, k - k_p).  All sums are exact int64: the
 * largest, sum w dk^2 at R = 100, W = 32, drop = 32768 over a constant volume, stays below 1.2e18.
 * Output record of peak p, out_nk16[n][p], int64 [16]: {i, j, k, s, |T|, sum w, sum w di, sum w dj, sum w dk, sum w di^2,
 * sum w di dj, sum w di dk, sum w dj^2, sum w dj dk, sum w dk^2, 0}.  The records out_count[n] .. K - 1 are all zero.
 * It reads no particle's map and changes no engine state; it runs on the handle's stream; host outputs are complete on return.
 * A NULL scores or out_nk16 (out_count may be NULL), n_items < 1, a parameter out of the ranges above, n_items * nk * nw^2 >=
 * 2^31, an unknown flag, a host drop_n value out of range or a host volume with a value outside 0 .. 32768 is RBPF_EINVAL; a call
 * between rbpf_scan_update_begin and _end is RBPF_ESTATE; both are checked before anything is queued, and nothing is written.
 * More than 4 GiB of scratch is RBPF_ENOMEM: a host volume is staged, 4 bytes per candidate and 4 per host drop, and host outputs
 * take 128 K + 4 bytes per item.  A device volume (and a device drop_n) is not validated: no score is ever used as an index, so a
 * value out of range can only give meaningless numbers, never an access outside the buffers.  DESIGN.md 3.20 has the kernel. */
#define RBPF_SURFACE_DEVICE_IN  1u   /* scores and drop_n are device pointers */
#define RBPF_SURFACE_DEVICE_OUT 2u   /* out_nk16 / out_count are device pointers, written in stream order, no host wait */
int  rbpf_score_surface(rbpf_handle* h, const int32_t* scores, int32_t n_items, int32_t n_rot, int32_t n_trans,
                        const int32_t* drop_n, int32_t ex_trans, int32_t ex_rot, int32_t n_peaks,
                        int64_t* out_nk16, int32_t* out_count, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* RBPF_HIP_H */
