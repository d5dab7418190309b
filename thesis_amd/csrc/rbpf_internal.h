// rbpf_internal.h -- what the kernels and their launchers share in librbpf_hip.so (gfx950 only); the handle: rbpf_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "../../include/rbpf_hip.h"
#include "rbpf_math.h"
#include "rbpf_blockrelax.h"

namespace rbpf {

// The dynamic-LDS limit of a kernel is a per-DEVICE attribute; a process may hold handles on several GPUs.  `set` is the
// launcher's own table of what it has set so far (one entry per device).
static const int MAX_DEVICES = 16;
inline void ensure_dynamic_lds(const void* fn, size_t bytes, size_t* set) {
    static std::mutex mu;                              // handles on several host threads share the launchers' tables
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool tracked = dev >= 0 && dev < MAX_DEVICES;
    if (tracked && bytes <= set[dev]) return;
    const hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc != hipSuccess) { (void)hipGetLastError(); return; }   // not recorded as set: the launch that follows reports the error
    if (tracked) set[dev] = bytes;
}


static const int BLOCK = 256;          // 4 waves of 64
static const int WIN = 128;            // LDS window edge (storage cells)
static const int MAX_ITEMS_PER_PARTICLE = 64;

// beam range classes, computed on the host from the float64 distance (rbpf_set_scan)
enum { BF_WEIGHT = 1, BF_MATCH = 2, BF_LONG = 4, BF_MATCH_ADJ = 8 };

// The map update's kernels (RBPF_MAP_KERNEL); each first kernel is followed by the 128x128-window kernel for the particles it gives back.
enum MapKernelMode : int {
    MU_DEFAULT,    // the event-walk kernel (kernels_mapev.hip) on grids with dim <= 1024, the global-index kernel (kernels_mapray.hip) on
                   // finer ones, either where the other one is not available (e.g. more than 1536 beams)
    MU_WINDOW,     // "window": 128x128 windows only (kernels_mapupdate.hip)
    MU_RAY,        // "ray": the global-index kernel first
    MU_EV,         // "ev": the event-walk kernel first
};

// Everything a kernel needs, passed by value.
struct DevView {
    // configuration
    int P, K, B, dim, R, L;            // L = 2R+1 lattice edge
    int pool_tiles;
    int reach;                         // longest ray in cells (+ margin)
    double cs, tile_len;
    double quantum, inv_quantum;       // inv_quantum = round(1/quantum) when exact, else 0
    CellConsts cc;
    double w_min_range, w_max_range;
    // LUT over global cell indices g in [g_min, g_min + n_lut)
    const uint32_t* lut; int g_min, n_lut;
    const int32_t* gwin;               // [L][KW+1] first global index of each 128-cell window of a lattice row (KW = ceil(dim/WIN)); [KW] = next tile
    // particle state, SoA, logical particle order
    double *px, *py, *pth;             // [P]
    double *cov;                       // [9][P]
    double *weight;                    // [P]
    int32_t* slot;                     // [P] logical particle -> map slot
    int32_t* global_id;                // [P] id of the particle in the multi-GPU job
    // maps
    int32_t* tile_tab;                 // [P slots][L*L] pool tile id or -1
    int8_t*  pool;                     // [pool_tiles][dim*dim], cell[x*dim + y]
    uint32_t* occ;                     // [pool_tiles][dim][ow] occupancy bits (cell > threshold), bit y&31 of word y>>5
    int ow;                            // words per occupancy row = ceil(dim / 32)
    int32_t* tile_bbox;                // [pool_tiles][4] x_min, x_max, y_min, y_max (inclusive)
    int32_t* free_stack;               // [pool_tiles]
    int32_t* free_top;                 // [1] number of free tiles on the stack
    // scan (sensor frame)
    const double *bx, *by, *bscale;    // [B]
    const uint8_t* bflags;             // [B]
    float *msel_x, *msel_y; int n_msel;  // beams with BF_MATCH, compacted (metres, sensor frame)
    float *asel_x, *asel_y; int n_asel;  // beams with BF_MATCH_ADJ, compacted
    const float *wsel_x, *wsel_y; const uint16_t* wsel_idx; int n_wsel;   // beams with BF_WEIGHT, compacted, single precision (x = NaN: outside
                                         // the fast look-up's error budget), padded with NaN to a multiple of 64; their beam numbers
    // per-update scratch
    double*  upd_pose;                 // [3][P] poses used by the current map update
    double*  prop_prep;                // [P][24] proposal frame of the current scan update (kernels_propose.hip: U, A, mean, log c)
    double*  prop_samp;                // [P][256] its K samples: cos, sin, pose, motion probability, single-precision frame
    int32_t* mu_fallback;              // [P] != 0: the map-update kernel that ran first gave the particle back to the next one
    MapKernelMode mu_mode;             // which map-update kernels run (RBPF_MAP_KERNEL)
    // the particles a map update leaves out (the update that rbpf_resample launches behind its plan: DESIGN.md 3.4); all three
    // null: nobody, the list is the identity
    const uint8_t* mu_skip;            // [P] != 0: the coming resample discards the particle, no kernel of the chain touches it
    const int32_t* mu_keep;            // [*mu_n_keep] the other particles, ascending: what a position of the event walk's queue stands for
    const int32_t* mu_n_keep;          // [1]
    uint32_t* ev_queue;                // [2] the event-walk kernel's particle queue: draws of this launch, workgroups that have left; zero between launches (the kernel re-arms it)
    int ev_resident, ev_grid;          // 1: resident workgroups draw particles from ev_queue (0, RBPF_EV_RESIDENT=0: one workgroup per particle); > 0: cap on their number (RBPF_EV_GRID, tests)
    uint32_t* ndt_occ; double* ndt_aux; // NDT stage: the matcher's staged field per particle, its grid optimum (kernels_match.hip)
    int ndt_refine;                    // rbpf_config.ndt_refine: NDT stage of matchScanCustom.m:32-50 (0 off, 1 reference rule, 2 always)
    int32_t* dup_of; int dups_valid;    // representative of each particle's group of exact duplicates since the last resample (kernels_resample.hip); valid until the next proposal
    float wsafe_override;              // >= 0: the weighting's guard band in cells (RBPF_WSAFE, a test knob); < 0: the built-in value
    int weight_entry_f64;              // 1: rbpf_weight_samples runs the float64 kernel of round 1 (RBPF_WEIGHT_ENTRY=f64) instead of the product's look-ups
    int match_stage_slow;              // 1 = the matcher stages its field bit by bit (RBPF_MATCH_STAGE=slow; the check of the fast path)
    unsigned long long* stats;         // [8] device counters
    int32_t* err;                      // [1] sticky device error code
};

// double buffers and scratch of the resample step
struct ResampleBuffers {
    int32_t *T, *idx, *did;            // [P], [P], [1]
    int32_t *slot2, *dead_list, *jobs; // [P], [P], [P][2]
    int32_t *n_jobs;                   // [2] job count, queue head
    int32_t *pending_free, *n_pending; // [pool_tiles], [1]
    double *px2, *py2, *pth2, *cov2, *w2;
    uint8_t* skip; int32_t* keep;      // [P], [P] DevView::mu_skip, mu_keep of the map update between the two plan launches
    int32_t* plan;                     // [2] that list's length; 1: the first plan launch made the plan, 0: the second one has to
};

enum { ST_RAY_CELLS = 0, ST_CELLS_WRITTEN = 1, ST_GATHERS = 2, ST_SLOW_CELLS = 3,
       ST_COPIES = 4, ST_COPY_BYTES = 5, ST_WINDOW_FALLBACKS = 6, ST_FALLBACK_REASONS = 7,
       /* 8..15: phase stamps of a -DRBPF_STAMPS build */
       ST_NDT_RUNS = 16, ST_NDT_EVALS = 17, ST_NDT_ACCEPTED = 18, ST_MATCH_SHARED = 19, ST_MAP_WINDOWS = 20,
       ST_FB_BOUND = 21, ST_FB_TABLES = 22, ST_MAP_EVENTS = 23, ST_EV_OVERFLOWS = 24, ST_MU_SKIPPED = 25,
       ST_POOL_CELLS = 26, ST_NEAR_CELLS = 27, ST_COUNT = 28 };   // ST_FALLBACK_REASONS (7) counts reason 1 (geometry / index map)

// map rendering (kernels_render.hip): one workgroup per job, up to 16 storage rows x 256 storage columns of one lattice tile
struct RenderJob {
    int32_t pos;                       // lattice position a * L + b, or -1 outside the lattice
    int32_t i0, j0;                    // tile-local row and column of the job's first lane (j0 % 16 == 0)
    int32_t ni, jlo, jhi;              // rows i0 .. i0 + ni - 1, tile-local columns [jlo, jhi) lie in the box
    int32_t ox, oy;                    // output row and column of (i0, j0): X - x0, Y - y0 (oy < 0 when jlo > j0)
};
struct RenderFilter {
    const RenderJob* jobs;
    const double* lut;                 // [256] sigma(int8(k) * quantum) on the host, float64
    const double* w;                   // [P] particle weights
    double S;                          // sum of w, in the kernels' order (groups of C)
    int C, ngroups;                    // particles per group, groups
    long long ny;                      // output columns (y1 - y0)
    size_t ncell;                      // output cells
    float *prob, *occ;                 // outputs (either may be null)
    double *part_p, *part_o;           // [ngroups][ncell] group sums of a split render
};
// map loading (kernels_load.hip): the box cut into RenderJobs whose column blocks start at multiples of 32 (one occupancy word
// per lane pair), and the lattice positions it touches with (box n tile) in tile-local cells, inclusive
struct LoadTile { int32_t pos, i0, i1, j0, j1; };
struct LoadArgs {
    const RenderJob* jobs;
    const LoadTile* tiles; int n_tiles;
    const int8_t* cells;               // raster [nx][ny] (device)
    long long ny, ncell;
    int p_lo, p_hi;                    // particles [p_lo, p_hi)
    int32_t* bad;                      // [1] != 0: validation found a value out of range - the alloc and write kernels do nothing
};
// map placement (kernels_place.hip): a source raster with its own cell size and world pose, resampled onto the
// mosaic cells of a box.  The trigonometry is done on the host.
struct PlaceArgs {
    const int8_t* src;                 // [nsx][nsy] (device)
    int nsx, nsy;
    double c, s, ox, oy;               // cos and sin of the source yaw, world position of the corner of source cell (0, 0)
    double src_cell, cs;               // metres per source cell, metres per mosaic cell (tile_len / dim)
    int S, mode;                       // samples per axis and cell (1 .. 8), RBPF_PLACE_REPLACE / _KNOWN / _ADD
    int x0, y0;                        // mosaic cell of output element [0][0]
    long long ny, ncell;               // output columns and cells
    int8_t* warped; uint8_t* covered;  // [nx][ny] outputs of place_warp_kernel (either may be null)
    const int32_t* bad;                // LoadArgs::bad of the same call
};
// scan casting (kernels_cast.hip): ray r = pose * B + beam; the trigonometry is done on the host
struct CastArgs {
    const double* pose4;               // [n_poses][4] x, y, cos(theta), sin(theta)
    const double* beam2;               // [B][2] cos(angle), sin(angle)
    int n_poses, B;
    int particle;                      // >= 0: every pose in this particle's map; -1: pose n in particle n's
    double inv, tlim, max_range;       // cells per metre (dim / tile_len), max_range * inv, max_range
    double* ranges; uint8_t* status;   // [n_poses][B]; status may be null
};
// view gain (kernels_gain.hip): the set of cells the beams of a pose test, reduced against a particle's map; one
// workgroup per (particle, pose), result r = particle * n_poses + pose (particle counted from 0 only when every particle is asked for)
struct GainArgs {
    const double* pose4;               // [n_poses][4] x, y, cos(theta), sin(theta)
    const double* beam2;               // [B][2] cos(angle), sin(angle)
    const int32_t* table;              // [nv] value of a seen cell by its lattice value: table[v - vmin]
    int n_poses, B, nv;
    int particle;                      // >= 0: every pose in this particle's map; -1: every pose in every particle's map
    int M, W;                          // window half-width in cells: ceil(max_range * inv) + 2; words per bitmap row
    double inv, tlim;                  // cells per metre (dim / tile_len), max_range * inv
    int64_t* gain; int32_t *seen, *unknown;   // [particles][n_poses]; seen and unknown may be null
};
// map building (kernels_build.hip): hit and visit counts of n_scans scans taken at given poses, over a box of
// cells of any size; one workgroup per scan.  No particle map is read.
struct BuildArgs {
    const double* pose4;               // [n_scans][4] x, y, cos(theta), sin(theta)
    const double* beam2;               // [B][2] cos(angle), sin(angle)
    const double* ranges;              // [n_scans][B] metres; NaN and +-inf are data
    uint32_t* ends;                    // [n_scans][B] scratch: (row * 32 W + bit) << 1 | 1 of a return beam's end cell in the window, else 0
    int n_scans, B;
    int M, W;                          // window half-width in cells: ceil(max_range * inv) + 2; words per bitmap row
    int x0, y0, nx, ny;                // the box: first cell, rows (x1 - x0) and columns (y1 - y0)
    double inv, tlim;                  // cells per metre, max_range * inv
    double min_range, max_range;
    int32_t *hits, *seen;              // [nx][ny], added to; either may be null
};
// scan-to-map refinement (kernels_refine.hip): N scans with N guessed poses against one particle's map, every
// candidate (i, j, k) of a window of sub-cell translations and rotations.  The field is locate's over the union of the scans'
// windows cut to the lattice: a LocateArgs with particle, x0, y0, M = 0, rows, W and field set describes it
static const int REFINE_BLOCK = 512;   // lanes of a workgroup, one task (rotation, i, run of j) each
static const int REFINE_RUN = 8;       // values of j of one task, substeps apart
static const int REFINE_TABLE = 2048;  // (PX, PY) entries of the beam table in LDS: rotations of the workgroup x beams of a chunk
// runs of j per i: the 2 W + 1 values of j fall into S residue classes, each cut into runs of REFINE_RUN
__host__ __device__ inline int refine_runs(int nw, int s) { return ((((nw + (1 << s) - 1) >> s) + REFINE_RUN - 1) / REFINE_RUN) << s; }
struct RefineArgs {
    int N, B;                          // scans, beams per scan
    int Wt, R, s, nk, kpw;             // n_trans, n_rot, log2 substeps, rotations 2 R + 1, rotations per workgroup (<= 16)
    int Mw, WW;                        // window half-width in cells; {occ, dil} word pairs per window row (odd)
    int fx0, fy0, frows, fW;           // the field: first cell, rows, word pairs per row; frows = 0: no window meets the lattice
    double invS, min_range, max_range; // sub-cells per metre (dim / tile_len * substeps); a beam is used iff min < r < max
    const double* guess;               // [N][2] gx, gy
    const int32_t* cell0;              // [N][2] floor(gx * inv), floor(gy * inv): the window's centre cell (host)
    const double* rot;                 // [N][nk][4] cos, sin of theta_k and theta_k itself (host libm), one pad
    const double* beam2;               // [B][2] cos, sin of the beam angles (host libm)
    const double* ranges;              // [N][B] metres; NaN and +-inf are data
    const uint2* field;                // [frows][fW]
    unsigned long long* packed;        // [N] max over candidates of score << 41 | complemented tie key, preset to 0
    int32_t *guess_score, *n_used;     // [N] scratch: score(0, 0, 0) and the number of used beams
    int32_t* scores;                   // [N][nk][2 Wt + 1][2 Wt + 1] or null
    double* out_pose; int32_t* out_n6; // [N][3], [N][6]; either may be null
};
// scan-to-submap matching (kernels_pairs.hip): M pairs of a query scan and a run of reference scans.  The search
// is refinement's over a RefineArgs with N = M, one item per pair; this describes the field each pair draws for itself
static const int PAIRS_BLOCK = 512;    // lanes of a field workgroup, one per pair
struct PairsArgs {
    int M, B;                          // pairs, beams per scan
    int Mw, WW;                        // as RefineArgs: a pair's field is its window, 2 Mw + 1 rows of WW {occ, dil} word pairs
    double inv, min_range, max_range;  // cells per metre; a beam is used iff min < r < max
    const double* pose4;               // [n_scans][4] px, py, cos, sin of the scans' current poses (host libm)
    const double* beam2;               // [B][2] cos, sin of the beam angles (host libm)
    const double* ranges;              // [n_scans][B]
    const int32_t* query;              // [M] the query scan of each pair
    const int32_t* runs;               // [M][2] reference scans r0 .. r1 - 1
    const int32_t* cell0;              // [M][2] floor(gx * inv), floor(gy * inv): the window's centre cell (host)
    uint2* fields;                     // [M][2 Mw + 1][WW]; bit 0 of a row is cell Y0 - Mw
    int32_t* n_ref;                    // [M] used reference beams of the run
    double* out_pose; int32_t* out_m8; // [M][3], [M][8]; either may be null
};
// places by appearance (kernels_places.hip): nq query descriptors against nr reference descriptors of R ring words,
// the k best references of every query.  References are cut into chunks of `chunk`; a (query, chunk) leaves a list in `partial`
struct PlacesArgs {
    int nq, nr, R, k;
    int chunk, nch;                    // references per chunk, chunks = ceil(nr / chunk)
    const unsigned long long* qd;      // [nq][R]
    const unsigned long long* rd;      // [nr][R]
    const int32_t* limit;              // [nq] query q admits the references r < limit[q], 0 <= limit[q] <= nr
    unsigned long long* dil;           // [nr][R] D', written by the field kernel
    int32_t* w;                        // [nr] popcount(D) + popcount(D')
    int4* partial;                     // [nq][nch][k] {r, s, v, w} best first, {-1, 0, 0, 0} behind the last
    int32_t *out_qk4, *out_q2;         // [nq][k][4], [nq][2]; either may be null
};
// peaks and moments of score volumes (kernels_surface.hip): the K best candidates of each of N volumes that lie
// outside one another's exclusion boxes, each with the size and the weighted sums of its plateau
static const int SURFACE_BLOCK = 512;      // lanes of a workgroup, one workgroup per item
static const int SURFACE_MAX_PEAKS = 8;
static const int SURFACE_SUMS = 11;        // |T|, sum w, three first and six second moments
struct SurfaceArgs {
    int N, R, W;                       // items; n_rot and n_trans of the volume, [2 R + 1][2 W + 1][2 W + 1] per item
    int ex_t, ex_r, K;                 // the exclusion box's half-widths in translation and rotation steps; peaks per item
    const int32_t* scores;             // [N][2 R + 1][2 W + 1][2 W + 1]
    const int32_t* drop;               // [N] or null (0): the plateau reaches this far below its peak
    long long* out;                    // [N][K][16]
    int32_t* count;                    // [N] peaks found, or null
};
// global localization (kernels_locate.hip): one scan against one particle's map over a box of candidate cells
struct LocateArgs {
    int particle;
    int x0, y0, nx, ny;                // the box: first mosaic cell, rows (x1 - x0) and columns (y1 - y0)
    int nyw;                           // candidate words per box row = ceil(ny / 32)
    int M;                             // largest beam offset in cells: the field is the box grown by M on every side
    int rows, W;                       // field rows (nx + 2 M) and {occ, dil} word pairs per field row (nyw + (2 M >> 5) + 2)
    int n_rot, nb, rpw;                // rotations, used beams, rotations per workgroup
    double inv;                        // cells per metre (dim / tile_len)
    const double* cs;                  // [n_rot][2] cos, sin of theta_r (host libm)
    const double* bxy;                 // [nb][2] end points of the used beams, sensor frame, metres (host libm)
    int32_t* offs;                     // [n_rot][nb] u << 16 | (M + w): offset in rows, and in bits of a field row
    uint2* field;                      // [rows][W]
    uint32_t* cand;                    // [nx][nyw] bit Y & 31: the cell is a candidate
    int32_t* items; int32_t* n_items;  // the words of cand that are not 0, in any order; their number
    uint32_t* packed;                  // [nx][ny] max over rotations of score << 16 | (n_rot - 1 - r), preset to 0
    int32_t *best, *rot;               // [nx][ny] outputs; rot may be null
};
// alignment of a point set (kernels_align.hip): occupied and free points against one particle's map over a box of cells and a
// window of rotations.  The field is locate's: a LocateArgs with particle, x0, y0, M, rows, W and field set describes it
struct AlignArgs {
    int x0, y0, nx, ny;                // the box: first mosaic cell, rows (x1 - x0) and columns (y1 - y0)
    int nyw;                           // words per box row = ceil(ny / 32)
    int M;                             // largest point offset in cells: the field is the box grown by M on every side
    int W;                             // {occ, dil} word pairs per field row (nyw + (2 M >> 5) + 2)
    int n_rot, r_begin, r_count, rpw;  // rotations of the full turn, the window searched, rotations per workgroup
    int n_occ, np;                     // occupied points; all points (the free ones follow the occupied ones)
    double inv;                        // cells per metre (dim / tile_len)
    const double* cs;                  // [r_count][2] cos, sin of theta_r, r = r_begin .. (host libm)
    const double* pxy;                 // [np][2] the points, metres, frame of the point set
    int32_t* offs;                     // [r_count][np] u << 16 | (M + w): offset in rows, and in bits of a field row
    const uint2* field;                // [nx + 2 M][W]
    uint32_t* packed;                  // [nx][ny] max over rotations of biased score << 16 | (n_rot - 1 - r), preset to 0
    int32_t *best, *rot;               // [nx][ny] outputs; rot may be null
};
// travel cost (kernels_travel.hip): clearance, traversable set and shortest-path cost over a box of one particle's
// map, or of a batch of particles' maps.  The box is cut into 64 x 64 blocks, block k = bx * nby + by; a particle of the batch
// is blockIdx.y.  Cells are box-relative: (i, j) = (X - x0, Y - y0).
static const int TRAVEL_INF = 0x3f3f3f3f;   // "not reached" in the cost field (the byte 0x3f four times: a memset fills it); 7 * 2^27 < it
struct TravelArgs : BlockRelaxArgs {      // ras: the cost field, TRAVEL_INF on the rim and wherever no path is known yet
    int particle;                      // the first particle of this launch
    int x0, y0, nx, ny;                // the box: first mosaic cell, rows (x1 - x0) and columns (y1 - y0)
    int m;                             // margin read round a block: ceil(clear_max / 5) <= 64
    int inflate, clear_max;            // T needs d > inflate; the clearance output is min(d, clear_max)
    int through_unknown;               // 1: blocked = occupied; 0: blocked = v >= 0
    int n_start, start_each;           // start_each 1: start (particle + blockIdx.y) only; 0: all n_start in every particle
    int n_goals;
    const int32_t* starts;             // [n_start][2] box-relative cell, (-1, -1) outside the box
    const int32_t* goals;              // [n_goals][2] likewise
    uint16_t* tbits; long long t_stride;            // [n_part][nbx * 64][nby * 4]: bit j & 15 of halfword j >> 4 of row i: cell in T
    uint16_t* clearance;               // [nx][ny] output or null (single particle only)
    int32_t* cost_out;                 // [nx][ny] output or null (single particle only)
    int32_t* goal_out;                 // [n_part][n_goals] output or null
};

// path checks (kernels_paths.hip): polylines of waypoint cells walked through one particle's map, every particle's map
// or each its own particle's; one wave per (particle, path), result r = particle * n_paths + path (particle counted from 0 only
// when every particle is asked for), or r = path where a path belongs to one particle (own_k)
struct PathArgs {
    const int32_t* cells;              // [n_waypoints][2] waypoint cells, counted from the lattice's first cell
    const int32_t* wstep;              // [n_waypoints] the step of its path at which the walk stands on the waypoint
    const int32_t* path_start;         // [n_paths + 1] first waypoint of each path
    int n_paths;
    int particle;                      // the map of result 0: the particle asked for, or 0
    int own_k;                         // > 0: path k is checked in the map of particle k / own_k alone
    long long pairs;                   // results: n_paths, or n_particles * n_paths
    int inflate, clear_max;            // a cell carries the robot if d > inflate; min_clearance is capped at clear_max
    int through_unknown, start_exempt; // 1: blocked = occupied, else v >= 0; 1: the cell of step 0 always carries the robot
    int32_t* out;                      // [pairs][4] first_blocked, first_unknown, min_clearance, n_unknown
};

// rollout checks (kernels_paths.hip): templates in the robot's frame placed at poses on the device and walked as
// paths; one wave per (pose, template), result r = pose * n_tmpl + template
struct RolloutArgs {
    const double* pose4;               // [n_poses][4] x, y, cos(theta), sin(theta)
    const double* tmpl_xy;             // [n_waypoints][2] metres in the robot's frame
    const int32_t* tmpl_start;         // [n_tmpl + 1] first waypoint of each template; every template has 1 .. PATH_STAGE
    int n_tmpl;
    int particle;                      // >= 0: every pose in this particle's map; -1: pose n in particle n's
    int off;                           // mosaic cell X + off counts from the lattice's first cell
    double inv;                        // cells per metre (dim / tile_len)
    long long pairs;                   // results: n_poses * n_tmpl
    int inflate, clear_max;            // as PathArgs
    int through_unknown, start_exempt;
    int32_t* out;                      // [pairs][4] first_blocked, first_unknown, min_clearance, n_unknown
    int32_t* steps;                    // [pairs] or null
};

// footprint checks (kernels_footprint.hip): the rollouts of RolloutArgs, every step also testing the cells an
// oriented footprint covers; one wave per (row, template), result r = row * n_tmpl + template, row a pose or a particle
struct FootArgs {
    const double* pose4;               // [n_poses][4] x, y, cos(theta), sin(theta)
    const int32_t* pose_bin;           // [n_poses] heading bin of the pose
    const double* tmpl_xy;             // [n_waypoints][2] metres in the robot's frame
    const int32_t* tmpl_bin;           // [n_waypoints] heading bin of the waypoint in the robot's frame
    const int32_t* tmpl_start;         // [n_tmpl + 1] first waypoint of each template; every template has 1 .. PATH_STAGE
    const int32_t* fp_start;           // [n_bins + 1] first span of each bin
    const int32_t* fp_span;            // [n_spans] dx, y0, y1 as signed bytes 0, 1, 2 (rbpf_footbatch.h, footprint_pack)
    int n_tmpl, n_bins;
    int particle;                      // >= 0: every pose in this particle's map; -1: row n is particle n
    int one_pose;                      // 1: every row takes pose 0 (one pose in every particle's map); 0: row n takes pose n
    int off;                           // mosaic cell X + off counts from the lattice's first cell
    double inv;                        // cells per metre (dim / tile_len)
    long long pairs;                   // results: rows * n_tmpl
    int inflate, clear_max;            // as PathArgs, for the centre cell
    int through_unknown;               // 1: blocked = occupied, else v >= 0
    int exempt;                        // >= 0: cells within this Chebyshev distance of the cell of step 0 block nothing; -1: none
    int32_t* out;                      // [pairs][4] first_blocked, first_unknown, min_clearance, n_unknown
    int32_t* steps;                    // [pairs] or null
};

// scan checks (kernels_scancheck.hip): measured scans against the maps; ray r = pose * B + beam as in CastArgs
struct ScanCheckArgs {
    const double* pose4;               // [n_poses][4] x, y, cos(theta), sin(theta)
    const double* beam2;               // [B][2] cos(angle), sin(angle)
    const double* ranges;              // [n_scans][B] metres; NaN, +-inf, 0 and negatives are data
    const int32_t* tabs;               // class_cost8 [8], then hit_tab [2 half_bins + 1]
    int n_poses, B;
    int scan_each;                     // 1: scan n belongs to pose n; 0: one scan for every pose
    int particle;                      // >= 0: every pose in this particle's map; -1: pose n in particle n's
    int half_bins;
    double inv, tmax, ttol;            // cells per metre (dim / tile_len), max_range * inv, tol * inv
    double max_range, min_range, bins_per_cell;
    unsigned long long* cost;          // [n_poses], preset to 0
    int32_t* counts;                   // [n_poses][8] or null, preset to 0
    uint8_t* classes;                  // [n_poses][B] or null
    int32_t* votes;                    // [B][8] or null, preset to 0
};

// local map (kernels_local.hip): an n x n window in the robot's frame cut out of the map of every pose's particle
// (one workgroup per pose of a batch) and the four integer sums over the poses; the trigonometry and the tables come from the host
static const int LOCAL_GROUP_POSES = 64;   // poses of one group of the fusion (rbpf_localbatch.h: LOCAL_GROUP)
struct LocalArgs {
    const double* pose4;               // [n_poses][4] x, y, cos(theta), sin(theta), of the whole call
    const double *gx, *gy;             // [nq] sample coordinates in the robot's frame, metres
    const uint32_t* wq;                // [n_poses] integer weights, of the whole call
    int n, S, nq;                      // output cells a side, samples a cell and axis, n * S
    int reach, side, row_bytes;        // the LDS window: half-side, rows 2 reach + 1, bytes of a row (a multiple of 16, >= side + 15)
    int tab_lds;                       // 1: gx and gy stand in LDS behind the window
    int particle;                      // >= 0: every pose in this particle's map; -1: pose n in particle n's
    int off;                           // mosaic cell X + off counts from the lattice's first cell
    double inv;                        // cells per metre (dim / tile_len)
    int p0, nb;                        // the batch: its first pose, its poses
    int8_t* crops; size_t cstride;     // the crop of pose p0 + k: crops + k * cstride, [n][n]
    int wide;                          // 1: every crop starts on a 16-byte boundary and holds whole 16-byte strips
    int ngroups; size_t ncellp;        // groups of the batch; n * n rounded up to a multiple of 16
    uint32_t* part_w; long long* part_v;   // [ngroups][3][ncellp] occ_w, free_w, unknown_w and [ngroups][ncellp] sum_wv of the groups
    long long* fused;                  // [n][n][4], added to
};

// frontier regions (kernels_frontier.hip): frontier cells of a box of one particle's map, or of a batch of particles'
// maps, their connected components and a table of the largest.  Blocks, particles of the batch and box-relative cells as in
// TravelArgs; the label of a cell is L = i * ny + j.
static const int FRONTIER_NONE = 0x7f7f7f7f;   // "no frontier cell" in the label raster (the byte 0x7f four times); 2^27 < it
struct FrontierArgs : BlockRelaxArgs {    // ras: the labels, FRONTIER_NONE on the rim and wherever no frontier cell is
    int particle;                      // the first particle of this launch
    int x0, y0, nx, ny;                // the box: first mosaic cell, rows (x1 - x0) and columns (y1 - y0)
    int clear;                         // no occupied cell within this Chebyshev distance of a frontier cell (0 .. 16)
    int min_size, max_regions;         // the table: regions of at least min_size cells, the max_regions largest
    int32_t* aux;                      // the layout of ras, preset to 0: at a root (ras == L) the region's size, then -(row + 1) if the table keeps it
    int32_t* counts;                   // [n_part][3] |F|, regions, kept regions; preset to 0
    unsigned long long* table;         // [n_part][max_regions][10] the rows of include/rbpf_hip.h (two's complement); null: no table
    int32_t* label_out;                // [nx][ny] output or null (single particle only)
};

// map scores (kernels_score.hip): a box of one particle's map, or of every particle's, compared cell by cell with
// one reference raster.  Blocks, particles of a launch and box-relative cells as in TravelArgs.
static const int SCORE_FIELDS = RBPF_SCORE_FIELDS;
struct ScoreArgs {
    int particle, n_part;              // the first particle of this launch (blockIdx.y counts from it), particles of the launch
    int x0, y0, nx, ny;                // the box: first mosaic cell, rows (x1 - x0) and columns (y1 - y0)
    int nbx, nby;                      // 64 x 64 blocks along x and y
    int tol;                           // Chebyshev distance within which a wall confirms a wall (0 .. 16)
    const int8_t* ref;                 // [nx][ny] the reference (device)
    const int32_t* table;              // [vmax - vmin + 1] or null: tab = 0
    unsigned long long* near_r;        // [nbx * nby][64] bit j of row i of a block: a reference-occupied cell of the box within tol
    int32_t* ref_sums;                 // [nbx * nby][4] of the block's cells in the box: reference cells of class F, U, O; sum of |r|
    int32_t* bad;                      // [1] != 0: a reference value out of range (written only when `validate`)
    int validate;
    long long* scores;                 // [n_part][SCORE_FIELDS] of this launch, preset to 0
};

// trajectory log (kernels_track.hip).  A record is `stride` bytes: x[P], y[P], th[P] float64, the estimate row's
// 16 float64, parent[P] int32, the estimate row's 4 int32, padded to a multiple of 16.
static const int TRACK_SUMMARY_MAX_P = 65536;   // the P-bit bitmap of track_summary_kernel: 8 KB of LDS
__host__ __device__ inline size_t track_parent_offset(int P) { return (size_t)P * 24 + RBPF_EST_F64 * 8; }
__host__ __device__ inline size_t track_record_stride(int P) { return (track_parent_offset(P) + (size_t)P * 4 + RBPF_EST_I32 * 4 + 15) & ~(size_t)15; }
struct TrackLog { unsigned char* base; size_t stride; int P; };
// the walk back from the current particles through the records (rbpf_track_lineage, rbpf_track_summary); chunk c = records
// c * RBPF_TRACK_CHUNK .. + RBPF_TRACK_CHUNK - 1, rows of comp and start are counted from chunk c0
struct TrackWalk {
    TrackLog g;
    int t0, t1, N;                     // records written out [t0, t1); records in the log
    int c0, c1;                        // chunk of t0, chunk of N - 1
    int n;                             // walked particles
    const int32_t* particles;          // [n] current particle indices, or null: all (n == P)
    const int32_t* pending;            // [P] index at record N - 1 of every current particle
    int32_t* comp;                     // [c1 - c0 + 1][P] row c - c0: index at the last record of chunk c -> at the last of chunk c - 1 (row 0 unused)
    int32_t* start;                    // [c1 - c0 + 1][n] row c - c0: index of walked particle j's ancestor at the last record of chunk c
    int32_t* out_idx; double* out_pose;   // [t1 - t0][n], [t1 - t0][n][3]; either may be null
};

// pose modes (kernels_modes.hip): one workgroup clusters one set of P poses.  The tables of a set, in global scratch:
// keys u64 [S] | Q u64 [P] | bin root i32 [S] | up i32 [P] | slot i32 [P] | members i32 [P] | bins i32 [P] | label i32 [P]
static const int MODES_MAX_P = TRACK_SUMMARY_MAX_P;
inline int modes_slots(int P) { int s = 2; while (s < 2 * P) s *= 2; return s; }   // 2 * next_pow2(P): load factor <= 0.5
__host__ __device__ inline size_t modes_label_offset(int P, int S) { return (size_t)S * 12 + (size_t)P * 24; }
__host__ __device__ inline size_t modes_set_bytes(int P, int S) { return (modes_label_offset(P, S) + (size_t)P * 4 + 255) & ~(size_t)255; }
struct ModesArgs {
    int P, S;                          // particles of a set; slots of its bin table
    int n_th, K, mode;                 // heading bins, rows, weights_mode
    double inv, kth;                   // 1 / bin_xy, n_th / (2 pi): computed once on the host
    const double* w_raw; const double* w_given;
    unsigned char* tables;             // [sets][modes_set_bytes]
    long long* info;                   // [sets][4]
    double* rows_f; int32_t* rows_i;   // [sets][K][16], [sets][K][4]; both null: no rows
    int32_t* label;                    // [P] or null: the labels stay in the tables (one set only)
};

// kernel launchers (one translation unit per kernel family)
void launch_pose_modes(const DevView& v, const ModesArgs& a, hipStream_t s);
void launch_track_modes(const TrackLog& g, int t0, int n_sets, const int32_t* d_lineage, const ModesArgs& a, hipStream_t s);   // d_lineage [n_sets][P]
void launch_track_compose(int P, const int32_t* d_did, const int32_t* d_idx, const int32_t* d_pend, int32_t* d_pend2, hipStream_t s);
void launch_track_record(const DevView& v, const TrackLog& g, int t, int32_t* d_pend, hipStream_t s);   // record t from the current state; d_pend becomes the identity
void launch_estimate(const DevView& v, const double* d_given, int mode, double* d_out16, int32_t* d_out4, hipStream_t s);
void launch_track_walk(const TrackWalk& q, hipStream_t s);                        // the three stages
void launch_track_summary(const TrackLog& g, int t0, int t1, const int32_t* d_lineage, const double* d_weight, const double* d_given,
                          int mode, double* d_out_f, int32_t* d_out_i, hipStream_t s);   // d_lineage [t1 - t0][P]
void launch_weight_samples(const DevView& v, const double* d_guesses, const double* d_prs, int K,
                           double* d_out_w, hipStream_t s);
void launch_weight_samples_product(const DevView& v, const double* d_guesses, const double* d_prs, int K, double* d_out_w, hipStream_t s);
int map_update_first_kernel(const DevView& v);   // 0 none, 1 event walk, 2 global-index kernel
int launch_map_update_fused(const DevView& v, const uint8_t* d_bad, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);   // returns the event walk's workgroups (0: it did not run); picks the kernel(s) below; d_bad: NaN-branch weight increments after the update (or nullptr)
void launch_ingest(const void* mapped_src, void* d_dst, size_t bytes, hipStream_t s);   // bytes rounded up to 16
void launch_ingest2(const int32_t* mapped_a, int32_t* d_a, const int32_t* mapped_b, int32_t* d_b, int n, hipStream_t s);
void launch_readback(void* mapped_dst, const double* d_nan_elem, const int32_t* d_did, const int32_t* d_idx, int n, hipStream_t s);
bool map_update_ray_available(const DevView& v);
void launch_map_update_ray(const DevView& v, const int32_t* only, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
bool map_update_ev_available(const DevView& v);
int launch_map_update_ev(const DevView& v, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);   // returns the workgroups launched
void launch_get_odds(const DevView& v, int particle, const double* d_xy, int n, double* d_vals,
                     uint8_t* d_none, hipStream_t s);
void launch_last_scan(const DevView& v, int particle, double* d_out_xy, hipStream_t s);
void launch_imu_update(const DevView& v, int model, double d0, double d1, double d2, double dt_ticks,
                       const double* vel_noise, hipStream_t s);
void launch_resample_indices(int P, const double* d_w, double u, double spread, int32_t* d_T, int32_t* d_idx,
                             int32_t* d_did, int32_t* d_err, hipStream_t s);
void launch_resample_local(const DevView& v, const ResampleBuffers& b, const double* d_w, double u, double spread, hipStream_t s);
// the same in three pieces, for a map update that waits between them (rbpf_resample behind rbpf_scan_update): the plan from the
// weights as they are - unless d_bad marks a particle whose weight the map update still changes - with the particles that update
// may leave out (leave_out == 0: nobody); behind the update the plan once more, which returns at once if the first one stands;
// the copies and the release
void launch_resample_plan_early(const DevView& v, const ResampleBuffers& b, const uint8_t* d_bad, int leave_out, double u, double spread, hipStream_t s);
void launch_resample_plan_late(const DevView& v, const ResampleBuffers& b, double u, double spread, hipStream_t s);
void launch_resample_copies(const DevView& v, const ResampleBuffers& b, hipStream_t s);
void launch_export_weights(const DevView& v, double* d_out, int n_global, const uint8_t* d_bad, hipStream_t s);
void launch_gather_meta(const DevView& v, const int32_t* d_local, int n, int32_t* d_out, hipStream_t s);
void launch_pack(const DevView& v, const void* d_jobs, int n_jobs, void* d_buf, hipStream_t s);
void launch_unpack(const DevView& v, const ResampleBuffers& b, const void* d_jobs, int n_jobs, const void* d_buf, hipStream_t s);
struct PackJobHost { int32_t particle, tile, x0, x1, ya, yb; long long off; };
struct UnpackJobHost { int32_t particle, pos, has, x0, x1, y0, y1, pad; long long off; };
void launch_propose_weight(const DevView& v, const double* d_match, const int32_t* d_match_of, const double* d_guesses, uint8_t* d_bad,
                           uint64_t seed, uint32_t stream, double* d_dbg_w, int p0, int n, hipStream_t s, hipEvent_t done = nullptr);
void launch_bad_weight(const DevView& v, const uint8_t* d_bad, hipStream_t s);
size_t match_lds_bytes(int N, int B, int n_coarse, int per_rot);
int match_sc_capacity(int N, int B, size_t lds);
int match_per_rot(double max_range_m, double mcs);
size_t ndt_lds_bytes(int N, int B);
int ndt_cells(double mcs);
void match_geometry(const rbpf_config& c, double cell_size, int& N, int& ds, double& mcs, double& d0, int& n_coarse_rot);
int match_max_coarse(int n_coarse_rot, double max_range_m, double mcs);
bool launch_match_particles(const DevView& v, int mode, const double* d_ref, int n_ref, double* d_out, int N, int ds,
                            double mcs, double d0, int ncr, double max_range, int cap_sel, size_t lds, int stage, int p0, int n,
                            hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);   // t0 / t1: events carried by the stage's kernel dispatch
void launch_match_single(const DevView& v, const double* d_ref, int n_ref, const double* guess3, const double* range3,
                         const float* d_sel_x, const float* d_sel_y, int n_sel, double* d_out, int N, int ds, double mcs,
                         double d0, int ncr, int cap_sel, size_t lds, uint32_t* d_ndt_occ, double* d_ndt_aux, hipStream_t s);
void launch_match_inputs(const DevView& v, int particle, const double* guess3, double* d_all_curr, int* d_counts,
                         uint32_t* d_mask, int* d_row_cnt, double* d_ref, int cap_ref, double* d_curr, int win,
                         double match_max, hipStream_t s);
void launch_native_sincosf(const float* d_x, int n, float* d_s, float* d_c, hipStream_t s);
size_t raycast_lds_bytes(int B, int reach);
void launch_map_extent(const DevView& v, int particle, int32_t* d_box4, hipStream_t s);   // particle -1: all; d_box4 preset
void launch_render_cells(const DevView& v, int particle, const RenderJob* d_jobs, int n_jobs, long long ny, int8_t* d_out,
                         hipStream_t s);
void launch_render_filter(const DevView& v, const RenderFilter& f, int n_jobs, int G, hipStream_t s);   // G particle chunks
void launch_load_validate(const DevView& v, const LoadArgs& a, hipStream_t s);
void launch_load_map(const DevView& v, const LoadArgs& a, int n_jobs, hipStream_t s);   // tile allocation, then the cells
void launch_load_alloc(const DevView& v, const LoadArgs& a, hipStream_t s);             // the tile allocation alone
void launch_place_warp(const PlaceArgs& q, hipStream_t s);                              // warped / covered rasters of the box
void launch_place_map(const DevView& v, const LoadArgs& a, const PlaceArgs& q, int n_jobs, hipStream_t s);   // tile allocation, then the merge
void launch_cast_scans(const DevView& v, const CastArgs& a, hipStream_t s);
size_t view_gain_lds_bytes(int M, int W);
void launch_view_gain(const DevView& v, const GainArgs& a, hipStream_t s);
void launch_build_map(const BuildArgs& a, hipStream_t s);                       // adds to a.hits / a.seen
size_t refine_lds_bytes(int Mw, int WW);
void launch_refine_poses(const DevView& v, const LocateArgs& f, const RefineArgs& a, hipStream_t s);   // a.packed preset to 0
size_t pairs_field_lds_bytes(int Mw, int WW);
void launch_match_pairs(const PairsArgs& p, const RefineArgs& a, hipStream_t s);  // a.packed preset to 0; a.field unused
void launch_describe_scans(const double* d_ranges, const int32_t* d_sector, int n_scans, int n_beams, int n_rings, double min_range,
                           double max_range, double rings_per_m, unsigned long long* d_desc, int32_t* d_info, hipStream_t s);   // either output may be null
void launch_match_places(const PlacesArgs& a, hipStream_t s);                    // field, search and merge
void launch_score_surface(const SurfaceArgs& a, hipStream_t s);                  // every record and count is written
void launch_locate_scan(const DevView& v, const LocateArgs& a, hipStream_t s);   // a.packed and a.n_items preset to 0
void launch_locate_field(const DevView& v, const LocateArgs& a, hipStream_t s);  // the field kernel alone: particle, x0, y0, M, rows, W, field
void launch_align_points(const DevView& v, const LocateArgs& f, const AlignArgs& a, hipStream_t s);   // a.packed preset to 0
void launch_check_paths(const DevView& v, const PathArgs& a, hipStream_t s);   // one wave per (particle, path)
void launch_check_rollouts(const DevView& v, const RolloutArgs& a, hipStream_t s);   // one wave per (pose, template)
void launch_check_footprints(const DevView& v, const FootArgs& a, hipStream_t s);    // one wave per (pose or particle, template)
size_t local_lds_bytes(const LocalArgs& a);
void launch_local_crop(const DevView& v, const LocalArgs& a, hipStream_t s);        // one workgroup per pose of the batch
void launch_local_fuse(const DevView& v, const LocalArgs& a, hipStream_t s);        // the batch's sums, added into a.fused (preset to 0 before the first)
void launch_check_scans(const DevView& v, const ScanCheckArgs& a, hipStream_t s);   // a.cost, a.counts and a.votes preset to 0
void launch_travel_mask(const DevView& v, const TravelArgs& a, hipStream_t s);   // a.ras preset to TRAVEL_INF, a.dirty to 0: clearance, T, the starts
void launch_travel_round(const TravelArgs& a, int parity, int32_t* d_count, hipStream_t s);   // one round (rbpf_blockrelax.h); d_count[0] += blocks it changed, d_count[32] += blocks that ran
void launch_travel_output(const TravelArgs& a, hipStream_t s);                   // cost_out and goal_out from the finished field
void launch_frontier_mask(const DevView& v, const FrontierArgs& a, hipStream_t s);   // a.ras preset to FRONTIER_NONE, a.aux, a.dirty, a.counts to 0: F, its seeds, |F|
void launch_frontier_round(const FrontierArgs& a, int parity, int32_t* d_count, hipStream_t s);   // one labelling round; d_count as launch_travel_round
void launch_frontier_output(const FrontierArgs& a, hipStream_t s);               // from the finished labels: sizes, the table, label_out
void launch_score_ref(const DevView& v, const ScoreArgs& a, hipStream_t s);      // the reference's near_r rows and block sums; a.bad preset to 0
void launch_score_maps(const DevView& v, const ScoreArgs& a, hipStream_t s);     // a.scores preset to 0; after launch_score_ref
}  // namespace rbpf
