// rbpf_host.h -- host side of librbpf_hip.so (rbpf_api.hip only): the types that own memory and events, and the handle
// built from them.  An entry point never allocates, frees or creates an event itself: it asks one of these types, and
// rbpf_destroy releases each kind in one loop.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

#include "rbpf_internal.h"

static const size_t LDS_LIMIT = 160 * 1024;    // LDS of one gfx950 workgroup

// Grow-only memory of one kind.  Contents are not kept when it grows; a failed growth leaves {nullptr, 0}.
enum MemKind { MEM_DEVICE, MEM_PINNED, MEM_PAGEABLE };
struct Block {
    MemKind kind = MEM_DEVICE;
    unsigned char* p = nullptr; size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (p && cap >= bytes) return hipSuccess;
        release();
        const size_t want = kind == MEM_PINNED ? std::max<size_t>(bytes * 2, 1 << 16) : std::max<size_t>(bytes, 4096);   // pinning is slow: grow rarely
        hipError_t e = hipSuccess;
        if (kind == MEM_DEVICE) e = hipMalloc(reinterpret_cast<void**>(&p), want);
        else if (kind == MEM_PINNED) e = hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault);
        else if (!(p = static_cast<unsigned char*>(malloc(want)))) e = hipErrorOutOfMemory;
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
    void release() {
        if (kind == MEM_DEVICE) (void)hipFree(p); else if (kind == MEM_PINNED) (void)hipHostFree(p); else free(p);
        p = nullptr; cap = 0;
    }
    template <typename T> T* as(size_t byte_offset = 0) const { return reinterpret_cast<T*>(p + byte_offset); }
};
// the handle's device scratch: what each block holds ("host outputs": the staging of outputs the caller wants in host memory)
enum {
    B_SAMPLES,                      // the samples of rbpf_weight_samples
    B_GT, B_GIDX,                   // table and ancestors of the global resample
    B_I32, B_JOBS,                  // departing particles and job list of a migration
    B_DRAIN_FIRST,                  // from here on queued work may still read a block: h->reserve drains the stream before it grows
    B_RENDER = B_DRAIN_FIRST,       // LUT, weights and jobs of the last render
    B_RENDER_PART, B_RENDER_OUT,    // the group sums of a split render; the outputs of a render to host memory
    B_LOAD,                         // flag, touched tiles, jobs and host raster of a map load
    B_CAST,                         // poses, beams, host outputs
    B_LOCATE,                       // rotations, beams, offset table, field planes, candidate words, merge raster, host outputs
    B_PLACE,                        // flag, touched tiles, jobs, host source, host outputs
    B_ALIGN,                        // rotations, points, offset table, field planes, merge raster, host outputs
    B_GAIN,                         // poses, beams, table, host outputs
    B_TRAVEL,                       // start and goal cells, round counters, cost fields, traversable bits, dirty flags, host outputs
    B_FRONTIER,                     // round counters, region counts, tables, label and size rasters, dirty flags, host labels
    B_SCORE,                        // flag, table, reference raster, near rows, block sums, host scores
    B_TRACK,                        // particle list or weights, chunk maps, chunk starts, lineage table, mode tables, host outputs
    B_BUILD,                        // poses, beams, ranges, end cells, host rasters
    B_REFINE,                       // guesses, rotations, beams, ranges, centre cells, field planes, merge words, host outputs
    B_PAIRS,                        // guesses, rotations, scan poses, beams, ranges, pair lists, the pairs' fields, merge words, host outputs
    B_PLACES,                       // sectors and ranges, or limits and descriptor tables, dilated references, weights, chunk lists, host outputs
    B_SURFACE,                      // host volume, host drops, host outputs
    B_PATHS,                        // waypoint cells, waypoint steps, path offsets, host outputs
    B_SCANCHECK,                    // poses, beams, ranges, cost tables, host outputs
    B_ROLLOUTS,                     // poses, template waypoints, template offsets, host outputs
    B_FOOTPRINTS,                   // poses, pose bins, template waypoints and bins, template offsets, span offsets, spans, host outputs
    B_LOCAL,                        // poses, sample tables, weights, host outputs, the crops and the group sums of a batch
    B_COUNT
};

// A device temporary of one call (diagnostic entry points), freed on every return path.  hipFree waits for the device, so an
// early error return cannot pull memory from under queued work.
struct DevTemp : Block { DevTemp() = default; DevTemp(const DevTemp&) = delete; ~DevTemp() { release(); } };

// Host memory that work queued on a stream reads (an upload) or writes (the early read-back), guarded by an event created
// with it: begin() before the host touches it again, submitted() once that work is queued.
struct Staging : Block {
    unsigned ev_flags = hipEventDisableTiming | hipEventDisableSystemFence;     // guards host memory a copy only reads
    hipEvent_t ev = nullptr; bool used = false;
    hipError_t wait() { return used ? hipEventSynchronize(ev) : hipSuccess; }
    hipError_t reserve(size_t bytes) {
        if (!ev) { const hipError_t e = hipEventCreateWithFlags(&ev, ev_flags); if (e != hipSuccess) { ev = nullptr; return e; } }
        return Block::reserve(bytes);
    }
    hipError_t begin(size_t bytes) { const hipError_t e = wait(); return e != hipSuccess ? e : reserve(bytes); }
    hipError_t submitted(hipStream_t s) { const hipError_t e = hipEventRecord(ev, s); if (e == hipSuccess) used = true; return e; }
    hipError_t upload(void* dst, size_t bytes, hipStream_t s) {
        const hipError_t e = hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
        return e != hipSuccess ? e : submitted(s);
    }
    // the device address of pinned memory when the runtime maps it (a kernel then reads or writes it directly), else nullptr
    void* mapped() const {
        void* m = nullptr;
        if (hipHostGetDevicePointer(&m, p, 0) != hipSuccess) { (void)hipGetLastError(); m = nullptr; }
        return m;
    }
    void destroy_event() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; used = false; }
};
// host staging, pageable unless noted: what is uploaded into the block of the same name
enum {
    S_JOBS,                         // job lists of the pack / unpack kernels (pinned)
    S_EARLY,                        // the landing zone of the early resample read-back (pinned)
    S_RENDER, S_CAST, S_LOAD, S_LOCATE, S_PLACE, S_ALIGN, S_GAIN,   // the upload of B_RENDER .. B_GAIN
    S_TRAVEL,                       // the round counters a travel cost reads back and, behind them, its upload (pinned)
    S_FRONTIER,                     // the round counters a frontier labelling reads back (pinned)
    S_SCORE,                        // the table and the host reference
    S_TRACK,                        // the particle list or the weights
    S_BUILD, S_REFINE, S_PAIRS, S_PLACES, S_SURFACE,   // the upload of B_BUILD .. B_SURFACE: everything in front of the first '|' of its layout
    S_PATHS,                        // the upload of B_PATHS
    S_SCANCHECK,                    // the upload of B_SCANCHECK
    S_ROLLOUTS,                     // the upload of B_ROLLOUTS
    S_FOOTPRINTS,                   // the upload of B_FOOTPRINTS
    S_LOCAL,                        // the upload of B_LOCAL
    S_COUNT
};

// Pinned staging ring for the per-step uploads (scan block, previous scan, index vectors): a slot is reused only after the
// copy that read it has completed (its event), so uploading never drains the stream.
struct PinnedRing {
    static const int N = 4;
    Staging slot[N] = {{{MEM_PINNED}}, {{MEM_PINNED}}, {{MEM_PINNED}}, {{MEM_PINNED}}}; int next = 0;
    hipError_t create(size_t slot_bytes) {
        for (Staging& s : slot) { const hipError_t e = s.reserve(slot_bytes); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    void* acquire() { (void)slot[next].wait(); return slot[next].p; }
    void* mapped() const { return slot[next].mapped(); }
    void submitted(hipStream_t s) { (void)slot[next].submitted(s); next = (next + 1) % N; }
    // the first `bytes` of the acquired slot -> dst.  Pinned and device-mapped: a kernel pulls them over (no copy-engine latency
    // in the stream); DMA otherwise
    hipError_t upload(void* dst, size_t bytes, hipStream_t s) {
        if (void* m = mapped()) rbpf::launch_ingest(m, dst, bytes, s);
        else { const hipError_t e = hipMemcpyAsync(dst, slot[next].p, bytes, hipMemcpyHostToDevice, s); if (e != hipSuccess) return e; }
        submitted(s);
        return hipSuccess;
    }
};
enum { R_SCAN, R_LAST, R_IDX, R_COUNT };

// events that live as long as the handle (timing rings, ev_weights)
struct EventPool {
    std::vector<hipEvent_t> all;
    hipError_t create(hipEvent_t* out, unsigned flags) {
        const hipError_t e = hipEventCreateWithFlags(out, flags);
        if (e == hipSuccess) all.push_back(*out); else *out = nullptr;
        return e;
    }
    void destroy() { for (hipEvent_t ev : all) (void)hipEventDestroy(ev); all.clear(); }
};

struct rbpf_handle {
    rbpf_config cfg;
    rbpf::DevView v;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool profiling = false;
    unsigned prof_mask = 0;                     // kernel families whose launches are bracketed by timing events (bit k = family k)
    bool have_scan = false;
    bool dedup_enabled = true;                  // exact duplicates share one matcher run (RBPF_MATCH_DEDUP=0 turns it off)
    std::string err;
    std::vector<uint32_t> h_lut;
    std::vector<Block> allocs;                  // dev_alloc: device memory that lives as long as the handle
    Block buf[B_COUNT];
    Staging stage[S_COUNT] = {{{MEM_PINNED}}, {{MEM_PINNED}, hipEventDisableTiming},   // the host reads S_EARLY after its event: system-scope release
                              {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming},
                              {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming},
                              {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PINNED}, hipEventDisableTiming}, {{MEM_PINNED}, hipEventDisableTiming},
                              {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming},
                              {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming},
                              {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming},
                              {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming}, {{MEM_PAGEABLE}, hipEventDisableTiming}};
    // grows scratch buffer b; queued work may still read the old block of those from B_DRAIN_FIRST on, so the stream drains first
    hipError_t reserve(int b, size_t bytes) {
        if (buf[b].cap >= bytes) return hipSuccess;
        if (b >= B_DRAIN_FIRST) { const hipError_t e = hipStreamSynchronize(stream); if (e != hipSuccess) return e; }
        return buf[b].reserve(bytes);
    }
    PinnedRing rings[R_COUNT];
    EventPool events;
    template <typename F> void each_staging(F f) { for (Staging& s : stage) f(s); for (PinnedRing& r : rings) for (Staging& s : r.slot) f(s); }
    hipEvent_t ev_weights = nullptr; bool ev_weights_valid = false, record_ev_weights = false, begin_seen = false;   // recorded after the weighting kernel of rbpf_scan_update_begin
    int32_t* d_did_early = nullptr; bool scan_begun = false;
    int early_n = 0;                            // entries of the early resample read-back in flight (S_EARLY), 0 = none
    unsigned char* d_scan = nullptr; size_t scan_bytes = 0;   // device scan block (rbpf_create points the DevView's scan arrays into it)
    // a slot of rings[R_SCAN] is laid out as the device scan block: the slot's copy of one of the DevView's scan arrays
    template <typename T> T* in_slot(unsigned char* slot, const T* dev) const { return reinterpret_cast<T*>(slot + (reinterpret_cast<const unsigned char*>(dev) - d_scan)); }
    int mN = 0, mds = 1, mncr = 0; double mmcs = 0, md0 = 0; size_t mlds = 0;
    double* d_last_xy = nullptr; float* d_tmp_sel = nullptr;
    int n_last_dev = -1;                       // points of the device-resident previous scan (rbpf_refresh_last_scan), -1 = none
    int match_rows = 0;                        // d_match: 0 not written by the built-in matcher, 1 its rows, 2 its rows with duplicates skipped (dup_of)
    double* d_match = nullptr; uint8_t* d_bad = nullptr; double* d_guess_full = nullptr;
    unsigned long long resample_draws = 0;
    int ev_workgroups = 0;                                    // workgroups of the event-walk kernel in the last map update (0: it did not run); rbpf_get_map_update_workgroups
    bool map_updates = true;                                  // rbpf_set_map_updates: off = localization, the maps stay as they are
    // rbpf_scan_update holds its map update back (with the NaN-branch increments and the step's own trajectory record, whose place
    // in the log, mu_pending_rec, is taken at the call; -1: none) until the next call: rbpf_resample launches it behind its plan,
    // without the particles the plan discards; every other entry point launches it whole, first thing (ON_DEVICE)
    bool mu_pending = false; int mu_pending_rec = -1;
    // Holding back pays where leaving a tenth of the particles out saves rounds of the map kernel over the CUs: measured a loss
    // at four particles per CU (1024: the map kernel's four rounds stay four, the second plan launch and the list cost 8 us), a gain
    // at sixteen and forty.  hold_back: more than four particles per CU, or RBPF_SKIP_DISCARDED set (tests, A/B
    // runs: 1 holds back whatever the size, 0 does too and leaves nobody out - the same order of launches)
    bool hold_back = false, skip_discarded = true;
    // The front half of a scan step (matcher, NDT, proposal frame, samples, weighting) as two staggered half-batches: particles
    // [0, halves_first) on `side`, a stream of the handle's own with the device's highest priority, the rest on `stream`, so that
    // one half's kernels fill the CUs the other half's kernel leaves idle while its last workgroups drain.
    // Streams and the three events below are all the synchronisation there is.  halves_first = 0: one stream, as before
    // (RBPF_SCAN_HALVES=0, or unset below the size rule of rbpf_create); never while the match, ndt or weight family is timed
    hipStream_t side = nullptr;
    int halves_first = 0;
    hipEvent_t ev_fork = nullptr, ev_half_match = nullptr, ev_half_weight = nullptr;   // uploads queued; first half's match rows final; its weighting done
    bool halves_now() const { return halves_first > 0 && side && !(prof_mask & 0x1Au); }
    // profiling: a ring of HIP-event pairs per kernel family, recorded on the handle's stream
    static const int N_KERN = 5, RING = 512;        // 0 map update, 1 propose/weight, 2 resample, 3 match (grid stage), 4 match (NDT stage)
    std::vector<hipEvent_t> ring[N_KERN][2];
    int ring_n[N_KERN] = {0, 0, 0, 0, 0};
    std::vector<hipEvent_t> begin_used[N_KERN];     // the event that marks a launch's start: its own, or the previous family's end
    hipEvent_t last_end = nullptr;
    bool timed(int k) const { return (prof_mask >> k) & 1u; }
    void prof_begin(int k) { if (!timed(k)) return; hipEvent_t e = ring[k][0][ring_n[k] % RING]; (void)hipEventRecord(e, stream); begin_used[k][ring_n[k] % RING] = e; if (k == 2) rs_split[ring_n[k] % RING] = 0; }
    // the previous timed family ended right before this one starts (nothing enqueued in between): one record serves both
    void prof_begin_chained(int k) { if (!timed(k)) return; if (!last_end) { prof_begin(k); return; } begin_used[k][ring_n[k] % RING] = last_end; }
    void prof_end(int k) { if (!timed(k)) return; last_end = ring[k][1][ring_n[k] % RING]; (void)hipEventRecord(last_end, stream); ring_n[k]++; }
    // a resample whose launches stand on both sides of a map update (mu_pending) is still one entry of family 2: the time from
    // its begin to the pause plus the time from the resume to its end
    std::vector<hipEvent_t> rs_mid[2]; std::vector<char> rs_split;
    void prof_pause(int k) { if (!timed(k)) return; const int slot = ring_n[k] % RING; (void)hipEventRecord(rs_mid[0][slot], stream); rs_split[slot] = 1; }
    void prof_resume(int k) { if (!timed(k)) return; (void)hipEventRecord(rs_mid[1][ring_n[k] % RING], stream); }
    hipError_t family_ms(int k, int slot, float* ms) {
        if (k != 2 || !rs_split[slot]) return hipEventElapsedTime(ms, begin_used[k][slot], ring[k][1][slot]);
        float a = 0, b = 0;
        hipError_t e = hipEventElapsedTime(&a, begin_used[k][slot], rs_mid[0][slot]);
        if (e == hipSuccess) e = hipEventElapsedTime(&b, rs_mid[1][slot], ring[k][1][slot]);
        *ms = a + b;
        return e;
    }
    // a family that is one kernel: its timing events ride on the dispatch and take the kernel's own start and end (no event
    // records in the stream).  False, and both null, if the family is not timed.
    bool prof_take(int k, hipEvent_t& t0, hipEvent_t& t1) {
        t0 = t1 = nullptr;
        if (!timed(k)) return false;
        const int slot = ring_n[k] % RING;
        t0 = ring[k][0][slot]; t1 = ring[k][1][slot]; begin_used[k][slot] = t0; last_end = nullptr; ring_n[k]++;
        return true;
    }
    rbpf::ResampleBuffers rs;
    rbpf_counters counters;
    unsigned long long scan_updates = 0;
    // rbpf_set_proposal_capture / rbpf_get_proposal (tests): the raw sample weights of the last proposal, [P][K], allocated on first use
    bool prop_capture = false, prop_valid = false, prop_captured = false;
    double* d_prop_w = nullptr;
    uint64_t travel_stats[3] = {0, 0, 0};      // rbpf_travel_stats: rounds, block runs, (particle, block) pairs of the last rbpf_travel_cost
    uint64_t frontier_stats[3] = {0, 0, 0};    // rbpf_frontier_stats: the same of the last rbpf_frontier_regions
    // rbpf_track_*: the trajectory log.  Off unless rbpf_track_begin was called
    bool track_on = false; uint32_t track_flags = 0;
    int track_cap = 0, track_n = 0, track_dropped = 0, track_cur = 0;   // records allocated, written, dropped; which half of T_PENDING is current
    enum { T_LOG, T_PENDING, T_COUNT };
    Block track_mem[T_COUNT];                  // the records; pending[2][P], swapped after every local resample
    rbpf::TrackLog track_log() const { return {track_mem[T_LOG].p, rbpf::track_record_stride(v.P), v.P}; }
    int32_t* track_pending(int which) const { return track_mem[T_PENDING].as<int32_t>((size_t)which * v.P * 4); }
};
