// kernels_render.hip -- map read-out (include/rbpf_hip.h, rbpf_map_extent / rbpf_render_map): the written-cell extent of
// the maps, one particle's map as a dense int8 raster, and the filter-wide occupancy probability and occupied-weight share.
//
// A render box is cut on the host at lattice tile seams into jobs (RenderJob): up to 16 storage rows x 256 storage columns of
// ONE lattice tile position.  A job's tile id, its written box (tile_bbox) and the particle's slot are then the same in every
// lane of the workgroup (scalar loads).  Lane l owns row i0 + (l >> 4) and the 16 cells j0 + 16 (l & 15) .. + 15, read with
// one 16-byte load: pool rows are contiguous in y and j0 is a multiple of 16.  A lane whose cells miss the tile's written box
// loads nothing - outside tile_bbox a tile holds 0 (kernels_resample.hip relies on the same) - so the work per particle
// follows the explored area, not the lattice.
#include "rbpf_internal.h"

#include <limits.h>

namespace rbpf {

static const int RB = 256;            // 4 waves: 16 rows x 16 strips of 16 cells
static const int RU = 4;              // particles whose strips are loaded before any is accumulated

union Strip { uint4 u; int8_t c[16]; };

// the 16 cells of a lane's strip in tile `t` (zero where the strip leaves the written box: those cells are zero)
template <bool WIDE>
__device__ __forceinline__ Strip load_strip(const DevView& v, int t, int row, int js) {
    Strip s;
    s.u = make_uint4(0u, 0u, 0u, 0u);
    const int8_t* src = v.pool + (size_t)t * v.dim * v.dim + (size_t)row * v.dim + js;
    if (WIDE) {                                     // dim % 16 == 0: every strip is whole and 16-byte aligned
        s.u = *reinterpret_cast<const uint4*>(src);
    } else {
#pragma unroll
        for (int c = 0; c < 16; ++c) s.c[c] = js + c < v.dim ? src[c] : (int8_t)0;
    }
    return s;
}

// does the lane's strip (row, js .. js+15) touch tile t's written box?
__device__ __forceinline__ bool strip_written(const DevView& v, int t, int row, int js) {
    const int* bb = v.tile_bbox + 4 * (size_t)t;
    return row >= bb[0] && row <= bb[1] && js <= bb[3] && js + 15 >= bb[2];
}

__device__ __forceinline__ int lane_tile(const DevView& v, int pos, int p) {
    return pos < 0 ? -1 : v.tile_tab[(size_t)v.slot[p] * v.L * v.L + pos];
}

// ---- extent: union of the written boxes of every tile of particles [p_lo, p_hi), in mosaic cells -----------------------
__global__ __launch_bounds__(RB) void map_extent_kernel(DevView v, int p_lo, int p_hi, int32_t* box) {
    __shared__ int s[4];
    const int tid = threadIdx.x;
    if (tid < 4) s[tid] = (tid & 1) ? INT_MIN : INT_MAX;
    __syncthreads();
    const int LL = v.L * v.L, half = v.dim / 2;
    int m0 = INT_MAX, m1 = INT_MIN, m2 = INT_MAX, m3 = INT_MIN;
    const long long n = (long long)(p_hi - p_lo) * LL;
    for (long long k = (long long)blockIdx.x * RB + tid; k < n; k += (long long)gridDim.x * RB) {
        const int p = p_lo + (int)(k / LL), pos = (int)(k % LL);
        const int t = lane_tile(v, pos, p);
        if (t < 0) continue;
        const int* bb = v.tile_bbox + 4 * (size_t)t;
        const int b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
        if (b0 > b1 || b2 > b3) continue;           // allocated, nothing written yet
        const int ox = (pos / v.L - v.R) * v.dim - half, oy = (pos % v.L - v.R) * v.dim - half;
        m0 = min(m0, ox + b0); m1 = max(m1, ox + b1); m2 = min(m2, oy + b2); m3 = max(m3, oy + b3);
    }
    if (m0 <= m1) { atomicMin(&s[0], m0); atomicMax(&s[1], m1); atomicMin(&s[2], m2); atomicMax(&s[3], m3); }
    __syncthreads();
    if (tid == 0 && s[0] <= s[1]) { atomicMin(box + 0, s[0]); atomicMax(box + 1, s[1]); atomicMin(box + 2, s[2]); atomicMax(box + 3, s[3]); }
}

// ---- one particle: a plain gather ----------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(RB) void render_cells_kernel(DevView v, int p, const RenderJob* jobs, long long ny, int8_t* out) {
    const RenderJob j = jobs[blockIdx.x];
    const int tid = threadIdx.x, r = tid >> 4, row = j.i0 + r, js = j.j0 + 16 * (tid & 15);
    if (r >= j.ni || js >= j.jhi || js + 16 <= j.jlo) return;
    const int t = lane_tile(v, j.pos, p);
    Strip s;
    s.u = make_uint4(0u, 0u, 0u, 0u);
    if (t >= 0 && strip_written(v, t, row, js)) s = load_strip<WIDE>(v, t, row, js);
    int8_t* dst = out + (long long)(j.ox + r) * ny + (j.oy + 16 * (tid & 15));
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (js + c >= j.jlo && js + c < j.jhi) dst[c] = s.c[c];
}

// ---- the whole filter ----------------------------------------------------------------------------------------------------
// Particles are summed in groups of f.C, in index order inside a group and group after group: per cell and lane
//   acc_g = 0 + w_p sigma(v_p) + ...   over the group,   total = 0 + acc_0 + acc_1 + ...
// in float64.  blockIdx.y takes the groups [y * ngroups / G, (y+1) * ngroups / G).  With G = 1 (SPLIT = false) the kernel
// adds the group sums itself; with G > 1 it stores each group's sums in f.part_* and render_reduce_kernel adds them in the
// same order.  Both perform the same float64 operations, so the result does not depend on G.
template <bool SPLIT, bool WIDE>
__global__ __launch_bounds__(RB) void render_filter_kernel(DevView v, RenderFilter f) {
    __shared__ double s_lut[256];                   // sigma(value * quantum), indexed by the cell's byte
    const int tid = threadIdx.x;
    s_lut[tid] = f.lut[tid];
    __syncthreads();
    const RenderJob j = f.jobs[blockIdx.x];
    const int r = tid >> 4, row = j.i0 + r, js = j.j0 + 16 * (tid & 15);
    const bool lane_ok = r < j.ni && js < j.jhi && js + 16 > j.jlo;
    const int g_lo = (int)((long long)blockIdx.y * f.ngroups / gridDim.y);
    const int g_hi = (int)((long long)(blockIdx.y + 1) * f.ngroups / gridDim.y);
    const int thr = v.cc.thr;
    double tp[16], to[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { tp[c] = 0.0; to[c] = 0.0; }
    for (int g = g_lo; g < g_hi; ++g) {
        double ap[16], ao[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) { ap[c] = 0.0; ao[c] = 0.0; }
        const int p_end = min(v.P, (g + 1) * f.C);
        int t_next = lane_tile(v, j.pos, g * f.C);
        for (int p0 = g * f.C; p0 < p_end; p0 += RU) {
            Strip d[RU];
            double w[RU];
#pragma unroll
            for (int u = 0; u < RU; ++u) {          // issue up to RU loads before the first use
                const int p = p0 + u;
                d[u].u = make_uint4(0u, 0u, 0u, 0u);
                w[u] = 0.0;
                if (p < p_end) {
                    const int t = t_next;
                    t_next = p + 1 < p_end ? lane_tile(v, j.pos, p + 1) : -1;   // next particle's tile id ahead of its use
                    w[u] = f.w[p];
                    if (t >= 0 && lane_ok && strip_written(v, t, row, js)) d[u] = load_strip<WIDE>(v, t, row, js);
                }
            }
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                if (p0 + u >= p_end) break;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int cv = d[u].c[c];
                    ap[c] += w[u] * s_lut[cv & 255];
                    ao[c] += cv > thr ? w[u] : 0.0;
                }
            }
        }
        if (SPLIT) {
            if (lane_ok) {
                const size_t base = (size_t)g * f.ncell + (size_t)(j.ox + r) * f.ny + (j.oy + 16 * (tid & 15));
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (js + c >= j.jlo && js + c < j.jhi) {
                        if (f.prob) f.part_p[base + c] = ap[c];
                        if (f.occ) f.part_o[base + c] = ao[c];
                    }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c) { tp[c] += ap[c]; to[c] += ao[c]; }
        }
    }
    if (!SPLIT && lane_ok) {
        const size_t base = (size_t)(j.ox + r) * f.ny + (j.oy + 16 * (tid & 15));
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (js + c >= j.jlo && js + c < j.jhi) {
                if (f.prob) f.prob[base + c] = (float)(tp[c] / f.S);
                if (f.occ) f.occ[base + c] = (float)(to[c] / f.S);
            }
    }
}

__global__ __launch_bounds__(RB) void render_reduce_kernel(RenderFilter f) {
    for (size_t c = (size_t)blockIdx.x * RB + threadIdx.x; c < f.ncell; c += (size_t)gridDim.x * RB) {
        if (f.prob) {
            double s = 0.0;
            for (int g = 0; g < f.ngroups; ++g) s += f.part_p[(size_t)g * f.ncell + c];
            f.prob[c] = (float)(s / f.S);
        }
        if (f.occ) {
            double s = 0.0;
            for (int g = 0; g < f.ngroups; ++g) s += f.part_o[(size_t)g * f.ncell + c];
            f.occ[c] = (float)(s / f.S);
        }
    }
}

static unsigned grid_for(long long n) { return (unsigned)std::max(1LL, std::min((n + RB - 1) / RB, 2048LL)); }

void launch_map_extent(const DevView& v, int particle, int32_t* d_box4, hipStream_t s) {
    const int p_lo = particle < 0 ? 0 : particle, p_hi = particle < 0 ? v.P : particle + 1;
    map_extent_kernel<<<grid_for((long long)(p_hi - p_lo) * v.L * v.L), RB, 0, s>>>(v, p_lo, p_hi, d_box4);
}

void launch_render_cells(const DevView& v, int particle, const RenderJob* d_jobs, int n_jobs, long long ny, int8_t* d_out,
                         hipStream_t s) {
    if (v.dim % 16 == 0) render_cells_kernel<true><<<n_jobs, RB, 0, s>>>(v, particle, d_jobs, ny, d_out);
    else render_cells_kernel<false><<<n_jobs, RB, 0, s>>>(v, particle, d_jobs, ny, d_out);
}

void launch_render_filter(const DevView& v, const RenderFilter& f, int n_jobs, int G, hipStream_t s) {
    const dim3 grid(n_jobs, G);
    const bool wide = v.dim % 16 == 0;
    if (G == 1) {
        if (wide) render_filter_kernel<false, true><<<grid, RB, 0, s>>>(v, f);
        else render_filter_kernel<false, false><<<grid, RB, 0, s>>>(v, f);
        return;
    }
    if (wide) render_filter_kernel<true, true><<<grid, RB, 0, s>>>(v, f);
    else render_filter_kernel<true, false><<<grid, RB, 0, s>>>(v, f);
    render_reduce_kernel<<<grid_for((long long)f.ncell), RB, 0, s>>>(f);
}

}  // namespace rbpf
