// kernels_load.hip -- map loading (include/rbpf_hip.h, rbpf_load_map): a dense int8 raster written into the tiles of one
// particle or of every particle, the inverse of kernels_render.hip's render_cells_kernel.
//
// The box is cut on the host at lattice tile seams into jobs (RenderJob) of up to 16 storage rows x 256 storage columns of
// ONE lattice position, with column blocks starting at multiples of 32: lanes 2k and 2k+1 then hold the two halves of one
// occupancy word, and no word or 16-cell group is shared by two jobs.  Lane l owns row i0 + (l >> 4) and the 16 cells
// j0 + 16 (l & 15) .. + 15.  It reads its raster cells once per workgroup (byte loads: the raster offset is arbitrary) and
// keeps them in registers while it walks the workgroup's chunk of particles (grid.y, at most 256, their tile ids staged in
// LDS first).  Per particle it merges them with the tile's current cells where its group sticks out of the box, writes the
// group with one 16-byte store (dim % 16 == 0: the pool rows are 16-byte aligned) and forms its 16 occupancy bits; the pair
// joins them with one cross-lane exchange and the even lane stores the word.  Lanes outside the box whose word touches it
// still read their cells for the word's bits.
//
// load_alloc_kernel runs first: one thread per (particle, touched lattice position) pops a missing tile from the free stack
// (free tiles are zero-filled, as alloc_missing_tiles in rbpf_mapupdate.h) and widens the tile's written box by (box n tile).
// The host has counted the missing tiles against free_top before, so the pops cannot run dry.
#include "rbpf_internal.h"

#include <limits.h>

namespace rbpf {

static const int LB = 256;            // 4 waves: 16 rows x 16 groups of 16 cells

union Cells16 { uint4 u; int8_t c[16]; };

// ---- device input: every value in [vmin, vmax] -------------------------------------------------------------------------
__global__ __launch_bounds__(LB) void load_validate_kernel(LoadArgs a, int vmin, int vmax) {
    bool bad = false;
    for (long long k = (long long)blockIdx.x * LB + threadIdx.x; k < a.ncell; k += (long long)gridDim.x * LB) {
        const int c = a.cells[k];
        bad |= c < vmin || c > vmax;
    }
    if (bad) atomicOr(a.bad, 1);
}

// ---- tiles: allocate the missing ones, widen the written boxes -----------------------------------------------------------
__global__ __launch_bounds__(LB) void load_alloc_kernel(DevView v, LoadArgs a) {
    if (*a.bad) return;
    const long long k = (long long)blockIdx.x * LB + threadIdx.x;
    if (k >= (long long)(a.p_hi - a.p_lo) * a.n_tiles) return;
    const int p = a.p_lo + (int)(k / a.n_tiles);
    const LoadTile lt = a.tiles[k % a.n_tiles];
    int32_t* e = v.tile_tab + (size_t)v.slot[p] * v.L * v.L + lt.pos;
    int t = *e;
    int b0, b1, b2, b3;
    if (t < 0) {
        const int idx = atomicSub(v.free_top, 1) - 1;
        if (idx < 0) {                                  // not reached: the host counted the tiles first
            atomicAdd(v.free_top, 1);
            atomicCAS(v.err, 0, RBPF_ENOMEM);
            return;
        }
        t = v.free_stack[idx];
        *e = t;
        b0 = INT_MAX; b1 = -1; b2 = INT_MAX; b3 = -1;
    } else {
        const int* bb = v.tile_bbox + 4 * (size_t)t;
        b0 = bb[0]; b1 = bb[1]; b2 = bb[2]; b3 = bb[3];
    }
    int* bb = v.tile_bbox + 4 * (size_t)t;
    bb[0] = min(b0, lt.i0); bb[1] = max(b1, lt.i1); bb[2] = min(b2, lt.j0); bb[3] = max(b3, lt.j1);
}

// ---- cells and occupancy words ---------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(LB) void load_cells_kernel(DevView v, LoadArgs a) {
    if (*a.bad) return;
    const RenderJob j = a.jobs[blockIdx.x];
    const int tid = threadIdx.x, r = tid >> 4, g = tid & 15, row = j.i0 + r, js = j.j0 + 16 * g, wj = js & ~31;
    const bool row_ok = r < j.ni;
    const int c_lo = max(j.jlo - js, 0), c_hi = min(j.jhi - js, 16);         // the lane's cells [c_lo, c_hi) lie in the box
    const bool mine = row_ok && c_lo < c_hi;
    const bool word = row_ok && wj < j.jhi && wj + 32 > j.jlo && js < v.dim; // the pair's word touches the box
    const int n_tile = min(16, v.dim - js);                                  // cells of the group inside the tile (<= 0: none)
    Cells16 in;
    in.u = make_uint4(0u, 0u, 0u, 0u);
    unsigned inmask = 0u;
    if (mine) {
        const int8_t* src = a.cells + (long long)(j.ox + r) * a.ny + (j.oy + 16 * g);
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c >= c_lo && c < c_hi) in.c[c] = src[c];
        inmask = ((1u << c_hi) - 1u) & ~((1u << c_lo) - 1u);
    }
    const bool whole = inmask == 0xFFFFu;
    const int* bbox = v.tile_bbox;
    const int n = a.p_hi - a.p_lo;
    const int q_lo = a.p_lo + (int)((long long)blockIdx.y * n / gridDim.y);
    const int q_hi = a.p_lo + (int)((long long)(blockIdx.y + 1) * n / gridDim.y);   // at most LB particles
    // the chunk's tile ids up front: the stores below then follow one another without a dependent load in between
    __shared__ int s_tile[LB];
    if (q_lo + tid < q_hi) s_tile[tid] = v.tile_tab[(size_t)v.slot[q_lo + tid] * v.L * v.L + j.pos];
    __syncthreads();
    for (int p = q_lo; p < q_hi; ++p) {
        const int t = s_tile[p - q_lo];
        if (t < 0) continue;                            // only after a failed allocation (RBPF_ENOMEM is set)
        int8_t* tile = v.pool + (size_t)t * v.dim * v.dim + (size_t)row * v.dim;
        Cells16 cur;
        cur.u = make_uint4(0u, 0u, 0u, 0u);
        if (word && !whole) {                           // outside the written box a tile holds 0
            const int* bb = bbox + 4 * (size_t)t;
            if (row >= bb[0] && row <= bb[1] && js <= bb[3] && js + 15 >= bb[2]) {
                if (WIDE) cur.u = *reinterpret_cast<const uint4*>(tile + js);
                else {
#pragma unroll
                    for (int c = 0; c < 16; ++c) if (c < n_tile) cur.c[c] = tile[js + c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) if ((inmask >> c) & 1u) cur.c[c] = in.c[c];
        if (mine) {
            if (WIDE) *reinterpret_cast<uint4*>(tile + js) = cur.u;
            else {
#pragma unroll
                for (int c = 0; c < 16; ++c) if (c < n_tile) tile[js + c] = cur.c[c];
            }
        }
        unsigned bits = 0u;
#pragma unroll
        for (int c = 0; c < 16; ++c) bits |= (c < n_tile && (int)cur.c[c] > v.cc.thr) ? 1u << c : 0u;
        const unsigned hi = (unsigned)__shfl_xor((int)bits, 1, 64);          // every lane takes part
        if (word && (g & 1) == 0)
            v.occ[((size_t)t * v.dim + row) * v.ow + (js >> 5)] = bits | (hi << 16);
    }
}

static unsigned grid_for(long long n) { return (unsigned)std::max(1LL, std::min((n + LB - 1) / LB, 2048LL)); }

void launch_load_validate(const DevView& v, const LoadArgs& a, hipStream_t s) {
    load_validate_kernel<<<grid_for(a.ncell), LB, 0, s>>>(a, v.cc.vmin, v.cc.vmax);
}

void launch_load_map(const DevView& v, const LoadArgs& a, int n_jobs, hipStream_t s) {
    const long long n = a.p_hi - a.p_lo, n_alloc = n * a.n_tiles;
    load_alloc_kernel<<<(unsigned)((n_alloc + LB - 1) / LB), LB, 0, s>>>(v, a);
    // enough workgroups to fill the GPU: the particles split into G chunks along grid.y, each chunk reads the raster once
    const int G = (int)std::max((n + LB - 1) / LB, std::min(n, (8192LL + n_jobs - 1) / n_jobs));   // chunks of <= LB particles
    const dim3 grid(n_jobs, G);
    if (v.dim % 16 == 0) load_cells_kernel<true><<<grid, LB, 0, s>>>(v, a);
    else load_cells_kernel<false><<<grid, LB, 0, s>>>(v, a);
}

}  // namespace rbpf
