// rbpf_tilewrite.h -- the kernel that writes a box of mosaic cells into the tiles of one particle or of every particle, shared
// by map loading (kernels_load.hip: the cells come from a raster) and map placement (kernels_place.hip: the cells are a source
// map resampled on the fly and merged with the old ones).  One lane layout, one store path and one occupancy-word rule.
//
// The box is cut on the host at lattice tile seams into jobs (RenderJob) of up to 16 storage rows x 256 storage columns of
// ONE lattice position, with column blocks starting at multiples of 32: lanes 2k and 2k+1 then hold the two halves of one
// occupancy word, and no word or 16-cell group is shared by two jobs.  Lane l owns row i0 + (l >> 4) and the 16 cells
// j0 + 16 (l & 15) .. + 15.  It fetches its new cells once per workgroup (Src::fetch) and keeps them in registers while it
// walks the workgroup's chunk of particles (grid.y, at most 256, their tile ids staged in LDS first).  Per particle it merges
// them with the tile's current cells (Src::merge), writes the group with one 16-byte store (dim % 16 == 0: the pool rows are
// 16-byte aligned) and forms its 16 occupancy bits; the pair joins them with one cross-lane exchange and the even lane stores
// the word.  Lanes outside the box whose word touches it still read their cells for the word's bits.
//
// Src (passed by value) supplies
//   unsigned fetch(a, j, r, g, c_lo, c_hi, in)   the lane's new cells into `in`; returns the mask of the cells of [c_lo, c_hi)
//                                                that the call changes (called by lanes with a cell in the box only)
//   bool keeps_old(m)                            false iff merge() ignores the tile's current cells under mask m
//   void merge(cur, in, m, vmin, vmax)           the new value of every cell of mask m into `cur`
#pragma once
#include "rbpf_internal.h"

#include <algorithm>

namespace rbpf {

static const int TW_LB = 256;         // 4 waves: 16 rows x 16 groups of 16 cells

union Cells16 { uint4 u; int8_t c[16]; };

template <bool WIDE, class Src>
__global__ __launch_bounds__(TW_LB) void tile_write_kernel(DevView v, LoadArgs a, Src src) {
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
    if (mine) inmask = src.fetch(a, j, r, g, c_lo, c_hi, in);
    const bool old = src.keeps_old(inmask);
    const int* bbox = v.tile_bbox;
    const int n = a.p_hi - a.p_lo;
    const int q_lo = a.p_lo + (int)((long long)blockIdx.y * n / gridDim.y);
    const int q_hi = a.p_lo + (int)((long long)(blockIdx.y + 1) * n / gridDim.y);   // at most TW_LB particles
    // the chunk's tile ids up front: the stores below then follow one another without a dependent load in between
    __shared__ int s_tile[TW_LB];
    if (q_lo + tid < q_hi) s_tile[tid] = v.tile_tab[(size_t)v.slot[q_lo + tid] * v.L * v.L + j.pos];
    __syncthreads();
    for (int p = q_lo; p < q_hi; ++p) {
        const int t = s_tile[p - q_lo];
        if (t < 0) continue;                            // only after a failed allocation (RBPF_ENOMEM is set)
        int8_t* tile = v.pool + (size_t)t * v.dim * v.dim + (size_t)row * v.dim;
        Cells16 cur;
        cur.u = make_uint4(0u, 0u, 0u, 0u);
        if (word && old) {                              // outside the written box a tile holds 0
            const int* bb = bbox + 4 * (size_t)t;
            if (row >= bb[0] && row <= bb[1] && js <= bb[3] && js + 15 >= bb[2]) {
                if (WIDE) cur.u = *reinterpret_cast<const uint4*>(tile + js);
                else {
#pragma unroll
                    for (int c = 0; c < 16; ++c) if (c < n_tile) cur.c[c] = tile[js + c];
                }
            }
        }
        src.merge(cur, in, inmask, v.cc.vmin, v.cc.vmax);
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

// enough workgroups to fill the GPU: the particles split into G chunks along grid.y, each chunk fetches its cells once
template <class Src>
void launch_tile_write(const DevView& v, const LoadArgs& a, int n_jobs, const Src& src, hipStream_t s) {
    const long long n = a.p_hi - a.p_lo;
    const int G = (int)std::max((n + TW_LB - 1) / TW_LB, std::min(n, (8192LL + n_jobs - 1) / n_jobs));   // chunks of <= TW_LB particles
    const dim3 grid(n_jobs, G);
    if (v.dim % 16 == 0) tile_write_kernel<true, Src><<<grid, TW_LB, 0, s>>>(v, a, src);
    else tile_write_kernel<false, Src><<<grid, TW_LB, 0, s>>>(v, a, src);
}

}  // namespace rbpf
