// kernels_load.hip -- map loading (include/rbpf_hip.h, rbpf_load_map): a dense int8 raster written into the tiles of one
// particle or of every particle, the inverse of kernels_render.hip's render_cells_kernel.
//
// The cells are written by tile_write_kernel (rbpf_tilewrite.h: the job cut, the lane layout and the occupancy words); its
// source here is the raster: a lane reads its cells once per workgroup (byte loads: the raster offset is arbitrary) and every
// cell of the box replaces the tile's.
//
// load_alloc_kernel runs first: one thread per (particle, touched lattice position) pops a missing tile from the free stack
// (free tiles are zero-filled, as alloc_missing_tiles in rbpf_mapupdate.h) and widens the tile's written box by (box n tile).
// The host has counted the missing tiles against free_top before, so the pops cannot run dry.  rbpf_place_map uses the same
// kernel (launch_load_alloc).
#include "rbpf_tilewrite.h"

#include <limits.h>

namespace rbpf {

static const int LB = TW_LB;

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

// ---- cells: the raster is the source of tile_write_kernel -------------------------------------------------------------------
struct LoadSrc {
    __device__ unsigned fetch(const LoadArgs& a, const RenderJob& j, int r, int g, int c_lo, int c_hi, Cells16& in) const {
        const int8_t* src = a.cells + (long long)(j.ox + r) * a.ny + (j.oy + 16 * g);
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c >= c_lo && c < c_hi) in.c[c] = src[c];
        return ((1u << c_hi) - 1u) & ~((1u << c_lo) - 1u);
    }
    __device__ bool keeps_old(unsigned m) const { return m != 0xFFFFu; }
    __device__ void merge(Cells16& cur, const Cells16& in, unsigned m, int, int) const {
#pragma unroll
        for (int c = 0; c < 16; ++c) if ((m >> c) & 1u) cur.c[c] = in.c[c];
    }
};

static unsigned grid_for(long long n) { return (unsigned)std::max(1LL, std::min((n + LB - 1) / LB, 2048LL)); }

void launch_load_validate(const DevView& v, const LoadArgs& a, hipStream_t s) {
    load_validate_kernel<<<grid_for(a.ncell), LB, 0, s>>>(a, v.cc.vmin, v.cc.vmax);
}

void launch_load_alloc(const DevView& v, const LoadArgs& a, hipStream_t s) {
    const long long n_alloc = (long long)(a.p_hi - a.p_lo) * a.n_tiles;
    load_alloc_kernel<<<(unsigned)((n_alloc + LB - 1) / LB), LB, 0, s>>>(v, a);
}

void launch_load_map(const DevView& v, const LoadArgs& a, int n_jobs, hipStream_t s) {
    launch_load_alloc(v, a, s);
    launch_tile_write(v, a, n_jobs, LoadSrc(), s);
}

}  // namespace rbpf
