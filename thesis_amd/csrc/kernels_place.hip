// kernels_place.hip -- map placement (include/rbpf_hip.h, rbpf_place_map): a source raster with its own cell
// size and its own pose in the world is resampled onto the mosaic cells of a box, and written or fused into the tiles of one
// particle or of every particle.
//
// The resampling rule is float64 with every operation rounded on its own, spelled with the __d*_rn intrinsics so that the
// order written in the header is the order executed (tests/place_oracle.py restates it in NumPy, bit for bit).  Sample (a, b)
// of mosaic cell (X, Y) lies at ((X + fa) cs, (Y + fb) cs); c dx and s dx depend on (X, a) only and c dy, s dy on (Y, b)
// only, so a lane forms the first pair once per a and walks its cells inside.
//
// place_warp_kernel writes the warped / covered rasters of a box, one thread per cell (the dry run, and the rasters a real
// placement was asked to return).  The placement itself is tile_write_kernel (rbpf_tilewrite.h) with PlaceSrc as its source:
// a lane resamples its 16 cells once per workgroup, keeps them and their covered mask in registers, and merges them with each
// particle's old cells under the mode.  No intermediate raster goes through memory.  The source cells are gathered from
// global memory: a job's footprint is a rotated, scaled patch of 16 x 256 cells that the caches serve.
#include "rbpf_tilewrite.h"

namespace rbpf {

// (a + 0.5) / S
__device__ __forceinline__ double place_frac(int a, int S) { return __ddiv_rn(__dadd_rn((double)a, 0.5), (double)S); }

// c dx and s dx of the sample column a of mosaic row X
__device__ __forceinline__ void place_x(const PlaceArgs& q, int X, double fa, double& cdx, double& sdx) {
    const double dx = __dsub_rn(__dmul_rn(__dadd_rn((double)X, fa), q.cs), q.ox);
    cdx = __dmul_rn(q.c, dx); sdx = __dmul_rn(q.s, dx);
}

// the source cell under the sample (cdx, sdx) x (Y, fb): true and its value when the sample lies inside the source
__device__ __forceinline__ bool place_sample(const PlaceArgs& q, double cdx, double sdx, int Y, double fb, int& val) {
    const double dy = __dsub_rn(__dmul_rn(__dadd_rn((double)Y, fb), q.cs), q.oy);
    const double u = __ddiv_rn(__dadd_rn(cdx, __dmul_rn(q.s, dy)), q.src_cell);
    const double w = __ddiv_rn(__dsub_rn(__dmul_rn(q.c, dy), sdx), q.src_cell);
    // 0 <= floor(u) < nsx iff 0 <= u < nsx (NaN and infinities fail); the conversion truncates, which is floor from 0 up
    if (!(u >= 0.0 && u < (double)q.nsx && w >= 0.0 && w < (double)q.nsy)) return false;
    val = q.src[(size_t)(int)u * q.nsy + (int)w];
    return true;
}

// ---- the warped / covered rasters of the box ------------------------------------------------------------------------------
__global__ __launch_bounds__(TW_LB) void place_warp_kernel(PlaceArgs q) {
    if (*q.bad) return;
    const long long k = (long long)blockIdx.x * TW_LB + threadIdx.x;
    if (k >= q.ncell) return;
    const long long ix = k / q.ny;
    const int X = q.x0 + (int)ix, Y = q.y0 + (int)(k - ix * q.ny);
    int best = -128;
    bool cov = false;
    for (int a = 0; a < q.S; ++a) {
        double cdx, sdx;
        place_x(q, X, place_frac(a, q.S), cdx, sdx);
        for (int b = 0; b < q.S; ++b) {
            int val;
            if (place_sample(q, cdx, sdx, Y, place_frac(b, q.S), val)) { cov = true; best = max(best, val); }
        }
    }
    if (q.warped) q.warped[k] = (int8_t)(cov ? best : 0);
    if (q.covered) q.covered[k] = cov ? 1 : 0;
}

// ---- the placement: the resampled source is the source of tile_write_kernel ------------------------------------------------
struct PlaceSrc {
    PlaceArgs q;
    __device__ unsigned fetch(const LoadArgs&, const RenderJob& j, int r, int g, int c_lo, int c_hi, Cells16& in) const {
        const int X = q.x0 + j.ox + r, Y0 = q.y0 + j.oy + 16 * g;
        int best[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) best[c] = -128;
        unsigned cov = 0u;
        for (int a = 0; a < q.S; ++a) {
            double cdx, sdx;
            place_x(q, X, place_frac(a, q.S), cdx, sdx);
            for (int b = 0; b < q.S; ++b) {
                const double fb = place_frac(b, q.S);
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    int val;
                    if (c >= c_lo && c < c_hi && place_sample(q, cdx, sdx, Y0 + c, fb, val)) { cov |= 1u << c; best[c] = max(best[c], val); }
                }
            }
        }
        unsigned known = 0u;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            in.c[c] = (int8_t)(((cov >> c) & 1u) ? best[c] : 0);
            known |= in.c[c] != 0 ? 1u << c : 0u;
        }
        return q.mode == RBPF_PLACE_KNOWN ? cov & known : cov;
    }
    __device__ bool keeps_old(unsigned m) const { return q.mode == RBPF_PLACE_ADD || m != 0xFFFFu; }
    __device__ void merge(Cells16& cur, const Cells16& in, unsigned m, int vmin, int vmax) const {
        const bool add = q.mode == RBPF_PLACE_ADD;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if ((m >> c) & 1u) cur.c[c] = (int8_t)(add ? min(max((int)cur.c[c] + (int)in.c[c], vmin), vmax) : (int)in.c[c]);
    }
};

void launch_place_warp(const PlaceArgs& q, hipStream_t s) {
    place_warp_kernel<<<(unsigned)((q.ncell + TW_LB - 1) / TW_LB), TW_LB, 0, s>>>(q);
}

void launch_place_map(const DevView& v, const LoadArgs& a, const PlaceArgs& q, int n_jobs, hipStream_t s) {
    launch_load_alloc(v, a, s);
    launch_tile_write(v, a, n_jobs, PlaceSrc{q}, s);
}

}  // namespace rbpf
