// kernels_local.hip -- the local map (include/rbpf_hip.h, rbpf_local_map): a window of n x n cells in the robot's
// frame, cut out of the map of every pose's particle and fused over the poses.
//   local_crop_kernel     one workgroup per pose.  The square of half-side `reach` round the pose's cell is staged into LDS as
//                         bytes, 16 at a time (a strip of a tile row, as kernels_render.hip reads them: nothing is loaded where
//                         a strip misses its tile's written box, has no tile or lies off the lattice).  Then every lane takes
//                         output cells, places its S x S samples with the six float64 operations of rbpf_check_rollouts, reads
//                         the window and keeps the largest value.  The sample tables stand in LDS behind the window where both
//                         fit (TAB), else a lane reads its 2 S entries from memory once per output cell.
//   local_fuse_kernel     lanes over output cells, 16 to a lane, a group of LOCAL_GROUP poses to a workgroup row: the four
//                         integer sums of the group, stored as the group's partial sums.
//   local_reduce_kernel   adds the groups' partial sums, in group order, into `fused`.
// All sums are integers: the result does not depend on groups or batches.
#include "rbpf_internal.h"

#include <algorithm>

namespace rbpf {

static const int LB = 256;            // 4 waves

union Cells16 { uint4 u; int8_t c[16]; };

// the 16 cells (X, Ys .. Ys + 15) of a particle's map, X and Ys counted from the lattice's first cell, Ys a multiple of 16: zero off
// the lattice, without a tile and where the strip misses the tile's written box.  dim % 16 == 0 (rbpf_create): the strip lies in
// one tile, whole and 16-byte aligned
__device__ __forceinline__ uint4 local_strip(const DevView& v, const int32_t* __restrict__ tab, int X, int Ys) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const int dim = v.dim, edge = v.L * dim;
    if (X < 0 || X >= edge || Ys < 0 || Ys >= edge) return zero;
    const int a = X / dim, i = X - a * dim, b = Ys / dim, j = Ys - b * dim;
    const int t = tab[a * v.L + b];
    if (t < 0) return zero;
    const int* bb = v.tile_bbox + 4 * (size_t)t;
    if (i < bb[0] || i > bb[1] || j > bb[3] || j + 15 < bb[2]) return zero;
    return *reinterpret_cast<const uint4*>(v.pool + (size_t)t * dim * dim + (size_t)i * dim + j);
}

template <bool TAB>
__global__ __launch_bounds__(LB) void local_crop_kernel(DevView v, LocalArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, k = blockIdx.x, pose = a.p0 + k;
    const double2 ps = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)pose], cs = reinterpret_cast<const double2*>(a.pose4)[2 * (size_t)pose + 1];
    const int p = a.particle >= 0 ? a.particle : pose;
    const int32_t* __restrict__ tab = v.tile_tab + (size_t)v.slot[p] * v.L * v.L;
    // the window: rows X0 .. X0 + side - 1, columns from Y0a, all counted from the lattice's first cell.  |x inv| < 2^30 (the host
    // checked) and reach < 192 keep everything inside 32 bits
    const int X0 = (int)__builtin_floor(__dmul_rn(ps.x, a.inv)) + a.off - a.reach;
    const int Y0a = ((int)__builtin_floor(__dmul_rn(ps.y, a.inv)) + a.off - a.reach) & ~15;
    const int rb = a.row_bytes, nstrip = rb >> 4;
    for (int t = tid; t < a.side * nstrip; t += LB) {
        const int r = t / nstrip, q = t - r * nstrip;
        *reinterpret_cast<uint4*>(smem + (size_t)r * rb + 16 * q) = local_strip(v, tab, X0 + r, Y0a + 16 * q);
    }
    const double* gx = a.gx; const double* gy = a.gy;
    if (TAB) {
        double* s_g = reinterpret_cast<double*>(smem + (size_t)a.side * rb);     // side * rb is a multiple of 16
        for (int q = tid; q < a.nq; q += LB) { s_g[q] = a.gx[q]; s_g[a.nq + q] = a.gy[q]; }
        gx = s_g; gy = s_g + a.nq;
    }
    __syncthreads();
    const int n = a.n, S = a.S, ncell = n * n;
    const int offx = a.off - X0, offy = a.off - Y0a;
    int8_t* __restrict__ out = a.crops + (size_t)k * a.cstride;
    for (int cell = tid; cell < ncell; cell += LB) {
        const int i = cell / n, j = cell - i * n;
        int m = -128;
        for (int qa = 0; qa < S; ++qa) {
            const double lx = gx[i * S + qa];
            const double cx = __dmul_rn(cs.x, lx), sx = __dmul_rn(cs.y, lx);
            for (int qb = 0; qb < S; ++qb) {
                const double ly = gy[j * S + qb];
                const double wx = __dadd_rn(ps.x, __dsub_rn(cx, __dmul_rn(cs.y, ly)));
                const double wy = __dadd_rn(ps.y, __dadd_rn(sx, __dmul_rn(cs.x, ly)));
                const int r = (int)__builtin_floor(__dmul_rn(wx, a.inv)) + offx;
                const int c = (int)__builtin_floor(__dmul_rn(wy, a.inv)) + offy;
                // inside the window by the bound on reach (rbpf_localbatch.h); the test keeps a wrong bound from reading past it
                const int val = (unsigned)r < (unsigned)a.side && (unsigned)c < (unsigned)rb ? (int)reinterpret_cast<const int8_t*>(smem)[r * rb + c] : 0;
                m = max(m, val);
            }
        }
        out[cell] = (int8_t)m;
    }
}

// Group g = blockIdx.y of the batch: poses g * LOCAL_GROUP .. of it.  The pose index is the workgroup's, so wq comes through scalar loads.
template <bool WIDE>
__global__ __launch_bounds__(LB) void local_fuse_kernel(LocalArgs a, int thr) {
    const size_t c0 = ((size_t)blockIdx.x * LB + threadIdx.x) * 16;
    if (c0 >= a.ncellp) return;
    const int g = blockIdx.y, k0 = g * LOCAL_GROUP_POSES, k1 = min(a.nb, k0 + LOCAL_GROUP_POSES);
    const size_t ncell = (size_t)a.n * a.n;
    uint32_t occ[16], fre[16], unk[16];
    long long sv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { occ[c] = 0u; fre[c] = 0u; unk[c] = 0u; sv[c] = 0; }
#pragma unroll 4
    for (int k = k0; k < k1; ++k) {
        const uint32_t w = a.wq[a.p0 + k];
        const int8_t* __restrict__ src = a.crops + (size_t)k * a.cstride + c0;
        Cells16 d;
        if (WIDE) d.u = *reinterpret_cast<const uint4*>(src);
        else {
#pragma unroll
            for (int c = 0; c < 16; ++c) d.c[c] = c0 + c < ncell ? src[c] : (int8_t)0;
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int m = d.c[c];
            occ[c] += m > thr ? w : 0u;
            fre[c] += m < 0 ? w : 0u;
            unk[c] += m == 0 ? w : 0u;
            sv[c] += (long long)w * (long long)m;
        }
    }
    uint32_t* pw = a.part_w + (size_t)g * 3 * a.ncellp + c0;
    long long* pv = a.part_v + (size_t)g * a.ncellp + c0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        reinterpret_cast<uint4*>(pw)[q] = make_uint4(occ[4 * q], occ[4 * q + 1], occ[4 * q + 2], occ[4 * q + 3]);
        reinterpret_cast<uint4*>(pw + a.ncellp)[q] = make_uint4(fre[4 * q], fre[4 * q + 1], fre[4 * q + 2], fre[4 * q + 3]);
        reinterpret_cast<uint4*>(pw + 2 * a.ncellp)[q] = make_uint4(unk[4 * q], unk[4 * q + 1], unk[4 * q + 2], unk[4 * q + 3]);
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) pv[c] = sv[c];
}

__global__ __launch_bounds__(LB) void local_reduce_kernel(LocalArgs a) {
    const size_t ncell = (size_t)a.n * a.n;
    for (size_t c = (size_t)blockIdx.x * LB + threadIdx.x; c < ncell; c += (size_t)gridDim.x * LB) {
        long long o = 0, f = 0, u = 0, s = 0;
        for (int g = 0; g < a.ngroups; ++g) {
            const uint32_t* pw = a.part_w + (size_t)g * 3 * a.ncellp + c;
            o += pw[0]; f += pw[a.ncellp]; u += pw[2 * a.ncellp];
            s += a.part_v[(size_t)g * a.ncellp + c];
        }
        long long* dst = a.fused + 4 * c;                                  // the batches before this one have added theirs
        dst[0] += o; dst[1] += f; dst[2] += u; dst[3] += s;
    }
}

size_t local_lds_bytes(const LocalArgs& a) { return (size_t)a.side * a.row_bytes + (a.tab_lds ? (size_t)a.nq * 16 : 0); }

void launch_local_crop(const DevView& v, const LocalArgs& a, hipStream_t s) {
    const size_t lds = local_lds_bytes(a);
    static size_t lds_set[2][MAX_DEVICES] = {};   // more than the default 64 KiB of dynamic LDS
    if (a.tab_lds) {
        ensure_dynamic_lds(reinterpret_cast<const void*>(local_crop_kernel<true>), lds, lds_set[0]);
        local_crop_kernel<true><<<(unsigned)a.nb, LB, lds, s>>>(v, a);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(local_crop_kernel<false>), lds, lds_set[1]);
        local_crop_kernel<false><<<(unsigned)a.nb, LB, lds, s>>>(v, a);
    }
}

void launch_local_fuse(const DevView& v, const LocalArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.ncellp / 16 + LB - 1) / LB), (unsigned)a.ngroups);
    if (a.wide) local_fuse_kernel<true><<<grid, LB, 0, s>>>(a, v.cc.thr);
    else local_fuse_kernel<false><<<grid, LB, 0, s>>>(a, v.cc.thr);
    const size_t ncell = (size_t)a.n * a.n;
    local_reduce_kernel<<<(unsigned)std::max<size_t>(1, std::min<size_t>((ncell + LB - 1) / LB, 2048)), LB, 0, s>>>(a);
}

}  // namespace rbpf
