// rbpf_blockrelax.h -- the block-relaxation round that rbpf_travel_cost and rbpf_frontier_regions share.
//
// An int32 raster per particle, [64 nbx + 2][cw = 64 nby + 2] with a one-cell rim, is driven to the least fixed point of a
// per-cell rule "c = min(c, f(the 8 neighbours))" that only ever lowers a value.  The raster is cut into 64 x 64 blocks; one
// 256-lane workgroup works on one (particle, block), and a lane owns 16 neighbouring cells of one row.
//
// One round (block_relax_round, one kernel launch).  A block runs if it or one of its 8 neighbours changed in the previous
// round (two sets of dirty bytes, read and written by the round's parity); any other workgroup clears its byte and leaves after
// reading nine.  A running block loads its cells with a one-cell halo (66 x 66, row stride 67) into LDS and sweeps to its local
// fixed point.  In a sweep a lane reads the three rows round its 16 cells (3 x 18 words), applies the rule to its active cells
// left to right and back (so a value crosses the lane's cells in one sweep) and writes its cells back if any fell; the workgroup
// votes on "anything changed" with __syncthreads_or.  Lanes read their neighbours' cells while those write them: either value is
// an upper bound, and a sweep in which nothing was written saw the final state.  The sweeps of one run are capped; a block that
// hits the cap has changed, so it is dirty and goes on in the next round.  A block that changed writes its active cells back,
// sets its dirty byte and adds 1 to count[0]; every block that ran adds 1 to count[32].
//
// Why this is right without any wait between workgroups.  Values only fall and never pass below the fixed point.  A block that
// reads a neighbour's edge while that neighbour writes it gets the old or the new value; both are upper bounds, and the
// neighbour is dirty, so the block runs again in the next round.  A round in which no block changed saw the final state
// everywhere.  There is no grid-wide barrier, no cooperative launch and no workgroup that waits on another's memory: a round
// is a kernel, and every wait is a kernel boundary.  The host queues rounds until one changed no block (relax_rounds in rbpf_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rbpf {

static const int BR_LANES = 256;       // lanes of a workgroup: 64 rows x 4 lanes of 16 cells
static const int BR_EDGE = 64;         // block edge
static const int BR_WIN = 66;          // block with its halo
static const int BR_STRIDE = 67;       // LDS row stride of the window: odd, so the rows of a wave's lanes fall into different banks
static const int BR_SWEEP_CAP = 4096;  // sweeps of one block run

// what a round needs of TravelArgs / FrontierArgs
struct BlockRelaxArgs {
    int n_part;                        // particles of this launch (gridDim.y)
    int nbx, nby;                      // blocks per axis: ceil(nx / 64), ceil(ny / 64); block k = bx * nby + by is blockIdx.x
    int32_t* ras; long long ras_stride; int cw;   // [n_part][nbx * 64 + 2][cw = nby * 64 + 2]: cell (i, j) at [i + 1][j + 1]
    uint8_t* dirty;                    // [2][n_part][nbx * nby]: block changed in the previous / in this round
};

static inline unsigned br_blocks(long long n) { return (unsigned)((n + BR_LANES - 1) / BR_LANES); }   // workgroups of BR_LANES lanes for n items
static inline dim3 block_relax_grid(const BlockRelaxArgs& g) { return dim3((unsigned)(g.nbx * g.nby), (unsigned)g.n_part); }

// One round of one (particle, block): the whole of a __global__ function launched on block_relax_grid with BR_LANES lanes.
// Bit k of a lane's mask says that cell k of its 16 is active; any other cell is never written and keeps its preset value.  A Rule has
//   static const bool MASK_FROM_WINDOW
//   uint32_t mask(pi, bx, by, i, seg, g) const   if false: the mask from global memory, read before the barrier beside the window's loads
//   uint32_t mask(sc) const                      if true: the mask from the lane's own row of the loaded window, sc[k + 1] cell k
//   static void cell(k, m, u, c, d, changed)     cell k, if bit k of m is set, from the rows above (u), of (c) and below (d) it: index k + 1
//                                                is the cell, k and k + 2 its row neighbours; lowers c[k + 1] and sets changed, or leaves both
template <class Rule>
__device__ __forceinline__ void block_relax_round(const BlockRelaxArgs& g, const Rule& rule, int parity, int32_t* count) {
    __shared__ int32_t s_c[BR_WIN * BR_STRIDE];
    const int tid = threadIdx.x, pi = blockIdx.y, nblk = g.nbx * g.nby;
    const int bx = blockIdx.x / g.nby, by = blockIdx.x - bx * g.nby;
    const uint8_t* __restrict__ din = g.dirty + ((size_t)parity * g.n_part + pi) * nblk;
    uint8_t* __restrict__ dout = g.dirty + ((size_t)(parity ^ 1) * g.n_part + pi) * nblk;
    int run = 0;
    for (int ex = max(bx - 1, 0); ex <= min(bx + 1, g.nbx - 1); ++ex)
        for (int ey = max(by - 1, 0); ey <= min(by + 1, g.nby - 1); ++ey) run |= din[ex * g.nby + ey];
    if (!run) {                                            // (uniform over the workgroup)
        if (tid == 0) dout[blockIdx.x] = 0;
        return;
    }
    int32_t* __restrict__ base = g.ras + (size_t)pi * g.ras_stride + (size_t)(BR_EDGE * bx) * g.cw + BR_EDGE * by;   // window cell [0][0]: the halo's corner
    for (int k = tid; k < BR_WIN * BR_WIN; k += BR_LANES) {
        const int r = k / BR_WIN, q = k - BR_WIN * r;
        s_c[r * BR_STRIDE + q] = base[(size_t)r * g.cw + q];
    }
    const int i = tid >> 2, seg = tid & 3;
    const int32_t* su = s_c + i * BR_STRIDE + 16 * seg;    // the row above the lane's, from the column left of its first cell
    int32_t* sc = s_c + (i + 1) * BR_STRIDE + 16 * seg;
    const int32_t* sd = s_c + (i + 2) * BR_STRIDE + 16 * seg;
    uint32_t m = 0u;
    if constexpr (!Rule::MASK_FROM_WINDOW) m = rule.mask(pi, bx, by, i, seg, g);
    __syncthreads();
    if constexpr (Rule::MASK_FROM_WINDOW) m = rule.mask(sc);
    int c[18], any = 0;
    for (int sweep = 0; sweep < BR_SWEEP_CAP; ++sweep) {
        int changed = 0;
        if (m) {
            int u[18], d[18];
#pragma unroll
            for (int k = 0; k < 18; ++k) { u[k] = su[k]; c[k] = sc[k]; d[k] = sd[k]; }
#pragma unroll
            for (int k = 0; k < 16; ++k) Rule::cell(k, m, u, c, d, changed);
#pragma unroll
            for (int k = 14; k >= 0; --k) Rule::cell(k, m, u, c, d, changed);
            if (changed) {
#pragma unroll
                for (int k = 0; k < 16; ++k) sc[k + 1] = c[k + 1];   // the lane's own cells: nobody else writes them
            }
        }
        if (!__syncthreads_or(changed)) break;
        any = 1;
    }
    if (any && m) {                                        // c holds the last state of the lane's cells
        int32_t* out = base + (size_t)(i + 1) * g.cw + 16 * seg + 1;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((m >> k) & 1u) out[k] = c[k + 1];
    }
    if (tid == 0) {
        dout[blockIdx.x] = (uint8_t)any;
        atomicAdd(count + 32, 1);                          // block runs of this round (rbpf_travel_stats, rbpf_frontier_stats)
        if (any) atomicAdd(count, 1);
    }
}

}  // namespace rbpf
