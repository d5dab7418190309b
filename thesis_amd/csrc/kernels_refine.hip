// kernels_refine.hip -- sub-cell scan-to-map search round given poses: N scans with N guessed poses scored at every candidate
// (i, j, k) of a window of translations and rotations in one particle's map (include/rbpf_hip.h, rbpf_refine_poses; the
// specification is DESIGN 3.17).
//
// The score of a candidate is the integer sum of F = occ + dil in {0, 1, 2} at the beams' end cells.  The end cell of beam b at
// rotation k and translation (i, j) is ((PX[k][b] + i) >> s, (PY[k][b] + j) >> s): the float64 transform is shared by all
// translations of a rotation, the rest is integer.
//   locate_field_kernel    (shared, launch_locate_field) the union of the scans' windows, cut to the lattice, as dense rows of
//                          {occ, dil} word pairs.
//   refine_search_kernel   one workgroup per (scan, run of kpw rotations).  It stages the scan's (2 Mw + 1)^2 window of the field
//                          in LDS (rows of WW word pairs, WW odd: neighbouring rows start on different banks), then takes the
//                          beams in chunks: a transform pass writes (PX, PY) of the chunk for the run's rotations into an LDS
//                          table (the only float64 work, explicit single operations), and the main loop reads it back.  A lane
//                          owns one task (rotation, i, run of RJ = 8 values of j that are S apart: j0 + S t): their columns
//                          (PY + j0 + S t) >> s are the eight neighbours from (PY + j0) >> s on, whatever PY is.  Per beam the
//                          lane reads the two word pairs of row (PX + i) >> s that hold them, funnel-shifts them onto bit 0 and
//                          adds bit t of occ and of dil into the t-th of eight register accumulators.  Lanes of one i share
//                          the row, lanes of one rotation the table entry (LDS broadcasts).  At the end a lane writes its eight
//                          scores into the volume, if asked for, and merges its best with a 64-bit max on
//                          score << 41 | complement of the tie key (|k|, i^2 + j^2, k, i, j), first in LDS, then one global
//                          atomic per workgroup.  The guess's own score and n_used are written by the lanes that hold them.
//   refine_final_kernel    packed -> out_n6 and out_pose_n3.
// All stores are vector stores; the only atomics are integer.
#include "rbpf_refine_search.h"

namespace rbpf {

static const int RB = REFINE_BLOCK;

// the body is rbpf_refine_search.h's, shared with the pair search (kernels_pairs.hip): the window comes from the shared field
__global__ __launch_bounds__(RB) void refine_search_kernel(RefineArgs a) { refine_search_body<false>(a, nullptr, nullptr); }

__global__ __launch_bounds__(256) void refine_final_kernel(RefineArgs a) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    int i, j, k;
    const int score = refine_unkey(a.packed[n], a.R, a.Wt, i, j, k);
    if (a.out_n6) {
        int32_t* o = a.out_n6 + 6 * (size_t)n;
        o[0] = i; o[1] = j; o[2] = k; o[3] = score; o[4] = a.guess_score[n]; o[5] = a.n_used[n];
    }
    if (a.out_pose) {
        const double2 g = reinterpret_cast<const double2*>(a.guess)[n];
        double* o = a.out_pose + 3 * (size_t)n;
        o[0] = __dadd_rn(g.x, __ddiv_rn((double)i, a.invS));
        o[1] = __dadd_rn(g.y, __ddiv_rn((double)j, a.invS));
        o[2] = a.rot[((size_t)n * a.nk + (k + a.R)) * 4 + 2];             // theta_k, formed on the host
    }
}

size_t refine_lds_bytes(int Mw, int WW) { return (size_t)REFINE_TABLE * 8 + (size_t)(2 * Mw + 1) * WW * 8; }

void launch_refine_poses(const DevView& v, const LocateArgs& f, const RefineArgs& a, hipStream_t s) {
    if (f.rows > 0) launch_locate_field(v, f, s);
    const size_t lds = refine_lds_bytes(a.Mw, a.WW);
    static size_t lds_set[MAX_DEVICES] = {};   // more than the default 64 KiB of dynamic LDS
    ensure_dynamic_lds(reinterpret_cast<const void*>(refine_search_kernel), lds, lds_set);
    refine_search_kernel<<<dim3((unsigned)a.N, (unsigned)((a.nk + a.kpw - 1) / a.kpw)), RB, lds, s>>>(a);
    refine_final_kernel<<<(unsigned)((a.N + 255) / 256), 256, 0, s>>>(a);
}

}  // namespace rbpf
