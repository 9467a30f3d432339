// dp_cons_hold.h -- argument block and LDS budget of dp_cons_hold.hip: dp_terms_seq_kernel (dp_cons_seq.h) with holds
// (include/dragposer_holds.h), shared with the host side (dp_host.cpp).  dp_cons.h's, dp_cons_skel.h's and dp_cons_seq.h's structs and
// constants stay as they are: the six other kernels' code does not change with this unit.
#pragma once
#include "dp_cons_seq.h"

namespace dpcons {

// LDS: dp_cons_seq.h's table layout, unchanged.  A hold's state (x, y, z, held) of the wave's sequence lives in the held term's row of the
// wave's block (W_ROW + 4 * term), which lane `term` writes every step anyway: read from `state` before the first step, screened and read
// by the terms from there, updated in place by the step's epilogue, written back to `state` after the last step.  Nothing of a hold is kept
// in a register across the iteration loop.
constexpr int HD_LDS_BYTES = SQ_LDS_BYTES_T;
static_assert(HD_LDS_BYTES == 76464 && HD_LDS_BYTES <= 160 * 1024, "the LDS budget stated in DESIGN.md section 13d");

constexpr int MAX_HOLDS = 4; // DP_MAX_HOLDS

// A held term is a point-DISTANCE term, which never reads its staged axis_a words: the host puts the hold's floor level and its two
// thresholds there.
constexpr int T_HLEVEL = T_AXA, T_HLO = T_AXA + 1, T_HHI = T_AXA + 2;
static_assert(T_HHI < T_AXB, "the three words of axis_a");

struct HoldFields {
    float* state;   // [S][n_holds][4] in / out
    float* trace;   // [T][S][n_holds][4] or NULL
    int n_holds;    // 0..MAX_HOLDS
    unsigned terms; // byte h: the term hold h refers to (the hold-to-term map; no two holds share a term)
};
static_assert(MAX_HOLDS * 8 <= 32 && MAX_TERMS <= 256, "a term index per byte of HoldFields::terms");

struct HoldSeqArgs : SeqTermArgs {
    HoldFields h;
};

#ifdef __HIPCC__
// the hold on term t, or -1 (n and map: HoldFields::n_holds and ::terms, wave-uniform; re-derived where it is needed, never kept).  The
// one copy for dp_cons_hold.hip and the four units on top of it; dp_cons_tether.h's map has the same width, so it walks that one too.
__device__ __forceinline__ int hold_of(int n, unsigned map, int t)
{
    int h = -1;
#pragma unroll
    for (int k = 0; k < MAX_HOLDS; ++k) h = k < n && (int)((map >> (8 * k)) & 0xffu) == t ? k : h;
    return h;
}
#endif

} // namespace dpcons

hipError_t dp_launch_terms_hold_seq(const dpcons::HoldSeqArgs* args, hipStream_t stream);
