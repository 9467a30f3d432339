// dp_cons_gap.h -- argument blocks and LDS budget of dp_cons_gap.hip: dp_terms_hold_seq_kernel (dp_cons_hold.h) and dp_terms_ar_seq_kernel
// (dp_cons_ar.h) with a tracker set decided per step (include/dragposer_gaps.h), shared with the host side (dp_host.cpp).  The structs and
// constants of dp_cons.h .. dp_cons_ar.h stay as they are: the nine other kernels' code does not change with this unit.
#pragma once
#include "dp_cons_ar.h"

namespace dpcons {

// LDS: dp_cons_hold.h's layout (dp_terms_gap_seq_kernel) and dp_cons_ar.h's (dp_terms_gap_ar_seq_kernel), both unchanged: nothing beyond
// AR_LDS_BYTES.  A joint's gap state is a row of 16 floats in GLOBAL memory (dp_gaps.state), lane j's own: the lane updates it before a
// step's iteration loop and reads the held rotation and the weight factor from it inside the loop, where the other sequence kernels read
// tgt_rot.  Nothing of a gap is kept in a vector register across the iteration loop but the lane's effective position target, which
// dp_cons_seq.h's kernels keep there already.
constexpr int GAP_LDS_BYTES = HD_LDS_BYTES, GAP_AR_LDS_BYTES = AR_LDS_BYTES;
static_assert(GAP_LDS_BYTES <= GAP_AR_LDS_BYTES && 2 * GAP_AR_LDS_BYTES <= 160 * 1024, "two workgroups of either kernel fit a CU's LDS");

// a state row (include/dragposer_gaps.h)
constexpr int GAP_ROW = 16, G_P = 0, G_R = 3, G_VALID = 12, G_AGE = 13, G_FACTOR = 14;
constexpr int GAP_PRESENT = 1, GAP_HELD = 2, GAP_LOST = 3; // a joint's code of a step (0: not tracked by configuration)

struct GapFields {
    float* state;                 // [S][22][16] in / out
    const unsigned char* present; // [T][S][22] or NULL
    unsigned char* trace;         // [T][S][22] or NULL: every joint's code, 0xFF in a step refused as bad state
    float decay, max_hold;        // (max_hold as a float: 0..65535 is exact, and `age` is one)
};

struct GapSeqArgs : HoldSeqArgs {
    GapFields g;
};
struct GapArSeqArgs : ArSeqArgs {
    GapFields g;
};

} // namespace dpcons

hipError_t dp_launch_terms_gap_seq(const dpcons::GapSeqArgs* args, hipStream_t stream);
hipError_t dp_launch_terms_gap_ar_seq(const dpcons::GapArSeqArgs* args, hipStream_t stream);
