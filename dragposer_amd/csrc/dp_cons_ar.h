// dp_cons_ar.h -- argument block and LDS budget of dp_cons_ar.hip: dp_terms_hold_seq_kernel (dp_cons_hold.h) with the pull term's target
// formed inside the step loop by a linear autoregressive predictor (include/dragposer_latent_ar.h), shared with the host side (dp_host.cpp).
// dp_cons.h's, dp_cons_skel.h's, dp_cons_seq.h's and dp_cons_hold.h's structs and constants stay as they are: the seven other kernels' code does
// not change with this unit.
#pragma once
#include "dp_cons_hold.h"

namespace dpcons {

constexpr int MAX_AR_ORDER = 4; // DP_MAX_AR_ORDER

// LDS: dp_cons_hold.h's layout, unchanged, and a second array with one area per wave: the sequence's last MAX_AR_ORDER history rows
// [k][24], row 0 = h_1, the newest.  Lane i shifts and writes column i at a step's `stop`; every lane below 24 reads all of it when the next
// step begins, behind the step's closing wave_sync().  Nothing of the predictor is kept in a register across the iteration loop.
constexpr int AR_W_FLOATS = MAX_AR_ORDER * 24;
constexpr int AR_LDS_BYTES = HD_LDS_BYTES + WPB * 4 * AR_W_FLOATS;
static_assert(AR_LDS_BYTES == 79536, "the LDS budget stated in DESIGN.md section 13e");
static_assert(2 * AR_LDS_BYTES <= 160 * 1024, "two workgroups of this kernel fit a CU's LDS");

struct ArFields {
    const float* coeffs;     // [order][24][24], row = output component
    const float* bias;       // [24]
    float* trace;            // [T][S][24] or NULL: the z_tgt row every step used
    const float* latent_buf; // [S][history][24], the state's array: read before the first step, newest row last
    int order, history;      // 1..MAX_AR_ORDER <= history
};

struct ArSeqArgs : HoldSeqArgs {
    ArFields r;
};

} // namespace dpcons

hipError_t dp_launch_terms_ar_seq(const dpcons::ArSeqArgs* args, hipStream_t stream);
