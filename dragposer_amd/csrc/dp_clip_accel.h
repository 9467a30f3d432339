// dp_clip_accel.h -- argument block, workspace layout and LDS layout of dp_optimize_clip_lm_accel's kernels (dp_clip_accel.hip), shared with the
// host side (dp_host.cpp).  Reference of what is computed: include/dragposer_clip_accel.h.
//
// dp_clip_rows_kernel          dp_clip.hip's, unchanged (dp_launch_clip_rows): A_t | g_t, the frames' loss numbers, the first-difference parts.
// dp_clip_accel_chain_kernel   one wave per sequence: the block recursion with lower bandwidth 2 over the sequence's frames, forwards and backwards.
// dp_clip_accel_decide_kernel  one wave per sequence: dp_clip_decide_kernel's decision with the second-difference totals, which it reads from the
//                              latent buffers, in its sums.
// A call is dp_clip.h's train() with the two as its chain and decision (dp_launch_clip_accel); what connects the launches is the workspace,
// dp_clip.h's Layout with this unit's factor block.
#pragma once
#include <hip/hip_runtime.h>

#include "dp_clip.h"

namespace dpclipacc {

constexpr int LAT = dpclip::LAT;
constexpr int LI_FLOATS = dpclip::LI_FLOATS;        // a frame's L_t^-1 (rows 0..23) | y_t (row 24) ...
constexpr int LF_FLOATS = LI_FLOATS + LAT * LAT;    // ... | F_t (rows 0..23): what the backward sweep reads back

// chain kernel LDS (floats), one wave per workgroup.  Every matrix has 24 rows of stride CS (odd: a lane per row meets no bank twice).
constexpr int CS = 25;
constexpr int MAT = 24 * CS;
constexpr int C_S = 0;            // S_t, then L_t in place
constexpr int C_P = C_S + MAT;    // [2] P_(t-2) and P_(t-1), by the parity of t (P = L^-T L^-1)
constexpr int C_I = C_P + 2 * MAT; // L_(t-1)^-1, then L_t^-1
constexpr int C_F = C_I + MAT;    // F_t
constexpr int C_Q = C_F + MAT;    // L_(t-2)^-T F_(t-1)^T, formed one frame ahead
constexpr int C_V = C_Q + MAT;    // [6][32] vectors handed from lane to lane: g_t / the right-hand side, 1 / L_kk, y_t, w_t, Delta_(t+1), Delta_(t+2)
constexpr int CHAIN_LDS_FLOATS = C_V + 6 * 32;
constexpr int CHAIN_LDS_BYTES = 4 * CHAIN_LDS_FLOATS;
static_assert(CHAIN_LDS_BYTES == 15168, "the LDS budget stated in DESIGN.md section 18a");

// The workspace is dp_clip.h's Layout: layout(S, B, LF_FLOATS, true), the wider factor block and, last, the kept second-difference total.

struct Args {
    dpclip::Args c;     // dp_clip.h's block; c.wli is [B][LF_FLOATS] here
    float lam_accel;
    double* accel_loss; // [S], nullable
    double* wacc;       // [S]
};

} // namespace dpclipacc

hipError_t dp_launch_clip_accel(const dpclipacc::Args* args, hipStream_t stream);
hipError_t dp_launch_clip_accel_train(const dpclipacc::Args* args, const dpclip::Rows* rows, hipStream_t stream); // ... with `rows` as its rows pass
