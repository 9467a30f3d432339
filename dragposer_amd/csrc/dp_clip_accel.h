// dp_clip_accel.h -- argument block, workspace layout and LDS layout of dp_optimize_clip_lm_accel's kernels (dp_clip_accel.hip), shared with the
// host side (dp_host.cpp).  Reference of what is computed: include/dragposer_clip_accel.h.
//
// dp_clip_rows_kernel          dp_clip.hip's, unchanged (dp_launch_clip_rows): A_t | g_t, the frames' loss numbers, the first-difference parts.
// dp_clip_accel_chain_kernel   one wave per sequence: the block recursion with lower bandwidth 2 over the sequence's frames, forwards and backwards.
// dp_clip_accel_decide_kernel  one wave per sequence: dp_clip_decide_kernel's decision with the second-difference totals, which it reads from the
//                              latent buffers, in its sums.
// A call is dp_launch_clip's train with the two in their places (dp_launch_clip_accel); what connects the launches is the workspace.
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

// The workspace (bytes from its start; every part 16-byte aligned).  B = S T.  dp_clip.h's, with the wider factor block and the kept second-difference
// total; the names are dp_clip.h's so that one host routine fills both.
struct Layout {
    size_t z[2];    // float [B][24] the kept latents and the trial's, by W_CUR
    size_t ag;      // float [B][AG_FLOATS]
    size_t li;      // float [B][LF_FLOATS]
    size_t loss[2]; // float [B][4]
    size_t cpl[2];  // double [B] |z_t - z_(t-1)|^2 (0 for t = 0), by W_CUR
    size_t flags;   // int [B]
    size_t tot;     // double [S][2] L_s of the kept Z, its coupling part (both sums)
    size_t word;    // int [S]
    size_t solved;  // int [S]
    size_t mu;      // float [S]
    size_t nacc;    // int [S]
    size_t acc;     // double [S] the second-difference part of L_s of the kept Z
    size_t bytes;
};
inline Layout layout(int S, long long B)
{
    Layout l;
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t o = at; at = dpclip::up16(at + bytes); return o; };
    for (int i = 0; i < 2; ++i) l.z[i] = take((size_t)B * LAT * 4);
    l.ag = take((size_t)B * dpclip::AG_FLOATS * 4);
    l.li = take((size_t)B * LF_FLOATS * 4);
    for (int i = 0; i < 2; ++i) l.loss[i] = take((size_t)B * 16);
    for (int i = 0; i < 2; ++i) l.cpl[i] = take((size_t)B * 8);
    l.flags = take((size_t)B * 4);
    l.tot = take((size_t)S * 16);
    l.word = take((size_t)S * 4);
    l.solved = take((size_t)S * 4);
    l.mu = take((size_t)S * 4);
    l.nacc = take((size_t)S * 4);
    l.acc = take((size_t)S * 8);
    l.bytes = at;
    return l;
}

struct Args {
    dpclip::Args c;     // dp_clip.h's block; c.wli is [B][LF_FLOATS] here
    float lam_accel;
    double* accel_loss; // [S], nullable
    double* wacc;       // [S]
};

} // namespace dpclipacc

hipError_t dp_launch_clip_accel(const dpclipacc::Args* args, hipStream_t stream);
hipError_t dp_launch_clip_accel_train(const dpclipacc::Args* args, const dpclip::Rows* rows, hipStream_t stream); // ... with `rows` as its rows pass
