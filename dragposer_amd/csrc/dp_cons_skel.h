// dp_cons_skel.h -- argument blocks and LDS layout of dp_cons_skel.hip: dp_cons.hip's two kernels with the bones of each frame's own skeleton
// (include/dragposer_skeleton.h), shared with the host side (dp_host.cpp).  dp_cons.h's structs and constants stay as they are: the plain
// kernels' code does not change with this unit.
#pragma once
#include "dp_cons.h"

namespace dpcons {

// the wave's block grows by one area: the frame's skeleton [22][3] (row 0 zero, never read), appended after the plain block (after the per-frame
// rows in the table instantiation) and padded to the block's 16-byte alignment.  L_OFF keeps its place and is neither staged nor read.
constexpr int W_SKEL_PAD = (66 + 3) & ~3;                      // 68 floats per wave
constexpr int W_SKEL = W_FLOATS, W_SKEL_T = W_FLOATS_T;         // where the area starts in the wave's block
constexpr int SK_W_FLOATS = W_FLOATS + W_SKEL_PAD, SK_W_FLOATS_T = W_FLOATS_T + W_SKEL_PAD;
constexpr int SK_LDS_FLOATS = L_WAVE0 + WPB * SK_W_FLOATS, SK_LDS_FLOATS_T = L_WAVE0_T + WPB * SK_W_FLOATS_T;
constexpr int SK_LDS_BYTES = 4 * SK_LDS_FLOATS, SK_LDS_BYTES_T = 4 * SK_LDS_FLOATS_T;
static_assert(SK_LDS_BYTES == LDS_BYTES + WPB * 4 * W_SKEL_PAD && SK_LDS_BYTES == 73008, "the LDS budget stated in DESIGN.md section 13b");
static_assert(SK_LDS_BYTES_T == LDS_BYTES_T + WPB * 4 * W_SKEL_PAD && SK_LDS_BYTES_T == 76464 && SK_LDS_BYTES_T <= 160 * 1024,
              "the LDS budget stated in DESIGN.md section 13b");
static_assert(SK_W_FLOATS % 4 == 0 && SK_W_FLOATS_T % 4 == 0, "every wave's block stays 16-byte aligned");

struct SkelArgs : Args {
    const float* skel; // [N][22][3]: frame f reads skel + f * skel_stride (rows 1..21)
    int skel_stride;   // 66 (one skeleton per frame) or 0 (one for the launch)
};
struct TermSkelArgs : TermArgs {
    const float* skel;
    int skel_stride;
};

} // namespace dpcons

hipError_t dp_launch_cons_skel(const dpcons::SkelArgs* args, hipStream_t stream);
hipError_t dp_launch_terms_skel(const dpcons::TermSkelArgs* args, hipStream_t stream);
