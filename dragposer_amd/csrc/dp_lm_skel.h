// dp_lm_skel.h -- argument block and LDS layout of dp_lm_skel.hip: dp_lm.hip's kernel with the bones of each frame's own skeleton
// (include/dragposer_clip_skeleton.h), shared with the host side (dp_host.cpp) and with dp_clip_skel.hip, whose rows kernel has the same
// layout.  dp_lm.h's struct and constants stay as they are: the plain kernels' code does not change with these units.
#pragma once
#include "dp_lm.h"

namespace dplm {

// Beside dp_lm.h's array a second one: a block of bones per wave, [22][3] (row 0 zero, never read) padded to 16 bytes.  The waves of a
// workgroup hold different frames -- in the clip's rows kernel frames of different sequences -- so nothing of it is shared.  L_OFF keeps its
// place in the first array and is neither staged nor read.
constexpr int SK_W = (66 + 3) & ~3; // 68 floats per wave
constexpr int SK_LDS_BYTES = LDS_BYTES + 4 * WPB * SK_W;
static_assert(SK_LDS_BYTES == 122576 && SK_LDS_BYTES <= 160 * 1024, "the LDS budget stated in DESIGN.md section 18b");

struct SkelArgs : Args {
    const float* skel; // [N][22][3]: frame f reads skel + f * skel_stride (rows 1..21)
    int skel_stride;   // 66 (one skeleton per frame) or 0 (one for the launch)
};

} // namespace dplm

hipError_t dp_launch_lm_skel(const dplm::SkelArgs* args, hipStream_t stream);
