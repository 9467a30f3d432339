// dp_clip_skel.h -- argument block of dp_clip_skel.hip: the clip solve's rows kernel with the bones of each sequence's own skeleton
// (include/dragposer_clip_skeleton.h), shared with the host side (dp_host.cpp).  dp_clip.h's struct stays as it is; the LDS layout is
// dp_lm_skel.h's.  The chain and decision kernels never see a bone and are launched as they are: the launch trains of dp_clip.hip and
// dp_clip_accel.hip take the rows launcher as a parameter (dpclip::Rows), and this unit supplies one.
#pragma once
#include "dp_clip.h"
#include "dp_lm_skel.h"

namespace dpclip {

struct SkelArgs : Args {
    const float* skel; // [N][22][3]: a frame of sequence s reads skel + s * skel_stride (rows 1..21)
    int skel_stride;   // 66 (one skeleton per sequence) or 0 (one for the launch)
};

struct SkelOwn { // what the rows launcher adds to the train's argument block
    const float* skel;
    int skel_stride;
};

} // namespace dpclip

// a dpclip::Rows launcher: own is a dpclip::SkelOwn
hipError_t dp_launch_clip_rows_skel(const dpclip::Args* args, int mode, const void* own, hipStream_t stream);
