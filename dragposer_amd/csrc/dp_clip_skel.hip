// dp_clip_skel.hip -- dp_optimize_clip_lm_skeleton (include/dragposer_clip_skeleton.h): the rows kernel of the joint clip solve with the bones
// of each sequence's own skeleton.  The frame's pass is dp_clip_rows_body.h's, statement for statement, in all four modes.  Frame f of a
// launch belongs to sequence f % S, so the four waves of a workgroup hold frames of different sequences: each wave takes its sequence's
// [22][3] offsets from global memory into a block of its own beside dp_lm.h's array (dp_lm_skel.h), with the frame's other input loads, and
// the lane's own bone and the tangents (which read another joint's bone) read that block.  A row out of range refuses the frame like a bad
// z0 -- every frame of the sequence, so no step runs for it.  The chains and the decisions are dp_clip.hip's and dp_clip_accel.hip's kernels.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_clip_lm.h"
#include "dp_clip_skel.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"

namespace K = dpclip;
static_assert(K::LAT == LAT && K::WPB == WPB, "dp_lm.h's frame");

#define DP_CLIP_SKEL 1
__global__ __launch_bounds__(WPB * 64) void dp_clip_rows_skel_kernel(K::SkelArgs a)
#include "dp_clip_rows_body.h"
#undef DP_CLIP_SKEL

hipError_t dp_launch_clip_rows_skel(const K::Args* args, int mode, const void* own, hipStream_t stream)
{
    K::SkelArgs k;
    static_cast<K::Args&>(k) = *args;
    k.mode = mode;
    k.skel = static_cast<const K::SkelOwn*>(own)->skel;
    k.skel_stride = static_cast<const K::SkelOwn*>(own)->skel_stride;
    hipLaunchKernelGGL(dp_clip_rows_skel_kernel, dim3((unsigned)((k.n_frames + WPB - 1) / WPB)), dim3(WPB * 64), 0, stream, k);
    return hipGetLastError();
}
