// dp_lm_skel.hip -- dp_optimize_lm_skeleton (include/dragposer_clip_skeleton.h): dp_lm.hip's kernel with the bones of each frame's own skeleton.
// The frame is dp_lm_body.h's, statement for statement; what differs is where its bones come from: each wave takes its frame's [22][3] offsets
// from global memory into a block of its own beside dp_lm.h's array (dp_lm_skel.h), with the frame's other input loads, and the lane's own
// bone, the tangents (which read another joint's bone) and the reported loss's pass in double all read that block.  A row out of range
// refuses the frame like a bad z0.  Nothing else changes: one launch, no atomics, two launches give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "dp_lm_skel.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"

#define DP_LM_SEQ 0
#define DP_LM_SKEL 1
__global__ __launch_bounds__(WPB * 64) void dp_lm_skel_kernel(SkelArgs a)
#include "dp_lm_body.h"
#undef DP_LM_SKEL
#undef DP_LM_SEQ

hipError_t dp_launch_lm_skel(const SkelArgs* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(dp_lm_skel_kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}
