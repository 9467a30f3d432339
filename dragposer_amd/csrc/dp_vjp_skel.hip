// dp_vjp_skel.hip -- dp_forward_vjp_skeleton (include/dragposer_grad.h): dp_forward_vjp with the bone offsets of each frame's own skeleton
// (include/dragposer_skeleton.h) and, on request, their gradient.  The kernel is dp_vjp_impl.h's text with DP_VJP_SKEL 1: the frame's
// bones are loaded and screened in the prologue into an LDS column beside F, and read from there instead of the image; everything else,
// arithmetic and order included, is dp_vjp_kernel's.
#define DP_VJP_SKEL 1
#include "dp_vjp_impl.h"

hipError_t dp_launch_vjp_skel(const SkelArgs* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + FPB - 1) / FPB);
    hipLaunchKernelGGL(dp_vjp_skel_kernel, dim3(grid), dim3(FPB), 0, stream, args->img, *args);
    return hipGetLastError();
}
