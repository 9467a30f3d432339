// dp_vjp.hip -- dp_forward_vjp (include/dragposer_grad.h): the vector-Jacobian product of decode + FK at (z, cur_rot), with the bones
// of the context's image.  The kernel is dp_vjp_impl.h's text with DP_VJP_SKEL 0; its per-frame-skeleton form is dp_vjp_skel.hip.
#define DP_VJP_SKEL 0
#include "dp_vjp_impl.h"

hipError_t dp_launch_vjp(const Args* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + FPB - 1) / FPB);
    hipLaunchKernelGGL(dp_vjp_kernel, dim3(grid), dim3(FPB), 0, stream, args->img, *args);
    return hipGetLastError();
}
