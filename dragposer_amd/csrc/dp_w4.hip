// dp_w4.hip -- the wave-private kernel (dp_w4_impl.h) in the DENSE row layout of layer 2 (dp_w4.h): both 64-row blocks hold
// channels of every quad's two items, so each runs all 15 K-groups.  Any decoder and skeleton the item plan accepts runs here;
// dp_create takes the body-part unit (dp_w4_bp.hip) instead when the decoder's block sparsity fits its placement.
#include "dp_w4_impl.h"

extern "C" hipError_t dp_launch_w4(const KArgs* args, hipStream_t stream)
{
    constexpr int NW = 4;
    const int grid = (args->n_frames + NW * FPW - 1) / (NW * FPW);
    const bool lng = args->n_iter > MAX_ITERS;
    if (args->seq.n_steps > 0) {
        if (lng) hipLaunchKernelGGL((dp_w4_kernel<NW, true, true, true>), dim3(grid), dim3(NW * 64), 0, stream, *args);
        else hipLaunchKernelGGL((dp_w4_kernel<NW, true, true>), dim3(grid), dim3(NW * 64), 0, stream, *args);
    } else if (args->early_stop && args->mode == 0) {
        if (lng) hipLaunchKernelGGL((dp_w4_kernel<NW, true, false, true>), dim3(grid), dim3(NW * 64), 0, stream, *args);
        else hipLaunchKernelGGL((dp_w4_kernel<NW, true>), dim3(grid), dim3(NW * 64), 0, stream, *args);
    } else {
        if (lng) hipLaunchKernelGGL((dp_w4_kernel<NW, false, false, true>), dim3(grid), dim3(NW * 64), 0, stream, *args);
        else hipLaunchKernelGGL((dp_w4_kernel<NW, false>), dim3(grid), dim3(NW * 64), 0, stream, *args);
    }
    return hipGetLastError();
}

extern "C" int dp_w4_lds_bytes(void) { return lds_total<4>() * 4; }
extern "C" int dp_w4_frames_per_block(void) { return 4 * FPW; }
