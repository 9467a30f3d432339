// dp_w4_skel.hip -- the wave-private kernel (dp_w4_impl.h) in the DENSE row layout of layer 2 (as dp_w4.hip), with the bone offsets read per
// frame (whole-sequence launches: per sequence) from the caller's skeleton rows instead of the context's constants: include/dragposer_skeleton.h.
// The offsets enter the set-up only (W4_SKEL in dp_w4_impl.h); the iteration loop is dp_w4.hip's.
#define W4_SKEL 1
#define W4_KERNEL dp_w4sk_kernel
#include "dp_w4_impl.h"

extern "C" hipError_t dp_launch_w4sk(const KArgs* args, hipStream_t stream, LaunchPick* pick)
{
    constexpr int NW = 4;
    const bool lng = args->n_iter > MAX_ITERS;
    if (args->seq.n_steps > 0) {
        if (lng) w4_launch<NW, true, true, true>(args, stream, pick);
        else w4_launch<NW, true, true>(args, stream, pick);
    } else if (args->early_stop && args->mode == 0) {
        if (lng) w4_launch<NW, true, false, true>(args, stream, pick);
        else w4_launch<NW, true>(args, stream, pick);
    } else {
        if (lng) w4_launch<NW, false, false, true>(args, stream, pick);
        else w4_launch<NW, false>(args, stream, pick);
    }
    return hipGetLastError();
}
