// dp_w4_bp_skel.hip -- the wave-private kernel (dp_w4_impl.h) in the BODY-PART row layout of layer 2 (as dp_w4_bp.hip), with the bone offsets
// read per frame (whole-sequence launches: per sequence) from the caller's skeleton rows: include/dragposer_skeleton.h.  dp_create's choice
// between the two layouts applies unchanged.
#define W4_BP 1
#define W4_B2_RES_A 5 // (as dp_w4_bp.hip)
#define W4_SKEL 1
#define W4_KERNEL dp_w4sk_bp_kernel
#include "dp_w4_impl.h"

extern "C" hipError_t dp_launch_w4sk_bp(const KArgs* args, hipStream_t stream, LaunchPick* pick)
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
