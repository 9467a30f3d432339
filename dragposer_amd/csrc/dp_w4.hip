// dp_w4.hip -- the wave-private kernel (dp_w4_impl.h) in the DENSE row layout of layer 2 (dp_w4.h): both 64-row blocks hold
// channels of every quad's two items, so each runs all 15 K-groups.  Any decoder and skeleton the item plan accepts runs here;
// dp_create takes the body-part unit (dp_w4_bp.hip) instead when the decoder's block sparsity fits its placement.
#include "dp_w4_impl.h"

extern "C" hipError_t dp_launch_w4(const KArgs* args, hipStream_t stream, LaunchPick* pick)
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

extern "C" int dp_w4_lds_bytes(void) { return lds_total<4>() * 4; }
extern "C" int dp_w4_frames_per_block(void) { return 4 * FPW; }
