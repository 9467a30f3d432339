// dp_w4_bp.hip -- the wave-private kernel (dp_w4_impl.h) in the BODY-PART row layout of layer 2 (dp_w4.h: block A = the legs and the
// root displacement, block B = the spine, the arms and the virtual items): 7 + 13 K-groups of layer 2 instead of 15 + 15, 40 MFMAs fewer
// per iteration, the same bits.  dp_create takes it when every K-group it leaves out is exactly zero for the model (dp_host.cpp).
#define W4_BP 1
// Layer 2 holds 80 accumulator registers here instead of 120: two more head groups of bL2 stay resident (5 + 2 in vector registers): -0.9 %
// against 3 (profiles/r07_bp_tuning.txt; the dense unit keeps 3, its accumulator half is full)
#define W4_B2_RES_A 5
#define W4_KERNEL dp_w4_bp_kernel
#include "dp_w4_impl.h"

extern "C" hipError_t dp_launch_w4_bp(const KArgs* args, hipStream_t stream, LaunchPick* pick)
{
    constexpr int NW = 4;
    const bool lng = args->n_iter > MAX_ITERS;
    if (args->seq.n_steps > 0) {
        if (lng) w4_launch<NW, true, true, true>(args, stream, pick);
        else w4_launch<NW, true, true>(args, stream, pick);
    } else if (args->early_stop && args->mode == 0) {
        if (lng) w4_launch<NW, true, false, true>(args, stream, pick);
        else w4_launch<NW, true>(args, stream, pick);
    } else if (args->mode == 0 && !(DBG_DUMP && args->dbg)) {
        return dp_launch_w4_bp_lv(args, stream, pick); // fixed-count optimising launches: the kernel with the loop versions (dp_w4_bp_lv.hip)
    } else {
        if (lng) w4_launch<NW, false, false, true>(args, stream, pick);
        else w4_launch<NW, false>(args, stream, pick);
    }
    return hipGetLastError();
}
