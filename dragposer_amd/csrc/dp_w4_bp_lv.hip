// dp_w4_bp_lv.hip -- the body-part kernel (dp_w4_bp.hip) for fixed-count OPTIMISING launches, with the iteration loop compiled once per loop
// version (dp_w4_impl.h: W4_LOOP_VERSIONS, dp_w4_iter.h): a wave picks the version without the rare paths when none of its frames tracks more
// than six joints, the general loop otherwise.  Same arithmetic in the same order as dp_w4_bp.hip's kernel: the same bits, the headline launch
// -3.3 %.  dp_launch_w4_bp hands these launches over; forward-only launches, launches that ask for the debug dump, the
// while-condition and whole-sequence launches stay with dp_w4_bp.hip's kernels, whose loop stands once (tests/test_w4_bp_layout.py counts it).
#define W4_BP 1
#define W4_B2_RES_A 5 // (as dp_w4_bp.hip)
#define W4_LOOP_VERSIONS 1
#define W4_KERNEL dp_w4_bplv_kernel
#include "dp_w4_impl.h"

extern "C" hipError_t dp_launch_w4_bp_lv(const KArgs* args, hipStream_t stream, LaunchPick* pick)
{
    constexpr int NW = 4;
    if (args->n_iter > MAX_ITERS) w4_launch<NW, false, false, true>(args, stream, pick);
    else w4_launch<NW, false>(args, stream, pick);
    return hipGetLastError();
}
