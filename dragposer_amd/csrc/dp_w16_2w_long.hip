// dp_w16_2w_long.hip -- dp_w16_2w.hip's instantiation (two waves per SIMD) for n_iter > 256 (dp_w16_impl.h: LONG).
#include "dp_w16_impl.h"

extern "C" hipError_t dp_launch_w16_2w_long(const KArgs* args, hipStream_t stream, LaunchPick* pick)
{
    w16_launch<8, 2, false, true>(args, stream, pick);
    return hipGetLastError();
}
