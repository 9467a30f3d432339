// dp_w16_2w_es.hip -- the early-stop instantiation with two waves per SIMD (see dp_w16_es.hip, dp_w16_2w.hip).
#include "dp_w16_impl.h"

extern "C" hipError_t dp_launch_w16_2w_es(const KArgs* args, hipStream_t stream, LaunchPick* pick)
{
    w16_launch<8, 2, true>(args, stream, pick);
    return hipGetLastError();
}
