// dp_w16_2w_es_long.hip -- dp_w16_2w_es.hip's instantiation (early stop, two waves per SIMD) for n_iter > 256 (dp_w16_impl.h: LONG).
#include "dp_w16_impl.h"

extern "C" hipError_t dp_launch_w16_2w_es_long(const KArgs* args, hipStream_t stream, LaunchPick* pick)
{
    w16_launch<8, 2, true, true>(args, stream, pick);
    return hipGetLastError();
}
