// dp_w16_es_long.hip -- dp_w16_es.hip's instantiation (early stop, one wave per SIMD) for n_iter > 256 (dp_w16_impl.h: LONG).
#include "dp_w16_impl.h"

extern "C" hipError_t dp_launch_w16_es_long(const KArgs* args, hipStream_t stream, LaunchPick* pick)
{
    w16_launch<4, 1, true, true>(args, stream, pick);
    return hipGetLastError();
}
