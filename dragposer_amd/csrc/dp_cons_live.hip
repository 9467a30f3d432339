// dp_cons_live.hip -- dp_live_step (include/dragposer_live.h): one step of dp_optimize_sequence_gaps with the history append in the same
// launch.  The kernels are dp_cons_body.h's text twice more, under dp_cons_gap.hip's switches and DP_CONS_LIVE 1, without and with
// DP_CONS_AR, in a unit of its own so that the other units' kernels keep their instructions.  A sequence is one wave and a column of its
// history one lane of that wave: after the step's state write-back lane c < 27 + n_heights does for column c what
// dp_sequence_history_kernel does for it after a one-step launch (dp_cons_live.h).
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "../../include/dragposer_gaps.h"
#include "dp_cons_live.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 1
#define DP_CONS_SEQ 1
#define DP_CONS_HOLD 1
#define DP_CONS_GAP 1
#define DP_CONS_LIVE 1
#define DP_CONS_TABLE 1

__global__ __launch_bounds__(WPB * 64) void dp_live_kernel(LiveSeqArgs a)
#include "dp_cons_body.h"

#define DP_CONS_AR 1
__global__ __launch_bounds__(WPB * 64) void dp_live_ar_kernel(LiveArSeqArgs a)
#include "dp_cons_body.h"
#undef DP_CONS_AR
#undef DP_CONS_TABLE

hipError_t dp_launch_live(const LiveSeqArgs* args, hipStream_t stream) { return launch_waves(dp_live_kernel, args, stream); }
hipError_t dp_launch_live_ar(const LiveArSeqArgs* args, hipStream_t stream) { return launch_waves(dp_live_ar_kernel, args, stream); }
