// dp_cons_hold.hip -- dp_optimize_sequence_holds (include/dragposer_holds.h): dp_optimize_sequence_terms with joints held where they
// touched down.  The kernel is dp_cons_body.h's text once more, with DP_CONS_TABLE 1, DP_CONS_SKEL 1, DP_CONS_SEQ 1 and DP_CONS_HOLD 1, in a
// unit of its own so that dp_cons_seq.hip's two kernels keep their instructions.  A hold is a state machine of one sequence, so of one wave:
// (x, y, z, held) sits in the held term's row of the wave's block (dp_cons_hold.h), where the term reads its point and its scale as it reads a
// per_frame row; run()'s epilogue at each step's `stop` latches the joint's world position when it comes down and releases it when it lifts,
// in the operations and order the header states, and the step's closing wave_sync() orders that write before the next step's reads.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "dp_cons_hold.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 1
#define DP_CONS_SEQ 1
#define DP_CONS_HOLD 1

__global__ __launch_bounds__(WPB * 64) void dp_terms_hold_seq_kernel(HoldSeqArgs a)
#define DP_CONS_TABLE 1
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

hipError_t dp_launch_terms_hold_seq(const HoldSeqArgs* args, hipStream_t stream) { return launch_waves(dp_terms_hold_seq_kernel, args, stream); }
