// dp_cons_gap.hip -- dp_optimize_sequence_gaps (include/dragposer_gaps.h): dp_optimize_sequence_holds / dp_optimize_sequence_ar with a
// tracker set decided per step -- a sample that is absent (marked so, or refused by the screening) is replaced by the joint's last good one
// for up to max_hold steps at a decaying weight, and the joint leaves the loss after that, instead of ending the sequence.  The kernels are
// dp_cons_body.h's text twice more, with DP_CONS_TABLE 1, DP_CONS_SKEL 1, DP_CONS_SEQ 1, DP_CONS_HOLD 1 and DP_CONS_GAP 1, without and
// with DP_CONS_AR, in a unit of its own so that the other units' kernels keep their instructions.  Lane j is joint j: the decision is the
// lane's, its state a row of dp_gaps.state in global memory (dp_cons_gap.h) that the lane writes before a step's iteration loop and reads
// inside it.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "../../include/dragposer_gaps.h"
#include "dp_cons_gap.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 1
#define DP_CONS_SEQ 1
#define DP_CONS_HOLD 1
#define DP_CONS_GAP 1
#define DP_CONS_TABLE 1

__global__ __launch_bounds__(WPB * 64) void dp_terms_gap_seq_kernel(GapSeqArgs a)
#include "dp_cons_body.h"

#define DP_CONS_AR 1
__global__ __launch_bounds__(WPB * 64) void dp_terms_gap_ar_seq_kernel(GapArSeqArgs a)
#include "dp_cons_body.h"
#undef DP_CONS_AR
#undef DP_CONS_TABLE

hipError_t dp_launch_terms_gap_seq(const GapSeqArgs* args, hipStream_t stream) { return launch_waves(dp_terms_gap_seq_kernel, args, stream); }
hipError_t dp_launch_terms_gap_ar_seq(const GapArSeqArgs* args, hipStream_t stream) { return launch_waves(dp_terms_gap_ar_seq_kernel, args, stream); }
