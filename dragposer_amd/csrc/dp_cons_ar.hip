// dp_cons_ar.hip -- dp_optimize_sequence_ar (include/dragposer_latent_ar.h): dp_optimize_sequence_holds with the pull term's target formed
// inside the step loop, z_tgt(t) = c + sum_k A_k h_k over the sequence's last K history rows.  The kernel is dp_cons_body.h's text once more,
// with DP_CONS_TABLE 1, DP_CONS_SKEL 1, DP_CONS_SEQ 1, DP_CONS_HOLD 1 and DP_CONS_AR 1, in a unit of its own so that the other units' kernels
// keep their instructions.  The history rows are a sequence's, so a wave's: they sit in an LDS area of the wave's own (dp_cons_ar.h), loaded
// from the state's latent_buf before the first step and shifted at each step's `stop` by the row the step hands to hist_scratch; lane i forms
// component i of the target at the top of a step, in the operations and order the header states, and the step's existing screening sees it.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "dp_cons_ar.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 1
#define DP_CONS_SEQ 1
#define DP_CONS_HOLD 1
#define DP_CONS_AR 1

__global__ __launch_bounds__(WPB * 64) void dp_terms_ar_seq_kernel(ArSeqArgs a)
#define DP_CONS_TABLE 1
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

hipError_t dp_launch_terms_ar_seq(const ArSeqArgs* args, hipStream_t stream) { return launch_waves(dp_terms_ar_seq_kernel, args, stream); }
