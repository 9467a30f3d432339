// dp_lm_seq.hip -- dp_optimize_sequence_lm (include/dragposer_sequence_lm.h): dp_optimize_lm's frame for T consecutive steps of S sequences in ONE
// launch.  The kernel is dp_lm_body.h's text once more, with DP_LM_SEQ 1, in a unit of its own so that dp_lm_kernel keeps its instructions.
//
// Layout: one SEQUENCE per wave, WPB waves per workgroup; the staging and the wave's block are dp_lm.h's, and a second LDS array holds the
// latent predictor's history rows, an area per wave (dp_lm_seq.h).  No workgroup barrier after the staging -- the waves of a workgroup finish
// their steps at different times -- and no atomics: a sequence's results depend on that sequence's inputs only.
// Per step: the step's targets (tgt_pos shifted by tgt_root - the carried global position; the pull's row from z_tgt or from the predictor),
// their screening, dp_lm_kernel's iteration unchanged, and at the step's end the results with run()'s epilogue in dp_sequence_advance_kernel's
// arithmetic and order.  The latent, the global position and rotation and mu are carried in registers and written once after the last step;
// a step refused as bad state writes its NaN rows and the wave goes on to the next.  The steps' history rows go to hist_scratch; the host's
// second launch (dp_sequence_history_kernel) appends them.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "dp_lm_seq.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"

#define DP_LM_SEQ 1
__global__ __launch_bounds__(WPB * 64) void dp_lm_seq_kernel(SeqArgs a)
#include "dp_lm_body.h"
#undef DP_LM_SEQ

hipError_t dp_launch_lm_seq(const SeqArgs* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(dp_lm_seq_kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}
