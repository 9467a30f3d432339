// dp_lm_terms.hip -- dp_optimize_lm_terms (include/dragposer_lm_terms.h): dp_optimize_lm's frame with a table of constraint terms
// (include/dragposer_terms.h) in its loss, every step of every frame in ONE launch.  The kernel is dp_lm_body.h's text once more, with
// DP_LM_TERMS 1, in a unit of its own so that dp_lm_kernel and dp_lm_seq_kernel keep their instructions.
//
// Layout: dp_lm.hip's -- one frame per wave, WPB waves per workgroup, the staging and the wave's block of dp_lm.h -- and a second LDS array
// with the term table, staged once per workgroup, and a block of the frame's rows per wave (dp_lm_terms.h).  No workgroup barrier after the
// staging, no atomics: a frame's results depend on that frame's inputs only.
//   screening  lane t reads and screens term t's per-frame row once, the dp_cons family's rule; the frame's active terms (c_t = weight s_f
//              != 0) are a 16-bit mask the wave holds
//   loss       every forward pass: lane t evaluates c_t T_t with the true T on the pass's P_j and G_j; the sum that decides the steps adds
//              them, term 0 first, behind the three numbers.  The pass in double does the same for loss_terms at the returned latent
//   rows       after the tracker pairs, before the latent pull: rounds of eight active terms, four per half of the wave, three rows each,
//              into the Jacobian rows' place [24][32] and onto the same four accumulator tiles by the same six MFMA groups.  A PLANE, a
//              DISTANCE below lo and an ALIGN are one row, a DISTANCE above hi three; lane n < 24 walks the paths of the term's joints for
//              column n (dp_lm_terms_dev.h: joint_tangent, the tracker loop's arithmetic for any joint), lane 24 forms the residuals
// With no active term the kernel adds nothing to A, g or the loss: dp_optimize_lm's bits.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "dp_lm_terms.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"
#include "dp_lm_terms_dev.h"

#define DP_LM_SEQ 0
#define DP_LM_TERMS 1
__global__ __launch_bounds__(WPB * 64) void dp_lm_terms_kernel(TermArgs a)
#include "dp_lm_body.h"
#undef DP_LM_TERMS
#undef DP_LM_SEQ

hipError_t dp_launch_lm_terms(const TermArgs* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(dp_lm_terms_kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}
