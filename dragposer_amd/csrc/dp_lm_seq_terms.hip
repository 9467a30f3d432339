// dp_lm_seq_terms.hip -- dp_optimize_sequence_lm_terms (include/dragposer_sequence_lm_terms.h): dp_optimize_lm_terms' frame for T consecutive
// steps of S sequences in ONE launch.  The kernel is dp_lm_body.h's text once more, with DP_LM_SEQ 1 and DP_LM_TERMS 1, in a unit of its own so
// that dp_lm_kernel, dp_lm_seq_kernel and dp_lm_terms_kernel keep their instructions.
//
// Layout: dp_lm_seq.hip's -- one SEQUENCE per wave, WPB waves per workgroup, the latent, the global position and rotation and mu carried in
// registers -- with dp_lm_terms.hip's second LDS array beside the predictor's history rows (dp_lm_seq_terms.h).  No workgroup barrier after the
// staging, no atomics: a sequence's results depend on that sequence's inputs only.
// What the step loop changes of the table's handling, all of it redone every step:
//   global position  the terms' g is the carried position BEFORE the step (registers), never an array read; it is screened with the state only
//                    when an active PLANE or point-DISTANCE term exists (need_gp), as dp_lm_terms_kernel screens dp_terms.global_pos
//   rows             lane t reads term t's row of THIS step, per_frame + stp * T_STEP + s * 4 (T_STEP 0: one row held), screens it and writes
//                    it to the wave's RW rows; the active mask (c_t = weight s != 0) is taken again, so the places the terms take in the term
//                    pass and in the loss's sum change from step to step as a table without the terms that are off would have them
//   loss_terms       [T][S][n_terms] at the step's row: NaN on a bad-state or bad-target step, 0 for a term that is off on that step
//
// LDS hazards across steps.  A wave's LDS words are written and read by that wave alone, and wave_sync() orders its earlier LDS accesses before
// its later ones.  Every step that runs the frame ends in the step's closing wave_sync(), which stands between ALL of the step's reads -- the RW
// rows (term_rows reads other lanes' rows; term_value its own), the term pass's [24][32] place, which the solve then reuses, the pass in
// double's P / G arrays in the tangents' place (themselves closed by the pass's own last wave_sync()), the epilogue's reads of other lanes' P_j
// and the predictor's history rows -- and the next step's writes.  A step refused as bad state leaves the loop's body early, WITHOUT that
// closing wave_sync(): by then it has written row t of RW from lane t (the rows are written before the ballot that decides bad_state) and read
// nothing from LDS but the staged table, which no step writes.  The next step's first LDS write is the same lane's store to the same words,
// in program order, and its first read of another lane's row stands behind the wave_sync() that follows the ballot of the active mask.  So no
// wave_sync() is needed on that path -- and once a step is bad state the carried latent is NaN and every later step takes the same path.
// Inside a step the order is dp_lm_terms_kernel's, and the epilogue keeps dp_lm_seq_kernel's: the pass in double (its last reads closed), then
// wave_sync(), then the reads of W_P.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "dp_lm_seq_terms.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"
#include "dp_lm_terms_dev.h"

#define DP_LM_SEQ 1
#define DP_LM_TERMS 1
__global__ __launch_bounds__(WPB * 64) void dp_lm_seq_terms_kernel(SeqTermArgs a)
#include "dp_lm_body.h"
#undef DP_LM_TERMS
#undef DP_LM_SEQ

hipError_t dp_launch_lm_seq_terms(const SeqTermArgs* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(dp_lm_seq_terms_kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}
