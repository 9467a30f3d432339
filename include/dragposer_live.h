/* dragposer_live.h -- C ABI of libdragposer_hip.so: dp_optimize_sequence_gaps (include/dragposer_gaps.h) for ONE step in ONE launch.
 *
 * Every dp_optimize_sequence_* call is two launches: the step loop, then dp_sequence_history_kernel, which appends the steps' rows
 * (dp_seq_results.hist_scratch) to the three history buffers of dp_seq_state.  Over a clip the second launch is paid once; a live caller --
 * the Unity plug-in, DragPose.run -- runs one step per call and pays it every frame.  dp_live_step is the one-step call with the append done
 * by the kernel itself: the wave that owns a sequence moves each column of the sequence's latent_buf, disp_buf and heights_buf up by one row
 * and stores the step's value in the last row, after the step's state write-back.
 *
 * Arguments and rules: dp_optimize_sequence_gaps', all of them (`ar`, `holds`, `skeleton`, `adjust` and `extra` may be NULL as there), and
 * frames->n_steps must be 1.
 *
 * Equivalence.  The call returns the bits of dp_optimize_sequence_gaps with the same arguments on every output and state array: latent, the
 * results, dp_seq_state's global position and rotation and its three history buffers, dp_holds' state and trace, dp_gaps' state and trace,
 * dp_latent_ar's trace, and hist_scratch, which is still written -- on every exit of the step, a step refused as bad state included (its
 * row, and so the appended one, is NaN).
 *
 * Refusals: a NULL ctx; then a non-positive n_sequences or a NULL latent, frames, params, terms, gaps, state or out; then
 * frames->n_steps != 1; then everything dp_optimize_sequence_gaps refuses after its NULL arguments, in its order (all DP_ERR_INVALID).
 * After those, DP_ERR_UNSUPPORTED from a library built without the kernel.
 */
#ifndef DRAGPOSER_LIVE_H
#define DRAGPOSER_LIVE_H

#include "dragposer_gaps.h"

#ifdef __cplusplus
extern "C" {
#endif

int dp_live_step(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params, const dp_terms* terms,
                 const dp_holds* holds, const dp_latent_ar* ar, const dp_gaps* gaps, const dp_skeleton_in* skeleton, const dp_seq_state* state,
                 const dp_seq_step* adjust, const dp_seq_results* out, const dp_seq_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_LIVE_H */
