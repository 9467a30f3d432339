/* dragposer_sequence_lm_terms.h -- C ABI of libdragposer_hip.so: dp_optimize_lm_terms (include/dragposer_lm_terms.h) for n_steps consecutive
 * frames of S sequences in ONE launch, the state carried from step to step on the device -- dp_optimize_sequence_lm
 * (include/dragposer_sequence_lm.h) with a table of constraint terms (include/dragposer_terms.h) in the Levenberg-Marquardt loss, what
 * dp_optimize_sequence_terms is to dp_optimize_terms.
 *
 * Equivalence.  On every output and state array the launch returns the bits of this per-frame composition, for t = 0 .. n_steps - 1:
 *   dp_optimize_lm_terms with z0 = the carried latent, cur_rot = the carried global_rot, dp_terms.global_pos = the carried global position
 *   BEFORE the step, dp_lm_extra.mu carried in place, tgt_pos / tgt_rot = the step's rows (tgt_pos shifted by tgt_root[t] - that global
 *   position: a subtraction and an addition in fp32, unfused, in that order), z_tgt = the step's row, or the predictor's row when `ar` is
 *   given, each term's per_frame = the step's rows of that term, w and tracked the launch's;
 *   dp_sequence_advance on the result (dp_seq_step.tgt_pos = the same shifted targets);
 *   the copy of dp_result.z into `latent`.
 * A second, tiny launch (dp_sequence_history_kernel) appends the steps' hist_scratch rows to the three history buffers, as
 * dp_optimize_sequence_lm's does.
 *
 * Terms.  dp_terms is used as dp_optimize_sequence_terms uses it: the table and up_axis as given; global_pos must be NULL or
 * state->global_pos (the terms read the sequence's own carried position); dp_terms.loss_terms must be NULL -- the per-step array is
 * term_extra->loss_terms, [T][S][n_terms].  Joints 0..21 only.  term_extra is dp_seq_extra of include/dragposer_sequence_constraints.h (may be
 * NULL): row_step[k] and loss_terms are read as dp_optimize_sequence_terms reads them -- term k's row of step t and sequence s is
 * per_frame + t * row_step[k] + s * 4, with row_step 0 meaning one [S][4] array held for all steps; loss_extra is ignored; a non-NULL
 * joint_pos there is refused, because the joint positions of every step are dp_seq_lm_extra.joint_pos here and the two arrays must not be
 * confused.  Everything else -- dp_seq_results, dp_seq_lm_extra (mu, mu_trace, n_accepted, loss0, joint_pos), tgt_root, the predictor and its
 * trace -- is dp_optimize_sequence_lm's.
 *
 * loss_terms [T][S][n_terms]: each weighted term c_k T_k at the step's returned latent, from the pass in double; 0 for a term that is off on
 * that step (weight 0, or s = 0 in the step's row); NaN on a bad-state or bad-target step.  The pass in double runs only when loss, loss0 or
 * loss_terms is asked for.
 *
 * Special cases.  With n_terms = 0, or with every weight 0, every result has the bits of dp_optimize_sequence_lm.  A step on which a term is
 * off has the bits of the table without that term: the active set is taken again at every step.
 *
 * Status (dp_seq_results.status) is what the composition produces.  A refused per-frame row of an active term at step t (not finite, beyond
 * DP_INPUT_LIMIT, or s < 0) gives DP_STATUS_BAD_TARGETS for that step -- the warm start's pose, NaN z and loss_terms, mu unchanged -- and
 * every later step of that sequence is DP_STATUS_BAD_STATE, as after any bad target (include/dragposer_sequence_lm.h).  The carried global
 * position is screened with the state at every step, but only when an active PLANE or point-DISTANCE term exists: a refused global position at
 * entry then makes every step DP_STATUS_BAD_STATE; without such a term it is handled as dp_optimize_sequence_lm handles it.  A sequence is a
 * wave: the other sequences of the launch are bit-identical to a launch without the fault.
 *
 * The call is asynchronous on the given HIP stream: no allocation, no host synchronisation, graph-capturable.  The table travels in the launch;
 * the per-frame rows, mu, latent and state are read at replay time.  No atomics: two calls on the same inputs give identical bits.
 * Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).  Refusals, DP_ERR_INVALID, in this order:
 *   1. dp_optimize_sequence_lm's, in its order, up to and including dp_seq_lm_extra: NULL ctx; n_sequences not positive or NULL latent, frames,
 *      params, terms, state or out; dp_lm_params (struct_size, then values); dp_seq_results; frames, state, adjust; dp_seq_lm_extra's
 *      struct_size / reserved0;
 *   2. what dp_terms and its table refuse (struct_size, reserved0, a global_pos that is neither NULL nor state->global_pos, a non-NULL
 *      dp_terms.loss_terms, n_terms, a NULL `terms`, up_axis, each term);
 *   3. dp_seq_extra: struct_size, reserved0, a negative row_step, a non-NULL joint_pos;
 *   4. the predictor's: with `ar`, dp_latent_ar's own refusals in its order (a non-NULL frames->z_tgt -- "both" -- last); without it, a NULL
 *      frames->z_tgt -- "neither";
 *   5. then DP_ERR_UNSUPPORTED from the test-only library or a library linked without dp_lm_seq_terms.hip, DP_ERR_DEVICE from a context without
 *      a device image.
 *
 * Not covered: points (include/dragposer_points.h), holds, gaps and tethers in the LM loss, per-frame skeletons, dp_live_step and the
 * plug-in.
 */
#ifndef DRAGPOSER_SEQUENCE_LM_TERMS_H
#define DRAGPOSER_SEQUENCE_LM_TERMS_H

#include "dragposer_lm_terms.h"
#include "dragposer_sequence_constraints.h"
#include "dragposer_sequence_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

int dp_optimize_sequence_lm_terms(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_lm_params* params,
                                  const dp_terms* terms, const dp_latent_ar* ar /* may be NULL */, const dp_seq_state* state,
                                  const dp_seq_step* adjust, const dp_seq_results* out, const dp_seq_lm_extra* extra /* may be NULL */,
                                  const dp_seq_extra* term_extra /* may be NULL */, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_SEQUENCE_LM_TERMS_H */
