/* dragposer_sequence_constraints.h -- C ABI of libdragposer_hip.so, whole-sequence launches with extra loss terms: dp_optimize_sequence
 * (include/dragposer.h) with the four terms of dp_optimize_constrained (include/dragposer_constraints.h) or the term table of
 * dp_optimize_terms (include/dragposer_terms.h) in every frame's loss.
 *
 * n_steps consecutive frames of S sequences in ONE launch, plus dp_optimize_sequence's tiny second launch for the three history buffers.
 * Per step t and sequence s the launch does what these per-frame calls do, in their arithmetic and order, and returns their bits:
 *   dp_optimize_constrained[_skeleton] / dp_optimize_terms[_skeleton] with early_stop = 1 on z0 = the latent, cur_rot = state->global_rot,
 *     global_pos = state->global_pos, this step's targets and temporal target (dp_seq_frames' arrays and strides; with tgt_root the position
 *     targets are tgt_pos[t] + (tgt_root[t] - state->global_pos), in that operation order), Adam started afresh;
 *   dp_sequence_advance on that frame's result (global position / rotation update, joint adjustment against the step's effective targets,
 *     the history row, the returned pose with its root channels replaced by the normalised world rotation);
 *   the frame's `z` copied over the latent.
 * The floor term, PLANE terms and point-DISTANCE terms therefore see the sequence's own running global position: `global_pos` of
 * dp_constraints / dp_terms must be NULL or state->global_pos, and their per-frame outputs (loss_extra / loss_terms) must be NULL -- the
 * per-step ones are dp_seq_extra's.  A term's per_frame array is [S][4] held for all steps (row step 0) or [T][S][4] (row step S * 4): step
 * t of sequence s reads per_frame + t * row_step + s * 4, the row step given per term in dp_seq_extra.
 * skeleton: NULL = the context's own bones; otherwise a dp_skeleton_in (include/dragposer_skeleton.h), stride 66 = sequence s uses skeleton
 * s, stride 0 = one for the launch, read once and kept for all steps.  A sequence on skeleton X gets the bits of a context created with X.
 *
 * Status per step (dp_seq_results.status), as the per-frame calls give it: a step with a refused target returns the warm start's pose after
 * one pass with DP_STATUS_BAD_TARGETS (| DP_STATUS_NONFINITE_RESULT: its latent is NaN, as the reference's); the sequence is
 * DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE with every result NaN from the next step on and in later launches (its latent, global
 * position and rotation are NaN).  A refused state at entry or a refused bone fills all steps that way.  A sequence is a wave that shares
 * nothing: the other sequences of the launch are bit-identical to a launch without the fault.
 *
 * Asynchronous on the given HIP stream, no allocation, no host synchronisation, no copy of caller data; no atomics.  Returns DP_OK or a
 * negative dp_status and never throws; message: dp_last_error(ctx).  Refusals, in this order (all DP_ERR_INVALID): NULL ctx; n_sequences
 * <= 0 or a NULL latent / frames / params / constraints (terms) / state / out; what dp_params refuses; what dp_seq_results refuses; what
 * dp_constraints (dp_terms) refuses, the two pointer rules above included; dp_seq_extra -- a bad struct_size, a non-zero reserved0, a
 * negative row step; the skeleton struct (as dp_optimize_skeleton checks it); what dp_optimize_sequence refuses of frames, state, scratch
 * and joint adjustment; Adam's parameters.  Then DP_ERR_UNSUPPORTED from a library built without the kernels, DP_ERR_DEVICE from a context
 * without a device image.  dp_params.kernel and dp_params.early_stop are ignored (one kernel per call; the while-condition always runs).
 */
#ifndef DRAGPOSER_SEQUENCE_CONSTRAINTS_H
#define DRAGPOSER_SEQUENCE_CONSTRAINTS_H

#include "dragposer.h"
#include "dragposer_constraints.h"
#include "dragposer_skeleton.h"
#include "dragposer_terms.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dp_seq_extra {  /* DEVICE pointers, per step; all optional */
    unsigned struct_size; /* sizeof(dp_seq_extra) in the caller's translation unit (DP_SEQ_EXTRA_INIT sets it); checked like dp_result's */
    unsigned reserved0;   /* must be 0 */
    float* loss_extra;    /* [T][S][4] or NULL (dp_optimize_sequence_constrained): the four weighted terms of every step's last forward pass */
    float* loss_terms;    /* [T][S][n_terms] or NULL (dp_optimize_sequence_terms): each weighted term of every step's last forward pass */
    float* joint_pos;     /* [T][S][22][3] or NULL: P_j of every step (world: the global position before the step + P_j) */
    int row_step[DP_MAX_TERMS]; /* dp_optimize_sequence_terms: floats between two steps' rows of term k's per_frame array; 0 = [S][4], held.
                                   Must be >= 0; NOT checked against the array's extent (the caller's array holds t * row_step + S * 4 floats
                                   for every step t).  dp_optimize_sequence_constrained ignores row_step and loss_terms, and
                                   dp_optimize_sequence_terms ignores loss_extra */
} dp_seq_extra;
#define DP_SEQ_EXTRA_INIT {(unsigned)sizeof(dp_seq_extra), 0u, (float*)0, (float*)0, (float*)0, {0}}

/* latent [S][24], state, adjust and out as dp_optimize_sequence takes them; skeleton and extra may be NULL. */
int dp_optimize_sequence_constrained(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params,
                                     const dp_constraints* cons, const dp_skeleton_in* skeleton, const dp_seq_state* state,
                                     const dp_seq_step* adjust, const dp_seq_results* out, const dp_seq_extra* extra, void* hip_stream);

int dp_optimize_sequence_terms(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params,
                               const dp_terms* terms, const dp_skeleton_in* skeleton, const dp_seq_state* state, const dp_seq_step* adjust,
                               const dp_seq_results* out, const dp_seq_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_SEQUENCE_CONSTRAINTS_H */
