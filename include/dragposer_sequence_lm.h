/* dragposer_sequence_lm.h -- C ABI of libdragposer_hip.so: dp_optimize_lm (include/dragposer_lm.h) for n_steps consecutive frames of S
 * sequences in ONE launch, the state carried from step to step on the device -- what dp_optimize_sequence is to dp_optimize.  Per step: the
 * Levenberg-Marquardt frame of include/dragposer_lm.h, then run()'s epilogue (what dp_sequence_advance does).  Optionally the pull term's target
 * is formed inside the step loop by the linear predictor of include/dragposer_latent_ar.h, which a launch that does not own the frame loop
 * cannot offer: the target depends on the previous step's result.
 *
 * Equivalence.  On every output and state array the launch returns the bits of this per-frame composition, for t = 0 .. n_steps - 1:
 *   dp_optimize_lm with z0 = the carried latent, cur_rot = the carried global_rot, dp_lm_extra.mu carried in place, z_tgt = the step's row,
 *   tgt_pos / tgt_rot = the step's rows (tgt_pos shifted as below), w and tracked the launch's;
 *   dp_sequence_advance on the result (dp_seq_step.tgt_pos = the same shifted targets);
 *   the copy of dp_result.z into `latent`.
 * A second, tiny launch (dp_sequence_history_kernel) appends the steps' hist_scratch rows to the three history buffers, as dp_optimize_sequence's
 * does, so two chained launches see what one launch sees.
 *
 * Per-step outputs (dp_seq_results, [T][S] each, any but hist_scratch may be NULL): pose_ret, pos_ret, world_rot and status as
 * dp_optimize_sequence returns them; `iters` is the number of LM steps executed; `loss` is the loss at the returned latent evaluated in
 * double, as dp_optimize_lm reports it.  dp_seq_lm_extra (may be NULL, and every pointer in it may be NULL): `mu` [S] in/out -- the damping a
 * sequence starts from and ends with, read as dp_lm_extra.mu is (NULL: every sequence starts at mu0 and the final value is not returned);
 * `mu_trace` [T][S], mu after every step; `n_accepted` [T][S]; `loss0` [T][S][3], the loss at each step's warm start, in double; `joint_pos`
 * [T][S][22][3], dp_result.pos of every step.  The double passes behind `loss` and `loss0` cost about 7 us each per launch, per frame: each runs
 * only when its pointer is non-NULL.
 *
 * frames->tgt_root, when given, is honoured with dp_optimize_sequence's arithmetic: the shift of step t is tgt_root[t] - the sequence's global
 * position before step t, and it is added to tgt_pos -- a subtraction and an addition in fp32, unfused, in that order.
 *
 * The predictor.  With `ar` given the step's z_tgt row is c + sum_k A_k h_k, formed exactly as include/dragposer_latent_ar.h states under "The
 * predictor" (fp32, unfused, in that loop order).  Before the first step h_1 .. h_K are the last K rows of the sequence's latent_buf, the
 * newest last; after a step the step's z (its history row) becomes h_1 and the older rows shift.  frames->z_tgt must then be NULL and
 * state->history >= order.  ar->trace [T][S][24] receives the row each step used; a step refused as bad state, which used none, writes NaN
 * there.  The row goes through the usual z_tgt screening: a refused row gives DP_STATUS_BAD_TARGETS for that step.  Without `ar` the rows
 * are frames->z_tgt's, by its two strides.
 *
 * Status (dp_seq_results.status) is what the composition produces.  A step with a bad target (DP_STATUS_BAD_TARGETS) returns the warm start's
 * pose, a NaN z (so a NaN latent and history row), mu unchanged, iters 0.  Every later step of that sequence is DP_STATUS_BAD_STATE: its
 * results NaN, mu still unchanged, its history rows NaN as the per-frame epilogue makes them, and the state's global position and rotation NaN
 * at the end.  A sequence is a wave: the other sequences of the launch are bit-identical to a launch without the fault.
 *
 * The call is asynchronous on the given HIP stream: no allocation, no host synchronisation, graph-capturable (the parameters travel in the
 * launch; latent, state and `mu` are read and written at replay time).  No atomics: two calls on the same inputs give identical bits.  fp32 and
 * bf16-rounded contexts both work.  Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).
 * Refusals, DP_ERR_INVALID, in this order: NULL ctx; n_sequences not positive or NULL latent, frames, params, state or out; what dp_optimize_lm
 * refuses of dp_lm_params (its struct_size, then its values in that call's order); what dp_optimize_sequence refuses of dp_seq_results
 * (struct_size / reserved0), frames, state (hist_scratch required) and adjust -- a NULL frames->z_tgt is not among them here;
 * dp_seq_lm_extra.struct_size / reserved0; when `ar` is given, dp_latent_ar's own refusals in its order (struct_size / reserved0, order, NULL
 * coeffs or bias, state->history < order, a non-NULL frames->z_tgt -- "both"); without `ar`, a NULL frames->z_tgt -- "neither".  Then
 * DP_ERR_UNSUPPORTED from the test-only library or a library linked without dp_lm_seq.hip, DP_ERR_DEVICE from a context without a device image.
 *
 * Not covered: points (include/dragposer_points.h), holds, gaps and tethers in the LM loss, per-frame skeletons, dp_live_step and the
 * plug-in.  A term table in the LM loss of a clip is dp_optimize_sequence_lm_terms (include/dragposer_sequence_lm_terms.h).
 */
#ifndef DRAGPOSER_SEQUENCE_LM_H
#define DRAGPOSER_SEQUENCE_LM_H

#include "dragposer_latent_ar.h"
#include "dragposer_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dp_seq_lm_extra { /* DEVICE pointers, all optional */
    unsigned struct_size; /* sizeof(dp_seq_lm_extra) in the caller's translation unit (DP_SEQ_LM_EXTRA_INIT sets it) */
    unsigned reserved0;   /* must be 0 */
    float* mu;            /* [S] in/out: the damping a sequence starts from and ends with (NULL: mu0, not returned) */
    float* mu_trace;      /* [T][S] mu after every step */
    int* n_accepted;      /* [T][S] accepted LM steps */
    float* loss0;         /* [T][S][3] the loss at each step's warm start, in double as dp_optimize_lm reports it */
    float* joint_pos;     /* [T][S][22][3] dp_result.pos of every step */
} dp_seq_lm_extra;
#define DP_SEQ_LM_EXTRA_INIT {(unsigned)sizeof(dp_seq_lm_extra), 0u, (float*)0, (float*)0, (int*)0, (float*)0, (float*)0}

/* latent [S][24]: in = the warm start of the first step, out = the latent after the last.  state: global_pos / global_rot in and out, the three
 * history buffers advanced by n_steps.  adjust: the joint-adjustment fields of dp_seq_step (its pointers are ignored; may be NULL). */
int dp_optimize_sequence_lm(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_lm_params* params,
                            const dp_latent_ar* ar /* may be NULL */, const dp_seq_state* state, const dp_seq_step* adjust,
                            const dp_seq_results* out, const dp_seq_lm_extra* extra /* may be NULL */, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_SEQUENCE_LM_H */
