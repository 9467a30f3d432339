/* dragposer_latent_ar.h -- C ABI of libdragposer_hip.so: dp_optimize_sequence_holds (include/dragposer_holds.h) with the pull term's target
 * formed INSIDE the step loop by a linear autoregressive predictor over the sequence's own recent latents.
 *
 * The loss pulls the latent towards a target, lambda_temporal * mse(z, z_tgt).  dp_seq_frames.z_tgt must be known before the launch starts;
 * a target that depends on what the previous step produced is not.  This call forms it per step:
 *
 *   z_tgt(t) = c + sum_{k=1..K} A_k h_k
 *
 * h_k is the history row that step t - k appended to dp_seq_state.latent_buf (the reference's current_latent; the z_pre of the per-frame
 * calls; the first 24 floats of the step's hist_scratch row).  The form covers "hold the last latent" (K = 1, A_1 = I), constant velocity with
 * or without damping (K = 2, A_1 = (1 + d) I, A_2 = -d I) and any vector-AR model fitted in closed form.
 *
 * The predictor.  Component i, in fp32, unfused, in exactly this order (A = coeffs, row = output component):
 *   acc = c[i]
 *   for k = 1..K: for j = 0..23: acc = add_rn(acc, mul_rn(A[k-1][i][j], h_k[j]))
 * The result is the step's z_tgt row and goes through the step's z_tgt screening: a value that is not finite or beyond DP_INPUT_LIMIT gives
 * DP_STATUS_BAD_TARGETS for that step, with the consequences include/dragposer_sequence_constraints.h states.
 *
 * The history.  Before the first step h_1..h_K are the last K rows of the sequence's latent_buf, the newest last (history >= K).  After a
 * step its history row becomes h_1 and the older rows shift.  A step refused as bad state, which skips the loop, leaves the history as it
 * was (its row of `trace` is NaN: it used no target).  Nothing else is written: the call's second launch appends the steps' rows to
 * latent_buf as dp_optimize_sequence_holds' does, so two chained launches see what one launch sees.
 *
 * Equivalence.  The launch returns the bits of this per-frame composition: dp_optimize_terms[_skeleton] with z_tgt = the row above formed from
 * the last K rows of latent_buf, then dp_sequence_advance, then the latent copy, then the hold update -- on every output of
 * dp_optimize_sequence_holds, on the state arrays, on the holds' state and trace, and on `trace`.
 *
 * Arguments: dp_optimize_sequence_holds', with two differences.  `holds` may be NULL (no hold; the same as n_holds = 0), and a table with
 * n_terms = 0 is allowed.  frames->z_tgt must be NULL and its two strides are ignored: the targets have one source.
 *
 * Refusals: dp_optimize_sequence_holds' in its order (a NULL `holds` is not one; a NULL `ar` is refused with the NULL arguments), then, as
 * DP_ERR_INVALID and in this order: a bad dp_latent_ar.struct_size or a non-zero reserved0; `order` outside 1..DP_MAX_AR_ORDER; NULL coeffs or
 * bias; state->history < order; a non-NULL frames->z_tgt.  After those, DP_ERR_UNSUPPORTED from a library built without the kernel.
 */
#ifndef DRAGPOSER_LATENT_AR_H
#define DRAGPOSER_LATENT_AR_H

#include "dragposer_holds.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_MAX_AR_ORDER 4

typedef struct dp_latent_ar {
    unsigned struct_size; /* sizeof(dp_latent_ar) in the caller's translation unit (DP_LATENT_AR_INIT sets it); checked like dp_result's */
    unsigned reserved0;   /* must be 0 */
    int order;            /* K, 1..DP_MAX_AR_ORDER */
    const float* coeffs;  /* DEVICE [K][24][24]: A_1 .. A_K, row = output component */
    const float* bias;    /* DEVICE [24]: c */
    float* trace;         /* DEVICE [T][S][24] or NULL: the z_tgt row each step used */
} dp_latent_ar;
#define DP_LATENT_AR_INIT {(unsigned)sizeof(dp_latent_ar), 0u, 0, (const float*)0, (const float*)0, (float*)0}

/* latent, frames, params, terms, holds (may be NULL), skeleton (may be NULL), state, adjust, out and extra (may be NULL) as
 * dp_optimize_sequence_holds takes them. */
int dp_optimize_sequence_ar(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params,
                            const dp_terms* terms, const dp_holds* holds, const dp_latent_ar* ar, const dp_skeleton_in* skeleton,
                            const dp_seq_state* state, const dp_seq_step* adjust, const dp_seq_results* out, const dp_seq_extra* extra,
                            void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_LATENT_AR_H */
