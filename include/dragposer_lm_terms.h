/* dragposer_lm_terms.h -- C ABI of libdragposer_hip.so: dp_optimize_lm (include/dragposer_lm.h) with a table of constraint terms
 * (include/dragposer_terms.h) in its loss, in one launch.  dp_optimize_lm's algorithm stays unchanged apart from the loss and the rows:
 * L is its three numbers plus sum_k c_k T_k, with c_k = weight_k * s_f and T_k as include/dragposer_terms.h defines it.
 *
 * The algorithm.  Extra rows of [J | r] are formed at the latent the step starts from.  The active set is taken there with strict
 * inequalities.  A term with c_k = 0 has no row.
 *   PLANE     active when two-sided, or when d < 0.  One row r = sqrt(c) d, dr = sqrt(c) dir^T dP_a.
 *   DISTANCE  with u = h(P_a - P_b) or h(g + P_a - point) and q = |u|^2:
 *             q > hi^2: three rows r = sqrt(c) u, dr = sqrt(c) h(dP_a - dP_b).  A pin (lo = hi = 0) is this case.
 *             q < lo^2: one row r = sqrt(c (lo^2 - q)), dr = -sqrt(c) u^T du / sqrt(lo^2 - q).
 *             Otherwise no row.  lo^2 and hi^2 are the float products dp_optimize_terms uses.
 *   ALIGN     active when |u| > p0 and c < 1.  One row r = sqrt(c_k) (1 - c), dr = -sqrt(c_k) dc, through both normalisations and h;
 *             joint-to-joint: both joints' dG.
 * Then A = J^T J and g = J^T r over tracker, term and pull rows; g is half of the gradient of L exactly.  Above hi the band c (q - hi^2)
 * is convex in u and the pin's rows have half its gradient and a PSD curvature; below lo the band is concave, and the square-root row has
 * half its gradient and a curvature that grows as the joint nears the edge of the band, which keeps the step from overshooting.  The trial
 * is accepted iff L(z') < L(z) with the TRUE T_k (the bands' relu included).  Everything else -- damping, Cholesky, the rejection paths, the
 * bookkeeping of mu, the early stop on the two tracker losses, "keep A and g after a rejection" -- is dp_optimize_lm's.  A row that is not
 * finite, because lo^2 - q underflowed, takes the existing path: a pivot that is not finite, a NaN trial, a rejection.
 *
 * Outputs.  dp_result and dp_lm_extra as in dp_optimize_lm: `loss` and `loss0` stay the three numbers.  dp_terms.loss_terms [B][n_terms],
 * when not NULL, is each weighted term c_k T_k at the returned latent, from the pass in double; a term that is off (weight 0, or s_f = 0 on
 * that frame) has 0.  The steps are decided on fp32 passes that add the weighted terms in the table's order, term 0 first, after the
 * three numbers.  With n_terms = 0, or with every weight 0, every result has the bits of dp_optimize_lm; a frame on which a term is off
 * has the bits of the table without that term.
 *
 * dp_terms is used as dp_optimize_terms uses it: the table, up_axis, global_pos, loss_terms, per-frame rows.  Joints 0..21 only.
 * Status.  A refused per-frame row of an active term (not finite, beyond DP_INPUT_LIMIT, or s < 0): DP_STATUS_BAD_TARGETS with
 * dp_optimize_lm's results for it -- no step, the warm start's pose, NaN z, loss, loss0 and loss_terms, mu unchanged.  A refused global_pos,
 * read only when an active PLANE or point-DISTANCE term exists: DP_STATUS_BAD_STATE, every result NaN.  The other frames are
 * bit-identical to a launch without the fault.  The rows and mu are read at launch time: a captured graph sees their contents at replay.
 *
 * Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).  Refusals, DP_ERR_INVALID, in this order: NULL ctx;
 * NULL batch, params or terms; dp_lm_params.struct_size; what dp_result refuses; dp_lm_extra.struct_size / reserved0; what dp_terms and its
 * table refuse (include/dragposer_terms.h: struct_size, reserved0, n_terms, a NULL `terms`, up_axis, each term, a NULL global_pos that
 * an active term needs); the LM parameters' values in dp_optimize_lm's order; what the batch refuses.  Then DP_ERR_UNSUPPORTED from
 * the test-only library or a library linked without the kernel, DP_ERR_DEVICE from a context without a device image.
 *
 * Not covered: points (include/dragposer_points.h), holds, gaps and tethers in the LM loss, per-frame skeletons, dp_live_step and the
 * plug-in.  The frame loop on the device with the table is dp_optimize_sequence_lm_terms' (include/dragposer_sequence_lm_terms.h): a clip in
 * one launch, the bits of this call followed by dp_sequence_advance, frame by frame.
 */
#ifndef DRAGPOSER_LM_TERMS_H
#define DRAGPOSER_LM_TERMS_H

#include "dragposer_lm.h"
#include "dragposer_terms.h"

#ifdef __cplusplus
extern "C" {
#endif

int dp_optimize_lm_terms(dp_ctx* ctx, const dp_batch* in, const dp_lm_params* params, const dp_terms* terms, const dp_result* out,
                         const dp_lm_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_LM_TERMS_H */
