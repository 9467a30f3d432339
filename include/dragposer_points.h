/* dragposer_points.h -- C ABI of libdragposer_hip.so: dp_optimize_terms (include/dragposer_terms.h) with POINTS -- terms on weighted
 * combinations of the joints' positions, still one launch.
 *
 * Every term of dragposer_terms.h names one or two of the 22 joints.  A constraint on a point that is not a joint -- the centre of mass
 * over the support midpoint of the feet, the midpoint of two hands on a tracked prop, the pelvis between the feet, the head over the
 * mid-hip -- has the same shape with one change: a point V = sum_j m_j P_j, sum_j m_j = 1, stands where a joint's position stands.
 *
 * Points.  Point k (0 <= k < n_points <= DP_MAX_POINTS) is row k of `coeff`, 22 coefficients m_k[j].  In the notation of
 * dragposer_terms.h its position is P_(22+k) = sum_j m_k[j] P_j and, the coefficients summing to 1, its world position is
 * W_(22+k) = g + P_(22+k).  In a table launched through the entry points below, joint_a and joint_b of a DP_TERM_PLANE or
 * DP_TERM_DISTANCE term may be 22 + k:
 *   a DISTANCE between two points, or between a point and a joint in either order, is the joint-to-joint form (g cancels);
 *   a point with joint_b = -1 is the point-DISTANCE form, with `point` or per_frame rows as for a joint;
 *   DP_TERM_DROP_UP, DP_TERM_ONE_SIDED, p0 / p1, weight, s_f, loss_terms and the while-condition's total keep their meaning;
 *   a term may name the same point twice (its value and its gradient are then 0), or a point and one of its member joints: the
 *   gradients add.
 * The gradient is dL/dP_j += m_k[j] * dL/dP_(22+k); a joint with coefficient 0 takes no part in the term.  A point has no rotation: a
 * DP_TERM_ALIGN term naming one is refused.
 *
 * Arithmetic.  fp32.  P_(22+k)'s components are formed once per iteration as s = 0; s = fmaf(m_k[j], P_j, s) for j = 0 .. 21 in that
 * order, and the gradient's factor is multiplied by the coefficient, rounded, before the joint's fused multiply-add.  Hence a UNIT point
 * (one coefficient 1, the others 0) gives the bits of the same term naming that joint directly, on every output, and a table without
 * points (n_points = 0 included) gives the bits of dp_optimize_terms / dp_optimize_terms_skeleton / dp_optimize_sequence_terms.
 *
 * The coefficients are HOST data: read during the call, they travel in the launch (graph-capturable, as the term table).  There is no new
 * device input and no new per-frame status.
 *
 * The calls.  dp_optimize_terms_points, dp_optimize_terms_points_skeleton and dp_optimize_sequence_terms_points are dp_optimize_terms,
 * dp_optimize_terms_skeleton (include/dragposer_terms.h) and dp_optimize_sequence_terms (include/dragposer_sequence_constraints.h) with
 * one more argument, `points`, after `terms`; everything else is those calls' contract, argument for argument: per-frame rows [B][4] or,
 * in a sequence, [S][4] / [T][S][4] by dp_seq_extra.row_step, the dp_seq_extra outputs, the statuses, asynchronous, no allocation, no
 * atomics -- two calls on the same inputs give identical bits.
 *
 * Refusals.  Those calls' in their order (a NULL `points` is refused with the NULL arguments); dp_terms is checked as there except that an
 * index up to 21 + DP_MAX_POINTS passes it; then dp_points, after what dp_terms refuses and before the skeleton struct, as
 * DP_ERR_INVALID with a message in dp_last_error and in this order: a bad struct_size or a non-zero reserved0 or reserved1; n_points
 * outside 0..DP_MAX_POINTS; a NULL coeff with n_points > 0; a coefficient that is not finite; a row whose sum (in double) differs from 1
 * by more than 1e-4; a term whose joint_a or joint_b is >= 22 + n_points; a DP_TERM_ALIGN term naming a point.  After everything else,
 * DP_ERR_UNSUPPORTED from a library built without the kernel.
 *
 * Not in holds / tethers / gaps / the latent predictor / dp_live_step / the plug-in: dp_optimize_terms and its relatives, and every other
 * entry point, keep refusing index 22.  Not covered either: dp_optimize_constrained, the dp_w4 / dp_w16 kernels, points of rotations.
 */
#ifndef DRAGPOSER_POINTS_H
#define DRAGPOSER_POINTS_H

#include "dragposer_sequence_constraints.h"
#include "dragposer_terms.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_MAX_POINTS 4

typedef struct dp_points {
    unsigned struct_size; /* sizeof(dp_points) in the caller's translation unit (DP_POINTS_INIT sets it); checked like dp_terms' */
    unsigned reserved0;   /* must be 0 */
    int n_points;         /* 0..DP_MAX_POINTS */
    int reserved1;        /* must be 0 */
    const float* coeff;   /* HOST [n_points][22], read during the call: row k = the coefficients of point k (index 22 + k), sum 1 */
} dp_points;
#define DP_POINTS_INIT {(unsigned)sizeof(dp_points), 0u, 0, 0, (const float*)0}

int dp_optimize_terms_points(dp_ctx* ctx, const dp_batch* in, const dp_params* params, const dp_terms* terms, const dp_points* points,
                             const dp_result* out, void* hip_stream);

int dp_optimize_terms_points_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* params, const dp_terms* terms, const dp_points* points,
                                      const dp_skeleton_in* skel, const dp_result* out, void* hip_stream);

int dp_optimize_sequence_terms_points(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params,
                                      const dp_terms* terms, const dp_points* points, const dp_skeleton_in* skeleton, const dp_seq_state* state,
                                      const dp_seq_step* adjust, const dp_seq_results* out, const dp_seq_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_POINTS_H */
