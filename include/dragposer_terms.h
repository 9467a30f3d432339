/* dragposer_terms.h -- C ABI of libdragposer_hip.so, user-defined constraint terms: dp_optimize with a table of up to DP_MAX_TERMS extra
 * loss terms, each one of three primitives, in one launch.  The reference's four `# Additional Losses` terms (drag_pose.py:129-183,
 * include/dragposer_constraints.h) are one such table; so are a hand above a table, a foot held where it touched down, stairs, knees
 * kept apart or a head facing a given direction.
 *
 * Notation, per frame f: g = global_pos[f]; P_j, G_j what dp_forward returns as pos and rot of joint j; W_j = g + P_j (the world
 * position); h(v) = v with its up_axis component set to 0 when the term's DP_TERM_DROP_UP flag is set, h(v) = v otherwise; s_f the
 * term's per-frame factor (1 without a per-frame row).  Each term adds weight * s_f * T to the loss that is back-propagated and to the
 * total the while-condition's loss_incr test uses:
 *   DP_TERM_PLANE     (joint_a; joint_b must be -1)  d = dir . (W_a - point);  T = d^2, or relu(-d)^2 with DP_TERM_ONE_SIDED (the joint
 *                     is kept on the normal's side of the plane without being pulled onto it)
 *   DP_TERM_DISTANCE  (joint_a with joint_b, or with point when joint_b = -1)  q = |h(P_a - P_b)|^2 (g cancels) or |h(W_a - point)|^2;
 *                     T = relu(q - hi^2) + relu(lo^2 - q) with lo = p0, hi = p1.  lo = hi = 0 is a soft pin (or the reference's
 *                     colinear term when DROP_UP)
 *   DP_TERM_ALIGN     (joint_a with joint_b, or with dir when joint_b = -1)  u = h(G_a axis_a), v = h(G_b axis_b) or h(dir);  T = 0 if
 *                     |u| <= p0 (threshold), otherwise c = u/|u| . v/|v| + p1 (margin) and T = (1 - min(1, c))^2.  v is not
 *                     screened: a v of length 0 makes the frame's loss NaN (as the reference's head_hips_forward would)
 * A term may name the same joint twice; the gradients then add.  Flags a type does not use (ONE_SIDED outside PLANE, DROP_UP on a
 * PLANE) are accepted and ignored.  A term with weight 0 is off: it is not evaluated, its per-frame row is not read, its loss slot is 0.
 *
 * Per-frame rows.  dp_term.per_frame, when not NULL, is a DEVICE array [B][4] of rows (x, y, z, s): (x, y, z) replaces `point` (PLANE and
 * point-DISTANCE) or `dir` (world ALIGN; it need not be unit length there, v is normalised) and is ignored by joint-to-joint terms; s is
 * s_f (0 switches the term off for that frame).  A row of an active term with a component that is not finite or beyond DP_INPUT_LIMIT in
 * magnitude, or with s < 0, refuses the frame with DP_STATUS_BAD_TARGETS (z and loss NaN, as for a bad tracker target); the other
 * frames of the launch are bit-identical to a launch without that row's fault.  The rows are read once per launch: a captured graph
 * sees the contents at replay time.
 *
 * Everything else is dp_optimize_constrained's contract, per frame: Adam, early_stop (dp_params) and the outputs (dp_result) are
 * dp_optimize's; the while-condition's loss_incr uses the total above; dp_params.kernel is ignored; n_iter may be up to DP_MAX_ITERS;
 * the rotation loss is the element-wise |G - T|_F^2 (DP_STATUS_TARGET_NOT_ROTATION is never set); a refused global_pos (read only
 * when an active PLANE or point-DISTANCE term exists) is DP_STATUS_BAD_STATE.  Asynchronous on the given HIP stream, no allocation, no
 * host synchronisation; the term table is read during the call and its values travel in the launch (graph-capturable); no atomics:
 * two calls on the same inputs give identical bits.
 * Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).  DP_ERR_INVALID: NULL ctx / batch / params /
 * terms / result; a bad struct_size or a non-zero reserved0; n_terms outside 0..DP_MAX_TERMS, a NULL `terms` with n_terms > 0, up_axis
 * outside 0..2; an unknown type or flag bit; joint_a outside 0..21, joint_b outside -1..21, a PLANE with joint_b != -1; a negative or
 * non-finite weight, a non-finite point / dir / axis / p0 / p1, a negative lo, hi or threshold, lo > hi; a dir that is not unit length
 * within 1e-4 where it is read (a PLANE's normal; a world ALIGN's direction unless a per-frame row replaces it); a zero axis_a (ALIGN) or
 * axis_b (joint-to-joint ALIGN); a NULL global_pos while an active PLANE or point-DISTANCE term exists; anything dp_optimize refuses.
 * DP_ERR_UNSUPPORTED from a library built without the kernel.
 *
 * Per-frame skeletons.  dp_optimize_terms_skeleton is the same call with the performer's bone offsets passed as a dp_skeleton_in
 * (include/dragposer_skeleton.h): stride 66 = frame f uses skeleton f, stride 0 = one skeleton for the launch; the topology stays the
 * context's and row 0 of every skeleton is never read.  A frame given the context's own offsets gets dp_optimize_terms' bits.  A row 1..21
 * with a component that is not finite or beyond DP_INPUT_LIMIT refuses that frame: every result NaN, loss_terms included, iters as for a
 * bad z0, status DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE; the other frames are bit-identical to a launch without the fault.
 * Refusals, in this order: NULL ctx; NULL batch / params / terms / result; a NULL skeleton; what dp_params and dp_result refuse; what
 * dp_terms and its table refuse (above); the skeleton struct -- a bad struct_size, a non-zero reserved0, NULL `offsets`, a stride other than
 * 0 or 66 (checked like dp_optimize_skeleton's); what the batch and Adam's parameters refuse (all DP_ERR_INVALID); then
 * DP_ERR_UNSUPPORTED from a library built without the kernel.
 */
#ifndef DRAGPOSER_TERMS_H
#define DRAGPOSER_TERMS_H

#include "dragposer.h"
#include "dragposer_skeleton.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_MAX_TERMS 16
enum { DP_TERM_PLANE = 1, DP_TERM_DISTANCE = 2, DP_TERM_ALIGN = 3 };
enum { DP_TERM_ONE_SIDED = 1, DP_TERM_DROP_UP = 2 }; /* flags */

typedef struct dp_term {
    int type;           /* DP_TERM_PLANE / _DISTANCE / _ALIGN */
    int joint_a;        /* 0..21 */
    int joint_b;        /* 0..21, or -1: the term's point (DISTANCE) or dir (ALIGN) instead of a second joint; PLANE: -1 */
    int flags;          /* DP_TERM_ONE_SIDED | DP_TERM_DROP_UP */
    float weight;       /* >= 0, finite; 0 = off */
    float point[3];     /* PLANE: a point of the plane; DISTANCE with joint_b = -1: the point (world, metres) */
    float dir[3];       /* PLANE: unit normal; ALIGN with joint_b = -1: unit world direction */
    float axis_a[3];    /* ALIGN: local axis of joint_a (non-zero) */
    float axis_b[3];    /* ALIGN: local axis of joint_b (non-zero when joint_b >= 0) */
    float p0, p1;       /* DISTANCE: lo, hi (0 <= lo <= hi); ALIGN: threshold (>= 0), margin; PLANE: unused */
    const float* per_frame; /* DEVICE [B][4] or NULL: (vector, weight factor s_f) per frame, see above */
} dp_term;
#define DP_TERM_INIT                                                                                                             \
    {0, 0, -1, 0, 0.f, {0.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}, {0.f, 0.f, 1.f}, 0.f, 0.f, (const float*)0}

typedef struct dp_terms {
    unsigned struct_size; /* sizeof(dp_terms) in the caller's translation unit (DP_TERMS_INIT sets it); checked like dp_constraints' */
    unsigned reserved0;   /* must be 0 */
    int n_terms;          /* 0..DP_MAX_TERMS (0: dp_optimize's loss, in this kernel) */
    int up_axis;          /* 0, 1 or 2: the component DP_TERM_DROP_UP zeroes (1) */
    const dp_term* terms; /* HOST [n_terms], read during the call */
    const float* global_pos; /* DEVICE [B][3]; required iff an active PLANE or point-DISTANCE term exists */
    float* loss_terms;       /* DEVICE [B][n_terms] or NULL: each weighted term (weight * s_f * T) of the last forward pass */
} dp_terms;
#define DP_TERMS_INIT {(unsigned)sizeof(dp_terms), 0u, 0, 1, (const dp_term*)0, (const float*)0, (float*)0}

int dp_optimize_terms(dp_ctx* ctx, const dp_batch* in, const dp_params* params, const dp_terms* terms, const dp_result* out,
                      void* hip_stream);

/* dp_optimize_terms with per-frame skeletons: frame f uses skeleton f (stride 66) or the single one (stride 0). */
int dp_optimize_terms_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* params, const dp_terms* terms, const dp_skeleton_in* skel,
                               const dp_result* out, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_TERMS_H */
