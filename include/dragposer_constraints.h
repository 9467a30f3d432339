/* dragposer_constraints.h -- C ABI of libdragposer_hip.so, constrained optimisation: dp_optimize with the four extra loss terms the
 * reference ships in DragPose.loss's `# Additional Losses` block (drag_pose.py:129-183), in one launch.
 *
 * What it replaces in the reference (UPC-ViRVIG/DragPoser, python/src): DragPose.run's optimise loop (drag_pose.py:296-355) with the
 * block un-commented -- its terms added to the loss that is back-propagated and to the total the while-condition's loss_incr test uses
 * (drag_pose.py:338,354).  Per frame b, with g = global_pos[b] (the reference's current_global_pos), P_j / G_j dp_forward's pos / rot,
 * h(v) = v with its up component set to 0, f = fwd_axis:
 *   total = loss_pos + lambda_rot loss_rot + lambda_tmp loss_tmp (as dp_optimize) + sum_k w_k term_k, where
 *   feet_floor          mean over floor_joints of (g_up + P_j,up - floor_level)^2; with floor_one_sided = 1 relu(floor_level - g_up - P_j,up)^2
 *                       instead (a ground plane: keeps the feet above the floor without pulling them down)
 *   head_hips_forward   a = h(G_head f); if |a| > fwd_threshold: b = h(G_hips f) / |h(G_hips f)|, term (1 - min(1, a/|a| . b + fwd_margin))^2;
 *                       otherwise 0.  The reference takes quat.from_matrix(G) (x) f, which is G f for a rotation matrix -- what G is
 *                       whenever cur_rot is a unit quaternion, as every reference caller passes it; G f is what is computed
 *   head_hips_colinear  |h(P_head - P_hips)|^2 (g cancels)
 *   hips_feet_colinear  sum over foot_joints of max(|h(P_hips - P_j)|^2 - feet_radius^2, 0)
 * The reference's block as written is every w_k = 1 with the defaults below (the Xsens skeleton).
 *
 * Adam, early_stop (dp_params) and the outputs (dp_result) are dp_optimize's; the while-condition's loss_incr uses the total above.
 * dp_params.kernel is ignored; Adam's bias corrections are computed on the device, so n_iter may be up to DP_MAX_ITERS.  The rotation
 * loss is the reference's element-wise |G - T|_F^2 on the matrices themselves: DP_STATUS_TARGET_NOT_ROTATION is never set here.
 * Per frame, dp_result.status is dp_optimize's contract; a refused global_pos (read only when w_feet_floor != 0) is DP_STATUS_BAD_STATE.
 * A bad frame leaves the other frames bit-identical.  Asynchronous on the given HIP stream, no allocation, no host synchronisation,
 * no copy of caller data (graph-capturable); no atomics: two calls on the same inputs give identical bits.
 * Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).  DP_ERR_INVALID: NULL ctx / batch / params /
 * result, a bad struct_size or reserved0, a joint index outside 0..21, up_axis outside 0..2, a negative or non-finite weight, a NULL
 * global_pos while the floor term is on, anything dp_optimize refuses.  DP_ERR_UNSUPPORTED from a library built without the kernel.
 *
 * Per-frame skeletons.  dp_optimize_constrained_skeleton is the same call with the performer's bone offsets passed as a dp_skeleton_in
 * (include/dragposer_skeleton.h): stride 66 = frame f uses skeleton f, stride 0 = one skeleton for the launch; the topology stays the
 * context's and row 0 of every skeleton is never read.  A frame given the context's own offsets gets dp_optimize_constrained's bits.  A row
 * 1..21 with a component that is not finite or beyond DP_INPUT_LIMIT refuses that frame: every result NaN, loss_extra included, iters as
 * for a bad z0, status DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE; a frame is a wave that shares nothing, so the other frames are
 * bit-identical to a launch without the fault.  Refusals, in this order: NULL ctx; NULL batch / params / constraints / result; a NULL
 * skeleton; what dp_params and dp_result refuse; what dp_constraints refuses (above); the skeleton struct -- a bad struct_size, a non-zero
 * reserved0, NULL `offsets`, a stride other than 0 or 66 (checked like dp_optimize_skeleton's); what the batch and Adam's parameters
 * refuse (all DP_ERR_INVALID); then DP_ERR_UNSUPPORTED from a library built without the kernel.
 */
#ifndef DRAGPOSER_CONSTRAINTS_H
#define DRAGPOSER_CONSTRAINTS_H

#include "dragposer.h"
#include "dragposer_skeleton.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dp_constraints {
    unsigned struct_size; /* sizeof(dp_constraints) in the caller's translation unit (DP_CONSTRAINTS_INIT sets it); checked like dp_result's */
    unsigned reserved0;   /* must be 0 */
    float w_feet_floor, w_head_hips_forward, w_head_hips_colinear, w_hips_feet_colinear; /* >= 0, finite; 0 = off */
    int floor_joints[2];  /* feet_floor's joints (Xsens: 4, 8) */
    int foot_joints[2];   /* hips_feet_colinear's joints (3, 7) */
    int head_joint;       /* 13 */
    int hips_joint;       /* 0 */
    int up_axis;          /* 0, 1 or 2 (1) */
    int floor_one_sided;  /* 0: the reference's two-sided feet_floor; 1: relu(floor_level - height)^2 */
    float floor_level;    /* 0 */
    float fwd_axis[3];    /* (0, 0, 1) */
    float fwd_threshold;  /* 0.5 */
    float fwd_margin;     /* 0.2 */
    float feet_radius;    /* 0.2 */
    const float* global_pos; /* DEVICE [B][3]; required iff w_feet_floor != 0 */
    float* loss_extra;       /* DEVICE [B][4] or NULL: the four weighted terms of the last forward pass, in the order of the weights */
} dp_constraints;
#define DP_CONSTRAINTS_INIT                                                                                                      \
    {(unsigned)sizeof(dp_constraints), 0u, 0.f, 0.f, 0.f, 0.f, {4, 8}, {3, 7}, 13, 0, 1, 0, 0.f, {0.f, 0.f, 1.f}, 0.5f, 0.2f, 0.2f, \
     (const float*)0, (float*)0}

int dp_optimize_constrained(dp_ctx* ctx, const dp_batch* in, const dp_params* params, const dp_constraints* cons, const dp_result* out,
                            void* hip_stream);

/* dp_optimize_constrained with per-frame skeletons: frame f uses skeleton f (stride 66) or the single one (stride 0). */
int dp_optimize_constrained_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* params, const dp_constraints* cons,
                                     const dp_skeleton_in* skel, const dp_result* out, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_CONSTRAINTS_H */
