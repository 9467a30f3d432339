/* dragposer_calibration.h -- C ABI of libdragposer_hip.so, bone lengths from tracker data: dp_fit_bones.  Every per-frame-skeleton call
 * (include/dragposer_skeleton.h) takes the performer's [22][3] offsets; this call makes them from frames of tracker data, without a BVH
 * file of the performer.
 *
 * The problem.  For fixed joint rotations a joint's position is linear in the bones,
 *     P_j = world_disp + sum over the bones b on the path 0 -> j of G_parent(b) off_b
 * (G: the global rotations dp_forward returns as `rot`).  With every bone tied to a group, off_b = s_g(b) base_b (a bone whose group is
 * -1 stays base_b), the K scales s that minimise
 *     sum over the frames f of loss_pos_f(s)  +  ridge |s - prior|^2
 * (loss_pos: include/dragposer.h's, sum over the E_f tracked joints of w_pos |P_t - tgt_pos_t|^2 / (3 E_f)) solve a K x K linear
 * system.  A tracked joint t of frame f gives 3 rows of K + 1 columns, each times sqrt(w_pos,t / (3 E_f)):
 *     column g < K   sum over the path's bones of group g of G_parent(b) base_b
 *     column K       tgt_pos_t - world_disp - (the same sum over the path's bones of group -1)
 * and the call forms M = sum over the frames of [A b]^T [A b]: N = A^T A (rows and columns < K), g = A^T b (column K), b^T b (the corner).
 * Joint 0, and a tracked joint whose path holds no grouped bone, contribute to b^T b only.  Then H = N + ridge I, rhs = g + ridge prior,
 * H s = rhs by Cholesky without pivoting.  The rotations are those of decode + FK of in->z0 under in->cur_rot on the context's model:
 * alternating this call with dp_optimize_skeleton (z0 = the latents it returned, offsets = this call's) is block coordinate descent on
 * dp_optimize's loss, whose rotation and latent terms do not depend on the bones.
 *
 * Inputs.  dp_batch: z0 (the latent each frame is evaluated at), cur_rot, tgt_pos, w and tracked as everywhere else; z_tgt and tgt_rot may
 * be NULL and are not read.  dp_bone_fit: every HOST field is copied into the kernels' argument block, so a call makes no host-to-device
 * copy and can be captured in a graph; `workspace` is DEVICE memory of at least dp_fit_bones_workspace_bytes(n_frames) bytes that the
 * caller owns (written by the first kernel, read by the second; its contents before the call do not matter).
 *
 * Outputs (dp_bone_fit_result; DEVICE, every pointer but `scales` may be NULL; any subset has the bits of the whole):
 *   scales  [K] float    the fitted scales
 *   offsets [22][3]      base_j * s_g(j), one rounded product per component; base_j for group -1; row 0 zero.  With stride 0 it is a
 *                        dp_skeleton_in for the next launch, with no host round trip
 *   normal  [K+1][K+1]   double: M as above, summed over the frames that were used (no ridge)
 *   rms     [2] float    sqrt(q(s) / frames used) at s = prior and at s = scales, q(s) = b^T b - 2 s^T g + s^T N s = the summed loss_pos
 *                        (a negative q from rounding reads as 0); both 0 when no frame was used
 *   info    [2] int      frames used, DP_FIT_* flag bits
 *   status  [B] int      per frame, include/dragposer.h: DP_STATUS_BAD_STATE (z0 or cur_rot refused), DP_STATUS_BAD_TARGETS (a tracked
 *                        joint's tgt_pos or one of its two weights refused), else 0
 * A refused frame contributes nothing and is not counted, and neither is a frame without a tracked joint; the other frames' part is
 * bit-identical to a launch without it.  DP_FIT_NO_FRAMES: no frame was used -- scales = prior.  DP_FIT_SINGULAR: a Cholesky pivot of
 * N + ridge I was <= 0 or not finite (a group that no tracked joint's path crosses, at ridge 0) -- scales = prior.  In both cases offsets
 * follow from those scales.
 *
 * Arithmetic.  The forward pass and the rows are fp32, M is accumulated per frame on v_mfma_f32_16x16x4_f32; the frames of a workgroup are
 * added in fp32 in a fixed order and the workgroups' partial sums in double in index order, and the solve is in double.  No atomics: two
 * calls on the same inputs give identical bits.  Asynchronous on the given HIP stream (two kernels, one behind the other): no allocation,
 * no host synchronisation, graph-capturable.  Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).
 *
 * Refusals, DP_ERR_INVALID, in this order: (1) NULL ctx; NULL batch, fit or result; dp_bone_fit.struct_size / reserved0;
 * dp_bone_fit_result.struct_size / reserved0; a NULL `scales`; (2) n_groups outside 1..DP_FIT_MAX_GROUPS; (3) a NULL `groups` or an entry
 * 1..21 outside -1..n_groups-1 (entry 0 is ignored); (4) a group without a bone; (5) a `base`, `prior` or `ridge` that is not finite, or a
 * negative ridge; (6) a workspace that is NULL or smaller than dp_fit_bones_workspace_bytes(n_frames); (7) what the batch refuses
 * (n_frames <= 0, a NULL z0, cur_rot, tgt_pos, w or tracked).  Then DP_ERR_UNSUPPORTED from the test-only library, DP_ERR_DEVICE from a
 * context without a device image.
 *
 * Not covered: a fit per sequence in one launch (one call fits one performer from all its frames); the Unity plug-in; bone directions
 * (only lengths, by group, are fitted); rotation targets (they do not depend on the bones).
 */
#ifndef DRAGPOSER_CALIBRATION_H
#define DRAGPOSER_CALIBRATION_H

#include <stddef.h>

#include "dragposer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_FIT_MAX_GROUPS 24
#define DP_FIT_NO_FRAMES 1
#define DP_FIT_SINGULAR 2

typedef struct dp_bone_fit {
    unsigned struct_size; /* sizeof(dp_bone_fit) in the caller's translation unit (DP_BONE_FIT_INIT sets it) */
    unsigned reserved0;   /* must be 0 */
    int n_groups;         /* K in 1..DP_FIT_MAX_GROUPS */
    float ridge;          /* >= 0, finite */
    const int* groups;    /* HOST [22]: bone j's group in -1..K-1 (-1: the bone stays at base); entry 0 is ignored */
    const float* base;    /* HOST [22][3], or NULL: the context's bones */
    const float* prior;   /* HOST [K], or NULL: ones */
    void* workspace;      /* DEVICE, dp_fit_bones_workspace_bytes(n_frames) bytes */
    size_t workspace_bytes;
} dp_bone_fit;
#define DP_BONE_FIT_INIT {(unsigned)sizeof(dp_bone_fit), 0u, 1, 1.0e-3f, (const int*)0, (const float*)0, (const float*)0, (void*)0, (size_t)0}

typedef struct dp_bone_fit_result {
    unsigned struct_size; /* sizeof(dp_bone_fit_result) in the caller's translation unit (DP_BONE_FIT_RESULT_INIT sets it) */
    unsigned reserved0;   /* must be 0 */
    float* scales;        /* DEVICE [K], required */
    float* offsets;       /* DEVICE [22][3] or NULL */
    double* normal;       /* DEVICE [K+1][K+1] or NULL */
    float* rms;           /* DEVICE [2] or NULL */
    int* info;            /* DEVICE [2] or NULL: frames used, DP_FIT_* bits */
    int* status;          /* DEVICE [B] or NULL */
} dp_bone_fit_result;
#define DP_BONE_FIT_RESULT_INIT {(unsigned)sizeof(dp_bone_fit_result), 0u, (float*)0, (float*)0, (double*)0, (float*)0, (int*)0, (int*)0}

size_t dp_fit_bones_workspace_bytes(int n_frames); /* 0 for n_frames <= 0 */
int dp_fit_bones(dp_ctx* ctx, const dp_batch* in, const dp_bone_fit* fit, const dp_bone_fit_result* out, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_CALIBRATION_H */
