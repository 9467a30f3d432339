/* dragposer_grad.h -- C ABI of libdragposer_hip.so, gradient entry point: the vector-Jacobian product of dp_forward.
 *
 * What it replaces in the reference (UPC-ViRVIG/DragPoser, python/src):
 *   dp_forward_vjp   loss.backward() through Decoder.forward (autoencoder.py:224-256) and the FK part of DragPose.loss
 *                    (drag_pose.py:84-113, with from_root_quat_to_rotmat + fk_rotmat, utils.py:80-149), for ANY loss on their
 *                    outputs: the caller's loss supplies the upstream gradients, this returns dL/dz and dL/dcur_rot.  What lets
 *                    a user add a constraint ("constraints can be dynamically defined as losses", docs/index.html:174) the
 *                    way DragPose.loss (drag_pose.py:66-194) does, without a kernel of its own.
 *
 * The function differentiated is exactly what dp_forward computes, as torch autograd derives it through the reference:
 *   the folded decoder with LeakyReLU(0.2) after its first two layers (slope 1 only where the pre-activation is > 0);
 *   de-normalisation, per-joint quaternion normalisation and re-normalisation into `pose` (autoencoder.py:242-250);
 *   `disp` = the de-normalised displacement (drag_pose.py:84-85);
 *   `world_rot` = cur_rot (x) q_root with cur_rot used as given, NOT normalised (drag_pose.py:88);
 *   `world_disp` = world_rot applied to disp (drag_pose.py:102);
 *   the FK chain: `pos`, `rot` (utils.py:95-105,140-146).
 * Conventions are dragposer.h's (w-first quaternions, fp32, row-major, frame-major, 22 joints, latent 24); every skeleton
 * dp_create accepts is supported, with the weights of the context's own folded model (fp32 or bf16-rounded).
 *   dp_forward_vjp_skeleton   the same with the performer's bone offsets passed per call (include/dragposer_skeleton.h: one skeleton per
 *                    frame or one for the launch, the context's topology) -- the reference's fk_rotmat(..., offsets) -- and, on request,
 *                    the gradient with respect to those offsets as well.
 *
 * The forward pass is recomputed inside the kernel: nothing is saved between dp_forward and dp_forward_vjp, and they may be
 * called in any order.  Asynchronous on the given HIP stream, no allocation, no host synchronisation, no host<->device copy
 * of caller data (graph-capturable); no atomics: two calls on the same inputs give bit-identical results.  Returns DP_OK or
 * a negative dp_status and never throws; message: dp_last_error(ctx).
 */
#ifndef DRAGPOSER_GRAD_H
#define DRAGPOSER_GRAD_H

#include "dragposer.h"
#include "dragposer_skeleton.h" /* dp_skeleton_in */

#ifdef __cplusplus
extern "C" {
#endif

/* Upstream gradients dL/d(output), DEVICE pointers with the shapes of dp_result's fields; NULL = zero. */
typedef struct dp_grad_in {
    unsigned struct_size; /* sizeof(dp_grad_in) in the caller's translation unit (DP_GRAD_IN_INIT sets it); checked like dp_result's */
    unsigned reserved0;   /* must be 0 */
    const float* pose;       /* [B][88] */
    const float* disp;       /* [B][3]  (de-normalised) */
    const float* world_disp; /* [B][3]  */
    const float* world_rot;  /* [B][4]  */
    const float* pos;        /* [B][22][3] */
    const float* rot;        /* [B][22][9] */
} dp_grad_in;
#define DP_GRAD_IN_INIT {(unsigned)sizeof(dp_grad_in)} /* dp_grad_in g = DP_GRAD_IN_INIT;  (every gradient zero) */

/* dz [B][24] (required), dcur_rot [B][4] and status [B] (DP_STATUS_* bits) may be NULL; z / cur_rot [B][24] / [B][4] as for
 * dp_forward.  Per frame: a z or cur_rot that is not finite or beyond DP_INPUT_LIMIT in magnitude is refused -- the frame's
 * gradients are NaN and its status DP_STATUS_BAD_STATE (dp_forward's rule); a non-finite dz gives DP_STATUS_NONFINITE_RESULT.
 * The other frames are not affected.  DP_ERR_INVALID: NULL ctx / z / cur_rot / g / dz, n_frames <= 0, a bad struct_size;
 * DP_ERR_UNSUPPORTED from a library built without the kernel. */
int dp_forward_vjp(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_grad_in* g,
                   float* dz, float* dcur_rot, int* status, void* hip_stream);

/* dp_forward_vjp with per-frame skeletons: frame f's bones are row 1..21 of skeleton f (skel->stride 66) or of the single one (stride 0),
 * under dragposer_skeleton.h's rules (row 0 ignored, the topology the context's).  Everything else is dp_forward_vjp's contract.
 * doffsets: NULL, or a DEVICE [n_frames][22][3] that receives dL/d(offsets) of each frame -- written per frame even when stride is 0 (the
 * caller sums over the frames); row 0 is written as 0 (no output depends on it).
 * Screening, per frame (dp_forward_skeleton's rule): a skeleton row 1..21 with a component that is not finite or beyond DP_INPUT_LIMIT in
 * magnitude refuses the frame -- status DP_STATUS_BAD_STATE (dp_forward_vjp's word for a refused z), dz, dcur_rot and every row of its
 * doffsets NaN.  The refused frame is computed with zero in place of the bad rows, so its arithmetic stays finite; every other frame,
 * lane neighbours included, is bit-identical to a launch without the fault.  Row 0 is never read: a NaN there leaves the frame clean.
 * Bits: with the context's own skeleton (stride 0 or 66), dz, dcur_rot and status equal dp_forward_vjp's bits; a frame given skeleton X
 * gets the bits dp_forward_vjp gives it on a context created with X.
 * DP_ERR_INVALID: whatever dp_forward_vjp refuses, a NULL skeleton or NULL offsets, a stride other than 0 or 66, a bad struct_size or a
 * non-zero reserved0 of the skeleton; DP_ERR_UNSUPPORTED from a library built without the kernel. */
int dp_forward_vjp_skeleton(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_skeleton_in* skel,
                            const dp_grad_in* g, float* dz, float* dcur_rot, float* doffsets, int* status, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_GRAD_H */
