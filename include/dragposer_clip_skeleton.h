/* dragposer_clip_skeleton.h -- C ABI of libdragposer_hip.so: the joint clip solve (include/dragposer_clip_lm.h, dragposer_clip_accel.h) and
 * the per-frame Levenberg-Marquardt solver (include/dragposer_lm.h) with the performer's own bone offsets passed on the call, as
 * include/dragposer_skeleton.h passes them to dp_optimize.  What dp_fit_bones (include/dragposer_calibration.h) returns for a performer goes
 * into the only solver that sees the whole clip, and one launch holds clips of performers of different sizes.  Nothing here changes another
 * entry point; DP_VERSION stays.
 *
 * dp_optimize_clip_lm_skeleton.  `accel` NULL: dp_optimize_clip_lm's problem, launch train and workspace (dp_clip_lm_workspace_bytes).
 * `accel` given: dp_optimize_clip_lm_accel's (dp_clip_lm_accel_workspace_bytes); lambda_accel = 0 gives the bits of the NULL form, as it does
 * there.  `skel` is a dp_skeleton_in with its sequence-launch meaning: stride 66 is one skeleton per SEQUENCE (N = n_sequences), held for
 * all T frames of it -- frame t of sequence s, row t S + s of the batch, reads skeleton s; stride 0 is one skeleton for the launch.  Row 0 of
 * a skeleton is never read.  The topology stays the context's.  The offsets are read during the launch, by every pass of the rows kernel: a
 * captured graph sees offsets changed in place between replays.  A sequence given the context's own offsets gets the bits of the plain call.
 *
 * dp_optimize_lm_skeleton.  dp_optimize_lm with the skeleton after the parameters; stride 66 is one skeleton per FRAME (N = n_frames).  It
 * is the T = 1 twin of the clip call: a second-order solve for a batch of mixed performers.  The reported loss's pass in double runs on the
 * frame's own bones too.
 *
 * Kernels.  Only the rows pass of the clip solve sees a bone: dp_clip_rows_skel_kernel (dp_clip_skel.hip) is dp_clip_rows_kernel with each
 * wave's bones taken from global memory into a block of its own (68 floats of LDS per wave: the 66 of a skeleton, padded to 16 bytes), since the waves of a workgroup belong to
 * different sequences.  The block-tridiagonal and block-pentadiagonal chains and the decision kernels are launched as they are.  The launch
 * train, the workspace layout and size, every output, the asynchrony, the absence of atomics, repeatability and graph capture are those of
 * the plain calls.  dp_lm_skel_kernel (dp_lm_skel.hip) is dp_lm_kernel with the same change.  fp32 and bf16-rounded contexts both work.
 *
 * Screening follows dragposer_skeleton.h: a row 1..21 with a component that is not finite or beyond DP_INPUT_LIMIT in magnitude refuses the
 * frame with DP_STATUS_BAD_STATE, every result NaN.  In the clip call every frame of that skeleton's sequence is such a frame (with stride
 * 0: every frame of the launch): no step runs for the sequence and info[s] carries DP_CLIP_REFUSED_FRAME, as for any refused frame.  The
 * other sequences (frames, in dp_optimize_lm_skeleton) are bit-identical to a launch without the fault.
 *
 * Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).  Refusals, DP_ERR_INVALID, in this order: the plain
 * call's own, in their order -- for the clip call dp_optimize_clip_lm's up to and including lambda_smooth, then with `accel` given a bad
 * dp_clip_accel_params.struct_size and lambda_accel negative or not finite; for dp_optimize_lm_skeleton dp_optimize_lm's, all of them --
 * then dp_skeleton_in's as dp_optimize_skeleton states them: a NULL skeleton, its struct_size, a non-zero reserved0, NULL `offsets`, a
 * stride other than 0 or 66; then, in the clip call, a NULL workspace or one shorter than the size function of the form chosen.  Then
 * DP_ERR_UNSUPPORTED from the test-only library or a library linked without the units, DP_ERR_DEVICE from a context without a device image.
 *
 * Not covered: skeletons in dp_optimize_sequence_lm, dp_optimize_lm_terms and dp_optimize_sequence_lm_terms; a skeleton per frame inside one
 * sequence of the clip call (bones that change while a clip plays); DragPose and the plug-in.
 */
#ifndef DRAGPOSER_CLIP_SKELETON_H
#define DRAGPOSER_CLIP_SKELETON_H

#include "dragposer_clip_accel.h"
#include "dragposer_skeleton.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dp_optimize_clip_lm (accel == NULL) or dp_optimize_clip_lm_accel with one skeleton per sequence (stride 66) or one for the launch (stride 0) */
int dp_optimize_clip_lm_skeleton(dp_ctx* ctx, const dp_batch* in, int n_sequences, const dp_clip_lm_params* params, const dp_clip_accel_params* accel,
                                 const dp_skeleton_in* skel, const dp_result* out, const dp_clip_lm_extra* extra, void* hip_stream);

/* dp_optimize_lm with one skeleton per frame (stride 66) or one for the launch (stride 0) */
int dp_optimize_lm_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_lm_params* params, const dp_skeleton_in* skel, const dp_result* out,
                            const dp_lm_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_CLIP_SKELETON_H */
