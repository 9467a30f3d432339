/* dragposer_skeleton.h -- C ABI of libdragposer_hip.so, per-frame skeletons: dp_optimize, dp_forward and dp_optimize_sequence with the
 * performer's bone offsets passed on every call instead of the ones the context was created with.
 *
 * What it replaces in the reference (UPC-ViRVIG/DragPoser, python/src):
 *   DragPose.run(..., offsets, ...) hands `offsets` to fk_rotmat on every call (drag_pose.py:73,111,202,332); eval_drag.py reads them
 *   from each evaluated BVH and run_drag.py from the user's.  The decoder never sees the skeleton, so one trained model serves
 *   performers of any size -- and here one context, and one launch, serves frames (or sequences) of different skeletons.
 *
 * The topology (dp_model.parents) stays the context's: only the bone offsets vary.  Row 0 of every skeleton (the root's OFFSET) is
 * ignored, as it is in dp_model.offsets (the reference's train.py:340 zeroes it).  Everything else is the contract of the call each
 * entry point extends -- dp_optimize, dp_forward, dp_optimize_sequence (include/dragposer.h): asynchronous on the given HIP stream,
 * no allocation, no host synchronisation, the same outputs and status words.  A frame given the context's own offsets gets the bits
 * the plain call gives it.
 *
 * Screening, per frame (per sequence in a sequence launch): a skeleton row 1..21 with a component that is not finite or beyond
 * DP_INPUT_LIMIT in magnitude refuses the frame with DP_STATUS_BAD_STATE (every result NaN, as for a bad z0 / cur_rot).  The refused
 * frame is still computed, with zero in place of the rows a lane found out of range (the frame's other rows as given), so that its
 * arithmetic stays finite; the other frames of the launch -- its wave neighbours included -- are bit-identical to a launch without the fault.
 *
 * Kernels.  The per-frame offsets are a per-lane value of the wave-private kernel (4 frames per wave, DP_KERNEL_W4), loaded in its
 * set-up; its iteration loop is unchanged.  DP_KERNEL_AUTO takes DP_KERNEL_W4 at every batch size here -- beyond 8192 frames (two
 * rounds of 16 frames per CU on a 256-CU device) plain dp_optimize would switch to DP_KERNEL_W16, so such batches run extra rounds
 * of the 4-frames-per-wave kernel (about 1.3x the time of dp_w16 from three rounds on).  DP_KERNEL_W16 is refused
 * (DP_ERR_UNSUPPORTED): its slot map keeps the offsets in per-slot constants.  dp_forward_vjp's per-frame form, with the gradient of the
 * offsets, is dp_forward_vjp_skeleton (include/dragposer_grad.h).  The per-frame forms of dp_optimize_constrained and dp_optimize_terms are
 * dp_optimize_constrained_skeleton (include/dragposer_constraints.h) and dp_optimize_terms_skeleton (include/dragposer_terms.h): one frame
 * per wave there, the frame's bones read in the set-up into the wave's own block; a refused row makes every result of that frame NaN.
 *
 * Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).  DP_ERR_INVALID: a NULL skeleton or NULL
 * `offsets`, a `stride` other than 0 or 66, a bad struct_size or a non-zero reserved0 (checked like dp_grad_in's), and anything the
 * extended call refuses.  DP_ERR_UNSUPPORTED: dp_params.kernel == DP_KERNEL_W16, or a library built without the kernels.
 */
#ifndef DRAGPOSER_SKELETON_H
#define DRAGPOSER_SKELETON_H

#include "dragposer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dp_skeleton_in {
    unsigned struct_size; /* sizeof(dp_skeleton_in) in the caller's translation unit (DP_SKELETON_IN_INIT sets it) */
    unsigned reserved0;   /* must be 0 */
    const float* offsets; /* DEVICE [N][22][3] bone offsets (metres, the OFFSET table of a BVH); row 0 of each skeleton is ignored, as in dp_model.
                             N = n_frames (n_sequences in a sequence launch) when stride = 66, N = 1 when stride = 0.  Read during the launch. */
    int stride;           /* floats between consecutive skeletons: 66 = one per frame (per sequence in a sequence launch), 0 = one for the launch */
} dp_skeleton_in;
#define DP_SKELETON_IN_INIT {(unsigned)sizeof(dp_skeleton_in)} /* dp_skeleton_in s = DP_SKELETON_IN_INIT; s.offsets = ...; s.stride = 66; */
#define DP_SKELETON_STRIDE 66 /* 22 joints x 3 */

/* dp_optimize with per-frame skeletons: frame f uses skeleton f (stride 66) or the single one (stride 0). */
int dp_optimize_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* p, const dp_skeleton_in* skel, const dp_result* out, void* hip_stream);

/* dp_forward with per-frame skeletons. */
int dp_forward_skeleton(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_skeleton_in* skel, const dp_result* out,
                        void* hip_stream);

/* dp_optimize_sequence with one skeleton per SEQUENCE (stride 66) or one for all of them (stride 0), kept for every step of the launch. */
int dp_optimize_sequence_skeleton(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* p,
                                  const dp_skeleton_in* skel, const dp_seq_state* state, const dp_seq_step* step, const dp_seq_results* out,
                                  void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_SKELETON_H */
