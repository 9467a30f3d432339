/* dragposer_lm.h -- C ABI of libdragposer_hip.so, a second-order solver: dp_optimize's per-frame problem solved by Gauss-Newton steps with
 * Levenberg-Marquardt damping instead of Adam, in one launch.  The loss of a frame is a plain sum of squares in 24 unknowns; a step pushes
 * the latent's 24 tangent columns through the folded decoder on the matrix pipe, forms the 24 x 24 normal equations, solves them and tries
 * the result once.  Adam stays the default solver of every other entry point; nothing here changes one of them.
 *
 * The algorithm, per frame with E tracked joints (P_t, G_t: what dp_forward returns as pos and rot of tracked joint t):
 *   residuals  r_pos,t = sqrt(w_pos,t / (3E)) (P_t - tgt_pos_t)                   3 rows per tracker
 *              r_rot,t = sqrt(lambda_rot w_rot,t / (9E)) (G_t - tgt_rot_t)         9 rows per tracker: the reference's element-wise form
 *                        (drag_pose.py:121-124), not dp_optimize's quaternion form -- their Gauss-Newton matrices differ
 *              r_tmp   = sqrt(lambda_tmp / 24) (z - z_tgt)                        24 rows
 *              L = |r|^2 is the reference's total loss; its three parts are dp_result.loss's three numbers.
 *   J = dr/dz  through the folded decoder (the LeakyReLU slope at a pre-activation of exactly 0 is 0.2, as in the other kernels' backward),
 *              the de-normalisation, the per-joint quaternion normalisation, the incremental root rotation and FK.
 *   step       A = J^T J, g = J^T r, H = A + mu diag(A); H delta = -g by Cholesky without pivoting.  A pivot that is <= 0 or not finite
 *              rejects the step.  Trial z' = z + delta, L' = L(z'): accepted iff L' < L (a NaN rejects).
 *              accepted: z <- z', mu <- max(mu mu_down, mu_min);  rejected: mu <- min(mu mu_up, mu_max).
 *   A step is one trial, accepted or not; n_steps of them run.  With early_stop the frame ends BEFORE a step when loss_pos <= stop_eps_pos
 *   and lambda_rot loss_rot <= stop_eps_rot (the first half of the reference's while-condition), or after a rejection at mu = mu_max.
 *   The loss never increases.  After a rejection z has not moved: the kernel keeps A and g and repeats only the solve.
 *
 * Outputs.  Every dp_result array (z, z_pre = z, pose, disp, world_disp, world_rot, pos, rot, loss) belongs to the returned z, so
 * dp_sequence_advance consumes the result unchanged; iters is the number of steps executed.  `loss` and `loss0`, when asked for, are the
 * loss at that latent evaluated once more in double on the same fp32 weights (about 7 us each per launch): the steps are decided on fp32
 * passes, whose loss near the solution is good to 1e-4 only, so "accepted iff L' < L" holds in that arithmetic and the reported pair may
 * disagree with it in its last digits.  dp_result.clock is ignored.  dp_lm_extra (may be
 * NULL, and every pointer in it may be NULL): `mu` [B] in/out -- the damping a frame starts from and ends with, kept by the caller from
 * frame to frame (NULL: every frame starts at mu0; a value that is not finite or outside [mu_min, mu_max] is read as mu0);
 * `n_accepted` [B]; `loss0` [B][3], the loss at z0.
 *
 * Status (dp_result.status, include/dragposer.h).  DP_STATUS_BAD_STATE: z0 or cur_rot refused -- every result NaN, iters 0, mu unchanged.
 * DP_STATUS_BAD_TARGETS: a tracked joint's target or weight, or z_tgt, refused -- no step runs: z, z_pre, loss and loss0 are NaN (with
 * DP_STATUS_NONFINITE_RESULT), the pose results are those of the warm start z0, iters 0, mu unchanged.  DP_STATUS_TARGET_NOT_ROTATION: a
 * tracked joint's tgt_rot is not a rotation matrix within DP_ROTATION_TOL -- a report, the element-wise loss is computed as given.  A frame
 * is a wave: the other frames of the launch are bit-identical to a launch without the fault.
 *
 * The call is asynchronous on the given HIP stream: no allocation, no host synchronisation, graph-capturable (the parameters travel in the
 * launch; `mu` is read and written at replay time).  No atomics: two calls on the same inputs give identical bits.  fp32 and bf16-rounded
 * contexts both work.  Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).
 * Refusals, DP_ERR_INVALID, in this order: NULL ctx; NULL batch or params; dp_lm_params.struct_size; what dp_result refuses;
 * dp_lm_extra.struct_size / reserved0; n_steps outside 1..DP_LM_MAX_STEPS; a lambda that is not finite or negative, a mu, factor or stop
 * threshold that is not finite; mu_down outside (0, 1); mu_up <= 1; mu_min <= 0 or mu_min > mu_max; mu0 outside [mu_min, mu_max]; what the batch
 * refuses (n_frames, a NULL input array).  Then DP_ERR_UNSUPPORTED from the test-only library, DP_ERR_DEVICE from a context without a
 * device image.
 *
 * Not covered: points (include/dragposer_points.h), holds, gaps and tethers in the LM loss, per-frame skeletons, dp_live_step and the
 * plug-in.  A term table in the LM loss is dp_optimize_lm_terms (include/dragposer_lm_terms.h: the table's rows in [J | r], its relu bands by
 * their active sets).  The frame loop on the device is dp_optimize_sequence_lm's (include/dragposer_sequence_lm.h): a clip in one launch,
 * the bits of this call followed by dp_sequence_advance, frame by frame -- and with a term table dp_optimize_sequence_lm_terms'
 * (include/dragposer_sequence_lm_terms.h).
 */
#ifndef DRAGPOSER_LM_H
#define DRAGPOSER_LM_H

#include "dragposer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_LM_MAX_STEPS 64

typedef struct dp_lm_params {
    unsigned struct_size; /* sizeof(dp_lm_params) in the caller's translation unit (DP_LM_PARAMS_INIT sets it) */
    int n_steps;          /* 1..DP_LM_MAX_STEPS trials per frame */
    float lambda_rot, lambda_tmp; /* >= 0, finite */
    float mu0;            /* the damping a frame starts from when dp_lm_extra.mu is NULL */
    float mu_up, mu_down; /* > 1; in (0, 1) */
    float mu_min, mu_max; /* 0 < mu_min <= mu0 <= mu_max */
    int early_stop;       /* 1: a frame ends early as described above */
    float stop_eps_pos, stop_eps_rot;
} dp_lm_params;
#define DP_LM_PARAMS_INIT {(unsigned)sizeof(dp_lm_params), 3, 1.f, 0.f, 1.0e-2f, 4.f, 1.f / 3.f, 1.0e-6f, 1.0e6f, 0, 0.f, 0.f}

typedef struct dp_lm_extra {
    unsigned struct_size; /* sizeof(dp_lm_extra) in the caller's translation unit (DP_LM_EXTRA_INIT sets it) */
    unsigned reserved0;   /* must be 0 */
    float* mu;            /* DEVICE [B] in/out, or NULL */
    int* n_accepted;      /* DEVICE [B] or NULL: accepted steps */
    float* loss0;         /* DEVICE [B][3] or NULL: the three loss numbers at z0 */
} dp_lm_extra;
#define DP_LM_EXTRA_INIT {(unsigned)sizeof(dp_lm_extra), 0u, (float*)0, (int*)0, (float*)0}

int dp_optimize_lm(dp_ctx* ctx, const dp_batch* in, const dp_lm_params* params, const dp_result* out, const dp_lm_extra* extra,
                   void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_LM_H */
