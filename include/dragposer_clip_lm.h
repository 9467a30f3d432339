/* dragposer_clip_lm.h -- C ABI of libdragposer_hip.so, a clip solved JOINTLY: S sequences of T frames, every frame dp_optimize_lm's frame
 * (include/dragposer_lm.h), and the latents of a sequence tied frame to frame by a first-difference term inside the loss.  Every other entry
 * point solves a frame on its own and connects two frames by causal state only (the warm start, cur_rot, a hold, a tether, the latent
 * predictor); here frame t+1 may correct frame t.  The call is offline: it sees the whole clip.  Nothing here changes another entry point.
 *
 * The problem.  A launch holds B = S T rows of a dp_batch; frame t of sequence s is row t S + s (the layout of dp_optimize_sequence_*'s
 * per-step arrays).  Each frame has its own z0, z_tgt, cur_rot, targets, weights and `tracked` row and dp_optimize_lm's residuals r_pos,
 * r_rot, r_tmp (include/dragposer_lm.h, "The algorithm").  With c = lambda_smooth / 24 the loss of sequence s is
 *     L_s(Z) = sum_t |r_t(z_t)|^2  +  c sum_(t=1..T-1) |z_t - z_(t-1)|^2
 *
 * The step, per sequence.  Per frame A_t = J_t^T J_t and g_t = J_t^T r_t as dp_optimize_lm forms them.  H = blockdiag(A_t) + c Lap (x) I_24
 * with Lap the path graph's Laplacian (diagonal 1, 2, ..., 2, 1, off-diagonal -1; 0 for T = 1);  G_t = g_t + c (Lap Z)_t;
 * M = H + mu diag(H).  M Delta = -G by block Cholesky -- the system is block-tridiagonal, its off-diagonal blocks are -c I:
 *     S_0 = M_00;   S_t = M_tt - c^2 S_(t-1)^-1;   S_t = L_t L_t^T;   y_t = L_t^-1 (-G_t + c L_(t-1)^-T y_(t-1))
 *     backwards:    Delta_t = L_t^-T (y_t + c L_t^-1 Delta_(t+1))
 * A pivot that is <= 0 or not finite in any block rejects the step for the sequence.  The trial Z' = Z + Delta is accepted iff
 * L_s(Z') < L_s(Z) (a NaN rejects); both totals are the frames' fp32 loss numbers, each frame's three added in fp32, and the frames' coupling
 * parts, added in double in index order.  mu is ONE value per sequence: accepted, mu <- max(mu mu_down, mu_min); rejected, mu <- min(mu
 * mu_up, mu_max).  After a rejection Z has not moved: A and g are kept and only the chain is solved again.  Exactly n_steps trials run;
 * there is no early stop.  The loss never increases.
 *   T = 1 is dp_optimize_lm's problem.  lambda_smooth = 0 decouples the frames, but the decision stays per sequence.  A frame whose weights
 *   are all 0, with lambda_tmp = 0, has A_t = 0 exactly: it is determined by its neighbours alone (in-fill) -- and with lambda_smooth = 0 it
 *   makes every trial of its sequence a certain rejection.
 *
 * Outputs.  dp_result per frame as in dp_optimize_lm: every array belongs to the returned z (z_pre = z), iters is the number of steps run,
 * loss is the fp32 pass's three numbers at the returned z.  dp_result.clock is ignored.  dp_clip_lm_extra, every pointer nullable except the
 * workspace: `mu` [S] in/out (NULL: every sequence starts at mu0; a value that is not finite or outside [mu_min, mu_max] is read as mu0);
 * `n_accepted` [S]; `clip_loss` [S][2] double: L_s at the returned Z and its coupling part; `loss_hist` [S][n_steps + 1] double: L_s of the
 * kept latents before the first step and after each; `info` [S]: DP_CLIP_* flags.  `workspace`: DEVICE memory of at least
 * dp_clip_lm_workspace_bytes(n_sequences, n_frames) bytes (n_frames: the batch's), 16-byte aligned, the call's alone until it has run.
 *
 * A frame that dp_optimize_lm would refuse (DP_STATUS_BAD_STATE, DP_STATUS_BAD_TARGETS): no step runs for its sequence, info[s] carries
 * DP_CLIP_REFUSED_FRAME, mu[s] stays, n_accepted[s] is 0, clip_loss and loss_hist of s are NaN; that frame returns what dp_optimize_lm returns
 * for it, the sequence's other frames return the results of their z0 with iters 0.  The other sequences of the launch are bit-identical to
 * a launch without the fault.
 *
 * The call is asynchronous on the given HIP stream: a fixed train of launches (dp_clip.hip), no allocation, no host synchronisation,
 * graph-capturable (`mu` is read and written at replay time).  No atomics: two calls on the same inputs give identical bits.  fp32 and
 * bf16-rounded contexts both work.  Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).
 * Refusals, DP_ERR_INVALID, in this order: NULL ctx; NULL batch, params or extra; dp_clip_lm_params.struct_size; what dp_result refuses;
 * dp_clip_lm_extra.struct_size / reserved0; n_steps outside 1..DP_LM_MAX_STEPS; lambda_rot or lambda_tmp not finite or negative, a mu or
 * factor that is not finite; mu_down outside (0, 1); mu_up <= 1; mu_min <= 0 or mu_min > mu_max; mu0 outside [mu_min, mu_max]; what the
 * batch refuses (n_frames, a NULL input array); n_sequences <= 0 or not dividing n_frames; lambda_smooth negative or not finite; a NULL
 * or short workspace.  Then DP_ERR_UNSUPPORTED from the test-only library, DP_ERR_DEVICE from a context without a device image.
 *
 * Not covered: term tables, points, holds, gaps, tethers and per-frame skeletons in the clip loss; a parallel (cyclic-reduction) chain for
 * one very long sequence -- the chain is T dependent factorisations in one wave; DragPose and the plug-in.  (A second-difference
 * (acceleration) coupling beside the first-difference one is dp_optimize_clip_lm_accel, include/dragposer_clip_accel.h.)
 */
#ifndef DRAGPOSER_CLIP_LM_H
#define DRAGPOSER_CLIP_LM_H

#include <stddef.h>

#include "dragposer_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_CLIP_REFUSED_FRAME 1 /* info[s]: a frame of the sequence was refused, no step ran */

typedef struct dp_clip_lm_params {
    unsigned struct_size; /* sizeof(dp_clip_lm_params) in the caller's translation unit (DP_CLIP_LM_PARAMS_INIT sets it) */
    int n_steps;          /* 1..DP_LM_MAX_STEPS trials per sequence */
    float lambda_rot, lambda_tmp; /* >= 0, finite */
    float lambda_smooth;  /* >= 0, finite: c = lambda_smooth / 24 */
    float mu0;            /* the damping a sequence starts from when dp_clip_lm_extra.mu is NULL */
    float mu_up, mu_down; /* > 1; in (0, 1) */
    float mu_min, mu_max; /* 0 < mu_min <= mu0 <= mu_max */
} dp_clip_lm_params;
#define DP_CLIP_LM_PARAMS_INIT {(unsigned)sizeof(dp_clip_lm_params), 4, 1.f, 0.f, 1.f, 1.0e-2f, 4.f, 1.f / 3.f, 1.0e-6f, 1.0e6f}

typedef struct dp_clip_lm_extra {
    unsigned struct_size; /* sizeof(dp_clip_lm_extra) in the caller's translation unit (DP_CLIP_LM_EXTRA_INIT sets it) */
    unsigned reserved0;   /* must be 0 */
    float* mu;            /* DEVICE [S] in/out, or NULL */
    int* n_accepted;      /* DEVICE [S] or NULL: accepted steps */
    double* clip_loss;    /* DEVICE [S][2] or NULL: L_s at the returned Z, its coupling part */
    double* loss_hist;    /* DEVICE [S][n_steps + 1] or NULL: L_s of the kept latents */
    int* info;            /* DEVICE [S] or NULL: DP_CLIP_* flags */
    void* workspace;      /* DEVICE, dp_clip_lm_workspace_bytes(n_sequences, n_frames) bytes, 16-byte aligned */
    size_t workspace_bytes;
} dp_clip_lm_extra;
#define DP_CLIP_LM_EXTRA_INIT {(unsigned)sizeof(dp_clip_lm_extra), 0u, (float*)0, (int*)0, (double*)0, (double*)0, (int*)0, (void*)0, (size_t)0}

/* bytes of workspace a launch of n_sequences sequences over n_frames rows needs; 0 for arguments the call refuses */
size_t dp_clip_lm_workspace_bytes(int n_sequences, int n_frames);

int dp_optimize_clip_lm(dp_ctx* ctx, const dp_batch* in, int n_sequences, const dp_clip_lm_params* params, const dp_result* out,
                        const dp_clip_lm_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_CLIP_LM_H */
