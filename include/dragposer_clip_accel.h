/* dragposer_clip_accel.h -- C ABI of libdragposer_hip.so: dp_optimize_clip_lm (include/dragposer_clip_lm.h) with a second-difference
 * (acceleration) term in the loss beside its first-difference one.  A first difference penalises velocity: it pulls a moving performer towards
 * standing still and fills a stretch without data with a straight line whose ends are kinks.  A second difference costs constant-velocity
 * motion nothing, and an in-filled stretch becomes a cubic.  Nothing here changes another entry point.
 *
 * The problem.  A launch holds B = S T rows of a dp_batch; frame t of sequence s is row t S + s, and every frame is dp_optimize_lm's frame,
 * exactly as in dragposer_clip_lm.h.  With c1 = lambda_smooth / 24 and c2 = lambda_accel / 24 the loss of sequence s is
 *     L_s(Z) = sum_t |r_t(z_t)|^2  +  c1 sum_(t=1..T-1) |z_t - z_(t-1)|^2  +  c2 sum_(t=1..T-2) |z_(t+1) - 2 z_t + z_(t-1)|^2
 * K is the scalar T x T band matrix c1 Lap + c2 D2^T D2: Lap the path graph's Laplacian (dragposer_clip_lm.h), D2 the (T-2) x T
 * second-difference matrix.  D2^T D2 has the diagonal 1, 5, 6, ..., 6, 5, 1 for T >= 5 (1, 5, 5, 1 for T = 4; 1, 4, 1 for T = 3; nothing for
 * T <= 2), the first off-diagonal -2, -4, ..., -4, -2 and the second off-diagonal 1.  For T <= 2 this is dragposer_clip_lm.h's problem.
 *
 * The step, per sequence.  A_t and g_t per frame as dp_optimize_lm forms them.  H = blockdiag(A_t) + K (x) I_24;  G_t = g_t + (K Z)_t;
 * M = H + mu diag(H).  M Delta = -G by block Cholesky with lower bandwidth 2.  With k1 = K[t,t-1], k2 = K[t,t-2], and every term whose index
 * is below 0 absent:
 *     E_t = k2 L_(t-2)^-T                            (never stored: E_t E_t^T = k2^2 P_(t-2) with P = L^-T L^-1)
 *     F_t = (k1 I - E_t F_(t-1)^T) L_(t-1)^-T
 *     S_t = M_tt - E_t E_t^T - F_t F_t^T = L_t L_t^T
 *     y_t = L_t^-1 (-G_t - E_t y_(t-2) - F_t y_(t-1))
 *     backwards:  Delta_t = L_t^-T (y_t - F_(t+1)^T Delta_(t+1) - K[t+2,t] L_t^-1 Delta_(t+2))
 * With c2 = 0 this is dragposer_clip_lm.h's recursion, F_t = -c L_(t-1)^-T.  Everything else is dp_optimize_clip_lm's: a pivot that is <= 0 or
 * not finite in any block rejects the step for the sequence; Z' = Z + Delta is accepted iff L_s(Z') < L_s(Z) (a NaN rejects), both totals the
 * frames' fp32 loss numbers and the two coupling sums added in double in index order; mu is ONE value per sequence and moves as there; after
 * a rejection A and g are kept and only the chain is solved again; exactly n_steps trials run; the loss never increases.
 *
 * Conditioning.  The recursion and the decision's inputs are fp32.  The second-difference operator's condition number grows like T^4, and mu
 * damps only the diagonal: a very large lambda_accel at a very small mu is where fp32 gives out.  Against the same recursion in fp64 (the
 * oracle, T up to 65) one step of it in fp32 is 2e-6 to 2e-5 off in the latents at mu 1e-2, lambda_accel 500 included, and 4e-6 to 1.1e-3 at
 * mu 1e-6 for lambda_accel <= 50; at lambda_accel 500 and mu 1e-6 it is 4e-3 to 1.4e-2 off.  Three steps from mu0 with lambda_accel <= 50
 * stay within 6e-5 and take the fp64 decisions.  
 *
 * Outputs.  dp_result and dp_clip_lm_extra as in dragposer_clip_lm.h: loss_hist, mu, n_accepted and info keep their meaning, and
 * clip_loss[s][1] is the whole coupling part, both sums together.  dp_clip_accel_params.accel_loss [S] double (nullable): the
 * second-difference part of L_s at the returned Z (NaN for a sequence with a refused frame).  `workspace`: DEVICE memory of at least
 * dp_clip_lm_accel_workspace_bytes(n_sequences, n_frames) bytes, 16-byte aligned, the call's alone until it has run.
 * lambda_accel == 0 runs dp_optimize_clip_lm's own launch train and returns its bits; accel_loss is then written as 0.
 *
 * A refused frame, asynchrony, graph capture, repeatability, fp32 and bf16-rounded contexts: as in dragposer_clip_lm.h (the launch train is
 * dp_clip_accel.hip's).  Returns DP_OK or a negative dp_status and never throws; message: dp_last_error(ctx).
 * Refusals, DP_ERR_INVALID, in this order: dp_optimize_clip_lm's, in its order, up to and including lambda_smooth negative or not finite (NULL
 * ctx; NULL batch, params or extra; dp_clip_lm_params.struct_size; what dp_result refuses; dp_clip_lm_extra.struct_size / reserved0; n_steps;
 * the lambdas, mu and factors; what the batch refuses; n_sequences); then a NULL dp_clip_accel_params or its struct_size; lambda_accel negative
 * or not finite; a NULL workspace or one shorter than dp_clip_lm_accel_workspace_bytes.  Then DP_ERR_UNSUPPORTED from the test-only library or a
 * library linked without dp_clip_accel.hip, DP_ERR_DEVICE from a context without a device image.
 *
 * Not covered: term tables, points, holds, gaps, tethers and per-frame skeletons in the clip loss; a parallel (cyclic-reduction) chain for
 * one very long sequence -- the chain is T dependent factorisations in one wave; DragPose and the plug-in.
 */
#ifndef DRAGPOSER_CLIP_ACCEL_H
#define DRAGPOSER_CLIP_ACCEL_H

#include <stddef.h>

#include "dragposer_clip_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dp_clip_accel_params {
    unsigned struct_size; /* sizeof(dp_clip_accel_params) in the caller's translation unit (DP_CLIP_ACCEL_PARAMS_INIT sets it) */
    float lambda_accel;   /* >= 0, finite: c2 = lambda_accel / 24 */
    double* accel_loss;   /* DEVICE [S] or NULL: the second-difference part of L_s at the returned Z */
} dp_clip_accel_params;
#define DP_CLIP_ACCEL_PARAMS_INIT {(unsigned)sizeof(dp_clip_accel_params), 0.f, (double*)0}

/* bytes of workspace a launch of n_sequences sequences over n_frames rows needs; 0 for arguments the call refuses */
size_t dp_clip_lm_accel_workspace_bytes(int n_sequences, int n_frames);

int dp_optimize_clip_lm_accel(dp_ctx* ctx, const dp_batch* in, int n_sequences, const dp_clip_lm_params* params, const dp_clip_accel_params* accel,
                              const dp_result* out, const dp_clip_lm_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_CLIP_ACCEL_H */
