/* dragposer_encoder.h -- C ABI of libdragposer_hip.so, the pose encoder: how a sequence begins.
 *
 * What it replaces in the reference (UPC-ViRVIG/DragPoser, python/src):
 *   dp_encode           Encoder.forward + reparameterize (autoencoder.py:19-27,56-143, skeleton.py:8-130,178-210): three stages of
 *                       masked dense layer (kernel-size-1 SkeletonConv) -> SkeletonPool -> LeakyReLU(0.2), 176 -> 112 -> 72 -> 48, then
 *                       f_mu / f_logvar and latent = mu + eps * exp(logvar / 2) -- for n poses in one launch
 *   dp_sequence_begin   DragPose.set_initial_pose (drag_pose.py:47-64) for S sequences in one launch: the encoder, then the state
 *                       dp_optimize_sequence / dp_sequence_advance / dp_temporal_predict carry on from
 *   dp_fold_encoder     host-only helper: conv and pool have nothing non-linear between them, so A_l = P_l (W_l * M_l), c_l = P_l b_l
 *
 * Conventions are dragposer.h's: fp32, row-major, pose-major; every function returns DP_OK or a negative dp_status and never throws.
 * The handle is its own (as dp_temporal is) and owns only its device copy of the folded weights; it is not thread-safe.  dp_encode and
 * dp_sequence_begin are asynchronous on the given HIP stream and perform no allocation, no host synchronisation and no host<->device
 * copy of caller data (graph-capturable).  The library owns no random generator: the caller passes eps.
 * There is NO CPU fallback: without a usable gfx950 device dp_encoder_create fails with DP_ERR_DEVICE.
 */
#ifndef DRAGPOSER_ENCODER_H
#define DRAGPOSER_ENCODER_H

#include "dragposer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_ENCODER_IN 176 /* 22 joints x 8 normalised dual-quaternion channels */

/* Host pointers to the reference checkpoint's encoder tensors, fp32 row-major [out][in] (state_dict keys under
 * autoencoder.encoder.*). */
typedef struct dp_encoder_model {
    unsigned struct_size;       /* sizeof(dp_encoder_model) in the caller's translation unit (DP_ENCODER_MODEL_INIT sets it) */
    const float* conv_w[3];     /* layers.l.0.weight : [176][176], [112][112], [72][72] (kernel size 1) */
    const float* conv_mask[3];  /* layers.l.0.mask   : same shapes */
    const float* conv_b[3];     /* layers.l.0.bias   : [176], [112], [72] */
    const float* pool_w[3];     /* layers.l.1.weight : [112][176], [72][112], [48][72] */
    const float* f_mu_w;        /* [24][48] f_mu.weight */
    const float* f_mu_b;        /* [24]     f_mu.bias */
    const float* f_logvar_w;    /* [24][48] f_logvar.weight */
    const float* f_logvar_b;    /* [24]     f_logvar.bias */
} dp_encoder_model;
#define DP_ENCODER_MODEL_INIT {(unsigned)sizeof(dp_encoder_model)}

/* Folded encoder: four dense layers, LeakyReLU(0.2) after the first three; Ah = [f_mu.weight; f_logvar.weight]. */
typedef struct dp_encoder_folded {
    float A0[112 * 176], c0[112];
    float A1[72 * 112], c1[72];
    float A2[48 * 72], c2[48];
    float Ah[48 * 48], ch[48];
} dp_encoder_folded;

typedef struct dp_encoder dp_encoder;

/* host-only: fold the raw encoder tensors (double accumulation, fp32 result).  DP_ERR_INVALID names the missing pointer. */
int dp_fold_encoder(const dp_encoder_model* model, dp_encoder_folded* out);

int dp_encoder_create(dp_encoder** out, const dp_encoder_model* model, int device);
int dp_encoder_destroy(dp_encoder* enc);
const char* dp_encoder_last_error(const dp_encoder* enc); /* NULL: last failure on this thread of a call without a handle */

/* How a launch is cut: 16 poses per wavefront, the wavefronts of a workgroup, at most max_blocks workgroups -- each stages the weight
 * image once and its wavefronts loop over 16-pose tiles, so a launch of more than the product of the three takes a second trip. */
int dp_encoder_geometry(const dp_encoder* enc, int* poses_per_wave, int* waves_per_block, int* max_blocks);

/* n poses.  DEVICE pointers: pose [n][176]; eps [n][24] or NULL (latent = mu); mu, logvar, latent [n][24], any may be NULL;
 * status [n] or NULL.  Per pose: an input value (pose, eps) that is not finite or beyond DP_INPUT_LIMIT in magnitude makes that pose's
 * results NaN and its status DP_STATUS_BAD_STATE | DP_STATUS_NONFINITE_RESULT; a non-finite result of clean inputs carries
 * DP_STATUS_NONFINITE_RESULT alone.  The other poses are not affected, and a pose's bits do not depend on n or on where in the batch
 * it stands.  n == 0 does nothing.  DP_ERR_INVALID: NULL handle, n < 0, NULL pose. */
int dp_encode(dp_encoder* enc, int n, const float* pose, const float* eps, float* mu, float* logvar, float* latent, int* status,
              void* hip_stream);

/* set_initial_pose for n_seq sequences: dp_encode's latent, and every element of the state written --
 *   latent [S][24]            the encoded latent (required)
 *   state->latent_buf [S][H][24]  that latent in every row
 *   state->disp_buf [S][H][3]     zero
 *   state->heights_buf [S][H][NH] init_heights [S][NH] in every row
 *   state->global_pos [S][3], global_rot [S][4]  init_global_pos / init_global_rot copied unchanged (the reference does not normalise)
 * state->height_joints is not read.  Screening covers the initial position, rotation and heights too: a refused sequence's latent and
 * state are NaN throughout, its status as above.  n_seq == 0 does nothing.  DP_ERR_INVALID: whatever dp_encode refuses, a NULL state
 * or state pointer, NULL init_* or latent, n_heights < 0 or above DP_MAX_HEIGHT_JOINTS, history < 1. */
int dp_sequence_begin(dp_encoder* enc, int n_seq, const float* pose, const float* eps, const float* init_global_pos,
                      const float* init_global_rot, const float* init_heights, const dp_seq_state* state, float* latent, int* status,
                      void* hip_stream);

/* ---- debug (host only; the CPU tests read the kernel's weight image through it, as dp_debug_pairs_w4 serves dp_w4's) -------------
 * image: the words the kernel stages into LDS, for `folded`; table: three ints per word -- (layer, row, column) of the folded
 * network the word holds (layer 0..2 = A0..A2 / c0..c2, 3 = Ah / ch; column -1 = the bias of that row), or layer -1 for a padding
 * word, which is zero.  Either may be NULL; returns the number of words (a negative dp_status on a NULL `folded`). */
int dp_debug_encoder_image(const dp_encoder_folded* folded, float* image, int* table, int capacity_words);

#ifdef __cplusplus
}
#endif
#endif /* DRAGPOSER_ENCODER_H */
