// dp_lm.h -- argument block and LDS layout of dp_optimize_lm's kernel (dp_lm.hip), shared with the host side (dp_host.cpp).
//
// One frame per wave (64 lanes), WPB waves per workgroup; the folded decoder is staged once per workgroup into LDS from the context's
// dp_forward_vjp image (dp_vjp.h), as the dp_cons family does.  Reference of what is computed: include/dragposer_lm.h.
#pragma once
#include <hip/hip_runtime.h>

namespace dplm {

constexpr int WPB = 4; // waves (= frames in flight) per workgroup: a wave's block is 20 KB, four of them and the weights fill a CU's LDS to 3/4

// LDS (floats): the three weight matrices with rows padded to an odd stride (dp_cons.h's), the de-normalisation's scale, the skeleton,
// then a private block per wave
constexpr int S0 = 25, S1 = 41, S2 = 61;             // row strides of A0 [40][24], A1 [60][40], A2 [92][60]
constexpr int L_A0 = 0, L_A1 = L_A0 + 40 * S0, L_A2 = L_A1 + 60 * S1;
constexpr int L_SD = L_A2 + 92 * S2;                 // sigma[92] of the decoder's outputs
constexpr int L_PAR = L_SD + 92;                     // int parent[22]
constexpr int L_OFF = L_PAR + 22;                    // bone offsets [22][3]
constexpr int L_WAVE0 = (L_OFF + 66 + 3) & ~3;       // first wave's block (16-byte aligned)
// per-wave block: the forward pass's state ...
constexpr int W_Z = 0;          // [24] the latent the forward pass runs on
constexpr int W_H0 = 24;        // [40] h0
constexpr int W_H1 = 64;        // [60] h1
constexpr int W_D0 = 124;       // [40] LeakyReLU slope of layer 0 (1 or 0.2)
constexpr int W_D1 = 164;       // [60] ... of layer 1
constexpr int W_Q = 224;        // [92] de-normalised decoder output
constexpr int W_QN = 316;       // [22][4] unit quaternions
constexpr int W_RN = 404;       // [22] 1 / |q_j|, then [4] the world root quaternion
constexpr int W_WR = 426;
constexpr int W_R = 430;        // [22][9] R_j (root: R_0, the world root rotation)
constexpr int W_B = 628;        // [22][4] bone b_j = R_p off_j (root frame)
constexpr int W_V = 716;        // [22][4] v_j: the bones of j's path summed
constexpr int W_P = 804;        // [22][4] P_j
constexpr int W_G = 892;        // [22][9] G_j
constexpr int W_SW = 1090;      // [22][2] sqrt(w_pos / 3E), sqrt(lambda_rot w_rot / 9E)
// ... and the step's
constexpr int ST = 28;          // row stride of the tangents (24 columns; four row groups of an MFMA result land in distinct banks)
constexpr int W_T = 1136;       // [92][ST] S2 scaled by sigma: d(decoder output)/dz; before it [60][ST] D1 S1 in the same place
constexpr int SJ = 32;          // row stride of the Jacobian rows and of A
constexpr int W_J = W_T + 92 * ST; // [24][SJ] two tracked joints' rows of J (columns 0..23) and r (column 24); then [25][25] the solve's H | -g
constexpr int W_A = W_J + 24 * SJ; // [25][SJ] A = J^T J (rows and columns 0..23) and g = J^T r (column / row 24), kept until z moves
constexpr int W_FLOATS = W_A + 25 * SJ;
static_assert(25 * 25 <= 24 * SJ, "the solve's matrix fits the Jacobian rows' place");
constexpr int LDS_FLOATS = L_WAVE0 + WPB * W_FLOATS;
constexpr int LDS_BYTES = 4 * LDS_FLOATS;            // 121 488 bytes of a CU's 160 KB: one workgroup per CU, a wave per SIMD
static_assert(LDS_BYTES == 121488 && LDS_BYTES <= 160 * 1024, "the LDS budget stated in DESIGN.md section 16");

struct Args {
    const float* img; // dp_vjp.h image (IMG_WORDS)
    const float *z0, *z_tgt, *cur_rot, *tgt_pos, *tgt_rot, *w;
    const unsigned char* tracked;
    float *z, *z_pre, *pose, *disp, *world_disp, *world_rot, *pos, *rot, *loss; // nullable
    int *iters, *status;                                                       // nullable
    float* mu;       // [B] in/out, nullable
    int* n_accepted; // [B], nullable
    float* loss0;    // [B][3], nullable
    int n_frames, n_steps, early_stop;
    float lam_rot, lam_tmp;
    float mu0, mu_up, mu_down, mu_min, mu_max;
    float stop_eps_pos, stop_eps_rot;
};

} // namespace dplm

hipError_t dp_launch_lm(const dplm::Args* args, hipStream_t stream);
