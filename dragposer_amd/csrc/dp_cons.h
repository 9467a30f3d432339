// dp_cons.h -- argument block of dp_optimize_constrained's kernel (dp_cons.hip), shared with the host side (dp_host.cpp).
//
// One frame per wave (64 lanes), WPB waves per workgroup; the folded decoder is staged once per workgroup into LDS from the context's
// dp_forward_vjp image (dp_vjp.h), so no packing of its own.  Reference of what is computed: include/dragposer_constraints.h.
#pragma once
#include <hip/hip_runtime.h>

namespace dpcons {

constexpr int WPB = 8; // waves (= frames in flight) per workgroup

// LDS (floats): the three weight matrices with rows padded to an odd stride (a lane per row and a lane per column both conflict-free),
// the skeleton tables, then a private scratch block per wave
constexpr int S0 = 25, S1 = 41, S2 = 61;            // row strides of A0 [40][24], A1 [60][40], A2 [92][60]
constexpr int L_A0 = 0, L_A1 = L_A0 + 40 * S0, L_A2 = L_A1 + 60 * S1;
constexpr int L_PAR = L_A2 + 92 * S2;                // int parent[22]
constexpr int L_SUB = L_PAR + 22;                    // unsigned subtree mask[22] (bit d: joint d is in the subtree of j)
constexpr int L_CST = L_SUB + 22;                    // int cstart[23]
constexpr int L_CLS = L_CST + 23;                    // int clist[22]
constexpr int L_OFF = L_CLS + 22;                    // bone offsets [22][3]
constexpr int L_WAVE0 = (L_OFF + 66 + 3) & ~3;       // first wave's block (16-byte aligned)
// per-wave block
constexpr int W_Z = 0;          // [24] latent
constexpr int W_H0 = 24;        // [40] h0, then dL/dpre0
constexpr int W_H1 = 64;        // [60] h1, then dL/dpre1
constexpr int W_Q = 124;        // [92] de-normalised decoder output (88 quaternion channels, displacement, pad)
constexpr int W_DY = 216;       // [92] dL/dy
constexpr int W_R = 308;        // [22][9] R_j (root: R_0, the world root rotation)
constexpr int W_B = 508;        // [22][4] bone b_j = R~_p off_j (root-frame)
constexpr int W_P = 596;        // [22][4] P_j
constexpr int W_G = 684;        // [22][9] G_j
constexpr int W_GP = 884;       // [22][4] dL/dP_j
constexpr int W_F = 972;        // [22][4] subtree sums F_j
constexpr int W_FLOATS = 1060;
constexpr int LDS_FLOATS = L_WAVE0 + WPB * W_FLOATS;
constexpr int LDS_BYTES = 4 * LDS_FLOATS;           // 70 832 bytes: LDS alone would fit two workgroups per CU; the kernel's VGPRs
                                                    // (2 waves per SIMD) allow one
static_assert(LDS_BYTES == 70832, "the LDS budget stated in DESIGN.md section 13");

// the table instantiation (dp_optimize_terms, include/dragposer_terms.h): the staged term table after the skeleton tables, and a block
// of per-frame rows appended to each wave's block
constexpr int MAX_TERMS = 16;                        // DP_MAX_TERMS
constexpr int TW = 22;                               // words per staged term (T_* below)
constexpr int T_TYPE = 0, T_JA = 1, T_JB = 2, T_FLAGS = 3, T_W = 4, T_PT = 5, T_DIR = 8, T_AXA = 11, T_AXB = 14, T_P0 = 17, T_P1 = 18,
              T_ROW = 20;                            // (ints: type .. flags; T_ROW: the per-frame row pointer, 8-byte aligned)
constexpr int L_TBL = L_WAVE0;                       // [MAX_TERMS][TW]
constexpr int L_WAVE0_T = L_TBL + MAX_TERMS * TW;
constexpr int W_ROW = W_FLOATS;                      // [MAX_TERMS][4] the frame's rows (vector, s_f), defaults filled in
constexpr int W_FLOATS_T = W_ROW + 4 * MAX_TERMS;
constexpr int LDS_FLOATS_T = L_WAVE0_T + WPB * W_FLOATS_T;
constexpr int LDS_BYTES_T = 4 * LDS_FLOATS_T;       // 74 288 bytes: still one workgroup per CU
static_assert(LDS_BYTES_T == 74288 && LDS_BYTES_T <= 76 * 1024, "the LDS budget stated in DESIGN.md section 13");
static_assert(L_TBL % 2 == 0 && TW % 2 == 0 && T_ROW % 2 == 0, "per-frame row pointers are read from LDS as 8-byte words");

struct Args {
    const float* img; // dp_vjp.h image (IMG_WORDS)
    const float *z0, *z_tgt, *cur_rot, *tgt_pos, *tgt_rot, *w;
    const unsigned char* tracked;
    const float* global_pos; // [B][3], read only when w_floor != 0
    float *z, *z_pre, *pose, *disp, *world_disp, *world_rot, *pos, *rot, *loss, *loss_extra; // nullable
    int *iters, *status;                                                                   // nullable
    int n_frames, n_iter, early_stop;
    float stop_eps_pos, stop_eps_rot, min_loss_incr;
    float lam_rot, lam_tmp, ctmp; // ctmp = 2 lam_tmp / 24
    float one_m_b1, beta2, one_m_b2, eps;
    double beta1d, beta2d, lrd; // Adam's bias corrections, continued on the device in double (as torch does in Python)
    // constraint terms (include/dragposer_constraints.h)
    float w_floor, w_fwd, w_hcol, w_feet;
    int floor_j[2], foot_j[2], head, hips, up, one_sided;
    float floor_level, fwd[3], fwd_thr, fwd_margin, feet_r2;
};

// the table instantiation's arguments: Args (its four-term fields unused) and the term table, staged into LDS once per workgroup
struct TermArgs : Args {
    int n_terms, need_gp;            // need_gp: an active PLANE or point-DISTANCE term exists (global_pos is read)
    float* loss_terms;               // [B][n_terms], nullable
    unsigned tbl[MAX_TERMS * TW];    // T_* layout; DISTANCE's p0 / p1 hold lo^2 / hi^2
};

} // namespace dpcons

hipError_t dp_launch_cons(const dpcons::Args* args, hipStream_t stream);
hipError_t dp_launch_terms(const dpcons::TermArgs* args, hipStream_t stream);
