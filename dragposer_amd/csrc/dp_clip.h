// dp_clip.h -- argument block, workspace layout and LDS layout of dp_optimize_clip_lm's kernels (dp_clip.hip), shared with the host side
// (dp_host.cpp).  Reference of what is computed: include/dragposer_clip_lm.h.
//
// dp_clip_rows_kernel    one frame per wave, WPB waves per workgroup, dp_lm.h's LDS layout unchanged (the folded decoder staged once per
//                        workgroup, a private block per wave); what it writes goes to the workspace, not into a solve.
// dp_clip_chain_kernel   one wave per sequence: the block recursion over the sequence's frames, forwards and backwards.
// dp_clip_decide_kernel  one wave per sequence: the totals in double in index order, the decision, mu and the per-sequence word.
// A call is a fixed train of these on the caller's stream (dp_launch_clip); what connects them is the workspace.
// What dp_optimize_clip_lm_accel's unit (dp_clip_accel.h) takes from here instead of repeating it: the workspace's one list (Layout, layout()),
// the launch train (train(), its chain and decision launches as parameters) and plain_rows.
#pragma once
#include <hip/hip_runtime.h>

#include "dp_lm.h"

namespace dpclip {

constexpr int WPB = dplm::WPB;      // rows kernel: frames in flight per workgroup (dp_lm.h's budget: 121 488 bytes of LDS, a wave per SIMD)
constexpr int LAT = 24;
constexpr int AG_FLOATS = 25 * LAT; // a frame's A_t (rows 0..23) | g_t (row 24)
constexpr int LI_FLOATS = 25 * LAT; // a frame's L_t^-1 (rows 0..23) | y_t (row 24)

// the per-sequence word
constexpr int W_REFUSED = 1;  // a frame of the sequence was refused: no step runs
constexpr int W_REJECTED = 2; // the last trial was rejected: Z has not moved, A and g are kept
constexpr int W_CUR = 4;      // which of the two latent / loss buffers holds the kept Z

// rows kernel modes
constexpr int M_INIT = 0;    // screen, the pass of z0: Z, the loss, A | g
constexpr int M_NORMAL = 1;  // A | g at the kept Z (skipped after a rejection)
constexpr int M_TRIAL = 2;   // the forward pass of Z' only: its loss
constexpr int M_RESULTS = 3; // every dp_result array at the returned Z

// chain kernel LDS (floats), one wave per workgroup
constexpr int CS = 25;             // row stride of S_t / L_t and of P
constexpr int CI = 33;             // row stride of L_t^-1 as the matrix pipe reads it (columns 24..31 zero)
constexpr int C_S = 0;             // [24][CS] S_t, then L_t in place
constexpr int C_P = C_S + 24 * CS; // [24][CS] L_(t-1)^-T L_(t-1)^-1
constexpr int C_I = C_P + 24 * CS; // [24][CI] L_t^-1
constexpr int C_V = C_I + 24 * CI; // [4][32] vectors handed from lane to lane: g_t / the right-hand side, 1 / L_kk, y_t, w_t
constexpr int CHAIN_LDS_FLOATS = C_V + 4 * 32;
constexpr int CHAIN_LDS_BYTES = 4 * CHAIN_LDS_FLOATS;
static_assert(CHAIN_LDS_BYTES == 8480, "the LDS budget stated in DESIGN.md section 18");

// The workspace (bytes from its start; every part 16-byte aligned).  B = S T.  One list for both clip solves: what differs is the width of a
// frame's factor block (LI_FLOATS here, dp_clip_accel.h's LF_FLOATS there) and whether the last part exists.
struct Layout {
    size_t z[2];    // float [B][24] the kept latents and the trial's, by W_CUR
    size_t ag;      // float [B][AG_FLOATS]
    size_t li;      // float [B][factor_floats]
    size_t loss[2]; // float [B][4] a frame's three loss numbers and their fp32 sum, by W_CUR
    size_t cpl[2];  // double [B] |z_t - z_(t-1)|^2 (0 for t = 0), by W_CUR
    size_t flags;   // int [B] DP_STATUS_BAD_STATE / DP_STATUS_BAD_TARGETS of the frame
    size_t tot;     // double [S][2] L_s of the kept Z, its coupling part (every coupling sum the call has)
    size_t word;    // int [S]
    size_t solved;  // int [S] the chain's last solve went through
    size_t mu;      // float [S]
    size_t nacc;    // int [S]
    size_t acc;     // double [S] the second-difference part of L_s of the kept Z (with_acc; else no bytes)
    size_t bytes;
};
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
inline Layout layout(int S, long long B, int factor_floats = LI_FLOATS, bool with_acc = false)
{
    Layout l;
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t o = at; at = up16(at + bytes); return o; };
    for (int i = 0; i < 2; ++i) l.z[i] = take((size_t)B * LAT * 4);
    l.ag = take((size_t)B * AG_FLOATS * 4);
    l.li = take((size_t)B * factor_floats * 4);
    for (int i = 0; i < 2; ++i) l.loss[i] = take((size_t)B * 16);
    for (int i = 0; i < 2; ++i) l.cpl[i] = take((size_t)B * 8);
    l.flags = take((size_t)B * 4);
    l.tot = take((size_t)S * 16);
    l.word = take((size_t)S * 4);
    l.solved = take((size_t)S * 4);
    l.mu = take((size_t)S * 4);
    l.nacc = take((size_t)S * 4);
    l.acc = take(with_acc ? (size_t)S * 8 : 0);
    l.bytes = at;
    return l;
}

struct Args {
    const float* img; // dp_vjp.h image (IMG_WORDS)
    const float *z0, *z_tgt, *cur_rot, *tgt_pos, *tgt_rot, *w;
    const unsigned char* tracked;
    float *z, *z_pre, *pose, *disp, *world_disp, *world_rot, *pos, *rot, *loss; // nullable
    int *iters, *status;                                                       // nullable
    float* mu;         // [S] in/out, nullable
    int* n_accepted;   // [S], nullable
    double* clip_loss; // [S][2], nullable
    double* loss_hist; // [S][n_steps + 1], nullable
    int* info;         // [S], nullable
    // the workspace's parts
    float* wz[2];
    float *wag, *wli;
    float* wloss[2];
    double* wcpl[2];
    int* wflags;
    double* wtot;
    int *wword, *wsolved;
    float* wmu;
    int* wnacc;
    int n_frames, n_seq, n_t, n_steps; // B, S, T
    int mode, step;                    // rows kernel: M_*; decide kernel: the step decided (-1: the pass of z0)
    float lam_rot, lam_tmp, lam_smooth;
    float mu0, mu_up, mu_down, mu_min, mu_max;
};

// The rows pass of a launch train (host side only): plain_rows, or another unit's kernel on the same argument block with what that unit adds
// behind `own` (dp_clip_skel.hip).  The chain and the decision do not depend on it.
struct Rows {
    hipError_t (*launch)(const Args* args, int mode, const void* own, hipStream_t stream);
    const void* own;
};

} // namespace dpclip

hipError_t dp_launch_clip(const dpclip::Args* args, hipStream_t stream);
hipError_t dp_launch_clip_rows(const dpclip::Args* args, int mode, hipStream_t stream);
hipError_t dp_launch_clip_train(const dpclip::Args* args, const dpclip::Rows* rows, hipStream_t stream); // dp_launch_clip with `rows` as its rows pass

namespace dpclip {

static inline hipError_t plain_rows(const Args* args, int mode, const void*, hipStream_t stream) { return dp_launch_clip_rows(args, mode, stream); }

// The launch train of a clip solve (host side only), once for every unit: rows(z0) . decide | per step: [rows(A, g) unless it is the first
// step] . chain . rows(trial) . decide | rows(results).  `k` is dp_clip.h's part of the caller's own copy of its argument block; `chain()`
// and `decide()` launch the unit's two kernels on that copy as it then stands (k->step is set before each decision) and return the error.
template <class Chain, class Decide>
inline hipError_t train(Args* k, const Rows* rows, hipStream_t stream, const Chain& chain, const Decide& decide)
{
    const auto run_rows = [&](int mode) { return rows->launch(k, mode, rows->own, stream); };
    const auto run_decide = [&](int step) {
        k->step = step;
        return decide();
    };
    hipError_t e = run_rows(M_INIT);
    if (e == hipSuccess) e = run_decide(-1);
    for (int st = 0; st < k->n_steps && e == hipSuccess; ++st) {
        if (st > 0) e = run_rows(M_NORMAL);
        if (e == hipSuccess) e = chain();
        if (e == hipSuccess) e = run_rows(M_TRIAL);
        if (e == hipSuccess) e = run_decide(st);
    }
    if (e == hipSuccess) e = run_rows(M_RESULTS);
    return e;
}

} // namespace dpclip
