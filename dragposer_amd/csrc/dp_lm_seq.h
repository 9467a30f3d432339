// dp_lm_seq.h -- argument block and LDS budget of dp_lm_seq.hip: dp_lm.hip's frame with the step loop of a sequence around it
// (include/dragposer_sequence_lm.h), shared with the host side (dp_host.cpp).  dp_lm.h's struct and constants stay as they are: dp_lm_kernel's
// code does not change with this unit.
#pragma once
#include "dp_lm.h"

namespace dplm {

constexpr int MAX_AR_ORDER = 4; // DP_MAX_AR_ORDER

// LDS: dp_lm.h's layout, unchanged, and a second array with one area per wave: the sequence's last MAX_AR_ORDER history rows [k][24], row 0 =
// h_1, the newest (dp_cons_ar.h's arrangement).  Lane i shifts and writes column i at a step's end; every lane below 24 reads all of it when
// the next step begins, behind the step's closing wave_sync().  What else a sequence carries from step to step (latent, global position and
// rotation, mu) lives in registers.
constexpr int AR_W_FLOATS = MAX_AR_ORDER * 24;
constexpr int SEQ_LDS_BYTES = LDS_BYTES + WPB * 4 * AR_W_FLOATS;
static_assert(SEQ_LDS_BYTES == 123024 && SEQ_LDS_BYTES <= 160 * 1024, "the LDS budget stated in DESIGN.md section 16a");

// What the step loop adds to a frame's arguments.  Of Args, a sequence launch reads z0 = z = the latent [S][24] (in / out), cur_rot = the state's
// global_rot (in), w and tracked [S] (held for all steps), tgt_pos / tgt_rot [T][S], z_tgt by the two strides (NULL with a predictor), mu [S]
// (in / out); it writes per step [T][S] pose (the RETURNED pose: root channels = the normalised world rotation), pos (joint positions),
// world_rot, loss, loss0, iters, n_accepted and status -- each nullable -- and never z_pre, disp, world_disp or rot.
struct SeqFields { // (dp_cons_seq.h's fields under the same names: dp_host.cpp's fill_sequence writes either)
    int n_steps;
    int z_tgt_step, z_tgt_seq; // strides (floats) of z_tgt between steps / between sequences
    const float* tgt_root;     // [T][S][3] or NULL: position targets of step t are tgt_pos + (tgt_root[t] - the global position before step t)
    float* global_pos;         // [S][3] in / out
    float* global_rot;         // [S][4] out (in: Args::cur_rot, the same array)
    float* hist;               // [T][S][24 + 3 + NH] history rows of every step: z | displacement (joint adjustment included) | heights
    float* pos_ret;            // [T][S][3] returned global position, nullable
    int n_heights, height_joints[8];
    int adjust_joint, adjust_target_joint; // adjust_joint < 0: no joint adjustment
    float adjust_weight;
    float mean_q0[4], std_q0[4]; // normalisation of the returned pose's root channels
};
struct ArFields { // (dp_cons_ar.h's fields under the same names: dp_host.cpp's take_latent_ar writes either)
    const float* coeffs;     // [order][24][24], row = output component; NULL: no predictor, the targets are Args::z_tgt's rows
    const float* bias;       // [24]
    float* trace;            // [T][S][24] or NULL: the z_tgt row every step used
    const float* latent_buf; // [S][history][24], the state's array: read before the first step, newest row last
    int order, history;      // 1..MAX_AR_ORDER <= history
};
struct SeqArgs : Args {
    SeqFields q;
    ArFields r;
    float* mu_trace; // [T][S] mu after every step, nullable
};

} // namespace dplm

hipError_t dp_launch_lm_seq(const dplm::SeqArgs* args, hipStream_t stream);
