// dp_cons_seq.h -- argument blocks and LDS budget of dp_cons_seq.hip: dp_cons_skel.hip's two kernels with the frame loop of a sequence
// inside the launch (include/dragposer_sequence_constraints.h), shared with the host side (dp_host.cpp).  dp_cons.h's and dp_cons_skel.h's
// structs and constants stay as they are: the four per-frame kernels' code does not change with this unit.
#pragma once
#include "dp_cons_skel.h"

namespace dpcons {

// LDS: dp_cons_skel.h's layout, unchanged -- the staged weights and tables once per launch, and per wave the block of a frame with its
// sequence's skeleton.  What a sequence carries from step to step (latent, global position, global rotation) lives in registers.
constexpr int SQ_LDS_BYTES = SK_LDS_BYTES, SQ_LDS_BYTES_T = SK_LDS_BYTES_T;
static_assert(SQ_LDS_BYTES == 73008 && SQ_LDS_BYTES_T == 76464 && SQ_LDS_BYTES_T <= 160 * 1024, "the LDS budget stated in DESIGN.md section 13c");

// the staged term's free word (dp_cons.h: T_P1 = 18, T_ROW = 20): floats between two steps' rows of the term's per_frame array, 0 = one row
// per sequence held for all steps.  The per-frame kernels never read it.
constexpr int T_STEP = 19;
static_assert(T_STEP > T_P1 && T_STEP < T_ROW && T_STEP < TW, "T_STEP is the word dp_cons.h's layout leaves free");

// What the step loop adds to a frame's arguments (the fields of dp_kernel.h's SeqK that this kernel needs).  Of Args, a sequence launch
// reads z0 = z = the latent [S][24] (in / out), cur_rot = the state's global_rot (in; the carried position comes from q.global_pos -- global_pos
// only says, through reads_gp(), whether a term reads it, and is NULL for a table without such a term), w and
// tracked [S] (held for all steps), tgt_pos / tgt_rot [T][S], z_tgt by the two strides; it writes per step [T][S] pose (the RETURNED pose:
// root channels = the normalised world rotation), pos (joint positions), world_rot, loss, loss_extra / loss_terms, iters and status --
// each nullable -- and never z_pre, disp, world_disp or rot.
struct SeqFields {
    int n_steps;
    int z_tgt_step, z_tgt_seq; // strides (floats) of z_tgt between steps / between sequences
    const float* tgt_root;     // [T][S][3] or NULL: position targets of step t are tgt_pos + (tgt_root[t] - the global position before step t)
    float* global_pos;         // [S][3] in / out: the state's array, checked non-NULL by the host
    float* global_rot;         // [S][4] out (in: Args::cur_rot, the same array)
    float* hist;               // [T][S][24 + 3 + NH] history rows of every step: z_pre | displacement (joint adjustment included) | heights
    float* pos_ret;            // [T][S][3] returned global position, nullable
    int n_heights, height_joints[8];
    int adjust_joint, adjust_target_joint; // adjust_joint < 0: no joint adjustment
    float adjust_weight;
    float mean_q0[4], std_q0[4]; // normalisation of the returned pose's root channels
};
struct SeqConsArgs : SkelArgs {
    SeqFields q;
};
struct SeqTermArgs : TermSkelArgs {
    SeqFields q;
};

} // namespace dpcons

hipError_t dp_launch_cons_seq(const dpcons::SeqConsArgs* args, hipStream_t stream);
hipError_t dp_launch_terms_seq(const dpcons::SeqTermArgs* args, hipStream_t stream);
