/* dragposer_tethers.h -- C ABI of libdragposer_hip.so: dp_optimize_sequence_gaps (include/dragposer_gaps.h) with TETHERS -- joints tied to
 * their own recent path, the frame loop still inside one launch.
 *
 * Every frame is solved against that frame's trackers and a pull in latent space; nothing says how a joint moves from one frame to the
 * next, so a knee or an elbow that no tracker observes may land anywhere the decoder allows.  The point such a joint should stay near is
 * where the RECONSTRUCTION put it on the step before, which is not known before the launch, so no per_frame array can carry it.  A tether
 * is the hold's mechanism (include/dragposer_holds.h) with another update rule: its point-DISTANCE term's point follows the joint's own
 * reconstructed path.  The term's band [lo, hi] then has a physical meaning: hi is a speed limit, the metres per frame the joint may move
 * for free; lo = hi = 0 is quadratic velocity damping; alpha = 1 extrapolates the point at constant velocity, which turns velocity damping
 * into acceleration damping.  The state is in / out, so stretches chain.
 *
 * The call.  dp_optimize_sequence_gaps in every respect except one: term tethers[k].term reads its per-frame row from the tether state.
 *   `holds`, `ar` and `gaps` are taken exactly as that call takes them (`holds` and `ar` may be NULL, `gaps` may not).
 *   At step t of sequence s that term's row (x, y, z, live) is state[s][k][0..3] as it stood before the step.
 *   Screening.  The row is screened exactly as a per_frame row is: a non-finite or out-of-range component, or live < 0, gives
 *   DP_STATUS_BAD_TARGETS for that step, with the consequences include/dragposer_sequence_constraints.h states.  An all-zero state means
 *   "no path yet": live = 0 switches the term off for the first step.  A caller may store any live >= 0: it scales the weight, as s_f does.
 *   The kernel itself writes only 1.
 *
 * The state.  state [S][n_tethers][8] floats per sequence and tether: 0-2 the term's point, 3 live, 4-6 the joint's last world position
 * Wprev, 7 have (0: no last position yet).  `trace` [T][S][n_tethers][8] receives the eight words after every step.
 *
 * The term a tether refers to.  Its type is DP_TERM_DISTANCE, joint_b == -1, per_frame == NULL, and no other tether and no hold refers to
 * the same term; otherwise the call returns DP_ERR_INVALID with a message naming the tether.  A tether on a term with weight 0 is inert: its
 * rows of `state` and of `trace` are neither read nor written.
 *
 * The update.  After a step, and after that step's epilogue has produced the new global position gpn (joint adjustment included), in fp32,
 * unfused, with these operations in this order (P: the step's joint positions, dp_seq_extra.joint_pos; a = the term's joint_a):
 *   W = gpn + (P_a - P_0)                          per component: add_rn of a sub_rn, the hold's expression
 *   if |W_c| <= DP_INPUT_LIMIT for c = 0, 1, 2:    (the comparison form: a NaN fails it)
 *       point = have != 0 ? W + alpha * (W - Wprev) : W          add_rn(W, mul_rn(alpha, sub_rn(W, Wprev)))
 *       (x, y, z, live) = (point, 1);  (Wprev, have) = (W, 1)
 *   otherwise the state stays as it was.
 * A step refused as bad state, which skips the loop, does not touch the state (its rows of `trace` repeat it).  A DP_STATUS_BAD_TARGETS
 * step runs the update on the pose it returns, as it runs the hold's.  W is where a renderer puts the joint, and the point the next step's
 * term measures from: it evaluates gp_before' + P_a' with gp_before' = gpn.  An extrapolated point beyond DP_INPUT_LIMIT is found by the
 * next step's screening.
 *
 * Equivalence.  The launch returns the bits of this per-frame composition: dp_optimize_terms[_skeleton] with the tethered terms' per_frame
 * = the [S][4] rows state[:, k, 0:4] (holds and gaps composed as include/dragposer_holds.h and include/dragposer_gaps.h state), then
 * dp_sequence_advance, then the latent copy, then the update above on `pos` and the advanced global position -- on every output of
 * dp_optimize_sequence_gaps, on the state arrays, on dp_holds.state, dp_gaps.state, on `state` and on `trace`.  With n_tethers == 0 the
 * call returns the bits of dp_optimize_sequence_gaps.
 *
 * Refusals: dp_optimize_sequence_gaps' in its order (a NULL `tethers` is refused with the NULL arguments), then dp_tethers, after dp_gaps,
 * as DP_ERR_INVALID and in this order: a bad struct_size or a non-zero reserved0; n_tethers outside 0..DP_MAX_TETHERS; a NULL tethers or a
 * NULL state with n_tethers > 0; then per tether, each message naming the tether: a term index out of range; a term that breaks the rules
 * above (not DP_TERM_DISTANCE, a joint_b, a per_frame array, a term another tether or a hold refers to); an alpha that is not finite or
 * outside [0, 1].  After those, DP_ERR_UNSUPPORTED from a library built without the kernel.
 *
 * Not covered: dp_live_step and the plug-in, dp_optimize_sequence_constrained, the dp_w4 / dp_w16 kernels, joint-to-joint terms, gradients
 * through the tether.
 */
#ifndef DRAGPOSER_TETHERS_H
#define DRAGPOSER_TETHERS_H

#include "dragposer_gaps.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_MAX_TETHERS 4
#define DP_TETHER_STATE_FLOATS 8

typedef struct dp_tether {
    int term;    /* index into dp_terms.terms */
    float alpha; /* in [0, 1]: 0 = the point is the last position, 1 = the last position extrapolated by the last step's motion */
} dp_tether;

typedef struct dp_tethers {
    unsigned struct_size;     /* sizeof(dp_tethers) in the caller's translation unit (DP_TETHERS_INIT sets it); checked like dp_result's */
    unsigned reserved0;       /* must be 0 */
    int n_tethers;            /* 0..DP_MAX_TETHERS */
    const dp_tether* tethers; /* HOST [n_tethers], read during the call */
    float* state;             /* DEVICE [S][n_tethers][8], in / out: (x, y, z, live) the term's row, (wx, wy, wz, have) the last world position */
    float* trace;             /* DEVICE [T][S][n_tethers][8] or NULL: the state after every step */
} dp_tethers;
#define DP_TETHERS_INIT {(unsigned)sizeof(dp_tethers), 0u, 0, (const dp_tether*)0, (float*)0, (float*)0}

/* latent, frames, params, terms, holds (may be NULL), ar (may be NULL), gaps, skeleton (may be NULL), state, adjust, out and extra (may be
 * NULL) as dp_optimize_sequence_gaps takes them. */
int dp_optimize_sequence_tethers(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params,
                                 const dp_terms* terms, const dp_holds* holds, const dp_latent_ar* ar, const dp_gaps* gaps,
                                 const dp_tethers* tethers, const dp_skeleton_in* skeleton, const dp_seq_state* state,
                                 const dp_seq_step* adjust, const dp_seq_results* out, const dp_seq_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_TETHERS_H */
