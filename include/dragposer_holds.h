/* dragposer_holds.h -- C ABI of libdragposer_hip.so: dp_optimize_sequence_terms (include/dragposer_sequence_constraints.h) with HOLDS --
 * joints held where they touched down (foot lock), the frame loop still inside one launch.
 *
 * A point-DISTANCE term (include/dragposer_terms.h) pulls a joint towards a world point.  For a foot that should stay where it came down
 * the point is where the RECONSTRUCTION put the foot, which is not known before the frame has run, so no per_frame array can carry it.  A
 * hold is a tiny state machine per sequence, carried inside the step loop: it latches a joint's world position when the joint comes down,
 * feeds it to its term on the following steps, and releases it when the joint lifts.  The state is in / out, so stretches chain.
 *
 * The call.  dp_optimize_sequence_terms in every respect except one: term holds[h].term reads its per-frame row from the hold state.
 *   At step t of sequence s that term's row (x, y, z, s_f) is state[s][h] as it stood before the step.
 *   The row is screened exactly as a per_frame row is: a non-finite or out-of-range component, or s_f < 0, gives DP_STATUS_BAD_TARGETS
 *   for that step, with the consequences include/dragposer_sequence_constraints.h states.
 *   A caller may store any held >= 0: non-zero counts as held and scales the weight, as s_f does.  The kernel itself writes only 0 or 1.
 *
 * The term a hold refers to.  Its type is DP_TERM_DISTANCE, joint_b == -1, per_frame == NULL, and no other hold refers to the same term;
 * otherwise the call returns DP_ERR_INVALID with a message naming the hold.  A hold on a term with weight 0 is inert: its state is neither
 * read nor written (and its rows of `trace` are not written).
 *
 * The update.  After a step, and after that step's epilogue has produced the new global position gpn (joint adjustment included), in fp32
 * and with these operations in this order (P: the step's joint positions, dp_seq_extra.joint_pos; a = the term's joint_a):
 *   W    = gpn + (P_a - P_0)            per component, unfused: an add of a sub
 *   hgt  = W[up_axis] - level
 *   if held == 0:  if hgt <= contact_lo: (x, y, z, held) = (W, 1)
 *   else:          if hgt >  contact_hi: held = 0            (x, y, z stay)
 * By the comparison forms, a step whose results are NaN leaves the state as it was; a step refused as bad state, which skips the loop, does
 * not touch the state (its rows of `trace` repeat it).  W is where a renderer puts the joint, and the right point for the next step's
 * term, which evaluates gp_before' + P_a' with gp_before' = gpn.
 *
 * Equivalence.  The launch returns the bits of this per-frame composition: dp_optimize_terms[_skeleton] with that term's per_frame = the
 * [S][4] state rows, then dp_sequence_advance, then the latent copy, then the update above on `pos` and the advanced global position --
 * on every output of dp_optimize_sequence_terms, on the state arrays, on `state` and on `trace`.
 *
 * Refusals: dp_optimize_sequence_terms' order, with dp_holds after dp_terms and before dp_seq_extra.  dp_holds is refused (DP_ERR_INVALID)
 * for a NULL struct, a bad struct_size, a non-zero reserved0; n_holds outside 0..DP_MAX_HOLDS; a NULL holds or a NULL state with
 * n_holds > 0; a term index out of range; a term that breaks the rules above; a non-finite level, contact_lo or contact_hi, or
 * contact_lo > contact_hi.  DP_ERR_UNSUPPORTED from a library built without the kernel.
 */
#ifndef DRAGPOSER_HOLDS_H
#define DRAGPOSER_HOLDS_H

#include "dragposer_sequence_constraints.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_MAX_HOLDS 4

typedef struct dp_hold {
    int term;          /* index into dp_terms.terms */
    float level;       /* floor level along dp_terms.up_axis */
    float contact_lo;  /* touch-down: height <= contact_lo */
    float contact_hi;  /* release:    height >  contact_hi   (contact_lo <= contact_hi) */
} dp_hold;

typedef struct dp_holds {
    unsigned struct_size; /* sizeof(dp_holds) in the caller's translation unit (DP_HOLDS_INIT sets it); checked like dp_result's */
    unsigned reserved0;   /* must be 0 */
    int n_holds;          /* 0..DP_MAX_HOLDS */
    const dp_hold* holds; /* HOST [n_holds], read during the call */
    float* state;         /* DEVICE [S][n_holds][4], in / out: (x, y, z, held) */
    float* trace;         /* DEVICE [T][S][n_holds][4] or NULL: the state after every step */
} dp_holds;
#define DP_HOLDS_INIT {(unsigned)sizeof(dp_holds), 0u, 0, (const dp_hold*)0, (float*)0, (float*)0}

/* latent, frames, params, terms, skeleton (may be NULL), state, adjust, out and extra (may be NULL) as dp_optimize_sequence_terms takes them. */
int dp_optimize_sequence_holds(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params,
                               const dp_terms* terms, const dp_holds* holds, const dp_skeleton_in* skeleton, const dp_seq_state* state,
                               const dp_seq_step* adjust, const dp_seq_results* out, const dp_seq_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_HOLDS_H */
