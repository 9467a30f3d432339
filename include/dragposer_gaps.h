/* dragposer_gaps.h -- C ABI of libdragposer_hip.so: dp_optimize_sequence_ar (include/dragposer_latent_ar.h) for trackers that drop out and
 * come back.
 *
 * dp_seq_frames.w and .tracked are the same for every step, and a sample that is missing can only be sent as NaN: that step returns the warm
 * start's pose (DP_STATUS_BAD_TARGETS) and the sequence is DP_STATUS_BAD_STATE, every result NaN, for good.  This call keeps going: a joint
 * whose sample is absent is held at its last good sample for up to max_hold steps, at a weight that decays by `decay` per step, and leaves
 * the step's loss after that until a sample arrives again.
 *
 * The rule.  Per launch: max_hold (0..65535 steps) and decay (finite, 0 < decay <= 1).  Per sequence and joint a caller-owned DEVICE state
 * row, state [S][22][16] floats: 0-2 the world position P of the last good sample, 3-11 its rotation target R, 12 valid (0 / 1), 13 age,
 * 14 factor, 15 must stay 0.  Zeroed: nothing is held.  The state is carried from launch to launch, like dp_holds.state.  All arithmetic is
 * fp32, unfused (add_rn, sub_rn, mul_rn).
 *
 * For step t, sequence s, joint j with tracked[s][j] != 0 the sample is ABSENT when present [T][S][22] is given and 0 there, or when any
 * of the three effective position components or of the nine rotation components is refused (not finite, or beyond DP_INPUT_LIMIT).  The
 * effective position is what the step uses without this call: tpe = tgt_pos + (tgt_root[t] - global_pos), in that operation order, when
 * tgt_root is given, tgt_pos otherwise.  With present == 0 the sample is not read.
 *
 *   code 1, present:          the step's targets and weights are the sample's and w.  State: P = add_rn(tpe, gp) with gp the sequence's
 *                             global position before the step, R = the sample's rotation target, valid = 1, age = 0, factor = 1.
 *   code 2, absent and held:  when valid and age + 1 <= max_hold.  State: age += 1, factor = mul_rn(factor, decay).  The step runs with
 *                             tpe = sub_rn(P, gp), the held R and both weights mul_rn(w, factor).
 *   code 3, absent otherwise: lost.  valid = 0.  The joint is untracked in this step: not in the loss and not in E.
 *   code 0:                   tracked[s][j] == 0.
 *
 * E of the step is the number of joints with code 1 or 2; the loss denominators are 3E and 9E.  A step with E == 0 uses max(E, 1): both
 * tracker losses are exactly 0, the while-condition's first clause is false and the step is one pass (with the early stop); the pull term
 * and the table's terms act alone; the step carries DP_STATUS_NO_TRACKER.
 *
 * Joint adjustment reads the EFFECTIVE target of adjust_target_joint (on a held step the held one).  On a step where that joint is lost or
 * not tracked the target is the adjusted joint's own position: adj = mul_rn(sub_rn(P, P), w) = +0, added as usual.
 *
 * A step refused as bad state leaves the state as it is (its `trace` row is 0xFF).  Every other step updates the state before its loop, a
 * DP_STATUS_BAD_TARGETS step included: refused w, z_tgt and term rows (and an effective target beyond DP_INPUT_LIMIT after the shift of a
 * held position) remain DP_STATUS_BAD_TARGETS.
 *
 * Equivalence.  For every step with E >= 1 the launch returns the bits of this per-frame composition: dp_optimize_terms[_skeleton] on the
 * step's effective tgt_pos / tgt_rot / w / tracked (the rule above; dragposer_amd.Gaps.step is it in elementwise torch), then
 * dp_sequence_advance, then the latent copy, then the hold update -- on every output of dp_optimize_sequence_ar, on the state arrays, on
 * dp_gaps.state and on `trace`.  A clip in which every sample is present (and adjust_target_joint is tracked) returns the bits of
 * dp_optimize_sequence_ar, or of dp_optimize_sequence_holds when `ar` is NULL, on every output and state array.
 *
 * Arguments: dp_optimize_sequence_ar's and `gaps`.  `ar` may be NULL: the targets then come from frames->z_tgt, which is required as in
 * dp_optimize_sequence_holds.  `holds` may be NULL.
 *
 * Refusals: dp_optimize_sequence_ar's in its order (dp_latent_ar's own only when `ar` is given; a NULL `gaps` is refused with the NULL
 * arguments), then, as DP_ERR_INVALID and in this order: a bad dp_gaps.struct_size or a non-zero reserved0; max_hold outside 0..65535;
 * decay not in (0, 1]; a NULL state.  After those, DP_ERR_UNSUPPORTED from a library built without the kernel.
 */
#ifndef DRAGPOSER_GAPS_H
#define DRAGPOSER_GAPS_H

#include "dragposer_latent_ar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_GAP_STATE_FLOATS 16
#define DP_GAP_MAX_HOLD 65535

/* OR-ed into dp_seq_results.status beside dragposer.h's bits */
#define DP_STATUS_TRACKER_HELD 16 /* some joint of the step had code 2 */
#define DP_STATUS_TRACKER_LOST 32 /* some joint of the step had code 3 */
#define DP_STATUS_NO_TRACKER 64   /* the step had E == 0 */

typedef struct dp_gaps {
    unsigned struct_size;         /* sizeof(dp_gaps) in the caller's translation unit (DP_GAPS_INIT sets it); checked like dp_result's */
    unsigned reserved0;           /* must be 0 */
    int max_hold;                 /* 0..DP_GAP_MAX_HOLD steps */
    float decay;                  /* finite, 0 < decay <= 1 */
    float* state;                 /* DEVICE [S][22][16] in / out */
    const unsigned char* present; /* DEVICE [T][S][22] or NULL: 0 = the sample is absent */
    unsigned char* trace;         /* DEVICE [T][S][22] or NULL: every joint's code of every step (0xFF: the step was refused as bad state) */
} dp_gaps;
#define DP_GAPS_INIT {(unsigned)sizeof(dp_gaps), 0u, 0, 1.0f, (float*)0, (const unsigned char*)0, (unsigned char*)0}

/* latent, frames, params, terms, holds (may be NULL), ar (may be NULL), skeleton (may be NULL), state, adjust, out and extra (may be NULL)
 * as dp_optimize_sequence_ar takes them. */
int dp_optimize_sequence_gaps(dp_ctx* ctx, int n_sequences, float* latent, const dp_seq_frames* frames, const dp_params* params,
                              const dp_terms* terms, const dp_holds* holds, const dp_latent_ar* ar, const dp_gaps* gaps,
                              const dp_skeleton_in* skeleton, const dp_seq_state* state, const dp_seq_step* adjust, const dp_seq_results* out,
                              const dp_seq_extra* extra, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* DRAGPOSER_GAPS_H */
