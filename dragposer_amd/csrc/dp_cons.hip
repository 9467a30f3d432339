// dp_cons.hip -- dp_optimize_constrained (include/dragposer_constraints.h): the reference's whole per-frame loss, the four terms of its
// `# Additional Losses` block included (drag_pose.py:129-183), optimised with Adam and the while-condition in ONE launch.
//
// Layout: one frame per wave, WPB waves per workgroup (dp_cons.h).  The folded decoder's three matrices are staged once per workgroup
// into LDS (rows padded to an odd stride: a lane per output row in the forward pass and a lane per input column in the backward pass
// both read without bank conflicts); activations and per-joint vectors are exchanged through a block of LDS private to the wave.  The
// wave runs its frame's loop alone: no workgroup barrier after the staging, no atomics, nothing shared between frames, so a frame's
// results depend on that frame's inputs only.
//   forward   decoder rows dealt over the lanes (40, 60, 92 rows); then one lane per joint: normalise q_j, R_j = rotmat(q_j)
//             (root: cur_rot (x) q_0), bone b_j = R~_p off_j, v_j = the path sum of the bones (<= 7), P_j = world_disp + R_0 v_j,
//             G_j = R_0 R_j -- the decomposition of dp_vjp.hip (every non-root q_j is normalised, so the chain collapses)
//   losses    tracker terms per joint lane, temporal term per latent lane, the four constraint terms (a few joints: every lane
//             evaluates them on the same LDS values, the lane of a joint keeps that joint's upstream gradient); one butterfly
//             reduction gives the loss sums and the root's gradient together
//   backward  F_j = subtree sums of dL/dP (subtree masks built at staging), dL/dR_j = R_0^T (dL/dG_j + sum_c F_c off_c^T) per joint
//             lane, then A2^T, A1^T, A0^T with a lane per column; Adam per latent lane
// Two instantiations share every phase above but the terms: dp_cons_kernel runs the four reference terms with their parameters in
// the argument block (dp_optimize_constrained); dp_terms_kernel runs a table of up to 16 PLANE / DISTANCE / ALIGN terms
// (dp_optimize_terms, include/dragposer_terms.h), staged into LDS with the skeleton tables, its per-frame rows read once per launch into
// the wave's block, evaluated by a loop over the terms with a wave-uniform switch on the type.
// dp_cons_skel.hip holds both once more with the bones of each frame's own skeleton (DP_CONS_SKEL 1 of the same body).
// Rotations: the reference takes quat.from_matrix(G) (x) f for the forward axes; G is a rotation matrix (cur_rot a unit quaternion, as
// every reference caller passes it), so that is G f, which is what is computed.  The rotation loss is the element-wise |G - T|_F^2 of
// the reference on the matrices themselves: DP_STATUS_TARGET_NOT_ROTATION is never set by this kernel.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "dp_cons.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 0 // (1: dp_cons_skel.hip)
#define DP_CONS_SEQ 0  // (1: dp_cons_seq.hip)

__global__ __launch_bounds__(WPB * 64) void dp_cons_kernel(Args a)
#define DP_CONS_TABLE 0
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

__global__ __launch_bounds__(WPB * 64) void dp_terms_kernel(TermArgs a)
#define DP_CONS_TABLE 1
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

hipError_t dp_launch_cons(const Args* args, hipStream_t stream) { return launch_waves(dp_cons_kernel, args, stream); }
hipError_t dp_launch_terms(const TermArgs* args, hipStream_t stream) { return launch_waves(dp_terms_kernel, args, stream); }
