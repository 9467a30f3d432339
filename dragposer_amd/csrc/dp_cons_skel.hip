// dp_cons_skel.hip -- dp_optimize_constrained_skeleton (include/dragposer_constraints.h) and dp_optimize_terms_skeleton
// (include/dragposer_terms.h): dp_cons.hip's two kernels with the bone offsets of each frame's own skeleton (include/dragposer_skeleton.h).
// Both are dp_cons_body.h's text with DP_CONS_SKEL 1: in the prologue, beside the screening loads, lane j (1..21) reads row j of its
// frame's skeleton, screens it (a refused component sets the frame's bad_state, dp_optimize_skeleton's rule), keeps it as its off[] and
// stores it into a [22][3] area of the wave's private block (dp_cons_skel.h), from which the backward's child-bone loop reads instead of
// L_OFF.  The iteration loop, arithmetic and order included, is dp_cons.hip's: a frame given the context's own bones gets the plain
// kernel's bits.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "dp_cons_skel.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 1
#define DP_CONS_SEQ 0 // (1: dp_cons_seq.hip)

__global__ __launch_bounds__(WPB * 64) void dp_cons_skel_kernel(SkelArgs a)
#define DP_CONS_TABLE 0
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

__global__ __launch_bounds__(WPB * 64) void dp_terms_skel_kernel(TermSkelArgs a)
#define DP_CONS_TABLE 1
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

hipError_t dp_launch_cons_skel(const SkelArgs* args, hipStream_t stream) { return launch_waves(dp_cons_skel_kernel, args, stream); }
hipError_t dp_launch_terms_skel(const TermSkelArgs* args, hipStream_t stream) { return launch_waves(dp_terms_skel_kernel, args, stream); }
