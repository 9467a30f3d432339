// dp_cons_seq.hip -- dp_optimize_sequence_constrained and dp_optimize_sequence_terms (include/dragposer_sequence_constraints.h): a clip, or a
// stretch of a live sequence, with the reference's extra loss terms or a term table, its frame loop inside ONE launch.
// Both kernels are dp_cons_body.h's text with DP_CONS_SKEL 1 and DP_CONS_SEQ 1.  A wave is one SEQUENCE for the whole launch, 8 waves per
// workgroup as in dp_cons.hip; the decoder rows, the parent / child tables, the subtree masks and the term table are staged once per launch and
// the sequence's skeleton is read and screened once (without a caller skeleton the host passes the context's own bones, stride 0: two kernels
// instead of four, and a sequence on skeleton X carries the bits of a context created with X).  Per step the wave reads that step's targets
// (dp_seq_frames' strides; with tgt_root the position targets are tgt_pos[t] + (tgt_root[t] - the carried global position)), screens them and
// the carried state as a per-frame launch does, runs the per-frame iteration loop unchanged -- Adam restarted, early stop implied -- and at
// `stop` applies run()'s epilogue in the wave with dp_sequence_advance_kernel's arithmetic and order.  The latent, the global position and the
// global rotation stay in registers between steps and are written back after the last; the history rows of every step go to the caller's
// scratch, which dp_launch_sequence_history (dp_sequence.hip) appends to the three buffers in a second launch.
// A step with a refused target returns the warm start's pose (one pass, DP_STATUS_BAD_TARGETS) and leaves a NaN latent, so the sequence is
// DP_STATUS_BAD_STATE from the next step on, all results NaN -- what the per-frame path reaches through the NaN latent; bad bones or a bad
// state at entry fill every step that way.  The other sequences of the launch are not affected.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "dp_cons_seq.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 1
#define DP_CONS_SEQ 1

__global__ __launch_bounds__(WPB * 64) void dp_cons_seq_kernel(SeqConsArgs a)
#define DP_CONS_TABLE 0
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

__global__ __launch_bounds__(WPB * 64) void dp_terms_seq_kernel(SeqTermArgs a)
#define DP_CONS_TABLE 1
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

hipError_t dp_launch_cons_seq(const SeqConsArgs* args, hipStream_t stream) { return launch_waves(dp_cons_seq_kernel, args, stream); }
hipError_t dp_launch_terms_seq(const SeqTermArgs* args, hipStream_t stream) { return launch_waves(dp_terms_seq_kernel, args, stream); }
