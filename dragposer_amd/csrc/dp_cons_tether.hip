// dp_cons_tether.hip -- dp_optimize_sequence_tethers (include/dragposer_tethers.h): dp_optimize_sequence_gaps with point-DISTANCE terms whose
// point follows the joint's own reconstructed path.  The kernels are dp_cons_body.h's text twice more, with DP_CONS_TABLE 1, DP_CONS_SKEL 1,
// DP_CONS_SEQ 1, DP_CONS_HOLD 1, DP_CONS_GAP 1 and DP_CONS_TETHER 1, without and with DP_CONS_AR, in a unit of its own so that the other
// units' kernels keep their instructions.  Lane t is term t: a tethered term's row of the wave's block is the tether's, rewritten by the
// lane at each step's `stop` from the joint's new world position (dp_cons_tether.h).
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "../../include/dragposer_tethers.h"
#include "dp_cons_tether.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

#define DP_CONS_SKEL 1
#define DP_CONS_SEQ 1
#define DP_CONS_HOLD 1
#define DP_CONS_GAP 1
#define DP_CONS_TETHER 1
#define DP_CONS_TABLE 1

__global__ __launch_bounds__(WPB * 64) void dp_terms_tether_seq_kernel(TetherSeqArgs a)
#include "dp_cons_body.h"

#define DP_CONS_AR 1
__global__ __launch_bounds__(WPB * 64) void dp_terms_tether_ar_seq_kernel(TetherArSeqArgs a)
#include "dp_cons_body.h"
#undef DP_CONS_AR
#undef DP_CONS_TABLE

hipError_t dp_launch_terms_tether_seq(const TetherSeqArgs* args, hipStream_t stream) { return launch_waves(dp_terms_tether_seq_kernel, args, stream); }
hipError_t dp_launch_terms_tether_ar_seq(const TetherArSeqArgs* args, hipStream_t stream) { return launch_waves(dp_terms_tether_ar_seq_kernel, args, stream); }
