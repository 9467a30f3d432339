// dp_cons_points.hip -- dp_optimize_terms_points, dp_optimize_terms_points_skeleton and dp_optimize_sequence_terms_points
// (include/dragposer_points.h): the three table kernels of dp_cons.hip, dp_cons_skel.hip and dp_cons_seq.hip with PLANE and DISTANCE terms
// that may name a POINT, a weighted combination P_(22+k) = sum_j m_k[j] P_j of the joints' positions, in a joint's place.  The kernels are
// dp_cons_body.h's text three times more, with DP_CONS_TABLE 1 and DP_CONS_POINTS 1, in a unit of its own so that the other units' kernels
// keep their instructions.  Per iteration lanes 4k + c form the points' positions from W_P into an area of the wave's block
// (dp_cons_points.h); a term reads position `index` from one of the two areas, and the lane of joint j keeps the term's gradient times its
// own coefficient of the index (1 or 0 for a joint: the other kernels' `j == ja`).
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_terms.h"
#include "../../include/dragposer_points.h"
#include "dp_cons_points.h"
#include "dp_math.h"
#include "dp_vjp.h"

using namespace dpcons;

#include "dp_cons_dev.h"

static_assert(MAX_POINTS == DP_MAX_POINTS && PT_NJ == NJ, "dp_cons_points.h's table holds DP_MAX_POINTS rows of a coefficient per joint");

#define DP_CONS_TABLE 1
#define DP_CONS_POINTS 1

#define DP_CONS_SKEL 0
#define DP_CONS_SEQ 0
__global__ __launch_bounds__(WPB * 64) void dp_terms_points_kernel(PointTermArgs a)
#include "dp_cons_body.h"
#undef DP_CONS_SKEL

#define DP_CONS_SKEL 1
__global__ __launch_bounds__(WPB * 64) void dp_terms_points_skel_kernel(PointTermSkelArgs a)
#include "dp_cons_body.h"
#undef DP_CONS_SEQ

#define DP_CONS_SEQ 1
__global__ __launch_bounds__(WPB * 64) void dp_terms_points_seq_kernel(PointSeqTermArgs a)
#include "dp_cons_body.h"
#undef DP_CONS_POINTS
#undef DP_CONS_TABLE

hipError_t dp_launch_terms_points(const PointTermArgs* args, hipStream_t stream) { return launch_waves(dp_terms_points_kernel, args, stream); }
hipError_t dp_launch_terms_points_skel(const PointTermSkelArgs* args, hipStream_t stream) { return launch_waves(dp_terms_points_skel_kernel, args, stream); }
hipError_t dp_launch_terms_points_seq(const PointSeqTermArgs* args, hipStream_t stream) { return launch_waves(dp_terms_points_seq_kernel, args, stream); }
