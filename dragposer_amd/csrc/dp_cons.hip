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

#define DEV __device__ __forceinline__

namespace {

constexpr int NJ = dpvjp::NJ, LAT = dpvjp::LAT, H0 = dpvjp::H0, H1 = dpvjp::H1;
constexpr int NYU = 4 * NJ + 3; // decoder outputs that are used (the 92nd is not)
#ifndef UNR
#define UNR 4 // (the dot products' loops: unrolled further, their loads stay in flight in registers and the frame loop spills)
#endif

DEV void wave_sync()
{ // orders this wave's LDS writes before its later LDS reads (other lanes' data); no instruction
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

DEV float wsum(float x)
{ // sum over lanes 0..31 (every lane that contributes is below 32), result in every lane of the half
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) x += __shfl_xor(x, m, 32);
    return x;
}

DEV float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); } // lane 0's value, wave-uniform

// component `up` of a 3-vector without indexing registers at run time (no scratch)
DEV float comp(const float* v, int up) { return up == 0 ? v[0] : up == 1 ? v[1] : v[2]; }
DEV void flatten(float* v, int up)
{ // h(v): the up component set to 0
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = c == up ? 0.f : v[c];
}

// M v with M row-major 3x3
DEV void mv(const float* M, const float* v, float* o)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = M[3 * r] * v[0] + M[3 * r + 1] * v[1] + M[3 * r + 2] * v[2];
}

// global_pos is read: the floor term is on (four terms) / an active PLANE or point-DISTANCE term exists (table)
DEV bool reads_gp(const Args& a) { return a.w_floor != 0.f; }
DEV bool reads_gp(const TermArgs& a) { return a.need_gp != 0; }

DEV int uni_i(int x) { return __builtin_amdgcn_readfirstlane(x); } // (an int the wave holds in every lane)

} // namespace


__global__ __launch_bounds__(WPB * 64) void dp_cons_kernel(Args a)
#define DP_CONS_TABLE 0
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

__global__ __launch_bounds__(WPB * 64) void dp_terms_kernel(TermArgs a)
#define DP_CONS_TABLE 1
#include "dp_cons_body.h"
#undef DP_CONS_TABLE

hipError_t dp_launch_cons(const Args* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(dp_cons_kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}

hipError_t dp_launch_terms(const TermArgs* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(dp_terms_kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}
