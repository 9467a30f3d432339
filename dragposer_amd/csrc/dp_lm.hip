// dp_lm.hip -- dp_optimize_lm (include/dragposer_lm.h): dp_optimize's per-frame sum of squares solved by Gauss-Newton steps with
// Levenberg-Marquardt damping, every step of every frame in ONE launch.
//
// Layout: one frame per wave, WPB waves per workgroup (dp_lm.h); the folded decoder staged once per workgroup into LDS, a block of LDS
// private to the wave, no workgroup barrier after the staging, no atomics: a frame's results depend on that frame's inputs only.
//   forward   the dp_cons family's: decoder rows dealt over the lanes, then a lane per joint on G_j = R_0 R_j, P_j = world_disp + R_0 v_j;
//             it also leaves the LeakyReLU slopes, the unit quaternions and the v_j in the wave's block for the tangents
//   tangents  S0 = D0 A0 (a row scaling, formed as the B operand is read), S1 = A1 S0, S2 = A2 (D1 S1) on v_mfma_f32_16x16x4_f32:
//             the weights are the A operand (M = 16 output rows), the latent's 24 tangent columns N (two 16-column tiles, the last 8
//             columns zero), 4 x 2 x 10 + 6 x 2 x 15 = 260 instructions.  A lane's result register r of tile (mt, nt) is row
//             16 mt + 4 (lane >> 4) + r, column 16 nt + (lane & 15); it is written to the wave's block scaled by the row's slope / sigma.
//   J         two tracked joints at a time, one per half of the wave; lane n < 24 of a half forms column n of the joint's 12 rows
//             (dP/dz, dG/dz: a path of at most 7 bones, each through its parent's quaternion), lane 24 the 12 residuals, into [24][32]
//   A, g      [J r]^T [J r] accumulated over the pairs on the same instruction (K = the 24 rows, both operands the same values): rows and
//             columns 0..23 are J^T J, column 24 is J^T r; the latent pull adds lambda_tmp / 24 to the diagonal and to g directly
//   solve     H = A + mu diag(A) with -g as a 25th row, Cholesky in the wave's block (lane i owns row i; the 25th row comes out as the
//             forward substitution), the back substitution in registers; a pivot that is <= 0 or not finite makes the trial latent NaN,
//             which the trial's loss rejects
//   reported  loss0 (after the pass of z0) and loss (with the results), when asked for: that latent once more through the decoder and the
//             kinematics in double on the same fp32 weights, in the tangents' place; the steps are decided on the fp32 passes
// The loop has ONE forward pass in its text: of z0, of each trial, and -- when the last trial was rejected, so that the wave's block no
// longer belongs to the kept latent -- of the kept latent once more for the results.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "dp_lm.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"

// the frame, shared with dp_lm_seq.hip (DP_LM_SEQ 1: the step loop of a sequence around it)
#define DP_LM_SEQ 0
__global__ __launch_bounds__(WPB * 64) void dp_lm_kernel(Args a)
#include "dp_lm_body.h"
#undef DP_LM_SEQ

hipError_t dp_launch_lm(const Args* args, hipStream_t stream)
{
    const unsigned grid = (unsigned)((args->n_frames + WPB - 1) / WPB);
    hipLaunchKernelGGL(dp_lm_kernel, dim3(grid), dim3(WPB * 64), 0, stream, *args);
    return hipGetLastError();
}
