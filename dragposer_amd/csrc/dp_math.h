// dp_math.h -- the small device math shared by dp_forward_vjp's kernels (dp_vjp_impl.h) and the constrained optimise kernels (dp_cons.hip):
// the input refusal rule and the quaternion / rotation-matrix primitives.  tests/test_hip_vjp.py and tests/test_hip_constraints.py hold
// the gradients built on them to the fp64 oracles.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"

namespace {

__device__ __forceinline__ bool refused(float x) { return !(fabsf(x) <= DP_INPUT_LIMIT); } // NaN, Inf, or beyond the limit (dp_optimize's and dp_forward's rule)

// utils.py:49-74 (to_matrix_4, 3x3 block), w-first, no normalisation
__device__ __forceinline__ void rotmat(const float* q, float* R)
{
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float x2 = x + x, y2 = y + y, z2 = z + z;
    const float xx = x * x2, yy = y * y2, zz = z * z2, xy = x * y2, xz = x * z2, yz = y * z2, wx = w * x2, wy = w * y2, wz = w * z2;
    R[0] = 1.f - (yy + zz); R[1] = xy - wz;         R[2] = xz + wy;
    R[3] = xy + wz;         R[4] = 1.f - (xx + zz); R[5] = yz - wx;
    R[6] = xz - wy;         R[7] = yz + wx;         R[8] = 1.f - (xx + yy);
}

// dL/dq of rotmat(q) for dL/dR = g (row-major)
__device__ __forceinline__ void rotmat_vjp(const float* q, const float* g, float* dq)
{
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    dq[0] = 2.f * (z * (g[3] - g[1]) + y * (g[2] - g[6]) + x * (g[7] - g[5]));
    dq[1] = 2.f * (y * (g[1] + g[3]) + z * (g[2] + g[6]) + w * (g[7] - g[5]) - 2.f * x * (g[4] + g[8]));
    dq[2] = 2.f * (x * (g[1] + g[3]) + z * (g[5] + g[7]) + w * (g[2] - g[6]) - 2.f * y * (g[0] + g[8]));
    dq[3] = 2.f * (x * (g[2] + g[6]) + y * (g[5] + g[7]) + w * (g[3] - g[1]) - 2.f * z * (g[0] + g[4]));
}

// (pymotion quat_torch.mul, w-first Hamilton) a (x) b
__device__ __forceinline__ void quat_mul(const float* a, const float* b, float* o)
{
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

} // namespace
