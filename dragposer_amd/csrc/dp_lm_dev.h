// dp_lm_dev.h -- device helpers of the LM frame (dp_lm_frame_*.h) and of the two bodies around it: dp_lm_body.h's five units (dp_lm.hip,
// dp_lm_seq.hip, dp_lm_terms.hip, dp_lm_seq_terms.hip, dp_lm_skel.hip) and dp_clip_rows_body.h's two (dp_clip.hip, dp_clip_skel.hip); included
// once per unit, after dp_lm.h, dp_math.h and dp_vjp.h.
#pragma once
using namespace dplm;

#define DEV __device__ __forceinline__

namespace {

constexpr int NJ = dpvjp::NJ, LAT = dpvjp::LAT, H0 = dpvjp::H0, H1 = dpvjp::H1;
constexpr int NYU = 4 * NJ + 3; // decoder outputs that are used (the 92nd is not)
#define UNR 4

typedef float f4 __attribute__((ext_vector_type(4)));

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

DEV void mv(const float* M, const float* v, float* o)
{ // M v with M row-major 3x3
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = M[3 * r] * v[0] + M[3 * r + 1] * v[1] + M[3 * r + 2] * v[2];
}

// d rotmat(q) along dq (dp_math.h's rotmat is quadratic in q)
DEV void rotmat_jvp(const float* q, const float* t, float* D)
{
    const float w = q[0], x = q[1], y = q[2], z = q[3], dw = t[0], dx = t[1], dy = t[2], dz = t[3];
    const float xx = x * dx, yy = y * dy, zz = z * dz;
    const float xy = dx * y + x * dy, xz = dx * z + x * dz, yz = dy * z + y * dz, wx = dw * x + w * dx, wy = dw * y + w * dy, wz = dw * z + w * dz;
    D[0] = -4.f * (yy + zz); D[1] = 2.f * (xy - wz);   D[2] = 2.f * (xz + wy);
    D[3] = 2.f * (xy + wz);  D[4] = -4.f * (xx + zz);  D[5] = 2.f * (yz - wx);
    D[6] = 2.f * (xz - wy);  D[7] = 2.f * (yz + wx);   D[8] = -4.f * (xx + yy);
}

// the tangent of q / |q| along dq, for qn = q / |q| and rn = 1 / |q|
DEV void unit_jvp(const float* qn, float rn, const float* dq, float* o)
{
    const float dot = qn[0] * dq[0] + qn[1] * dq[1] + qn[2] * dq[2] + qn[3] * dq[3];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (dq[c] - qn[c] * dot) * rn;
}

// dp_math.h's rotmat and quat_mul and mv above, in double: the reported loss's pass
DEV void rotmat_d(const double* q, double* R)
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double x2 = x + x, y2 = y + y, z2 = z + z;
    const double xx = x * x2, yy = y * y2, zz = z * z2, xy = x * y2, xz = x * z2, yz = y * z2, wx = w * x2, wy = w * y2, wz = w * z2;
    R[0] = 1.0 - (yy + zz); R[1] = xy - wz;         R[2] = xz + wy;
    R[3] = xy + wz;         R[4] = 1.0 - (xx + zz); R[5] = yz - wx;
    R[6] = xz - wy;         R[7] = yz + wx;         R[8] = 1.0 - (xx + yy);
}
DEV void quat_mul_d(const double* a, const double* b, double* o)
{
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
DEV void mv_d(const double* M, const double* v, double* o)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = M[3 * r] * v[0] + M[3 * r + 1] * v[1] + M[3 * r + 2] * v[2];
}
DEV double wsum_d(double x)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) x += __shfl_xor(x, m, 32);
    return x;
}

// include/dragposer.h, DP_STATUS_TARGET_NOT_ROTATION (dp_device.h's test)
DEV bool not_rotation(const float* m)
{
    const float n0 = m[0] * m[0] + m[1] * m[1] + m[2] * m[2], n1 = m[3] * m[3] + m[4] * m[4] + m[5] * m[5], n2 = m[6] * m[6] + m[7] * m[7] + m[8] * m[8];
    const float d01 = m[0] * m[3] + m[1] * m[4] + m[2] * m[5], d02 = m[0] * m[6] + m[1] * m[7] + m[2] * m[8], d12 = m[3] * m[6] + m[4] * m[7] + m[5] * m[8];
    const float det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    const float tol = DP_ROTATION_TOL;
    return !(fabsf(n0 - 1.f) <= tol && fabsf(n1 - 1.f) <= tol && fabsf(n2 - 1.f) <= tol && fabsf(d01) <= tol && fabsf(d02) <= tol && fabsf(d12) <= tol && det > 0.f);
}

} // namespace
