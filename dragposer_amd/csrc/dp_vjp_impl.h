// dp_vjp_impl.h -- the vector-Jacobian product of decode + FK at (z, cur_rot), compiled once per unit (no include guard):
//   dp_vjp.hip       DP_VJP_SKEL 0: dp_vjp_kernel, dp_forward_vjp (include/dragposer_grad.h), the bones of the context's image;
//   dp_vjp_skel.hip  DP_VJP_SKEL 1: dp_vjp_skel_kernel, dp_forward_vjp_skeleton, the bones of each frame's own skeleton
//                    (include/dragposer_skeleton.h) and, on request, dL/d(offsets).
// The #if DP_VJP_SKEL blocks are the only difference; without them the text is the kernel dp_vjp.hip held before the skeleton form
// existed, and dp_vjp_kernel compiles to the same instructions.
//
// One frame per lane (dp_vjp.h).  The kernel recomputes the forward pass of dp_forward and runs its backward in the same
// lane; nothing is saved between calls and nothing is shared between lanes, so a frame's result depends on that frame's
// inputs alone (a non-finite frame stays in its own lane) and no atomics or barriers are needed.
//
// Kinematics.  The reference chains parent-local matrices (utils.py:95-105,140-146): G_j = G_p R_p^T R_j (R_j: root-space
// rotation of joint j, G_0 = R_0 = rotmat(cur_rot (x) q_0)), P_j = G_p off_j + P_p, P_0 = world_disp.  Every q_j, j >= 1, is
// normalised by the decoder, so R_p^T R_p = I holds identically in z and the chain collapses to
//     G_j = R_0 R_j,   P_j = world_disp + R_0 v_j,   v_j = v_p + R~_p off_j   (R~_0 = I, v_0 = 0)
// -- the same function of (z, cur_rot), hence the same derivatives.  Its backward needs, beyond the upstream gradients, only
// the root-frame positions v_j and the subtree sums F_j = sum_{d in subtree(j)} dL/dP_d:
//     dL/dR_j (j >= 1) = R_0^T (dL/dG_j + sum_{c child of j} F_c off_c^T)
//     dL/dR_0          = dL/dG_0 + sum_{j >= 1} dL/dG_j R_j^T + sum_j dL/dP_j v_j^T + dL/dworld_disp' d^T
// with dL/dworld_disp' = dL/dworld_disp + F_0 (world_disp = R_0 d exactly: quat_rotate and to_matrix_4 are one polynomial).
// v and F live in a column of LDS private to the lane (indexed by the run-time parent); everything else in registers.
// Bone offsets (DP_VJP_SKEL).  Every P depends on off_c linearly, through v_c only, and no rotation depends on it, so
//     dL/doff_c = (R_0 R~_p)^T F_c = R~_p^T (R_0^T F_c)   (p = parent of c)
// -- 18 FMAs per bone on what the bone's term above already holds.  The frame's bones sit in a second LDS column beside F.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "dp_math.h"
#include "dp_vjp.h"

#ifndef DP_VJP_SKEL
#define DP_VJP_SKEL 0
#endif

using namespace dpvjp;

#define DEV __device__ __forceinline__

namespace {

// qn = q / |q| (autoencoder.py:248), and 1 / |q|
DEV void unit(const float* q, float* qn, float& rn)
{
    rn = 1.f / sqrtf(fmaf(q[0], q[0], fmaf(q[1], q[1], fmaf(q[2], q[2], q[3] * q[3]))));
#pragma unroll
    for (int c = 0; c < 4; ++c) qn[c] = q[c] * rn;
}

// dL/dqn of the normalisation qn = q / |q| (q = y sd + mu) folded back to dL/dy, accumulated into dh1 through A2^T
DEV void quad_to_dh1(const float* __restrict__ W, int row0, const float* qn, float rn, const float* dqn, float* dh1)
{
    const float dot = qn[0] * dqn[0] + qn[1] * dqn[1] + qn[2] * dqn[2] + qn[3] * dqn[3];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float dy = (dqn[c] - qn[c] * dot) * rn * W[OFF_SD + row0 + c];
#pragma unroll
        for (int k = 0; k < H1; ++k) dh1[k] = fmaf(W[OFF_A2 + (row0 + c) * H1 + k], dy, dh1[k]);
    }
}

// child bone c of joint p (Rp: R_p, NULL for the root): dR0 += F_c (R~_p off_c)^T and, below the root, M += F_c off_c^T
#if DP_VJP_SKEL
// (off_c: the lane's own frame's bone, from its column `bone`)
DEV void bone_term(const float (*bone)[FPB], int c, int lane, const float (*col)[FPB], const float* Rp, float* dR0, float* M)
#else
DEV void bone_term(const float* __restrict__ W, int c, int lane, const float (*col)[FPB], const float* Rp, float* dR0, float* M)
#endif
{
    const float F0 = col[3 * c][lane], F1 = col[3 * c + 1][lane], F2 = col[3 * c + 2][lane];
#if DP_VJP_SKEL
    const float o0 = bone[3 * c][lane], o1 = bone[3 * c + 1][lane], o2 = bone[3 * c + 2][lane];
#else
    const float o0 = W[OFF_BONE + 3 * c], o1 = W[OFF_BONE + 3 * c + 1], o2 = W[OFF_BONE + 3 * c + 2];
#endif
    float b0 = o0, b1 = o1, b2 = o2;
    if (Rp) {
        b0 = Rp[0] * o0 + Rp[1] * o1 + Rp[2] * o2;
        b1 = Rp[3] * o0 + Rp[4] * o1 + Rp[5] * o2;
        b2 = Rp[6] * o0 + Rp[7] * o1 + Rp[8] * o2;
        M[0] = fmaf(F0, o0, M[0]); M[1] = fmaf(F0, o1, M[1]); M[2] = fmaf(F0, o2, M[2]);
        M[3] = fmaf(F1, o0, M[3]); M[4] = fmaf(F1, o1, M[4]); M[5] = fmaf(F1, o2, M[5]);
        M[6] = fmaf(F2, o0, M[6]); M[7] = fmaf(F2, o1, M[7]); M[8] = fmaf(F2, o2, M[8]);
    }
    dR0[0] = fmaf(F0, b0, dR0[0]); dR0[1] = fmaf(F0, b1, dR0[1]); dR0[2] = fmaf(F0, b2, dR0[2]);
    dR0[3] = fmaf(F1, b0, dR0[3]); dR0[4] = fmaf(F1, b1, dR0[4]); dR0[5] = fmaf(F1, b2, dR0[5]);
    dR0[6] = fmaf(F2, b0, dR0[6]); dR0[7] = fmaf(F2, b1, dR0[7]); dR0[8] = fmaf(F2, b2, dR0[8]);
}

#if DP_VJP_SKEL
// dL/doff_c = R~_p^T (R_0^T F_c) of child bone c of joint p (Rp as in bone_term), stored as row c of the frame's [22][3] (`row`); NaN
// for a refused frame
DEV void doff_row(float* __restrict__ row, int c, int lane, const float (*col)[FPB], const float* R0, const float* Rp, bool bad)
{
    const float F0 = col[3 * c][lane], F1 = col[3 * c + 1][lane], F2 = col[3 * c + 2][lane];
    const float u0 = R0[0] * F0 + R0[3] * F1 + R0[6] * F2;
    const float u1 = R0[1] * F0 + R0[4] * F1 + R0[7] * F2;
    const float u2 = R0[2] * F0 + R0[5] * F1 + R0[8] * F2;
    float g0 = u0, g1 = u1, g2 = u2;
    if (Rp) {
        g0 = Rp[0] * u0 + Rp[3] * u1 + Rp[6] * u2;
        g1 = Rp[1] * u0 + Rp[4] * u1 + Rp[7] * u2;
        g2 = Rp[2] * u0 + Rp[5] * u1 + Rp[8] * u2;
    }
    const float nan = __builtin_nanf("");
    row[3 * c] = bad ? nan : g0;
    row[3 * c + 1] = bad ? nan : g1;
    row[3 * c + 2] = bad ? nan : g2;
}
#endif

} // namespace

#if DP_VJP_SKEL
__global__ __launch_bounds__(FPB) void dp_vjp_skel_kernel(const float* __restrict__ W, SkelArgs a)
#else
__global__ __launch_bounds__(FPB) void dp_vjp_kernel(const float* __restrict__ W, Args a)
#endif
{
    __shared__ float col[3 * NJ][FPB]; // the lane's column: F_j (subtree sums of dL/dP)
#if DP_VJP_SKEL
    __shared__ float bone[3 * NJ][FPB]; // the lane's bones: rows 1..21 of its frame's skeleton (a refused row as zero; row 0 unused)
#endif
    const int lane = threadIdx.x;
    const long long f = (long long)blockIdx.x * FPB + lane;
    if (f >= a.n_frames) return;
    auto F = [&](int j, int c) -> float& { return col[3 * j + c][lane]; };
    const int* __restrict__ T = (const int*)W; // (the skeleton words of the image)

    float z[LAT], cr[4];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < LAT; ++k) { z[k] = a.z[f * LAT + k]; bad |= refused(z[k]); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { cr[k] = a.cur_rot[f * 4 + k]; bad |= refused(cr[k]); }
    if (bad) { // computed on neutral stand-ins (every intermediate finite), the results poisoned at the end
#pragma unroll
        for (int k = 0; k < LAT; ++k) z[k] = 0.f;
        cr[0] = 1.f; cr[1] = cr[2] = cr[3] = 0.f;
    }
#if DP_VJP_SKEL
    { // my frame's skeleton (stride 0: the launch's one), rows 1..21 -- row 0 is never read.  A row with a component out of range
      // refuses the frame (dp_forward_skeleton's rule) and is stored as zero, a neutral stand-in that keeps the arithmetic finite.
        const float* __restrict__ sk = a.skel + (size_t)f * a.skel_stride; // (64-bit: beyond 2^31 / 66 frames a 32-bit product wraps)
#pragma unroll
        for (int c = 1; c < NJ; ++c) {
            const float o0 = sk[3 * c], o1 = sk[3 * c + 1], o2 = sk[3 * c + 2];
            const bool rb = refused(o0) || refused(o1) || refused(o2);
            bone[3 * c][lane] = rb ? 0.f : o0;
            bone[3 * c + 1][lane] = rb ? 0.f : o1;
            bone[3 * c + 2][lane] = rb ? 0.f : o2;
            bad |= rb;
        }
    }
#endif

    // ---- forward: the folded decoder (autoencoder.py:224-256), LeakyReLU(0.2) after layers 0 and 1
    float h0[H0];
    unsigned long long m0 = 0ull, m1 = 0ull; // bit i: pre-activation > 0 (torch's leaky_relu_backward takes the slope 1 there only)
#pragma unroll
    for (int i = 0; i < H0; ++i) {
        float s = W[OFF_C0 + i];
#pragma unroll
        for (int k = 0; k < LAT; ++k) s = fmaf(W[OFF_A0 + i * LAT + k], z[k], s);
        m0 |= (unsigned long long)(s > 0.f) << i;
        h0[i] = s > 0.f ? s : s * 0.2f;
    }
    float h1[H1];
#pragma unroll
    for (int i = 0; i < H1; ++i) {
        float s = W[OFF_B1 + i];
#pragma unroll
        for (int k = 0; k < H0; ++k) s = fmaf(W[OFF_A1 + i * H0 + k], h0[k], s);
        m1 |= (unsigned long long)(s > 0.f) << i;
        h1[i] = s > 0.f ? s : s * 0.2f;
    }
    // de-normalised, per-joint normalised quaternions (autoencoder.py:242-250) and displacement (drag_pose.py:84-85)
    float q[NJ][4], d[3]; // (kept unnormalised: qn and 1/|q| are recomputed where used, 22 registers fewer)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int o = 4 * j + c;
            float s = W[OFF_B2 + o];
#pragma unroll
            for (int k = 0; k < H1; ++k) s = fmaf(W[OFF_A2 + o * H1 + k], h1[k], s);
            q[j][c] = fmaf(s, W[OFF_SD + o], W[OFF_MU + o]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int o = 4 * NJ + c;
        float s = W[OFF_B2 + o];
#pragma unroll
        for (int k = 0; k < H1; ++k) s = fmaf(W[OFF_A2 + o * H1 + k], h1[k], s);
        d[c] = fmaf(s, W[OFF_SD + o], W[OFF_MU + o]);
    }
    // world root rotation, cur_rot unnormalised (drag_pose.py:88)
    float wr[4], R0[9], qn0[4], rn0;
    unit(q[0], qn0, rn0);
    quat_mul(cr, qn0, wr);
    rotmat(wr, R0);

    // ---- backward
    float dR0[9];
    if (a.g_rot) {
#pragma unroll
        for (int k = 0; k < 9; ++k) dR0[k] = a.g_rot[f * NJ * 9 + k];
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) dR0[k] = 0.f;
    }
    // the column holds dL/dP_j, then summed up the tree (parent[j] < j): F_j
    if (a.g_pos) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) F(j, c) = a.g_pos[(f * NJ + j) * 3 + c];
        for (int j = NJ - 1; j >= 1; --j) {
            const int p = T[OFF_PARENT + j];
            F(p, 0) += F(j, 0); F(p, 1) += F(j, 1); F(p, 2) += F(j, 2);
        }
    } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j) F(j, 0) = F(j, 1) = F(j, 2) = 0.f;
    }
    // sum_j dL/dP_j v_j^T = sum_c F_c b_c^T over the bones b_c = R~_p off_c: the root's children here, the others with their parent below
#if DP_VJP_SKEL
    float* __restrict__ doff = a.doff ? a.doff + f * (3 * NJ) : nullptr; // (my frame's [22][3] rows of dL/d(offsets), on request)
    for (int k = T[OFF_CSTART]; k < T[OFF_CSTART + 1]; ++k) {
        bone_term(bone, T[OFF_CLIST + k], lane, col, nullptr, dR0, nullptr);
        if (a.doff) doff_row(doff, T[OFF_CLIST + k], lane, col, R0, nullptr, bad);
    }
#else
    for (int k = T[OFF_CSTART]; k < T[OFF_CSTART + 1]; ++k)
        bone_term(W, T[OFF_CLIST + k], lane, col, nullptr, dR0, nullptr);
#endif
    // world_disp = R_0 d (P_0 = world_disp, every P_j carries it)
    float gwd[3], dd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gwd[c] = F(0, c) + (a.g_wdisp ? a.g_wdisp[f * 3 + c] : 0.f);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) dR0[3 * r + c] = fmaf(gwd[r], d[c], dR0[3 * r + c]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        dd[c] = R0[c] * gwd[0] + R0[3 + c] * gwd[1] + R0[6 + c] * gwd[2] + (a.g_disp ? a.g_disp[f * 3 + c] : 0.f);

    float dh1[H1];
#pragma unroll
    for (int k = 0; k < H1; ++k) dh1[k] = 0.f;
#pragma unroll
    for (int j = 1; j < NJ; ++j) {
        float Rj[9], M[9], qn[4], rn;
        unit(q[j], qn, rn);
        rotmat(qn, Rj);
        if (a.g_rot) {
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = a.g_rot[(f * NJ + j) * 9 + k];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    dR0[3 * r + c] += M[3 * r] * Rj[3 * c] + M[3 * r + 1] * Rj[3 * c + 1] + M[3 * r + 2] * Rj[3 * c + 2];
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = 0.f;
        }
#if DP_VJP_SKEL
        for (int k = T[OFF_CSTART + j]; k < T[OFF_CSTART + j + 1]; ++k) {
            bone_term(bone, T[OFF_CLIST + k], lane, col, Rj, dR0, M);
            if (a.doff) doff_row(doff, T[OFF_CLIST + k], lane, col, R0, Rj, bad);
        }
#else
        for (int k = T[OFF_CSTART + j]; k < T[OFF_CSTART + j + 1]; ++k) bone_term(W, T[OFF_CLIST + k], lane, col, Rj, dR0, M);
#endif
        float dRj[9], dqn[4];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) dRj[3 * r + c] = R0[r] * M[c] + R0[3 + r] * M[3 + c] + R0[6 + r] * M[6 + c];
        rotmat_vjp(qn, dRj, dqn);
        if (a.g_pose)
#pragma unroll
            for (int c = 0; c < 4; ++c) dqn[c] += a.g_pose[f * 88 + 4 * j + c] / W[OFF_SD + 4 * j + c];
        quad_to_dh1(W, 4 * j, qn, rn, dqn, dh1);
    }
    // root: world_rot = cur_rot (x) q_0
    float dw[4], dq0[4], dc[4];
    rotmat_vjp(wr, dR0, dw);
    if (a.g_wrot)
#pragma unroll
        for (int c = 0; c < 4; ++c) dw[c] += a.g_wrot[f * 4 + c];
    {
        const float* b = qn0;
        dc[0] = dw[0] * b[0] + dw[1] * b[1] + dw[2] * b[2] + dw[3] * b[3];
        dc[1] = -dw[0] * b[1] + dw[1] * b[0] - dw[2] * b[3] + dw[3] * b[2];
        dc[2] = -dw[0] * b[2] + dw[1] * b[3] + dw[2] * b[0] - dw[3] * b[1];
        dc[3] = -dw[0] * b[3] - dw[1] * b[2] + dw[2] * b[1] + dw[3] * b[0];
        dq0[0] = dw[0] * cr[0] + dw[1] * cr[1] + dw[2] * cr[2] + dw[3] * cr[3];
        dq0[1] = -dw[0] * cr[1] + dw[1] * cr[0] + dw[2] * cr[3] - dw[3] * cr[2];
        dq0[2] = -dw[0] * cr[2] - dw[1] * cr[3] + dw[2] * cr[0] + dw[3] * cr[1];
        dq0[3] = -dw[0] * cr[3] + dw[1] * cr[2] - dw[2] * cr[1] + dw[3] * cr[0];
    }
    if (a.g_pose)
#pragma unroll
        for (int c = 0; c < 4; ++c) dq0[c] += a.g_pose[f * 88 + c] / W[OFF_SD + c];
    quad_to_dh1(W, 0, qn0, rn0, dq0, dh1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float dy = dd[c] * W[OFF_SD + 4 * NJ + c];
#pragma unroll
        for (int k = 0; k < H1; ++k) dh1[k] = fmaf(W[OFF_A2 + (4 * NJ + c) * H1 + k], dy, dh1[k]);
    }

    // ---- decoder backward: A1^T, A0^T with the recomputed LeakyReLU slopes
    float dh0[H0];
#pragma unroll
    for (int i = 0; i < H0; ++i) dh0[i] = 0.f;
#pragma unroll
    for (int k = 0; k < H1; ++k) {
        const float g = (m1 >> k) & 1ull ? dh1[k] : dh1[k] * 0.2f;
#pragma unroll
        for (int i = 0; i < H0; ++i) dh0[i] = fmaf(W[OFF_A1 + k * H0 + i], g, dh0[i]);
    }
    float gz[LAT];
#pragma unroll
    for (int k = 0; k < LAT; ++k) gz[k] = 0.f;
#pragma unroll
    for (int i = 0; i < H0; ++i) {
        const float g = (m0 >> i) & 1ull ? dh0[i] : dh0[i] * 0.2f;
#pragma unroll
        for (int k = 0; k < LAT; ++k) gz[k] = fmaf(W[OFF_A0 + i * LAT + k], g, gz[k]);
    }
    bool fin = true;
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < LAT; ++k) { a.dz[f * LAT + k] = bad ? nan : gz[k]; fin &= isfinite(gz[k]); }
    if (a.dcur)
#pragma unroll
        for (int k = 0; k < 4; ++k) a.dcur[f * 4 + k] = bad ? nan : dc[k];
#if DP_VJP_SKEL
    if (a.doff) // (row 0, the root's OFFSET, is no input of the function: its gradient is zero)
#pragma unroll
        for (int c = 0; c < 3; ++c) doff[c] = bad ? nan : 0.f;
#endif
    if (a.status) a.status[f] = bad ? DP_STATUS_BAD_STATE : fin ? 0 : DP_STATUS_NONFINITE_RESULT;
}
