// dp_clip.hip -- dp_optimize_clip_lm (include/dragposer_clip_lm.h): S sequences of T frames solved jointly by Levenberg-Marquardt steps, the
// latents of a sequence tied frame to frame.  The Gauss-Newton system of a sequence is block-tridiagonal with 24 x 24 blocks and off-diagonal
// blocks -c I.  Three kernels in a fixed train on the caller's stream (dp_launch_clip); what connects them is the caller's workspace (dp_clip.h).
//
// dp_clip_rows_kernel    one frame per wave, dp_lm.hip's layout: the forward pass, the tangents through the folded decoder and [J r]^T [J r]
//                        on v_mfma_f32_16x16x4_f32 are the text dp_lm_body.h includes, dp_lm_frame_*.h.  By mode it writes A_t | g_t and the frame's
//                        loss numbers (the pass of z0, and again wherever Z has moved), the loss alone (a trial), or every dp_result array (at
//                        the end).  A frame of a sequence whose last trial was rejected is skipped: its A and g stand.  Its text is
//                        dp_clip_rows_body.h, shared with dp_clip_skel.hip's kernel (the bones of each sequence's own skeleton).
// dp_clip_chain_kernel   one wave per sequence.  Forwards over t: S_t = M_tt - c^2 P_(t-1) with the damping on its diagonal; Cholesky
//                        left-looking, lane i on row i (dp_lm_body.h's); L_t^-1 by 24 forward substitutions, lane i on column i, in registers;
//                        y_t; P_t = L_t^-T L_t^-1 on the fp32 MFMA.  L_t^-1 | y_t go to the workspace.  Backwards over t:
//                        Delta_t = L_t^-T (y_t + c L_t^-1 Delta_(t+1)), Z' = Z + Delta.  The next frame's block is fetched while this
//                        frame's is worked on.  The recursion is fp32.
// dp_clip_decide_kernel  one wave per sequence: the frames' numbers added in double in index order, L_s(Z') < L_s(Z), mu, the word.
// No atomics, no host synchronisation, no allocation: two launches give the same bits.
//
// Shared with dp_clip_accel.hip, each written once: the chain's factor step (Cholesky with the pivot screen, L_t^-1, y_t) is the text
// dp_clip_factor.h, the block fetch dp_clip_dev.h's fetch64; the totals and the decision are the texts dp_clip_total.h and
// dp_clip_decide_body.h (DP_CLIP_ACCEL); the launch train is dp_clip.h's train(), with this unit's chain and decision as its parameters.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_clip_lm.h"
#include "dp_clip.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"
#include "dp_clip_dev.h"

namespace K = dpclip;
static_assert(K::LAT == LAT && K::WPB == WPB, "dp_lm.h's frame");

// the frame's pass, shared with dp_clip_skel.hip (DP_CLIP_SKEL 1: the bones of the frame's own sequence)
#define DP_CLIP_SKEL 0
__global__ __launch_bounds__(WPB * 64) void dp_clip_rows_kernel(K::Args a)
#include "dp_clip_rows_body.h"
#undef DP_CLIP_SKEL

// One wave per sequence: M Delta = -G by the block recursion of include/dragposer_clip_lm.h, then Z' = Z + Delta.
__global__ __launch_bounds__(64) void dp_clip_chain_kernel(K::Args a)
{
    __shared__ __attribute__((aligned(16))) float lds[K::CHAIN_LDS_FLOATS];
    const int lane = threadIdx.x, sq = blockIdx.x;
    const int word = a.wword[sq];
    if ((word & K::W_REFUSED) != 0) return;
    const int cur = (word & K::W_CUR) != 0 ? 1 : 0;
    const float* __restrict__ Z = a.wz[cur];
    float* __restrict__ ZN = a.wz[cur ^ 1];
    const int S = a.n_seq, T = a.n_t;
    const float c = a.lam_smooth / 24.f, c2 = c * c, mu1 = 1.f + a.wmu[sq];
    float *SB = lds + K::C_S, *PB = lds + K::C_P, *IB = lds + K::C_I, *GV = lds + K::C_V, *NV = GV + 32, *YV = GV + 64, *WV = GV + 96;
    constexpr int CS = K::CS, CI = K::CI, NPRE = (K::AG_FLOATS + 63) / 64;
    const int li = lane < LAT ? lane : LAT - 1; // (lanes beyond the 24 rows repeat the last one and store nothing)
    const bool in = lane < LAT;
    const int lr16 = lane & 15, lk = lane >> 4;

    for (int e = lane; e < LAT * 8; e += 64) IB[(e >> 3) * CI + LAT + (e & 7)] = 0.f; // columns 24..31 of L^-1 as the matrix pipe reads it
    float pre[NPRE]; // the next frame's block, in flight while this frame's is worked on
    const auto fetch = [&](const float* __restrict__ src) { fetch64(pre, src, K::AG_FLOATS, lane); }; // (= LI_FLOATS)
    fetch(a.wag + (long long)sq * K::AG_FLOATS);
    float zp = 0.f, zc = Z[(long long)sq * LAT + li], zn = 0.f;
    float xp[LAT]; // column `lane` of L_(t-1)^-1
#pragma unroll
    for (int r = 0; r < LAT; ++r) xp[r] = 0.f;
    bool ok = true;
    for (int t = 0; t < T; ++t) {
        const long long f = (long long)t * S + sq;
        const float deg = (t > 0 ? 1.f : 0.f) + (t < T - 1 ? 1.f : 0.f);
        // ---- S_t = M_tt - c^2 P_(t-1), g_t aside
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = lane + 64 * i;
            if (e < K::AG_FLOATS) {
                const int r = e / LAT, cc = e - LAT * r;
                float v = pre[i];
                if (r < LAT) {
                    if (r == cc) v = (v + c * deg) * mu1;
                    if (t > 0) v = fmaf(-c2, PB[r * CS + cc], v);
                    SB[r * CS + cc] = v;
                } else GV[cc] = v;
            }
        }
        if (t + 1 < T) {
            fetch(a.wag + (f + S) * K::AG_FLOATS);
            zn = Z[(f + S) * LAT + li];
        }
        // ---- Cholesky in place, 1 / L_kk (dp_clip_factor.h: the text dp_clip_accel.hip's chain runs)
#define CLIP_FACTOR 1
#include "dp_clip_factor.h"
#undef CLIP_FACTOR
        // the right-hand side: -G_t + c L_(t-1)^-T y_(t-1), lane i on component i (y_(t-1) is still in its place)
        float rhs = -(GV[li] + c * ((t > 0 ? zc - zp : 0.f) + (t < T - 1 ? zc - zn : 0.f)));
        if (t > 0) {
            float u = 0.f;
#pragma unroll
            for (int r = 0; r < LAT; ++r) u = fmaf(xp[r], YV[r], u);
            rhs = fmaf(c, u, rhs);
        }
        // ---- L_t^-1 | y_t into registers, LDS and the workspace
#define CLIP_FACTOR 2
#define CLIP_LI CI
#define CLIP_WS (a.wli + f * K::LI_FLOATS)
#include "dp_clip_factor.h"
#undef CLIP_WS
#undef CLIP_LI
#undef CLIP_FACTOR
        // ---- P_t = L_t^-T L_t^-1 on the matrix pipe (K = the 24 rows, both operands the same values)
        if (t + 1 < T) {
            f4 na[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) na[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const float v0 = IB[(4 * s + lk) * CI + lr16], v1 = IB[(4 * s + lk) * CI + 16 + lr16];
                na[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v0, na[0][0], 0, 0, 0);
                na[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v1, na[0][1], 0, 0, 0);
                na[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v0, na[1][0], 0, 0, 0);
                na[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v1, na[1][1], 0, 0, 0);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * mt + 4 * lk + r;
                    if (row < LAT) {
                        PB[row * CS + lr16] = na[mt][0][r];
                        if (lr16 < LAT - 16) PB[row * CS + 16 + lr16] = na[mt][1][r];
                    }
                }
        }
#pragma unroll
        for (int r = 0; r < LAT; ++r) xp[r] = x[r];
        zp = zc;
        zc = zn;
        wave_sync(); // (this frame's last reads of its block and of y before the next frame's writes)
    }
    if (lane == 0) a.wsolved[sq] = ok ? 1 : 0;
    if (!ok) return;

    // ---- backwards: Delta_t = L_t^-T (y_t + c L_t^-1 Delta_(t+1)).  Frame T-1's block is still in its place; the others come back from the
    // workspace, where this wave wrote them
    __threadfence();
    float dn = 0.f; // lane i: component i of Delta_(t+1)
    if (T > 1) fetch(a.wli + ((long long)(T - 2) * S + sq) * K::LI_FLOATS);
    for (int t = T - 1; t >= 0; --t) {
        const long long f = (long long)t * S + sq;
        if (t < T - 1) {
#pragma unroll
            for (int i = 0; i < NPRE; ++i) {
                const int e = lane + 64 * i;
                if (e < K::LI_FLOATS) {
                    const int r = e / LAT, cc = e - LAT * r;
                    if (r < LAT) IB[r * CI + cc] = pre[i];
                    else YV[cc] = pre[i];
                }
            }
            if (t > 0) fetch(a.wli + (f - S) * K::LI_FLOATS);
        }
        if (in) GV[lane] = dn;
        wave_sync();
        float v = 0.f;
#pragma unroll
        for (int m = 0; m < LAT; ++m) v = fmaf(IB[li * CI + m], GV[m], v);
        if (in) WV[lane] = fmaf(c, v, YV[lane]);
        wave_sync();
        float dl = 0.f;
#pragma unroll
        for (int r = 0; r < LAT; ++r) dl = fmaf(IB[r * CI + li], WV[r], dl);
        if (in) ZN[f * LAT + lane] = Z[f * LAT + lane] + dl;
        dn = dl;
        wave_sync(); // (this frame's last reads before the next block takes its place)
    }
}

// the per-sequence totals and the decision: shared with dp_clip_accel.hip (DP_CLIP_ACCEL 1: the second-difference part beside them)
#define DP_CLIP_ACCEL 0
DEV double clip_total(const K::Args& a, int b, int sq, int lane, double& cp)
#include "dp_clip_total.h"
__global__ __launch_bounds__(64) void dp_clip_decide_kernel(K::Args a)
#include "dp_clip_decide_body.h"
#undef DP_CLIP_ACCEL

// one pass of the rows kernel in `mode` (M_*): also what another unit's launch train (dp_clip_accel.hip) runs between its own kernels
hipError_t dp_launch_clip_rows(const K::Args* args, int mode, hipStream_t stream)
{
    K::Args k = *args;
    k.mode = mode;
    hipLaunchKernelGGL(dp_clip_rows_kernel, dim3((unsigned)((k.n_frames + WPB - 1) / WPB)), dim3(WPB * 64), 0, stream, k);
    return hipGetLastError();
}

hipError_t dp_launch_clip(const K::Args* args, hipStream_t stream)
{
    const K::Rows rows = {K::plain_rows, nullptr};
    return dp_launch_clip_train(args, &rows, stream);
}

hipError_t dp_launch_clip_train(const K::Args* args, const K::Rows* rows, hipStream_t stream)
{
    K::Args k = *args;
    const auto launch = [&](void (*kernel)(K::Args)) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)k.n_seq), dim3(64), 0, stream, k);
        return hipGetLastError();
    };
    return K::train(&k, rows, stream, [&] { return launch(dp_clip_chain_kernel); }, [&] { return launch(dp_clip_decide_kernel); });
}
