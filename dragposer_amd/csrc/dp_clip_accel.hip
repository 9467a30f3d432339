// dp_clip_accel.hip -- dp_optimize_clip_lm_accel (include/dragposer_clip_accel.h): dp_optimize_clip_lm's problem with a second-difference
// (acceleration) term beside the first-difference one.  The Gauss-Newton system of a sequence is block-pentadiagonal with 24 x 24 blocks; its
// off-diagonal blocks are K[t,t-1] I and K[t,t-2] I, and its Cholesky factor has dense blocks F_t and E_t = k2 L_(t-2)^-T below the diagonal.
// The rows kernel is dp_clip.hip's, unchanged; the launch train is dp_clip.h's train() with this unit's chain and decision as its parameters.
//
// dp_clip_accel_chain_kernel   one wave per sequence.  Forwards over t, four 24 x 24 x 24 products on v_mfma_f32_16x16x4_f32:
//                              F_t = (k1 I - k2 Q_t) L_(t-1)^-T,  F_t F_t^T,  Q_(t+1) = L_(t-1)^-T F_t^T (formed a frame ahead, while L_(t-1)^-1
//                              is still in its place),  P_t = L_t^-T L_t^-1.  S_t = M_tt - k2^2 P_(t-2) - F_t F_t^T; Cholesky, L_t^-1 and y_t are
//                              dp_clip_chain_kernel's text (dp_clip_factor.h).  L_t^-1 | y_t | F_t go to the workspace.  Backwards over t:
//                              Delta_t = L_t^-T (y_t - F_(t+1)^T Delta_(t+1) - K[t+2,t] L_t^-1 Delta_(t+2)), Z' = Z + Delta.  The next frame's
//                              block is fetched while this frame's is worked on, in both sweeps.  The recursion is fp32.
// dp_clip_accel_decide_kernel  one wave per sequence: dp_clip_decide_kernel's text (dp_clip_total.h, dp_clip_decide_body.h) with DP_CLIP_ACCEL 1:
//                              |z_(t+1) - 2 z_t + z_(t-1)|^2 of the kept and of the trial latents read from the latent buffers and added in
//                              double, each component in index order.
// No atomics, no host synchronisation, no allocation: two launches give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_clip_accel.h"
#include "dp_clip_accel.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"
#include "dp_clip_dev.h"

namespace K = dpclip;
namespace KA = dpclipacc;
static_assert(KA::LAT == LAT, "dp_lm.h's frame");

// Row t of the scalar band matrix K = c1 Lap + c2 D2^T D2 of a chain of T frames: kd = K[t,t], k1 = K[t,t-1], k2 = K[t,t-2], and w[i] = 1 where
// frame t-1+i is the centre of a second-difference window (1 <= centre <= T-2), else 0.  Every end row (T <= 4, the second and the second-to-last
// row) comes out of this: a window contributes 1, -2, 1 at its three frames.
struct Band {
    float kd, k1, k2, w[3];
};
DEV Band band(int t, int T, float c1, float c2)
{
    Band b;
#pragma unroll
    for (int i = 0; i < 3; ++i) b.w[i] = t - 1 + i >= 1 && t - 1 + i <= T - 2 ? 1.f : 0.f;
    b.kd = c1 * ((t > 0 ? 1.f : 0.f) + (t < T - 1 ? 1.f : 0.f)) + c2 * (b.w[0] + 4.f * b.w[1] + b.w[2]);
    b.k1 = t > 0 ? -c1 - 2.f * c2 * (b.w[0] + b.w[1]) : 0.f;
    b.k2 = c2 * b.w[0]; // (t-1 a centre: t >= 2)
    return b;
}

// One wave per sequence: M Delta = -G by the block recursion of include/dragposer_clip_accel.h, then Z' = Z + Delta.
__global__ __launch_bounds__(64) void dp_clip_accel_chain_kernel(KA::Args aa)
{
    __shared__ __attribute__((aligned(16))) float lds[KA::CHAIN_LDS_FLOATS];
    const K::Args& a = aa.c;
    const int lane = threadIdx.x, sq = blockIdx.x;
    const int word = a.wword[sq];
    if ((word & K::W_REFUSED) != 0) return;
    const int cur = (word & K::W_CUR) != 0 ? 1 : 0;
    const float* __restrict__ Z = a.wz[cur];
    float* __restrict__ ZN = a.wz[cur ^ 1];
    const int S = a.n_seq, T = a.n_t;
    const float c1 = a.lam_smooth / 24.f, c2 = aa.lam_accel / 24.f, mu1 = 1.f + a.wmu[sq];
    float *SB = lds + KA::C_S, *IB = lds + KA::C_I, *FB = lds + KA::C_F, *QB = lds + KA::C_Q, *GV = lds + KA::C_V, *NV = GV + 32, *YV = GV + 64,
          *WV = GV + 96, *D1 = GV + 128, *D2 = GV + 160;
    constexpr int CS = KA::CS, NPRE = (K::AG_FLOATS + 63) / 64, NPF = (KA::LF_FLOATS + 63) / 64;
    const int li = lane < LAT ? lane : LAT - 1; // (lanes beyond the 24 rows repeat the last one and store nothing)
    const bool in = lane < LAT;
    const int lr16 = lane & 15, lk = lane >> 4;

    // before frame 0 there is nothing: P, L^-1, F, Q and y are 0, and frames 0 and 1 run the same statements as every other
    for (int e = lane; e < KA::CHAIN_LDS_FLOATS; e += 64) lds[e] = 0.f;
    float pre[NPF]; // the next frame's block, in flight while this frame's is worked on
    const auto fetch = [&](const float* __restrict__ src, int n) { fetch64(pre, src, n, lane); };
    fetch(a.wag + (long long)sq * K::AG_FLOATS, K::AG_FLOATS);
    const auto zat = [&](int t) { return t < T ? Z[((long long)t * S + sq) * LAT + li] : 0.f; };
    float zm2 = 0.f, zm1 = 0.f, zc = zat(0), zp1 = zat(1), zp2 = zat(2); // component `lane` of z_(t-2) .. z_(t+2)
    float u1 = 0.f, u2 = 0.f;                                            // component `lane` of L^-T y of frames t-1 and t-2
    bool ok = true;
    wave_sync();
    for (int t = 0; t < T; ++t) {
        const long long f = (long long)t * S + sq;
        const Band kb = band(t, T, c1, c2);
        float* const PB = lds + KA::C_P + (t & 1) * KA::MAT; // P_(t-2) now, P_t at the end of the frame
        float* const lo = a.wli + f * KA::LF_FLOATS;
        f4 acc[2][2];
        // ---- F_t = (k1 I - k2 Q_t) L_(t-1)^-T
        mm24([&](int i, int m) { return fmaf(-kb.k2, QB[i * CS + m], i == m ? kb.k1 : 0.f); }, [&](int m, int j) { return IB[j * CS + m]; }, acc, lr16, lk);
        wave_sync(); // (Q_t's last reads before Q_(t+1) takes its place)
        each24(acc, lr16, lk, [&](int r, int cc, float v) {
            FB[r * CS + cc] = v;
            lo[K::LI_FLOATS + r * LAT + cc] = v;
        });
        wave_sync();
        // ---- Q_(t+1) = L_(t-1)^-T F_t^T, while L_(t-1)^-1 is in its place
        mm24([&](int i, int m) { return IB[m * CS + i]; }, [&](int m, int j) { return FB[j * CS + m]; }, acc, lr16, lk);
        each24(acc, lr16, lk, [&](int r, int cc, float v) { QB[r * CS + cc] = v; });
        // ---- S_t = M_tt - k2^2 P_(t-2) - F_t F_t^T, g_t aside
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = lane + 64 * i;
            if (e < K::AG_FLOATS) {
                const int r = e / LAT, cc = e - LAT * r;
                float v = pre[i];
                if (r < LAT) {
                    if (r == cc) v = (v + kb.kd) * mu1;
                    SB[r * CS + cc] = fmaf(-kb.k2 * kb.k2, PB[r * CS + cc], v);
                } else GV[cc] = v;
            }
        }
        if (t + 1 < T) fetch(a.wag + (f + S) * K::AG_FLOATS, K::AG_FLOATS);
        const float zp3 = zat(t + 3);
        mm24([&](int i, int m) { return FB[i * CS + m]; }, [&](int m, int j) { return FB[j * CS + m]; }, acc, lr16, lk);
        wave_sync();
        each24(acc, lr16, lk, [&](int r, int cc, float v) { SB[r * CS + cc] -= v; });
        // ---- Cholesky in place, 1 / L_kk (dp_clip_factor.h: dp_clip_chain_kernel's text)
#define CLIP_FACTOR 1
#include "dp_clip_factor.h"
#undef CLIP_FACTOR
        // the right-hand side: -G_t - E_t y_(t-2) - F_t y_(t-1), lane i on component i (y_(t-1) is still in its place).  (K Z)_t is formed from
        // the differences, not from K's entries: the windows centred on t-1, t and t+1
        const float at_m = (zc - 2.f * zm1) + zm2, at_0 = (zp1 - 2.f * zc) + zm1, at_p = (zp2 - 2.f * zp1) + zc;
        const float kz = c1 * ((t > 0 ? zc - zm1 : 0.f) + (t < T - 1 ? zc - zp1 : 0.f)) + c2 * ((kb.w[0] * at_m - 2.f * kb.w[1] * at_0) + kb.w[2] * at_p);
        float fy = 0.f;
#pragma unroll
        for (int m = 0; m < LAT; ++m) fy = fmaf(FB[li * CS + m], YV[m], fy);
        const float rhs = fmaf(-kb.k2, u2, -(GV[li] + kz)) - fy;
        // ---- L_t^-1 | y_t into registers, LDS and the workspace
#define CLIP_FACTOR 2
#define CLIP_LI CS
#define CLIP_WS lo
#include "dp_clip_factor.h"
#undef CLIP_WS
#undef CLIP_LI
#undef CLIP_FACTOR
        // ---- P_t = L_t^-T L_t^-1, for frame t+2
        if (t + 2 < T) {
            mm24([&](int i, int m) { return IB[m * CS + i]; }, [&](int m, int j) { return IB[m * CS + j]; }, acc, lr16, lk);
            each24(acc, lr16, lk, [&](int r, int cc, float v) { PB[r * CS + cc] = v; });
        }
        wave_sync();
        float u = 0.f; // L_t^-T y_t, from the column of L_t^-1 this lane holds
#pragma unroll
        for (int r = 0; r < LAT; ++r) u = fmaf(x[r], YV[r], u);
        u2 = u1; u1 = u;
        zm2 = zm1; zm1 = zc; zc = zp1; zp1 = zp2; zp2 = zp3;
    }
    if (lane == 0) a.wsolved[sq] = ok ? 1 : 0;
    if (!ok) return;

    // ---- backwards.  Frame T-1's block is still in its place; the others come back from the workspace, where this wave wrote them
    __threadfence();
    float d1 = 0.f, d2 = 0.f; // lane i: component i of Delta_(t+1), Delta_(t+2)
    if (T > 1) fetch(a.wli + ((long long)(T - 2) * S + sq) * KA::LF_FLOATS, KA::LF_FLOATS);
    for (int t = T - 1; t >= 0; --t) {
        const long long f = (long long)t * S + sq;
        if (in) { D1[lane] = d1; D2[lane] = d2; }
        wave_sync();
        float fv = 0.f; // F_(t+1)^T Delta_(t+1): F_(t+1) is the block of the frame before
#pragma unroll
        for (int r = 0; r < LAT; ++r) fv = fmaf(FB[r * CS + li], D1[r], fv);
        if (t < T - 1) {
            wave_sync();
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
                const int e = lane + 64 * i;
                if (e < K::LI_FLOATS) {
                    const int r = e / LAT, cc = e - LAT * r;
                    if (r < LAT) IB[r * CS + cc] = pre[i];
                    else YV[cc] = pre[i];
                } else if (e < KA::LF_FLOATS) {
                    const int g = e - K::LI_FLOATS, r = g / LAT, cc = g - LAT * r;
                    FB[r * CS + cc] = pre[i];
                }
            }
            if (t > 0) fetch(a.wli + (f - S) * KA::LF_FLOATS, KA::LF_FLOATS);
            wave_sync();
        }
        float v = 0.f;
#pragma unroll
        for (int m = 0; m < LAT; ++m) v = fmaf(IB[li * CS + m], D2[m], v);
        if (in) WV[lane] = fmaf(-band(t + 2, T, c1, c2).k2, v, YV[lane] - fv);
        wave_sync();
        float dl = 0.f;
#pragma unroll
        for (int r = 0; r < LAT; ++r) dl = fmaf(IB[r * CS + li], WV[r], dl);
        if (in) ZN[f * LAT + lane] = Z[f * LAT + lane] + dl;
        d2 = d1;
        d1 = dl;
        wave_sync(); // (this frame's last reads before the next block takes its place)
    }
}

// dp_clip.hip's totals and decision, with the second-difference part in the totals and kept beside them
#define DP_CLIP_ACCEL 1
DEV double clip_total(const KA::Args& aa, int b, int sq, int lane, double& cp, double& ap)
#include "dp_clip_total.h"
__global__ __launch_bounds__(64) void dp_clip_accel_decide_kernel(KA::Args aa)
#include "dp_clip_decide_body.h"
#undef DP_CLIP_ACCEL

hipError_t dp_launch_clip_accel(const KA::Args* args, hipStream_t stream)
{
    const K::Rows rows = {K::plain_rows, nullptr};
    return dp_launch_clip_accel_train(args, &rows, stream);
}

hipError_t dp_launch_clip_accel_train(const KA::Args* args, const K::Rows* rows, hipStream_t stream)
{
    KA::Args k = *args;
    if (k.lam_accel == 0.f) { // dp_optimize_clip_lm's own train (its chain reads the first 600 floats of a frame's factor block), the new output 0
        hipError_t e = dp_launch_clip_train(&k.c, rows, stream);
        if (e == hipSuccess && k.accel_loss) e = hipMemsetAsync(k.accel_loss, 0, sizeof(double) * (size_t)k.c.n_seq, stream);
        return e;
    }
    const auto launch = [&](void (*kernel)(KA::Args)) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)k.c.n_seq), dim3(64), 0, stream, k);
        return hipGetLastError();
    };
    return K::train(&k.c, rows, stream, [&] { return launch(dp_clip_accel_chain_kernel); }, [&] { return launch(dp_clip_accel_decide_kernel); });
}
