// dp_clip_accel.hip -- dp_optimize_clip_lm_accel (include/dragposer_clip_accel.h): dp_optimize_clip_lm's problem with a second-difference
// (acceleration) term beside the first-difference one.  The Gauss-Newton system of a sequence is block-pentadiagonal with 24 x 24 blocks; its
// off-diagonal blocks are K[t,t-1] I and K[t,t-2] I, and its Cholesky factor has dense blocks F_t and E_t = k2 L_(t-2)^-T below the diagonal.
// The rows kernel is dp_clip.hip's, unchanged; the launch train is dp_launch_clip's with this unit's chain and decision in their places.
//
// dp_clip_accel_chain_kernel   one wave per sequence.  Forwards over t, four 24 x 24 x 24 products on v_mfma_f32_16x16x4_f32:
//                              F_t = (k1 I - k2 Q_t) L_(t-1)^-T,  F_t F_t^T,  Q_(t+1) = L_(t-1)^-T F_t^T (formed a frame ahead, while L_(t-1)^-1
//                              is still in its place),  P_t = L_t^-T L_t^-1.  S_t = M_tt - k2^2 P_(t-2) - F_t F_t^T; Cholesky, L_t^-1 and y_t as
//                              dp_clip_chain_kernel has them.  L_t^-1 | y_t | F_t go to the workspace.  Backwards over t:
//                              Delta_t = L_t^-T (y_t - F_(t+1)^T Delta_(t+1) - K[t+2,t] L_t^-1 Delta_(t+2)), Z' = Z + Delta.  The next frame's
//                              block is fetched while this frame's is worked on, in both sweeps.  The recursion is fp32.
// dp_clip_accel_decide_kernel  one wave per sequence: dp_clip_decide_kernel's sums, with |z_(t+1) - 2 z_t + z_(t-1)|^2 of the kept and of the
//                              trial latents read from the latent buffers and added in double, each component in index order.
// No atomics, no host synchronisation, no allocation: two launches give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_clip_accel.h"
#include "dp_clip_accel.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"

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

// acc[mt][nt] += sum_k a(16 mt + i, k) b(k, 16 nt + j) over k < 24 on the fp32 matrix pipe.  Lane l: row l & 15 of an A tile, K-slot l >> 4;
// column l & 15 of a B tile.  Rows and columns 24..31 of the second tiles repeat row / column 23: their results are not kept.
template <class FA, class FB>
DEV void mm24(const FA& a, const FB& b, f4 (&acc)[2][2], int lr16, int lk)
{
    const int r1 = 16 + lr16 < LAT ? 16 + lr16 : LAT - 1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int k = 4 * s + lk;
        const float a0 = a(lr16, k), a1 = a(r1, k), b0 = b(k, lr16), b1 = b(k, r1);
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}
// what a lane holds of a product: f(row, column, value) for its elements inside 24 x 24
template <class F>
DEV void each24(const f4 (&acc)[2][2], int lr16, int lk, const F& f)
{
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * mt + 4 * lk + r;
            if (row < LAT) {
                f(row, lr16, acc[mt][0][r]);
                if (lr16 < LAT - 16) f(row, 16 + lr16, acc[mt][1][r]);
            }
        }
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
    const auto fetch = [&](const float* __restrict__ src, int n) {
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = lane + 64 * i;
            if (64 * i < n) pre[i] = e < n ? src[e] : 0.f;
        }
    };
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
        // ---- Cholesky in place, left-looking: lane i >= k forms s = S_ik - sum_(m<k) L_im L_km from its own row and row k
        float myinv = 0.f;
        for (int k = 0; k < LAT; ++k) {
            wave_sync();
            float s = SB[li * CS + k];
#pragma unroll 4
            for (int m = 0; m < k; ++m) s = fmaf(-SB[li * CS + m], SB[k * CS + m], s);
            const float piv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), k));
            ok = ok && piv > 0.f && piv <= 3.0e38f;
            const float inv = 1.f / sqrtf(piv);
            if (lane == k) myinv = inv;
            if (lane > k && in) SB[lane * CS + k] = s * inv;
        }
        if (!ok) break; // (wave-uniform: the pivots are)
        if (in) NV[lane] = myinv;
        // the right-hand side: -G_t - E_t y_(t-2) - F_t y_(t-1), lane i on component i (y_(t-1) is still in its place).  (K Z)_t is formed from
        // the differences, not from K's entries: the windows centred on t-1, t and t+1
        const float at_m = (zc - 2.f * zm1) + zm2, at_0 = (zp1 - 2.f * zc) + zm1, at_p = (zp2 - 2.f * zp1) + zc;
        const float kz = c1 * ((t > 0 ? zc - zm1 : 0.f) + (t < T - 1 ? zc - zp1 : 0.f)) + c2 * ((kb.w[0] * at_m - 2.f * kb.w[1] * at_0) + kb.w[2] * at_p);
        float fy = 0.f;
#pragma unroll
        for (int m = 0; m < LAT; ++m) fy = fmaf(FB[li * CS + m], YV[m], fy);
        const float rhs = fmaf(-kb.k2, u2, -(GV[li] + kz)) - fy;
        wave_sync();
        if (in) GV[lane] = rhs;
        // ---- L_t^-1: lane i solves L x = e_i (what lies above the diagonal comes out as 0)
        float x[LAT];
#pragma unroll
        for (int r = 0; r < LAT; ++r) {
            float s = r == lane ? 1.f : 0.f;
#pragma unroll
            for (int m = 0; m < r; ++m) s = fmaf(-SB[r * CS + m], x[m], s);
            x[r] = s * NV[r];
        }
        if (in)
#pragma unroll
            for (int r = 0; r < LAT; ++r) {
                IB[r * CS + lane] = x[r];
                lo[r * LAT + lane] = x[r];
            }
        wave_sync();
        // ---- y_t = L_t^-1 rhs, lane i on row i
        float y = 0.f;
#pragma unroll
        for (int m = 0; m < LAT; ++m) y = fmaf(IB[li * CS + m], GV[m], y);
        if (in) {
            YV[lane] = y;
            lo[LAT * LAT + lane] = y;
        }
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

// the frames' numbers of sequence sq in buffer b, added in double in index order: -> L_s; `cp`: both coupling sums; `ap`: the second-difference one
DEV double accel_total(const KA::Args& aa, int b, int sq, int lane, double& cp, double& ap)
{
    const K::Args& a = aa.c;
    const int S = a.n_seq, T = a.n_t;
    double tot = 0.0, cs = 0.0, as = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const float l = t < T ? a.wloss[b][((long long)t * S + sq) * 4 + 3] : 0.f;
        const double q = t < T ? a.wcpl[b][(long long)t * S + sq] : 0.0;
        const int lo = __double2loint(q), hi = __double2hiint(q);
        const int n = T - t0 < 64 ? T - t0 : 64;
        for (int i = 0; i < n; ++i) {
            tot += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(l), i));
            cs += __hiloint2double(__builtin_amdgcn_readlane(hi, i), __builtin_amdgcn_readlane(lo, i));
        }
    }
    // |z_(t+1) - 2 z_t + z_(t-1)|^2 from the latents themselves: lane k adds component k's squares over the frames in index order, and the 24
    // sums meet once at the end (a wave sum per frame, five dependent shuffles of a double, cost 0.35 us per frame)
    const float* __restrict__ Z = a.wz[b];
    const int li = lane < LAT ? lane : LAT - 1;
    const auto zat = [&](int t) { return (double)Z[((long long)t * S + sq) * LAT + li]; };
    double zm = T > 2 ? zat(0) : 0.0, zc = T > 2 ? zat(1) : 0.0;
    constexpr int AHEAD = 8; // frames loaded together
    for (int t0 = 1; t0 + 1 < T; t0 += AHEAD) {
        double zn[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) zn[u] = t0 + u + 1 < T ? zat(t0 + u + 1) : 0.0;
#pragma unroll
        for (int u = 0; u < AHEAD; ++u)
            if (t0 + u + 1 < T) { // (wave-uniform)
                const double d = (zn[u] - 2.0 * zc) + zm;
                as = fma(d, d, as);
                zm = zc;
                zc = zn[u];
            }
    }
    as = wsum_d(lane < LAT ? as : 0.0);
    ap = ((double)aa.lam_accel / 24.0) * as;
    cp = ((double)a.lam_smooth / 24.0) * cs + ap;
    return tot + cp;
}

// One wave per sequence: dp_clip_decide_kernel's steps, with the second-difference part in the totals and kept beside them.
__global__ __launch_bounds__(64) void dp_clip_accel_decide_kernel(KA::Args aa)
{
    const K::Args& a = aa.c;
    const int lane = threadIdx.x, sq = blockIdx.x, S = a.n_seq, T = a.n_t, NH = a.n_steps + 1;
    const double nan = __builtin_nan("");
    if (a.step < 0) {
        int fl = 0;
        for (int t = lane; t < T; t += 64) fl |= a.wflags[(long long)t * S + sq];
        const bool ref = __ballot(fl != 0) != 0ull;
        float mu = a.mu ? a.mu[sq] : a.mu0;
        if (!(mu >= a.mu_min && mu <= a.mu_max)) mu = a.mu0;
        double cp = nan, ap = nan, tot = nan;
        if (!ref) tot = accel_total(aa, 0, sq, lane, cp, ap);
        if (lane == 0) {
            a.wword[sq] = ref ? K::W_REFUSED : 0;
            a.wmu[sq] = mu;
            a.wnacc[sq] = 0;
            a.wtot[2 * sq] = tot;
            a.wtot[2 * sq + 1] = cp;
            aa.wacc[sq] = ap;
            if (a.loss_hist) a.loss_hist[(long long)sq * NH] = tot;
            if (ref) { // no step runs: what the sequence returns (mu stays as the caller holds it)
                if (a.n_accepted) a.n_accepted[sq] = 0;
                if (a.clip_loss) { a.clip_loss[2 * sq] = nan; a.clip_loss[2 * sq + 1] = nan; }
                if (aa.accel_loss) aa.accel_loss[sq] = nan;
                if (a.info) a.info[sq] = DP_CLIP_REFUSED_FRAME;
            }
        }
        if (ref && a.loss_hist)
            for (int k = 1 + lane; k < NH; k += 64) a.loss_hist[(long long)sq * NH + k] = nan;
        return;
    }
    const int word = a.wword[sq];
    if ((word & K::W_REFUSED) != 0) return;
    const int cur = (word & K::W_CUR) != 0 ? 1 : 0;
    double tot = a.wtot[2 * sq], cp = a.wtot[2 * sq + 1], ap = aa.wacc[sq], cpn = nan, apn = nan, totn = nan;
    if (a.wsolved[sq] != 0) totn = accel_total(aa, cur ^ 1, sq, lane, cpn, apn);
    const bool acc = totn < tot; // (a NaN rejects)
    if (lane == 0) {
        float mu = a.wmu[sq];
        int nacc = a.wnacc[sq];
        if (acc) {
            tot = totn; cp = cpn; ap = apn;
            ++nacc;
            mu = fmaxf(mu * a.mu_down, a.mu_min);
            a.wword[sq] = cur ? 0 : K::W_CUR;
            a.wtot[2 * sq] = tot;
            a.wtot[2 * sq + 1] = cp;
            aa.wacc[sq] = ap;
            a.wnacc[sq] = nacc;
        } else {
            mu = fminf(mu * a.mu_up, a.mu_max);
            a.wword[sq] = (cur ? K::W_CUR : 0) | K::W_REJECTED;
        }
        a.wmu[sq] = mu;
        if (a.loss_hist) a.loss_hist[(long long)sq * NH + a.step + 1] = tot;
        if (a.step == a.n_steps - 1) {
            if (a.mu) a.mu[sq] = mu;
            if (a.n_accepted) a.n_accepted[sq] = nacc;
            if (a.clip_loss) { a.clip_loss[2 * sq] = tot; a.clip_loss[2 * sq + 1] = cp; }
            if (aa.accel_loss) aa.accel_loss[sq] = ap;
            if (a.info) a.info[sq] = 0;
        }
    }
}

static hipError_t plain_rows(const K::Args* args, int mode, const void*, hipStream_t stream) { return dp_launch_clip_rows(args, mode, stream); }

hipError_t dp_launch_clip_accel(const KA::Args* args, hipStream_t stream)
{
    const K::Rows rows = {plain_rows, nullptr};
    return dp_launch_clip_accel_train(args, &rows, stream);
}

hipError_t dp_launch_clip_accel_train(const KA::Args* args, const K::Rows* rows, hipStream_t stream)
{
    KA::Args k = *args;
    const auto run_rows = [&](int mode) { return rows->launch(&k.c, mode, rows->own, stream); };
    if (k.lam_accel == 0.f) { // dp_optimize_clip_lm's own train (its chain reads the first 600 floats of a frame's factor block), the new output 0
        hipError_t e = dp_launch_clip_train(&k.c, rows, stream);
        if (e == hipSuccess && k.accel_loss) e = hipMemsetAsync(k.accel_loss, 0, sizeof(double) * (size_t)k.c.n_seq, stream);
        return e;
    }
    const dim3 seqs((unsigned)k.c.n_seq);
    const auto run_decide = [&](int step) {
        k.c.step = step;
        hipLaunchKernelGGL(dp_clip_accel_decide_kernel, seqs, dim3(64), 0, stream, k);
        return hipGetLastError();
    };
    hipError_t e = run_rows(K::M_INIT);
    if (e == hipSuccess) e = run_decide(-1);
    for (int st = 0; st < k.c.n_steps && e == hipSuccess; ++st) {
        if (st > 0) e = run_rows(K::M_NORMAL);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(dp_clip_accel_chain_kernel, seqs, dim3(64), 0, stream, k);
        e = hipGetLastError();
        if (e == hipSuccess) e = run_rows(K::M_TRIAL);
        if (e == hipSuccess) e = run_decide(st);
    }
    if (e == hipSuccess) e = run_rows(K::M_RESULTS);
    return e;
}
