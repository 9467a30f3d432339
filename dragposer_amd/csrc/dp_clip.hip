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
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_clip_lm.h"
#include "dp_clip.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"

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
    const auto fetch = [&](const float* __restrict__ src) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = lane + 64 * i;
            pre[i] = e < K::AG_FLOATS ? src[e] : 0.f;
        }
    };
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
        // the right-hand side: -G_t + c L_(t-1)^-T y_(t-1), lane i on component i (y_(t-1) is still in its place)
        float rhs = -(GV[li] + c * ((t > 0 ? zc - zp : 0.f) + (t < T - 1 ? zc - zn : 0.f)));
        if (t > 0) {
            float u = 0.f;
#pragma unroll
            for (int r = 0; r < LAT; ++r) u = fmaf(xp[r], YV[r], u);
            rhs = fmaf(c, u, rhs);
        }
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
        float* const lo = a.wli + f * K::LI_FLOATS;
        if (in)
#pragma unroll
            for (int r = 0; r < LAT; ++r) {
                IB[r * CI + lane] = x[r];
                lo[r * LAT + lane] = x[r];
            }
        wave_sync();
        // ---- y_t = L_t^-1 rhs, lane i on row i
        float y = 0.f;
#pragma unroll
        for (int m = 0; m < LAT; ++m) y = fmaf(IB[li * CI + m], GV[m], y);
        if (in) {
            YV[lane] = y;
            lo[LAT * LAT + lane] = y;
        }
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

// the frames' numbers of sequence sq in buffer b, added in double in index order: -> L_s, and the sum of the coupling parts in `cp`
__device__ __forceinline__ double clip_total(const K::Args& a, int b, int sq, int lane, double& cp)
{
    const int S = a.n_seq, T = a.n_t;
    double tot = 0.0, cs = 0.0;
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
    cp = ((double)a.lam_smooth / 24.0) * cs;
    return tot + cp;
}

// One wave per sequence.  step -1: after the pass of z0 -- is a frame refused, the damping the sequence starts from, L_s(Z0).  step k: trial
// k's decision.  The last step's also hands the per-sequence outputs over.
__global__ __launch_bounds__(64) void dp_clip_decide_kernel(K::Args a)
{
    const int lane = threadIdx.x, sq = blockIdx.x, S = a.n_seq, T = a.n_t, NH = a.n_steps + 1;
    const double nan = __builtin_nan("");
    if (a.step < 0) {
        int fl = 0;
        for (int t = lane; t < T; t += 64) fl |= a.wflags[(long long)t * S + sq];
        const bool ref = __ballot(fl != 0) != 0ull;
        float mu = a.mu ? a.mu[sq] : a.mu0;
        if (!(mu >= a.mu_min && mu <= a.mu_max)) mu = a.mu0;
        double cp = nan, tot = nan;
        if (!ref) tot = clip_total(a, 0, sq, lane, cp);
        if (lane == 0) {
            a.wword[sq] = ref ? K::W_REFUSED : 0;
            a.wmu[sq] = mu;
            a.wnacc[sq] = 0;
            a.wtot[2 * sq] = tot;
            a.wtot[2 * sq + 1] = cp;
            if (a.loss_hist) a.loss_hist[(long long)sq * NH] = tot;
            if (ref) { // no step runs: what the sequence returns (mu stays as the caller holds it)
                if (a.n_accepted) a.n_accepted[sq] = 0;
                if (a.clip_loss) { a.clip_loss[2 * sq] = nan; a.clip_loss[2 * sq + 1] = nan; }
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
    double tot = a.wtot[2 * sq], cp = a.wtot[2 * sq + 1], cpn = nan, totn = nan;
    if (a.wsolved[sq] != 0) totn = clip_total(a, cur ^ 1, sq, lane, cpn);
    const bool acc = totn < tot; // (a NaN rejects)
    if (lane == 0) {
        float mu = a.wmu[sq];
        int nacc = a.wnacc[sq];
        if (acc) {
            tot = totn; cp = cpn;
            ++nacc;
            mu = fmaxf(mu * a.mu_down, a.mu_min);
            a.wword[sq] = cur ? 0 : K::W_CUR;
            a.wtot[2 * sq] = tot;
            a.wtot[2 * sq + 1] = cp;
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
            if (a.info) a.info[sq] = 0;
        }
    }
}

// one pass of the rows kernel in `mode` (M_*): also what another unit's launch train (dp_clip_accel.hip) runs between its own kernels
hipError_t dp_launch_clip_rows(const K::Args* args, int mode, hipStream_t stream)
{
    K::Args k = *args;
    k.mode = mode;
    hipLaunchKernelGGL(dp_clip_rows_kernel, dim3((unsigned)((k.n_frames + WPB - 1) / WPB)), dim3(WPB * 64), 0, stream, k);
    return hipGetLastError();
}

static hipError_t plain_rows(const K::Args* args, int mode, const void*, hipStream_t stream) { return dp_launch_clip_rows(args, mode, stream); }

hipError_t dp_launch_clip(const K::Args* args, hipStream_t stream)
{
    const K::Rows rows = {plain_rows, nullptr};
    return dp_launch_clip_train(args, &rows, stream);
}

hipError_t dp_launch_clip_train(const K::Args* args, const K::Rows* rows, hipStream_t stream)
{
    K::Args k = *args;
    const dim3 seqs((unsigned)k.n_seq);
    const auto run_rows = [&](int mode) { return rows->launch(&k, mode, rows->own, stream); };
    const auto run_decide = [&](int step) {
        k.step = step;
        hipLaunchKernelGGL(dp_clip_decide_kernel, seqs, dim3(64), 0, stream, k);
        return hipGetLastError();
    };
    hipError_t e = run_rows(K::M_INIT);
    if (e == hipSuccess) e = run_decide(-1);
    for (int st = 0; st < k.n_steps && e == hipSuccess; ++st) {
        if (st > 0) e = run_rows(K::M_NORMAL);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(dp_clip_chain_kernel, seqs, dim3(64), 0, stream, k);
        e = hipGetLastError();
        if (e == hipSuccess) e = run_rows(K::M_TRIAL);
        if (e == hipSuccess) e = run_decide(st);
    }
    if (e == hipSuccess) e = run_rows(K::M_RESULTS);
    return e;
}
