// dp_fit.hip -- dp_fit_bones (include/dragposer_calibration.h): per-group bone scales from frames of tracker data, the least-squares
// problem that is linear in the bones once the joint rotations are fixed.  Two kernels, one behind the other on the caller's stream.
//
// dp_fit_rows_kernel   one frame per wave, WPB waves per workgroup (dp_fit.h); the folded decoder staged once per workgroup as
//                      dp_lm_body.h stages it, with `base` in the bones' place.
//   forward   the dp_cons / dp_lm family's: decoder rows dealt over the lanes, then a lane per joint; it leaves R_0, the world displacement
//             and the bones b_j = R_p base_j (root frame) in the wave's block
//   rows      eight tracked joints at a time, four per half of the wave: lane n <= K of a half forms column n of its joints' three rows
//             (n < K: R_0 times the path's bones of group n, summed; n = K: tgt - world_disp - R_0 times the path's ungrouped bones),
//             each times sqrt(w_pos / 3E), into [24][32]
//   M         [A b]^T [A b] accumulated over the rounds on v_mfma_f32_16x16x4_f32 (K = the 24 rows, both operands the same values), as
//             dp_lm_body.h accumulates [J r]^T [J r]
//   sum       the ONE workgroup barrier after the staging: every wave arrives -- a wave without a frame, or with a refused one, has zeroed
//             its matrix instead of leaving -- then element e of the workgroup's partial sum is the waves' element e added in wave order
// dp_fit_solve_kernel  one workgroup: thread e adds element e of the partial sums in index order in double; then its first wave forms
//                      H = N + ridge I with rhs as a further row, the Cholesky of dp_lm_body.h's solve (lane i on row i) in double, the
//                      back substitution in registers, and the outputs.
// No atomics anywhere: the result depends on the inputs alone.
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"
#include "../../include/dragposer_calibration.h"
#include "dp_fit.h"
#include "dp_math.h"
#include "dp_vjp.h"

#include "dp_lm_dev.h"

namespace F = dpfit;
static_assert(F::MAXK == DP_FIT_MAX_GROUPS && F::MAXK == LAT, "the matrix has dp_lm's 25 rows and columns");

__global__ __launch_bounds__(F::WPB * 64) void dp_fit_rows_kernel(F::Args a)
{
    __shared__ __attribute__((aligned(16))) float lds[F::LDS_FLOATS];
    const float* __restrict__ W = a.img;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    int* par = (int*)(lds + L_PAR);
    int* grp = (int*)(lds + F::L_GRP);
    const int* Ti = (const int*)W;

    // ---- staging (once per workgroup): padded weight rows, sigma, the skeleton with `base` as its bones, the bones' groups
    for (int i = tid; i < H0 * LAT; i += F::WPB * 64) lds[L_A0 + (i / LAT) * S0 + i % LAT] = W[dpvjp::OFF_A0 + i];
    for (int i = tid; i < H1 * H0; i += F::WPB * 64) lds[L_A1 + (i / H0) * S1 + i % H0] = W[dpvjp::OFF_A1 + i];
    for (int i = tid; i < dpvjp::NY * H1; i += F::WPB * 64) lds[L_A2 + (i / H1) * S2 + i % H1] = W[dpvjp::OFF_A2 + i];
    if (tid < dpvjp::NY) lds[L_SD + tid] = W[dpvjp::OFF_SD + tid];
    if (tid < NJ) {
        par[tid] = Ti[dpvjp::OFF_PARENT + tid];
        grp[tid] = tid == 0 ? -1 : a.grp[tid];
    }
    if (tid < 3 * NJ) lds[L_OFF + tid] = a.has_base ? a.base[tid] : W[dpvjp::OFF_BONE + tid];
    __syncthreads();

    const long long f = (long long)blockIdx.x * F::WPB + wv;
    const bool in_range = f < a.n_frames; // (a wave beyond the batch reads nothing of it and stays until the barrier below)
    float* wb = lds + F::L_WAVE0 + wv * F::W_FLOATS;
    float *ZB = wb + F::W_Z, *HB0 = wb + F::W_H0, *HB1 = wb + F::W_H1, *QB = wb + F::W_Q, *RB = wb + F::W_R, *BB = wb + F::W_B, *SW = wb + F::W_SW,
          *JB = wb + F::W_J, *AB = wb + F::W_A;
    const int j = lane; // joint of this lane (j < NJ)
    const bool jl = lane < NJ;

    // ---- screening (include/dragposer.h: DP_STATUS_*), the dp_cons family's, on what this call reads
    float cr[4] = {1.f, 0.f, 0.f, 0.f}, z0 = 0.f, wp = 0.f;
    bool trk = false, bs = false, bt = false;
    if (in_range) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cr[k] = a.cur_rot[f * 4 + k];
        if (lane < LAT) z0 = a.z0[f * LAT + lane];
        trk = jl && a.tracked[f * NJ + j] != 0;
        bs = refused(z0) || refused(cr[0]) || refused(cr[1]) || refused(cr[2]) || refused(cr[3]);
        if (trk) {
#pragma unroll
            for (int k = 0; k < 3; ++k) bt = bt || refused(a.tgt_pos[(f * NJ + j) * 3 + k]);
            wp = a.w[(f * NJ + j) * 2];
            bt = bt || refused(wp) || refused(a.w[(f * NJ + j) * 2 + 1]);
        }
    }
    const bool bad_state = __ballot(bs) != 0ull;
    const bool bad_tgt = !bad_state && __ballot(bt) != 0ull;
    const unsigned long long tmask = __ballot(trk);
    const int E = __popcll(tmask);
    const bool use = in_range && !bad_state && !bad_tgt && E > 0; // (wave-uniform)
    if (in_range && lane == 0 && a.status) a.status[f] = bad_state ? DP_STATUS_BAD_STATE : bad_tgt ? DP_STATUS_BAD_TARGETS : 0;

    if (use) {
        // per-lane constants of the forward pass
        const float c0 = lane < H0 ? W[dpvjp::OFF_C0 + lane] : 0.f;
        const float b1 = lane < H1 ? W[dpvjp::OFF_B1 + lane] : 0.f;
        const int oB = 64 + lane; // second decoder row of lanes 0..26
        const float b2A = W[dpvjp::OFF_B2 + lane], sdA = W[dpvjp::OFF_SD + lane], muA = W[dpvjp::OFF_MU + lane];
        const float b2B = lane < NYU - 64 ? W[dpvjp::OFF_B2 + oB] : 0.f, sdB = lane < NYU - 64 ? W[dpvjp::OFF_SD + oB] : 1.f,
                    muB = lane < NYU - 64 ? W[dpvjp::OFF_MU + oB] : 0.f;
        const int pj = jl ? par[j] : 0;
        float off[3] = {0.f, 0.f, 0.f};
        if (jl) {
#pragma unroll
            for (int c = 0; c < 3; ++c) off[c] = lds[L_OFF + 3 * j + c];
            SW[j] = trk ? sqrtf(wp / (3.f * (float)E)) : 0.f;
        }
        if (lane < LAT) ZB[lane] = z0;
        wave_sync();
        // ---- decoder (autoencoder.py:224-256, folded), LeakyReLU(0.2) after layers 0 and 1
        if (lane < H0) {
            float s = c0;
#pragma unroll UNR
            for (int k = 0; k < LAT; ++k) s = fmaf(lds[L_A0 + lane * S0 + k], ZB[k], s);
            HB0[lane] = s > 0.f ? s : s * 0.2f;
        }
        wave_sync();
        if (lane < H1) {
            float s = b1;
#pragma unroll UNR
            for (int k = 0; k < H0; ++k) s = fmaf(lds[L_A1 + lane * S1 + k], HB0[k], s);
            HB1[lane] = s > 0.f ? s : s * 0.2f;
        }
        wave_sync();
        {
            float s = b2A, t = b2B;
#pragma unroll UNR
            for (int k = 0; k < H1; ++k) {
                const float h = HB1[k];
                s = fmaf(lds[L_A2 + lane * S2 + k], h, s);
                if (lane < NYU - 64) t = fmaf(lds[L_A2 + oB * S2 + k], h, t);
            }
            QB[lane] = fmaf(s, sdA, muA);
            if (lane < NYU - 64) QB[oB] = fmaf(t, sdB, muB);
        }
        wave_sync();
        // ---- kinematics, a lane per joint: R_j, then the bones in the root's frame
        float q[4], qn[4], R[9], wr[4] = {1.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = jl ? QB[4 * j + c] : (c == 0 ? 1.f : 0.f);
        const float rn = 1.f / sqrtf(fmaf(q[0], q[0], fmaf(q[1], q[1], fmaf(q[2], q[2], q[3] * q[3]))));
#pragma unroll
        for (int c = 0; c < 4; ++c) qn[c] = q[c] * rn;
        if (j == 0) { quat_mul(cr, qn, wr); rotmat(wr, R); } // world root rotation, cur_rot as given (drag_pose.py:88)
        else rotmat(qn, R);
        if (jl)
#pragma unroll
            for (int k = 0; k < 9; ++k) RB[9 * j + k] = R[k];
        wave_sync();
        float R0[9], d[3], wd[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R0[k] = RB[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = QB[4 * NJ + c];
        mv(R0, d, wd); // world displacement (drag_pose.py:102)
        if (jl) {
            float b[3] = {off[0], off[1], off[2]};
            if (j == 0) b[0] = b[1] = b[2] = 0.f;
            else if (pj != 0) mv(RB + 9 * pj, off, b);
#pragma unroll
            for (int c = 0; c < 3; ++c) BB[4 * j + c] = b[c];
        }
        wave_sync();

        // ---- the rows, eight tracked joints at a time, and M = [A b]^T [A b] over them.  Lane l of an MFMA: row l & 15 of an A tile,
        // K-slot l >> 4; column l & 15 of a B tile
        const int lr16 = lane & 15, lk = lane >> 4;
        const int cn = lane & 31, hf = lane >> 5; // column of this lane and its half
        const int K = a.K;
        f4 na[2][2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) na[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
        for (unsigned long long tm = tmask; tm != 0ull;) {
            unsigned long long mine = tm;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (hf != 0) mine &= mine - 1ull; // (the second half skips the first half's four)
                tm &= tm - 1ull;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) tm &= tm - 1ull;
#pragma unroll 1
            for (int sl = 0; sl < 4; ++sl) {
                float r3[3] = {0.f, 0.f, 0.f};
                if (mine != 0ull && cn <= K) {
                    const int jj = __builtin_ctzll(mine);
                    const int want = cn < K ? cn : -1; // the group whose bones this column sums
                    float v[3] = {0.f, 0.f, 0.f}, t[3];
                    int c = jj;
                    for (int s = 0; s < NJ && c != 0; ++s) { // the path from jj to the root (<= 7 bones)
                        if (grp[c] == want) { v[0] += BB[4 * c]; v[1] += BB[4 * c + 1]; v[2] += BB[4 * c + 2]; }
                        c = par[c];
                    }
                    mv(R0, v, t);
                    const float sp = SW[jj];
#pragma unroll
                    for (int e = 0; e < 3; ++e) r3[e] = cn < K ? sp * t[e] : sp * ((a.tgt_pos[(f * NJ + jj) * 3 + e] - wd[e]) - t[e]);
                }
                mine &= mine - 1ull;
#pragma unroll
                for (int e = 0; e < 3; ++e) JB[(12 * hf + 3 * sl + e) * F::SJ + cn] = r3[e];
            }
            wave_sync();
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const float v0 = JB[(4 * s + lk) * F::SJ + lr16], v1 = JB[(4 * s + lk) * F::SJ + 16 + lr16];
                na[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v0, na[0][0], 0, 0, 0);
                na[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v1, na[0][1], 0, 0, 0);
                na[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v0, na[1][0], 0, 0, 0);
                na[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v1, na[1][1], 0, 0, 0);
            }
            wave_sync(); // (the rows' last reads before the next round's writes)
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mt + 4 * lk + r;
                if (row < F::MS) {
                    AB[row * F::SJ + lr16] = na[mt][0][r];
                    AB[row * F::SJ + 16 + lr16] = na[mt][1][r];
                }
            }
        if (lane == 0) wb[F::W_N] = 1.f;
    } else { // no frame, a refused one, or one without a tracker: a zero matrix, and the wave arrives at the barrier like the others
        for (int e = lane; e < F::MS * F::SJ; e += 64) AB[e] = 0.f;
        if (lane == 0) wb[F::W_N] = 0.f;
    }
    __syncthreads(); // every wave of the workgroup arrives: nothing above returns

    // ---- the workgroup's partial sum: element e of the waves' matrices in wave order; the last element counts the frames used
    const float* const w0 = lds + F::L_WAVE0;
    float* const part = a.workspace + (size_t)blockIdx.x * F::PART_FLOATS;
    for (int e = tid; e <= F::PART_COUNT; e += F::WPB * 64) {
        const int r = e / F::MS, c = e - r * F::MS;
        const int at = e < F::PART_COUNT ? F::W_A + r * F::SJ + c : F::W_N;
        float s = w0[at];
#pragma unroll
        for (int w = 1; w < F::WPB; ++w) s = __fadd_rn(s, w0[w * F::W_FLOATS + at]);
        part[e] = s;
    }
}

__global__ __launch_bounds__(F::SOLVE_THREADS) void dp_fit_solve_kernel(F::Args a)
{
    __shared__ double S[F::PART_FLOATS];   // the summed matrix [MS][MS], then the frames used
    __shared__ double HM[F::MS * F::MS];   // H, rhs as row K; the Cholesky factor in place
    __shared__ double QT[2 * F::MAXK];     // the two quadratic forms' per-row parts
    __shared__ float sc[F::MAXK];          // the scales as they are returned
    const int tid = threadIdx.x;
    {
        double s = 0.0;
        if (tid <= F::PART_COUNT) {
            const float* __restrict__ p = a.workspace + tid;
#pragma unroll 8
            for (int i = 0; i < a.n_parts; ++i) s += (double)p[(size_t)i * F::PART_FLOATS]; // index order
        }
        S[tid] = s;
    }
    __syncthreads(); // (the only one; what follows is the first wave's)
    if (tid >= 64) return;
    const int lane = tid, K = a.K, MS = F::MS;
    const int count = (int)S[F::PART_COUNT];
    const double ridge = (double)a.ridge;
    if (a.normal)
        for (int e = lane; e < (K + 1) * (K + 1); e += 64) {
            const int r = e / (K + 1), c = e - r * (K + 1);
            a.normal[e] = S[r * MS + c];
        }
    for (int e = lane; e < (K + 1) * K; e += 64) { // rows 0..K-1: H = N + ridge I; row K: rhs = g + ridge prior
        const int r = e / K, c = e - r * K;
        HM[r * MS + c] = r < K ? S[r * MS + c] + (r == c ? ridge : 0.0) : S[K * MS + c] + ridge * (double)a.prior[c];
    }
    // column by column, left-looking (dp_lm_body.h's solve): lane i >= k forms s = H_ik - sum_(m<k) L_im L_km, the pivot is lane k's s;
    // row K (rhs) comes out as y, L y = rhs
    bool ok = true;
    double myinv = 0.0;
    const int rw = lane <= K ? lane : K; // (lanes beyond the K + 1 rows repeat the last one and store nothing)
    for (int k = 0; k < K; ++k) {
        wave_sync();
        double s = HM[rw * MS + k];
        for (int m = 0; m < k; ++m) s = fma(-HM[rw * MS + m], HM[k * MS + m], s);
        const double piv = __shfl(s, k);
        ok = ok && piv > 0.0 && piv <= 1.0e300;
        const double inv = 1.0 / sqrt(piv);
        if (lane == k) myinv = inv;
        if (lane > k && lane <= K) HM[lane * MS + k] = s * inv;
    }
    wave_sync();
    double acc = lane < K ? HM[K * MS + lane] : 0.0, dl = 0.0; // L^T s = y: lane j reads column j of L, ends with s_j
    for (int i = K - 1; i >= 0; --i) {
        const double x = acc * myinv;
        const double xi = __shfl(x, i);
        if (lane == i) dl = xi;
        if (lane < i) acc = fma(-HM[i * MS + lane], xi, acc);
    }
    const int flags = count <= 0 ? DP_FIT_NO_FRAMES : ok ? 0 : DP_FIT_SINGULAR;
    const float pr = lane < K ? a.prior[lane] : 0.f;
    const float sf = flags == 0 ? (float)dl : pr;
    if (lane < K) {
        sc[lane] = sf;
        a.scales[lane] = sf;
    }
    wave_sync();
    if (lane < NJ && a.offsets) {
        const int g = lane == 0 ? -1 : a.grp[lane];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float b = a.has_base ? a.base[3 * lane + c] : a.img[dpvjp::OFF_BONE + 3 * lane + c];
            a.offsets[3 * lane + c] = lane == 0 ? 0.f : g < 0 ? b : __fmul_rn(b, sc[g]);
        }
    }
    // q(s) = b^T b - 2 s^T g + s^T N s at the prior and at the returned scales: lane i forms row i's part, lane 0 adds them in order
    if (lane < K) {
        double np = 0.0, ns = 0.0;
        for (int c = 0; c < K; ++c) {
            np = fma(S[lane * MS + c], (double)a.prior[c], np);
            ns = fma(S[lane * MS + c], (double)sc[c], ns);
        }
        QT[lane] = (double)pr * (np - 2.0 * S[K * MS + lane]);
        QT[F::MAXK + lane] = (double)sf * (ns - 2.0 * S[K * MS + lane]);
    }
    wave_sync();
    if (lane == 0) {
        double q0 = S[K * MS + K], q1 = q0;
        for (int i = 0; i < K; ++i) { q0 += QT[i]; q1 += QT[F::MAXK + i]; }
        if (a.rms) {
            a.rms[0] = count > 0 ? (float)sqrt(fmax(q0, 0.0) / (double)count) : 0.f;
            a.rms[1] = count > 0 ? (float)sqrt(fmax(q1, 0.0) / (double)count) : 0.f;
        }
        if (a.info) {
            a.info[0] = count;
            a.info[1] = flags;
        }
    }
}

hipError_t dp_launch_fit(const F::Args* args, hipStream_t stream)
{
    hipLaunchKernelGGL(dp_fit_rows_kernel, dim3((unsigned)args->n_parts), dim3(F::WPB * 64), 0, stream, *args);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dp_fit_solve_kernel, dim3(1), dim3(F::SOLVE_THREADS), 0, stream, *args);
    return hipGetLastError();
}
