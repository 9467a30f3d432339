// dp_encoder.hip -- the pose-VAE encoder (include/dragposer_encoder.h: dp_encode, dp_sequence_begin) on v_mfma_f32_16x16x4_f32.
//
// One wavefront owns 16 poses; the folded weights are the A operand, the poses the B operand (layout and the K-order rule that
// lets a layer's result registers be the next layer's B operands as they stand: dp_encoder.h).  A workgroup stages the whole weight
// image (137 KB) into LDS once and its wavefronts loop over 16-pose tiles; the activations never leave the register file.  Per
// K step group a lane reads one 16-byte word per output tile and issues four MFMAs per tile, the tiles interleaved so that every
// layer keeps 3 to 7 independent accumulator tiles in flight (the instruction issues every 32 cycles and a dependent one waits 40).
// The bias is the first MFMA's C operand; LeakyReLU is applied to the accumulators in place.
//
// A pose is a column of B and of D and no instruction mixes columns, so a pose's bits depend on nothing but its own inputs; the
// only cross-lane traffic is between the four lanes OF ONE POSE (the refusal flag, and one half-row of the head: dp_encoder.h).
#include <hip/hip_runtime.h>

#include "../../include/dragposer_encoder.h"
#include "dp_encoder.h"

namespace dpenc {

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool oor(float x, float limit) { return !(fabsf(x) <= limit); } // NaN, Inf and anything beyond the limit

template <int L>
__device__ __forceinline__ void dense(const float* lds, int lane, const float (&b)[enc_steps(L)], f4 (&acc)[enc_tiles(L)])
{
    constexpr int T = enc_tiles(L), S4 = enc_steps(L) / 4;
    const int g = lane >> 4;
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = *(const f4*)(lds + enc_b_off(L) + 16 * t + 4 * g);
#pragma unroll
    for (int s4 = 0; s4 < S4; ++s4) {
        f4 a[T];
#pragma unroll
        for (int t = 0; t < T; ++t) a[t] = *(const f4*)(lds + enc_w_off(L) + ((t * S4 + s4) * 64 + lane) * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][c], b[4 * s4 + c], acc[t], 0, 0, 0);
    }
}

// register r of tile t -> the next layer's K step 4 t + r, through LeakyReLU
template <int T>
__device__ __forceinline__ void activate(const f4 (&acc)[T], float (&b)[4 * T])
{
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) b[4 * t + r] = acc[t][r] > 0.f ? acc[t][r] : SLOPE * acc[t][r];
}

__global__ __launch_bounds__(THREADS) void dp_encoder_kernel(const EncArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[IMG_WORDS];
    for (int i = threadIdx.x; i < IMG_WORDS / 4; i += THREADS) ((f4*)lds)[i] = ((const f4*)a.image)[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, n = lane & 15;
    const int grid = gridDim.x;
    const float qnan = __builtin_nanf("");
    // tiles are dealt wave-major (tile = wave * grid + block, then in strides of grid * WAVES): a launch of few tiles puts them on
    // the first waves of many workgroups -- one per SIMD -- before any SIMD gets a second
    for (int tile = wave * grid + (int)blockIdx.x; tile < a.n_tiles; tile += grid * WAVES) {
        // (the weights are the same for every tile: without this the compiler hoists all 136 LDS reads out of the loop and spills them)
        asm volatile("" ::: "memory");
        const int p = tile * POSES + n;
        const bool valid = p < a.n;
        const size_t pl = valid ? p : a.n - 1; // a ragged tile's idle columns repeat the last pose and store nothing
        bool bad = false;

        float x[enc_steps(0)];
        const float* row = a.pose + pl * IN_CH + 4 * g;
#pragma unroll
        for (int j = 0; j < IN_CH / 16; ++j) {
            const f4 v = *(const f4*)(row + 16 * j);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool o = oor(v[c], a.limit);
                bad |= o;
                x[4 * j + c] = o ? qnan : v[c];
            }
        }
        // eps for the lane's share of the latent: k = 4 g + r (every lane) and k = 16 + 4 (g >> 1) + r (the even lane groups)
        const int kb = 16 + 4 * (g >> 1);
        f4 ea = {0.f, 0.f, 0.f, 0.f}, eb = {0.f, 0.f, 0.f, 0.f};
        if (a.eps) {
            ea = *(const f4*)(a.eps + pl * LAT + 4 * g);
            eb = *(const f4*)(a.eps + pl * LAT + kb);
#pragma unroll
            for (int c = 0; c < 4; ++c) bad |= oor(ea[c], a.limit) | oor(eb[c], a.limit);
        }
        float gp[3] = {0.f, 0.f, 0.f}, gr[4] = {0.f, 0.f, 0.f, 0.f}, hv[DP_MAX_HEIGHT_JOINTS];
        if (a.begin) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { gp[c] = a.init_pos[pl * 3 + c]; bad |= oor(gp[c], a.limit); }
#pragma unroll
            for (int c = 0; c < 4; ++c) { gr[c] = a.init_rot[pl * 4 + c]; bad |= oor(gr[c], a.limit); }
#pragma unroll
            for (int j = 0; j < DP_MAX_HEIGHT_JOINTS; ++j) {
                hv[j] = j < a.n_heights ? a.init_heights[pl * a.n_heights + j] : 0.f;
                bad |= oor(hv[j], a.limit);
            }
        }

        f4 h0[enc_tiles(0)], h1[enc_tiles(1)], h2[enc_tiles(2)], hd[enc_tiles(3)];
        float x1[enc_steps(1)], x2[enc_steps(2)], x3[enc_steps(3)];
        dense<0>(lds, lane, x, h0);
        activate(h0, x1);
        dense<1>(lds, lane, x1, h1);
        activate(h1, x2);
        dense<2>(lds, lane, x2, h2);
        activate(h2, x3);
        dense<3>(lds, lane, x3, hd);

        // head: tile 0 = mu[4 g + r], tile 1 = logvar[4 g + r]; tile 2 = mu[kb + r] on the even lane groups and logvar[kb + r] on
        // the odd ones, the partner 16 lanes away (the same pose)
        const bool even = (g & 1) == 0;
        f4 mu_a = hd[0], lv_a = hd[1], mu_b, lv_b;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float other = __shfl_xor(hd[2][r], 16);
            mu_b[r] = even ? hd[2][r] : other;
            lv_b[r] = even ? other : hd[2][r];
        }
        f4 z_a = mu_a, z_b = mu_b;
        if (a.eps) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                z_a[r] = mu_a[r] + ea[r] * expf(0.5f * lv_a[r]);
                z_b[r] = mu_b[r] + eb[r] * expf(0.5f * lv_b[r]);
            }
        }
        int flags = bad ? 1 : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (oor(mu_a[r], 3.0e38f) | oor(lv_a[r], 3.0e38f) | oor(z_a[r], 3.0e38f) | oor(mu_b[r], 3.0e38f) | oor(lv_b[r], 3.0e38f) | oor(z_b[r], 3.0e38f)) flags |= 2;
        flags |= __shfl_xor(flags, 16); // the four lanes of the pose agree
        flags |= __shfl_xor(flags, 32);
        bad = (flags & 1) != 0;
        if (bad) {
            mu_a = mu_b = lv_a = lv_b = z_a = z_b = f4{qnan, qnan, qnan, qnan};
#pragma unroll
            for (int c = 0; c < 3; ++c) gp[c] = qnan;
#pragma unroll
            for (int c = 0; c < 4; ++c) gr[c] = qnan;
#pragma unroll
            for (int j = 0; j < DP_MAX_HEIGHT_JOINTS; ++j) hv[j] = qnan;
        }
        if (!valid) continue;
        const size_t o = (size_t)p * LAT;
        if (a.mu) { *(f4*)(a.mu + o + 4 * g) = mu_a; if (even) *(f4*)(a.mu + o + kb) = mu_b; }
        if (a.logvar) { *(f4*)(a.logvar + o + 4 * g) = lv_a; if (even) *(f4*)(a.logvar + o + kb) = lv_b; }
        if (a.latent) { *(f4*)(a.latent + o + 4 * g) = z_a; if (even) *(f4*)(a.latent + o + kb) = z_b; }
        if (a.status && g == 0) a.status[p] = bad ? (DP_STATUS_BAD_STATE | DP_STATUS_NONFINITE_RESULT) : (flags & 2) ? DP_STATUS_NONFINITE_RESULT : 0;
        if (a.begin) {
            const int H = a.history, NH = a.n_heights;
            float* lb = a.latent_buf + (size_t)p * H * LAT;
            for (int h = 0; h < H; ++h) {
                *(f4*)(lb + (size_t)h * LAT + 4 * g) = z_a;
                if (even) *(f4*)(lb + (size_t)h * LAT + kb) = z_b;
            }
            float* db = a.disp_buf + (size_t)p * H * 3;
            const float zero = bad ? qnan : 0.f;
            for (int i = g; i < 3 * H; i += 4) db[i] = zero;
            float* hb = a.heights_buf + (size_t)p * H * NH;
            for (int h = g; h < H; h += 4)
#pragma unroll
                for (int j = 0; j < DP_MAX_HEIGHT_JOINTS; ++j)
                    if (j < NH) hb[(size_t)h * NH + j] = hv[j];
            if (g == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.global_pos[(size_t)p * 3 + c] = gp[c];
#pragma unroll
                for (int c = 0; c < 4; ++c) a.global_rot[(size_t)p * 4 + c] = gr[c];
            }
        }
    }
}

int launch_encoder(const EncArgs& a, int n_cu, void* stream)
{
    const int grid = enc_grid(a.n_tiles, n_cu);
    hipLaunchKernelGGL(dp_encoder_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace dpenc
