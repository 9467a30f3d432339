// dp_clip_dev.h -- device helpers of the clip solves' chain kernels: 24 x 24 x 24 products on the fp32 matrix pipe (dp_clip_accel.hip, and the
// next clip unit; dp_clip.hip's one product is written out, its reads are not these clamped ones) and the fetch of a frame's block into
// registers (both chains).  They touch no LDS of their own -- what an operand lambda reads is the caller's to wave_sync().  Included behind
// dp_lm_dev.h (DEV, f4, LAT).  What else the clip units share is text included in place: dp_clip_factor.h (the chains' factor step),
// dp_clip_total.h and dp_clip_decide_body.h (the decision).
#pragma once

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

// a frame's block on its way into registers: pre[i] = src[lane + 64 i] below n, 0 from n on; n is a constant of the call, and a register wholly
// beyond it keeps what it holds
template <int N>
DEV void fetch64(float (&pre)[N], const float* __restrict__ src, int n, int lane)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int e = lane + 64 * i;
        if (64 * i < n) pre[i] = e < n ? src[e] : 0.f;
    }
}
