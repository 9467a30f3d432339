// dp_clip_factor.h -- a fragment of text of the clip solves' chain kernels (dp_clip.hip, dp_clip_accel.hip), included in place inside the forward
// sweep's frame loop once S_t and g_t are written: the factor step of frame t, in two parts with the kernel's own right-hand side between.
//   parameters CLIP_FACTOR  1: the Cholesky of S_t in place, left-looking, lane i on row i, with the pivot screen, and 1 / L_kk
//                           2: L_t^-1 by 24 forward substitutions, lane i on column i, in registers; y_t = L_t^-1 rhs
//              CLIP_LI      (part 2) row stride of the L^-1 block IB
//              CLIP_WS      (part 2) an expression: the frame's factor block in the workspace
//   reads      lane, li, in; ok; SB = S_t (stride CS).  Part 2: rhs, component li of the right-hand side, which the including scope forms
//              between the parts, while GV still holds g_t and YV y_(t-1)
//   leaves     part 1: SB: L_t below the diagonal; NV: 1 / L_kk.  A pivot that is not positive and finite: ok false and `break`, out of the
//              frame loop, with nothing but SB written.  Part 2: GV: the right-hand side; x[LAT] (declared here): column `lane` of L_t^-1;
//              IB and floats 0..575 of CLIP_WS: L_t^-1; YV and floats 576..599: y_t
//   part 1     opens with a wave_sync() (each Cholesky column does): S_t and g_t may be other lanes' writes.  Closes without one: SB is
//              complete for every lane only behind part 2's first
//   part 2     opens with a wave_sync(): g_t's last read was the including scope's, now the right-hand side takes its place.  One more between
//              L_t^-1's stores and y_t's reads.  Closes without one: YV is the writing lane's alone until the including scope's next
#if CLIP_FACTOR == 1
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
#else
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
        float* const lw = CLIP_WS;
        if (in)
#pragma unroll
            for (int r = 0; r < LAT; ++r) {
                IB[r * CLIP_LI + lane] = x[r];
                lw[r * LAT + lane] = x[r];
            }
        wave_sync();
        // ---- y_t = L_t^-1 rhs, lane i on row i
        float y = 0.f;
#pragma unroll
        for (int m = 0; m < LAT; ++m) y = fmaf(IB[li * CLIP_LI + m], GV[m], y);
        if (in) {
            YV[lane] = y;
            lw[LAT * LAT + lane] = y;
        }
#endif
