// dp_lm_frame_tangents.h -- a fragment of text of the LM frame (dp_lm_body.h, dp_clip_rows_body.h), included in place behind
// dp_lm_frame_pass.h's pass of the latent at hand: the tangents of the decoder's outputs through the folded decoder, then J two tracked joints
// at a time and [J r]^T [J r] over them, all on v_mfma_f32_16x16x4_f32.
//   reads      lds, lane, par, cr, tmask, BONES, TGT_POS, TGT_ROT; the pass's R0 and d; the wave's block as the pass left it (DB0, DB1, QN, RN,
//              WR, RB, VB, PB, GB) and SW; TB and JB as its own place
//   leaves     lr16, lk, cn, hf, col, dR0, dwd (the root's part of the lane's column) and na, the four 16 x 16 tiles of [J r]^T [J r] so far:
//              further rows may be added through JB in the same way before dp_lm_frame_close.h stores them; TB holds the tangents
//   opens      with a wave_sync(): the pass's last writes into the wave's block
//   closes     with a wave_sync(): the last rows' reads from JB
    wave_sync(); // (the pass's last writes into the wave's block)
    // ---- tangents on the matrix pipe.  Lane l: row l & 15 of an A tile, K-slot l >> 4; column l & 15 of a B tile.
    const int lr16 = lane & 15, lk = lane >> 4;
    {
        f4 acc[4][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int s = 0; s < H0 / 4; ++s) {
            const int k = 4 * s + lk;
            const float dk = DB0[k];
            float b[2], av[4];
            b[0] = dk * lds[L_A0 + k * S0 + lr16];
            b[1] = lr16 < LAT - 16 ? dk * lds[L_A0 + k * S0 + 16 + lr16] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = 16 * mt + lr16;
                av[mt] = lds[L_A1 + (row < H1 ? row : H1 - 1) * S1 + k]; // (rows 60..63 of the last tile: results not kept)
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mt + 4 * lk + r;
                if (row < H1) {
                    const float dr = DB1[row];
                    TB[row * ST + lr16] = dr * acc[mt][0][r];
                    if (lr16 < LAT - 16) TB[row * ST + 16 + lr16] = dr * acc[mt][1][r];
                }
            }
    }
    wave_sync();
    {
        f4 acc[6][2];
#pragma unroll
        for (int mt = 0; mt < 6; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int s = 0; s < H1 / 4; ++s) {
            const int k = 4 * s + lk;
            float b[2], av[6];
            b[0] = TB[k * ST + lr16];
            b[1] = lr16 < LAT - 16 ? TB[k * ST + 16 + lr16] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 6; ++mt) {
                const int row = 16 * mt + lr16;
                av[mt] = lds[L_A2 + (row < dpvjp::NY ? row : dpvjp::NY - 1) * S2 + k];
            }
#pragma unroll
            for (int mt = 0; mt < 6; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
        wave_sync(); // (S1's last reads before S2 takes its place)
#pragma unroll
        for (int mt = 0; mt < 6; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mt + 4 * lk + r;
                if (row < NYU) {
                    const float sd = lds[L_SD + row];
                    TB[row * ST + lr16] = sd * acc[mt][0][r];
                    if (lr16 < LAT - 16) TB[row * ST + 16 + lr16] = sd * acc[mt][1][r];
                }
            }
    }
    wave_sync();
    // ---- J, two tracked joints at a time (one per half of the wave), and A = [J r]^T [J r] over them
    const int cn = lane & 31, hf = lane >> 5; // column of this lane and its half
    const bool col = cn < LAT;
    float dR0[9], dwd[3]; // the root's part of column cn: d R_0, d world_disp
#pragma unroll
    for (int k = 0; k < 9; ++k) dR0[k] = 0.f;
    dwd[0] = dwd[1] = dwd[2] = 0.f;
    if (col) {
        float dq[4], dqn[4], dw[4], wq[4], dd[3], t0[3], t1[3];
#pragma unroll
        for (int c = 0; c < 4; ++c) { dq[c] = TB[c * ST + cn]; wq[c] = WR[c]; }
        unit_jvp(QN, RN[0], dq, dqn);
        quat_mul(cr, dqn, dw);
        rotmat_jvp(wq, dw, dR0);
#pragma unroll
        for (int c = 0; c < 3; ++c) dd[c] = TB[(4 * NJ + c) * ST + cn];
        mv(dR0, d, t0);
        mv(R0, dd, t1);
#pragma unroll
        for (int c = 0; c < 3; ++c) dwd[c] = t0[c] + t1[c];
    }
    f4 na[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) na[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
    unsigned long long tm = tmask;
    while (tm != 0ull) {
        const int j0 = __builtin_ctzll(tm);
        tm &= tm - 1ull;
        const int j1 = tm != 0ull ? __builtin_ctzll(tm) : -1;
        if (tm != 0ull) tm &= tm - 1ull;
        const int jj = hf == 0 ? j0 : j1; // this half's joint (-1: none)
        float row[12];
#pragma unroll
        for (int r = 0; r < 12; ++r) row[r] = 0.f;
        if (jj >= 0 && cn <= LAT) {
            const float sp = SW[2 * jj], sr = SW[2 * jj + 1];
            if (col) {
                float dv[3] = {0.f, 0.f, 0.f}; // d v_jj: the bones of the path, each through its parent's quaternion
                int c = jj;
                for (int s = 0; s < NJ && c != 0; ++s) {
                    const int p = par[c];
                    if (p != 0) {
                        float dq[4], dqn[4], dRp[9], t[3];
#pragma unroll
                        for (int e = 0; e < 4; ++e) dq[e] = TB[(4 * p + e) * ST + cn];
                        unit_jvp(QN + 4 * p, RN[p], dq, dqn);
                        rotmat_jvp(QN + 4 * p, dqn, dRp);
                        mv(dRp, BONES + 3 * c, t);
                        dv[0] += t[0]; dv[1] += t[1]; dv[2] += t[2];
                    }
                    c = p;
                }
                float t0[3], t1[3];
                mv(dR0, VB + 4 * jj, t0);
                mv(R0, dv, t1);
#pragma unroll
                for (int e = 0; e < 3; ++e) row[e] = sp * ((dwd[e] + t0[e]) + t1[e]);
                if (jj == 0) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) row[3 + k] = sr * dR0[k];
                } else {
                    float dq[4], dqn[4], dRj[9];
#pragma unroll
                    for (int e = 0; e < 4; ++e) dq[e] = TB[(4 * jj + e) * ST + cn];
                    unit_jvp(QN + 4 * jj, RN[jj], dq, dqn);
                    rotmat_jvp(QN + 4 * jj, dqn, dRj);
                    const float* Rj = RB + 9 * jj;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int e = 0; e < 3; ++e)
                            row[3 + 3 * r + e] = sr * ((dR0[3 * r] * Rj[e] + dR0[3 * r + 1] * Rj[3 + e] + dR0[3 * r + 2] * Rj[6 + e]) +
                                                       (R0[3 * r] * dRj[e] + R0[3 * r + 1] * dRj[3 + e] + R0[3 * r + 2] * dRj[6 + e]));
                }
            } else { // cn == 24: the joint's 12 residuals
#pragma unroll
                for (int e = 0; e < 3; ++e) row[e] = sp * (PB[4 * jj + e] - TGT_POS(jj, e));
#pragma unroll
                for (int k = 0; k < 9; ++k) row[3 + k] = sr * (GB[9 * jj + k] - TGT_ROT(jj, k));
            }
        }
#pragma unroll
        for (int r = 0; r < 12; ++r) JB[(12 * hf + r) * SJ + cn] = row[r];
        wave_sync();
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const float v0 = JB[(4 * s + lk) * SJ + lr16], v1 = JB[(4 * s + lk) * SJ + 16 + lr16];
            na[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v0, na[0][0], 0, 0, 0);
            na[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v1, na[0][1], 0, 0, 0);
            na[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v0, na[1][0], 0, 0, 0);
            na[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v1, na[1][1], 0, 0, 0);
        }
        wave_sync(); // (the rows' last reads before the next pair's writes)
    }
