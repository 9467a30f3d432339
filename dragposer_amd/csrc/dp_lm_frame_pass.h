// dp_lm_frame_pass.h -- a fragment of text of the LM frame (dp_lm_body.h, dp_clip_rows_body.h), included in place: one forward pass of the
// latent FRAME_Z through the folded decoder and the kinematics, and the frame's three loss numbers.
//   parameter  FRAME_Z  the lane's component of the latent the pass runs on (lane k < 24: component k)
//   reads      lds, lane, j, jl, par, cr, zt, trk, wp, wrr, E, TGT_POS, TGT_ROT, a.lam_rot, a.lam_tmp; dp_lm_frame_consts.h's names; the
//              wave's block: ZB, HB0, HB1, DB0, DB1, QB, QN, RN, WR, RB, BB, VB, PB, GB
//   leaves     q, qn, rn, R, wr (the lane's joint; wr: lane 0's world root rotation), R0, d, wd (every lane's), vj, P, G, dpj, drj, dzz, dtj and
//              the wave-uniform lp, lr, lt; in the wave's block ZB, DB0, DB1, QN, RN, WR, RB, VB, PB, GB of this latent, for the tangents
//   opens      with its own wave_sync() behind the write of ZB: the includer's last reads of the wave's block lie behind one of its own
//   closes     WITHOUT one: the pass's last writes (PB, VB, GB) are the lane's own until the includer's next wave_sync()
    if (lane < LAT) ZB[lane] = FRAME_Z;
    wave_sync();
    // ---- decoder (autoencoder.py:224-256, folded), LeakyReLU(0.2) after layers 0 and 1
    if (lane < H0) {
        float s = c0;
#pragma unroll UNR
        for (int k = 0; k < LAT; ++k) s = fmaf(lds[L_A0 + lane * S0 + k], ZB[k], s);
        const bool p = s > 0.f;
        HB0[lane] = p ? s : s * 0.2f;
        DB0[lane] = p ? 1.f : 0.2f;
    }
    wave_sync();
    if (lane < H1) {
        float s = b1;
#pragma unroll UNR
        for (int k = 0; k < H0; ++k) s = fmaf(lds[L_A1 + lane * S1 + k], HB0[k], s);
        const bool p = s > 0.f;
        HB1[lane] = p ? s : s * 0.2f;
        DB1[lane] = p ? 1.f : 0.2f;
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
    // ---- kinematics, a lane per joint
    float q[4], qn[4], rn = 1.f, R[9], wr[4] = {1.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = jl ? QB[4 * j + c] : (c == 0 ? 1.f : 0.f);
    rn = 1.f / sqrtf(fmaf(q[0], q[0], fmaf(q[1], q[1], fmaf(q[2], q[2], q[3] * q[3]))));
#pragma unroll
    for (int c = 0; c < 4; ++c) qn[c] = q[c] * rn;
    if (j == 0) { quat_mul(cr, qn, wr); rotmat(wr, R); } // world root rotation, cur_rot as given (drag_pose.py:88)
    else rotmat(qn, R);
    if (jl) {
#pragma unroll
        for (int k = 0; k < 9; ++k) RB[9 * j + k] = R[k];
#pragma unroll
        for (int c = 0; c < 4; ++c) QN[4 * j + c] = qn[c];
        RN[j] = rn;
    }
    if (j == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) WR[c] = wr[c];
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
    float vj[3] = {0.f, 0.f, 0.f}, P[3], G[9];
    if (jl) {
        int c = j;
        for (int s = 0; s < NJ && c != 0; ++s) { // the path from j to the root (<= 7 bones)
            vj[0] += BB[4 * c]; vj[1] += BB[4 * c + 1]; vj[2] += BB[4 * c + 2];
            c = par[c];
        }
    }
    mv(R0, vj, P);
#pragma unroll
    for (int c = 0; c < 3; ++c) P[c] += wd[c];
    if (j == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) G[k] = R0[k];
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) G[3 * r + c] = R0[3 * r] * R[c] + R0[3 * r + 1] * R[3 + c] + R0[3 * r + 2] * R[6 + c];
    }
    if (jl) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { PB[4 * j + c] = P[c]; VB[4 * j + c] = vj[c]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) GB[9 * j + k] = G[k];
    }
    // ---- the loss (drag_pose.py:115-127)
    float dpj = 0.f, drj = 0.f;
    if (trk) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float e = P[c] - TGT_POS(j, c);
            dpj = fmaf(e, e, dpj);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float e = G[k] - TGT_ROT(j, k);
            drj = fmaf(e, e, drj);
        }
        dpj *= wp;
        drj *= wrr;
    }
    const float dzz = FRAME_Z - zt;
    const float dtj = lane < LAT ? dzz * dzz : 0.f;
    const float lp = uni(wsum(dpj)) / (3.f * (float)E), lr = a.lam_rot * (uni(wsum(drj)) / (9.f * (float)E)), lt = a.lam_tmp * (uni(wsum(dtj)) / 24.f);
