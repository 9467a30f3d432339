// dp_clip_rows_body.h -- the body of the clip solve's rows kernel, included behind the kernel's signature (its argument block is `a`, K is dpclip) with
//   DP_CLIP_SKEL 0  dp_clip_rows_kernel(K::Args): the bones are the context's, staged once per workgroup at L_OFF (dp_clip.hip)
//   DP_CLIP_SKEL 1  dp_clip_rows_skel_kernel(K::SkelArgs): the bones are those of the frame's own sequence, taken by each wave into a block of
//                   its own (dp_clip_skel.hip); everything it adds stands behind this switch, so the kernel above keeps its instructions
// BONES is where the frame's [22][3] bone offsets are read from, by the lane's own off[] and by the tangents, which read another joint's bone.
#define TGT_POS(jj, c) a.tgt_pos[(f * NJ + (jj)) * 3 + (c)]
#define TGT_ROT(jj, k) a.tgt_rot[(f * NJ + (jj)) * 9 + (k)]
#if DP_CLIP_SKEL
#define BONES (skb + wv * SK_W)
#else
#define BONES (lds + L_OFF)
#endif
{
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
#if DP_CLIP_SKEL
    __shared__ float skb[WPB * SK_W]; // [22][3] bones per wave (dp_lm_skel.h)
#endif
    const float* __restrict__ W = a.img;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    int* par = (int*)(lds + L_PAR);
    const int* Ti = (const int*)W;
    const int mode = a.mode;

    // ---- staging (once per workgroup): padded weight rows, sigma, the skeleton
    for (int i = tid; i < H0 * LAT; i += WPB * 64) lds[L_A0 + (i / LAT) * S0 + i % LAT] = W[dpvjp::OFF_A0 + i];
    for (int i = tid; i < H1 * H0; i += WPB * 64) lds[L_A1 + (i / H0) * S1 + i % H0] = W[dpvjp::OFF_A1 + i];
    for (int i = tid; i < dpvjp::NY * H1; i += WPB * 64) lds[L_A2 + (i / H1) * S2 + i % H1] = W[dpvjp::OFF_A2 + i];
    if (tid < dpvjp::NY) lds[L_SD + tid] = W[dpvjp::OFF_SD + tid];
    if (tid < NJ) par[tid] = Ti[dpvjp::OFF_PARENT + tid];
#if !DP_CLIP_SKEL
    if (tid < 3 * NJ) lds[L_OFF + tid] = W[dpvjp::OFF_BONE + tid];
#endif
    __syncthreads();

    const long long f = (long long)blockIdx.x * WPB + wv;
    if (f >= a.n_frames) return;
    const int sq = (int)(f % a.n_seq);
    const bool first = f < a.n_seq; // frame 0 of its sequence: no coupling part
    // the sequence's word: which frames this pass is for, and which buffer it reads
    const int word = mode == K::M_INIT ? 0 : a.wword[sq];
    const bool refused_seq = (word & K::W_REFUSED) != 0;
    if (mode == K::M_NORMAL && (word & (K::W_REFUSED | K::W_REJECTED)) != 0) return; // (A and g stand)
    if (mode == K::M_TRIAL && (refused_seq || a.wsolved[sq] == 0)) return;           // (no Z' to try)
    const int cur = (word & K::W_CUR) != 0 ? 1 : 0, buf = mode == K::M_TRIAL ? cur ^ 1 : cur;
    const float* __restrict__ zsrc = mode == K::M_INIT || refused_seq ? a.z0 : a.wz[buf]; // (a refused sequence stays at its z0)

    float* wb = lds + L_WAVE0 + wv * W_FLOATS;
    float *ZB = wb + W_Z, *HB0 = wb + W_H0, *HB1 = wb + W_H1, *DB0 = wb + W_D0, *DB1 = wb + W_D1, *QB = wb + W_Q, *QN = wb + W_QN, *RN = wb + W_RN,
          *WR = wb + W_WR, *RB = wb + W_R, *BB = wb + W_B, *VB = wb + W_V, *PB = wb + W_P, *GB = wb + W_G, *SW = wb + W_SW, *TB = wb + W_T,
          *JB = wb + W_J, *AB = wb + W_A;
    const float nan = __builtin_nanf("");
    const int j = lane; // joint of this lane (j < NJ)
    const bool jl = lane < NJ;

    // ---- screening (include/dragposer.h: DP_STATUS_*), dp_lm_body.h's, on the frame's own inputs in every mode
    float cr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cr[k] = a.cur_rot[f * 4 + k];
    const float z0 = lane < LAT ? a.z0[f * LAT + lane] : 0.f;
    const float zt = lane < LAT ? a.z_tgt[f * LAT + lane] : 0.f;
    const bool trk = jl && a.tracked[f * NJ + j] != 0;
#if DP_CLIP_SKEL
    // lane j: row j of the skeleton of the frame's sequence (stride 0: the launch's one) into the wave's own block -- the waves of a workgroup
    // belong to different sequences.  One unconditional load per row with the frame's other loads, the lanes beyond the joints on the last
    // row; what is no bone (row 0, those lanes) is selected away afterwards.  A component out of range refuses the frame, and so every frame
    // of the sequence (include/dragposer_skeleton.h's rule).
    bool bsk = false;
    {
        const float* __restrict__ sk = a.skel + (long long)sq * a.skel_stride + 3 * (jl ? j : NJ - 1);
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = sk[c];
        const bool bone = jl && j != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) bsk = bsk || (bone && refused(o[c]));
        if (jl)
#pragma unroll
            for (int c = 0; c < 3; ++c) BONES[3 * j + c] = bone ? o[c] : 0.f;
    }
    const bool bs = bsk || refused(z0) || refused(cr[0]) || refused(cr[1]) || refused(cr[2]) || refused(cr[3]);
#else
    const bool bs = refused(z0) || refused(cr[0]) || refused(cr[1]) || refused(cr[2]) || refused(cr[3]);
#endif
    bool bt = refused(zt), nrot = false;
    float wp = 0.f, wrr = 0.f;
    if (trk) {
        float m[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) bt = bt || refused(TGT_POS(j, k));
#pragma unroll
        for (int k = 0; k < 9; ++k) { m[k] = TGT_ROT(j, k); bt = bt || refused(m[k]); }
        wp = a.w[(f * NJ + j) * 2];
        wrr = a.w[(f * NJ + j) * 2 + 1];
        bt = bt || refused(wp) || refused(wrr);
        nrot = not_rotation(m);
    }
    const bool bad_state = __ballot(bs) != 0ull;
    const bool bad_tgt = !bad_state && __ballot(bt) != 0ull;
    const int not_rot = !bad_state && !bad_tgt && __ballot(nrot) != 0ull ? DP_STATUS_TARGET_NOT_ROTATION : 0;
    const unsigned long long tmask = __ballot(trk);
    const int E = __popcll(tmask);
    if (mode == K::M_INIT) {
        if (lane == 0) a.wflags[f] = bad_state ? DP_STATUS_BAD_STATE : bad_tgt ? DP_STATUS_BAD_TARGETS : 0;
        if (bad_state || bad_tgt) return; // (no step runs for this sequence: dp_clip_decide_kernel)
    }
    if (bad_state) { // (M_RESULTS: the other modes do not come here) every result NaN
        if (lane < LAT) {
            if (a.z) a.z[f * LAT + lane] = nan;
            if (a.z_pre) a.z_pre[f * LAT + lane] = nan;
        }
        if (jl) {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (a.pose) a.pose[f * 88 + 4 * j + c] = nan;
#pragma unroll
            for (int c = 0; c < 3; ++c) if (a.pos) a.pos[(f * NJ + j) * 3 + c] = nan;
#pragma unroll
            for (int c = 0; c < 9; ++c) if (a.rot) a.rot[(f * NJ + j) * 9 + c] = nan;
        }
        if (lane < 4 && a.world_rot) a.world_rot[f * 4 + lane] = nan;
        if (lane < 3) {
            if (a.disp) a.disp[f * 3 + lane] = nan;
            if (a.world_disp) a.world_disp[f * 3 + lane] = nan;
            if (a.loss) a.loss[f * 3 + lane] = nan;
        }
        if (lane == 0) {
            if (a.iters) a.iters[f] = 0;
            if (a.status) a.status[f] = DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE;
        }
        return;
    }

    // per-lane constants of the forward pass
    const float c0 = lane < H0 ? W[dpvjp::OFF_C0 + lane] : 0.f;
    const float b1 = lane < H1 ? W[dpvjp::OFF_B1 + lane] : 0.f;
    const int oB = 64 + lane; // second decoder row of lanes 0..26
    const float b2A = W[dpvjp::OFF_B2 + lane], sdA = W[dpvjp::OFF_SD + lane], muA = W[dpvjp::OFF_MU + lane];
    const float b2B = lane < NYU - 64 ? W[dpvjp::OFF_B2 + oB] : 0.f, sdB = lane < NYU - 64 ? W[dpvjp::OFF_SD + oB] : 1.f,
                muB = lane < NYU - 64 ? W[dpvjp::OFF_MU + oB] : 0.f;
    const int pj = jl ? par[j] : 0;
    float off[3] = {0.f, 0.f, 0.f};
    float sdj[4] = {1.f, 1.f, 1.f, 1.f}, muj[4] = {0.f, 0.f, 0.f, 0.f};
    if (jl) {
#pragma unroll
        for (int c = 0; c < 3; ++c) off[c] = BONES[3 * j + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) { sdj[c] = W[dpvjp::OFF_SD + 4 * j + c]; muj[c] = W[dpvjp::OFF_MU + 4 * j + c]; }
        SW[2 * j] = trk ? sqrtf(wp / (3.f * (float)E)) : 0.f;
        SW[2 * j + 1] = trk ? sqrtf(a.lam_rot * wrr / (9.f * (float)E)) : 0.f;
    }
    const float ct = a.lam_tmp / 24.f;

    const float z = lane < LAT ? zsrc[f * LAT + lane] : 0.f; // lane k < 24: component k of the latent this pass runs on
    if (lane < LAT) ZB[lane] = z;
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
    const float dzz = z - zt;
    const float dtj = lane < LAT ? dzz * dzz : 0.f;
    const float lp = uni(wsum(dpj)) / (3.f * (float)E), lr = a.lam_rot * (uni(wsum(drj)) / (9.f * (float)E)), lt = a.lam_tmp * (uni(wsum(dtj)) / 24.f);
    const float tot = (lp + lr) + lt;

    if (mode == K::M_INIT || mode == K::M_TRIAL) { // the frame's numbers for the decision: its loss, and |z_t - z_(t-1)|^2 in double
        double cd = 0.0;
        if (!first && lane < LAT) cd = (double)z - (double)zsrc[(f - a.n_seq) * LAT + lane];
        const double cp = wsum_d(cd * cd);
        if (lane == 0) {
            float* const o = a.wloss[buf] + f * 4;
            o[0] = lp; o[1] = lr; o[2] = lt; o[3] = tot;
            a.wcpl[buf][f] = cp;
        }
        if (mode == K::M_INIT && lane < LAT) a.wz[0][f * LAT + lane] = z;
        if (mode == K::M_TRIAL) return;
    }

    if (mode == K::M_RESULTS) { // every dp_result array at the returned latent, whose pass this was
        const bool nonfin = bad_tgt || __ballot(lane < LAT && !(fabsf(z) <= 3.0e38f)) != 0ull;
        if (lane < LAT) {
            if (a.z) a.z[f * LAT + lane] = bad_tgt ? nan : z;
            if (a.z_pre) a.z_pre[f * LAT + lane] = bad_tgt ? nan : z;
        }
        if (jl) {
            if (a.pose)
#pragma unroll
                for (int c = 0; c < 4; ++c) a.pose[f * 88 + 4 * j + c] = (qn[c] - muj[c]) / sdj[c];
            if (a.pos)
#pragma unroll
                for (int c = 0; c < 3; ++c) a.pos[(f * NJ + j) * 3 + c] = P[c];
            if (a.rot)
#pragma unroll
                for (int k = 0; k < 9; ++k) a.rot[(f * NJ + j) * 9 + k] = G[k];
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.disp) a.disp[f * 3 + c] = d[c];
                if (a.world_disp) a.world_disp[f * 3 + c] = wd[c];
            }
            if (a.world_rot)
#pragma unroll
                for (int c = 0; c < 4; ++c) a.world_rot[f * 4 + c] = wr[c];
            if (a.loss) {
                a.loss[f * 3] = bad_tgt ? nan : lp; a.loss[f * 3 + 1] = bad_tgt ? nan : lr; a.loss[f * 3 + 2] = bad_tgt ? nan : lt;
            }
            if (a.iters) a.iters[f] = refused_seq ? 0 : a.n_steps;
            if (a.status) a.status[f] = (nonfin ? DP_STATUS_NONFINITE_RESULT : 0) | (bad_tgt ? DP_STATUS_BAD_TARGETS : 0) | not_rot;
        }
        return;
    }

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
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * mt + 4 * lk + r;
            if (row <= LAT) {
                AB[row * SJ + lr16] = na[mt][0][r];
                AB[row * SJ + 16 + lr16] = na[mt][1][r];
            }
        }
    wave_sync();
    if (lane < LAT) { // the latent pull: sqrt(lambda_tmp / 24) on the diagonal of J, r = that times (z - z_tgt)
        AB[lane * SJ + lane] += ct;
        AB[lane * SJ + LAT] += ct * (z - zt);
    }
    wave_sync();
    // ---- A_t (rows 0..23) | g_t (row 24) to the workspace
    float* const ag = a.wag + f * K::AG_FLOATS;
    for (int e = lane; e < K::AG_FLOATS; e += 64) {
        const int r = e / LAT, c = e - LAT * r;
        ag[e] = r < LAT ? AB[r * SJ + c] : AB[c * SJ + LAT];
    }
}
#undef TGT_POS
#undef TGT_ROT
#undef BONES
