// dp_lm_body.h -- the body of the five per-frame LM kernels, included behind the kernel's signature (its argument block is `a`) with
//   DP_LM_SEQ 0  dp_lm_kernel(Args): one frame per wave, as dp_lm.hip describes it
//   DP_LM_SEQ 1  dp_lm_seq_kernel(SeqArgs): one SEQUENCE per wave, the step loop around the same frame (dp_lm_seq.hip)
//   DP_LM_TERMS 1 (with DP_LM_SEQ 0)  dp_lm_terms_kernel(TermArgs): the frame with a table of constraint terms in its loss (dp_lm_terms.hip);
//                 everything it adds stands behind this switch, so the other two kernels keep their instructions
//   DP_LM_SEQ 1 and DP_LM_TERMS 1  dp_lm_seq_terms_kernel(SeqTermArgs): the step loop around the frame with the table (dp_lm_seq_terms.hip).
//                 What only the two together need stands behind both switches, so the three kernels above keep their instructions
//   DP_LM_SKEL 1 (with DP_LM_SEQ 0, DP_LM_TERMS 0)  dp_lm_skel_kernel(SkelArgs): the frame on its own skeleton's bones, taken by each wave into a
//                 block of its own (dp_lm_skel.hip); what it adds stands behind this switch, so the four kernels above keep their instructions
// TGT_POS(jj, c) / TGT_ROT(jj, k) are joint jj's targets of the frame at hand: the batch's row, or the step's row with the step's shift.
// What is the body's own: the screening, the step loop of a sequence, the iteration loop with its decisions, the reported loss in double, the
// terms, the solve and the results.  The frame itself is text shared with the clip solve's rows kernel (dp_clip_rows_body.h), included in place
// from dp_lm_frame_*.h: stage (the staging, and BONES, where the frame's bones are read from), skel (a frame's own skeleton into the wave's
// block), consts, pass (decoder, kinematics, loss), tangents (with J and [J r]^T [J r]) and close (into AB, the latent pull).  Each names at
// its head what it reads from this scope, what it leaves behind and which wave_sync() it opens or closes with; what differs between the two
// bodies is a macro defined just before the include.
#ifndef DP_LM_TERMS
#define DP_LM_TERMS 0
#endif
#ifndef DP_LM_SKEL
#define DP_LM_SKEL 0
#endif
#if DP_LM_SKEL && (DP_LM_SEQ || DP_LM_TERMS)
#error "per-frame skeletons: the plain frame only (include/dragposer_clip_skeleton.h, Not covered)"
#endif
#if DP_LM_SEQ
#define TGT_POS(jj, c) (a.q.tgt_root ? __fadd_rn(a.tgt_pos[(ft * NJ + (jj)) * 3 + (c)], sh[c]) : a.tgt_pos[(ft * NJ + (jj)) * 3 + (c)])
#define TGT_ROT(jj, k) a.tgt_rot[(ft * NJ + (jj)) * 9 + (k)]
#else
#define TGT_POS(jj, c) a.tgt_pos[(f * NJ + (jj)) * 3 + (c)]
#define TGT_ROT(jj, k) a.tgt_rot[(f * NJ + (jj)) * 9 + (k)]
#endif
{
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
#if DP_LM_SEQ
    __shared__ float arh[WPB * AR_W_FLOATS];
#endif
#if DP_LM_TERMS
    __shared__ __attribute__((aligned(16))) float tl[TERM_LDS_FLOATS]; // the term table, then a block of rows per wave (dp_lm_terms.h)
#endif
    const float* __restrict__ W = a.img;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int* par = (int*)(lds + L_PAR);
    const int* Ti = (const int*)W;

#define FRAME_SKEL DP_LM_SKEL
#include "dp_lm_frame_stage.h" // staging (once per workgroup): padded weight rows, sigma, the skeleton; BONES
#undef FRAME_SKEL
#if DP_LM_TERMS
    for (int i = tid; i < a.n_terms * TW; i += WPB * 64) ((unsigned*)tl)[TL_TBL + i] = a.tbl[i];
#endif
    __syncthreads();

    const long long f = (long long)blockIdx.x * WPB + wv;
    if (f >= a.n_frames) return;
    float* wb = lds + L_WAVE0 + wv * W_FLOATS;
    float *ZB = wb + W_Z, *HB0 = wb + W_H0, *HB1 = wb + W_H1, *DB0 = wb + W_D0, *DB1 = wb + W_D1, *QB = wb + W_Q, *QN = wb + W_QN, *RN = wb + W_RN,
          *WR = wb + W_WR, *RB = wb + W_R, *BB = wb + W_B, *VB = wb + W_V, *PB = wb + W_P, *GB = wb + W_G, *SW = wb + W_SW, *TB = wb + W_T,
          *JB = wb + W_J, *AB = wb + W_A;
    const float nan = __builtin_nanf("");
    const int j = lane; // joint of this lane (j < NJ)
    const bool jl = lane < NJ;

#if DP_LM_SEQ
    // what the sequence carries from step to step: the latent (lane k: component k), the global rotation and position (every lane), and mu as
    // the caller's array holds it (a step that runs reads it as dp_lm_kernel does; a refused step leaves it as it is)
    float zc = lane < LAT ? a.z0[f * LAT + lane] : 0.f, crc[4], gpc[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) crc[k] = a.cur_rot[f * 4 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) gpc[k] = a.q.global_pos[f * 3 + k];
    float muc = a.mu ? a.mu[f] : a.mu0;
    const int NS = a.n_frames, NH = a.q.n_heights;
    const bool trk = jl && a.tracked[f * NJ + j] != 0; // (the trackers and their weights: one row per sequence, held for all steps)
    float wp = 0.f, wrr = 0.f;
    if (trk) {
        wp = a.w[(f * NJ + j) * 2];
        wrr = a.w[(f * NJ + j) * 2 + 1];
    }
    float* const hb = arh + wv * AR_W_FLOATS; // lane i: column i of the sequence's last `order` history rows, the newest (h_1) first
    if (a.r.coeffs) {
        if (lane < LAT)
#pragma unroll
            for (int k = 0; k < MAX_AR_ORDER; ++k)
                if (k < a.r.order) hb[k * LAT + lane] = a.r.latent_buf[(f * a.r.history + (a.r.history - 1 - k)) * LAT + lane];
        wave_sync();
    }
    for (int stp = 0; stp < a.q.n_steps; ++stp) { // ---- the step loop: frame stp of this sequence, row ft of every per-step array
    const long long ft = (long long)stp * NS + f;
    float cr[4] = {crc[0], crc[1], crc[2], crc[3]};
    const float z0 = zc;
    float zt = 0.f;
    if (a.r.coeffs) { // include/dragposer_latent_ar.h, "The predictor": lane i forms component i, unfused, in the stated order
        if (lane < LAT) {
            zt = a.r.bias[lane];
            for (int k = 0; k < a.r.order; ++k) {
                const float* __restrict__ Ak = a.r.coeffs + (k * LAT + lane) * LAT;
#pragma unroll
                for (int c = 0; c < LAT; ++c) zt = __fadd_rn(zt, __fmul_rn(Ak[c], hb[k * LAT + c]));
            }
        }
    } else if (lane < LAT) zt = a.z_tgt[(long long)stp * a.q.z_tgt_step + f * a.q.z_tgt_seq + lane];
    float sh[3] = {0.f, 0.f, 0.f}; // this step's target shift: tgt_root[stp] - the global position before the step
    if (a.q.tgt_root)
#pragma unroll
        for (int k = 0; k < 3; ++k) sh[k] = __fsub_rn(a.q.tgt_root[ft * 3 + k], gpc[k]);
#else
    // ---- screening (include/dragposer.h: DP_STATUS_*), the dp_cons family's
    float cr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cr[k] = a.cur_rot[f * 4 + k];
    const float z0 = lane < LAT ? a.z0[f * LAT + lane] : 0.f;
    const float zt = lane < LAT ? a.z_tgt[f * LAT + lane] : 0.f;
    const bool trk = jl && a.tracked[f * NJ + j] != 0;
#endif
#if DP_LM_SKEL
#define FRAME_SKEL_ROW (f * (long long)a.skel_stride) // this frame's
#include "dp_lm_frame_skel.h" // lane j: row j of the skeleton into the wave's own block; bsk
#undef FRAME_SKEL_ROW
#endif
#if DP_LM_TERMS
    float gp[3] = {0.f, 0.f, 0.f}; // global_pos: read, and screened, only when an active PLANE or point-DISTANCE term exists
    if (a.need_gp)
#pragma unroll
#if DP_LM_SEQ // (the carried position, as it stands before this step: what the composition hands dp_optimize_lm_terms)
        for (int k = 0; k < 3; ++k) gp[k] = gpc[k];
#else
        for (int k = 0; k < 3; ++k) gp[k] = a.global_pos[f * 3 + k];
#endif
    const bool bs = refused(z0) || refused(cr[0]) || refused(cr[1]) || refused(cr[2]) || refused(cr[3]) || refused(gp[0]) || refused(gp[1]) ||
                    refused(gp[2]);
#elif DP_LM_SKEL
    const bool bs = bsk || refused(z0) || refused(cr[0]) || refused(cr[1]) || refused(cr[2]) || refused(cr[3]);
#else
    const bool bs = refused(z0) || refused(cr[0]) || refused(cr[1]) || refused(cr[2]) || refused(cr[3]);
#endif
    bool bt = refused(zt), nrot = false;
#if !DP_LM_SEQ
    float wp = 0.f, wrr = 0.f;
#endif
    if (trk) {
        float m[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) bt = bt || refused(TGT_POS(j, k));
#pragma unroll
        for (int k = 0; k < 9; ++k) { m[k] = TGT_ROT(j, k); bt = bt || refused(m[k]); }
#if !DP_LM_SEQ
        wp = a.w[(f * NJ + j) * 2];
        wrr = a.w[(f * NJ + j) * 2 + 1];
#endif
        bt = bt || refused(wp) || refused(wrr);
        nrot = not_rotation(m);
    }
#if DP_LM_TERMS
    float* const RW = tl + TL_ROW0 + wv * TW_ROW; // [MAX_TERMS][4] the frame's rows (vector, s_f), defaults filled in
    float wst = 0.f;                              // lane t: c_t = weight_t * s_f
    if (lane < a.n_terms) { // lane t: term t's row of this frame (the term's own vector and s_f = 1 without one), the dp_cons family's screening
        const float* tb = tl + TL_TBL + lane * TW;
        const int type = __float_as_int(tb[T_TYPE]);
        const float* pf = *(const float* const*)(tb + T_ROW);
        float r[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = type == DP_TERM_ALIGN ? tb[T_DIR + c] : tb[T_PT + c];
        r[3] = 1.f;
        if (pf && tb[T_W] != 0.f) {
#pragma unroll
#if DP_LM_SEQ // (the term's rows of this step: T_STEP floats further per step, 0 = one row held, as dp_cons_body.h reads them)
            for (int c = 0; c < 4; ++c) r[c] = pf[(long long)stp * __float_as_int(tb[T_STEP]) + f * 4 + c];
#else
            for (int c = 0; c < 4; ++c) r[c] = pf[f * 4 + c];
#endif
            bt = bt || refused(r[0]) || refused(r[1]) || refused(r[2]) || refused(r[3]) || r[3] < 0.f;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) RW[4 * lane + c] = r[c];
        wst = tb[T_W] * r[3];
    }
#endif
    const bool bad_state = __ballot(bs) != 0ull;
    const bool bad_tgt = !bad_state && __ballot(bt) != 0ull;
#if DP_LM_TERMS
    // the frame's active terms, bit t: c_t != 0.  A term that is off has no row, no part in the loss and a loss slot of 0; the active ones
    // take their places in the term pass and in the loss's sum in the table's order, so a table without the others gives the same bits
    const unsigned tact = bad_tgt ? 0u : (unsigned)__ballot(wst != 0.f);
    wave_sync();
#endif
    const int not_rot = !bad_state && !bad_tgt && __ballot(nrot) != 0ull ? DP_STATUS_TARGET_NOT_ROTATION : 0;
    const unsigned long long tmask = __ballot(trk);
    const int E = __popcll(tmask);
#if DP_LM_SEQ
    if (bad_state) { // this step's results NaN and, as the per-frame epilogue makes them from such a frame, the carried state: every later step too
        float* const o = a.q.hist + ft * (LAT + 3 + NH);
        if (lane < LAT + 3 + NH) o[lane] = nan;
        if (jl) {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (a.pose) a.pose[ft * 88 + 4 * j + c] = nan;
#pragma unroll
            for (int c = 0; c < 3; ++c) if (a.pos) a.pos[(ft * NJ + j) * 3 + c] = nan;
        }
        if (lane < 4 && a.world_rot) a.world_rot[ft * 4 + lane] = nan;
        if (lane < LAT && a.r.trace) a.r.trace[ft * LAT + lane] = nan; // (the history stays as it is; the step used no target)
        if (lane < 3) {
            if (a.q.pos_ret) a.q.pos_ret[ft * 3 + lane] = nan;
            if (a.loss) a.loss[ft * 3 + lane] = nan;
            if (a.loss0) a.loss0[ft * 3 + lane] = nan;
        }
#if DP_LM_TERMS
        if (lane < a.n_terms && a.loss_terms) a.loss_terms[ft * a.n_terms + lane] = nan;
#endif
        if (lane == 0) {
            if (a.iters) a.iters[ft] = 0;
            if (a.n_accepted) a.n_accepted[ft] = 0;
            if (a.mu_trace) a.mu_trace[ft] = muc;
            if (a.status) a.status[ft] = DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE;
        }
        zc = nan;
#pragma unroll
        for (int k = 0; k < 4; ++k) crc[k] = nan;
#pragma unroll
        for (int k = 0; k < 3; ++k) gpc[k] = nan;
        // (nothing of the wave's block was touched: no wave_sync() needed before the next step.  With the table, lane t has written row t of
        // the wave's RW rows and nothing has read them; the next step's lane t writes the same words, in program order)
        continue;
    }
    if (lane < LAT && a.r.trace) a.r.trace[ft * LAT + lane] = zt;
#else
    if (bad_state) { // every result NaN
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
            if (a.loss0) a.loss0[f * 3 + lane] = nan;
        }
#if DP_LM_TERMS
        if (lane < a.n_terms && a.loss_terms) a.loss_terms[f * a.n_terms + lane] = nan;
#endif
        if (lane == 0) {
            if (a.iters) a.iters[f] = 0;
            if (a.n_accepted) a.n_accepted[f] = 0;
            if (a.status) a.status[f] = DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE;
        }
        return;
    }
#endif

#include "dp_lm_frame_consts.h" // per-lane constants of the forward pass: c0 .. muB, pj, off, sdj, muj, ct; SW

#if DP_LM_SEQ
    float mu = muc;
#else
    float mu = a.mu ? a.mu[f] : a.mu0;
#endif
    if (!(mu >= a.mu_min && mu <= a.mu_max)) mu = a.mu0;
    mu = uni(mu);

    float z = z0;          // lane k < 24: component k of the kept latent
    float zz = z0;         // ... of the latent the forward pass runs on
    float Lp = 0.f, Lr = 0.f, Lt = 0.f, Ltot = 0.f; // the kept latent's loss
    int mode = 0;          // 0: the pass of z0;  1: a trial;  2: the kept latent once more, for the results
    int steps = 0, nacc = 0;
    bool hit_max = false;
    for (;;) {
#define FRAME_Z zz
#include "dp_lm_frame_pass.h" // decoder, kinematics, loss: q, qn, rn, R, wr, R0, d, wd, vj, P, G and lp, lr, lt
#undef FRAME_Z
#if DP_LM_TERMS
        // the loss that decides the steps: the three numbers, then the frame's active terms c_t T_t in the table's order.  Lane t evaluates
        // term t on this pass's P_j and G_j with its true T (the bands' relu included), whatever rows the step used
        float tot = (lp + lr) + lt;
        if (tact != 0u) {
            wave_sync(); // (this pass's P_j and G_j are in the wave's block for every lane)
            float tv = 0.f;
            if (lane < MAX_TERMS && ((tact >> (lane & (MAX_TERMS - 1))) & 1u) != 0u) tv = term_value<float>(tl + TL_TBL + lane * TW, RW + 4 * lane, wst, PB, 4, GB, gp, a.up);
            for (unsigned m = tact; m != 0u; m &= m - 1u)
                tot += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tv), __builtin_ctz(m)));
        }
#else
        const float tot = (lp + lr) + lt;
#endif

        // ---- what the pass was for
        bool fresh = true; // the wave's block belongs to the kept latent
        if (mode == 0) {
            Lp = lp; Lr = lr; Lt = lt; Ltot = tot;
        } else if (mode == 1) {
            ++steps;
            if (tot < Ltot) { // (a NaN rejects)
                z = zz; Lp = lp; Lr = lr; Lt = lt; Ltot = tot;
                ++nacc;
                mu = fmaxf(mu * a.mu_down, a.mu_min);
                hit_max = false;
            } else {
                fresh = false;
                hit_max = mu >= a.mu_max;
                mu = fminf(mu * a.mu_up, a.mu_max);
            }
        }
        const bool done = mode == 2 || bad_tgt || steps >= a.n_steps ||
                          (a.early_stop && ((Lp <= a.stop_eps_pos && Lr <= a.stop_eps_rot) || hit_max));
        if (done && !fresh) { // the last trial was rejected: the kept latent's pass once more
            zz = z;
            mode = 2;
            continue;
        }
        // ---- the loss as it is REPORTED (loss0 after the pass of z0, loss with the results): the latent in the wave's block once more through
        // the decoder and the kinematics in double, on the same fp32 weights.  Near the solution a residual is millimetres and the fp32 pass
        // places a joint to 1e-7 .. 1e-6 m, which is 1e-5 .. 1e-4 of the loss; the steps are decided on the fp32 numbers above (they compare
        // two passes of the same arithmetic), the caller gets the value of the loss at the latent it is handed.  Only when asked for.
        float rep[3] = {Lp, Lr, Lt};
#if DP_LM_TERMS
        const bool rep0 = mode == 0 && a.loss0 != nullptr, rep1 = done && (a.loss != nullptr || (a.loss_terms != nullptr && tact != 0u));
        float tvr = 0.f; // lane t: loss_terms' slot t, the weighted term at the returned latent from the pass in double (0: the term is off)
#else
        const bool rep0 = mode == 0 && a.loss0 != nullptr, rep1 = done && a.loss != nullptr;
#endif
        if ((rep0 || rep1) && !bad_tgt) {
            double* const DH0 = (double*)TB; // [40] | [60] | [92] | [22][9] | [22][3]: the tangents' place, idle here
            double *const DH1 = DH0 + 40, *const DQ = DH1 + 60, *const DR = DQ + 92, *const DB = DR + 198;
            wave_sync();
            if (lane < H0) {
                double s = (double)c0;
#pragma unroll UNR
                for (int k = 0; k < LAT; ++k) s = fma((double)lds[L_A0 + lane * S0 + k], (double)ZB[k], s);
                DH0[lane] = s > 0.0 ? s : s * 0.2;
            }
            wave_sync();
            if (lane < H1) {
                double s = (double)b1;
#pragma unroll UNR
                for (int k = 0; k < H0; ++k) s = fma((double)lds[L_A1 + lane * S1 + k], DH0[k], s);
                DH1[lane] = s > 0.0 ? s : s * 0.2;
            }
            wave_sync();
            {
                double s = (double)b2A, t = (double)b2B;
#pragma unroll UNR
                for (int k = 0; k < H1; ++k) {
                    const double h = DH1[k];
                    s = fma((double)lds[L_A2 + lane * S2 + k], h, s);
                    if (lane < NYU - 64) t = fma((double)lds[L_A2 + oB * S2 + k], h, t);
                }
                DQ[lane] = fma(s, (double)sdA, (double)muA);
                if (lane < NYU - 64) DQ[oB] = fma(t, (double)sdB, (double)muB);
            }
            wave_sync();
            double qd[4], Rd[9];
#pragma unroll
            for (int c = 0; c < 4; ++c) qd[c] = jl ? DQ[4 * j + c] : (c == 0 ? 1.0 : 0.0);
            const double rnd = 1.0 / sqrt(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]);
#pragma unroll
            for (int c = 0; c < 4; ++c) qd[c] *= rnd;
            if (j == 0) {
                const double crd[4] = {(double)cr[0], (double)cr[1], (double)cr[2], (double)cr[3]};
                double wrd[4];
                quat_mul_d(crd, qd, wrd);
                rotmat_d(wrd, Rd);
            } else rotmat_d(qd, Rd);
            if (jl)
#pragma unroll
                for (int k = 0; k < 9; ++k) DR[9 * j + k] = Rd[k];
            wave_sync();
            double R0d[9], dd[3], wdd[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R0d[k] = DR[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) dd[c] = DQ[4 * NJ + c];
            mv_d(R0d, dd, wdd);
            if (jl) {
                const double od[3] = {(double)off[0], (double)off[1], (double)off[2]};
                double b[3] = {od[0], od[1], od[2]};
                if (j == 0) b[0] = b[1] = b[2] = 0.0;
                else if (pj != 0) mv_d(DR + 9 * pj, od, b);
#pragma unroll
                for (int c = 0; c < 3; ++c) DB[3 * j + c] = b[c];
            }
            wave_sync();
            double vd[3] = {0.0, 0.0, 0.0}, Pd[3];
            if (jl) {
                int c = j;
                for (int s = 0; s < NJ && c != 0; ++s) {
                    vd[0] += DB[3 * c]; vd[1] += DB[3 * c + 1]; vd[2] += DB[3 * c + 2];
                    c = par[c];
                }
            }
            mv_d(R0d, vd, Pd);
#if DP_LM_TERMS
            if (done && tact != 0u) { // the terms at the returned latent: every joint's P and G in double behind the pass's arrays, lane t on term t
                double *const DP = DB + 66, *const DG = DP + 66; // [22][3] | [22][9]
                if (jl) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) DP[3 * j + c] = Pd[c] + wdd[c];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            DG[9 * j + 3 * r + c] = j == 0 ? R0d[3 * r + c] : R0d[3 * r] * Rd[c] + R0d[3 * r + 1] * Rd[3 + c] + R0d[3 * r + 2] * Rd[6 + c];
                }
                wave_sync();
                if (lane < MAX_TERMS && ((tact >> (lane & (MAX_TERMS - 1))) & 1u) != 0u)
                    tvr = (float)term_value<double>(tl + TL_TBL + lane * TW, RW + 4 * lane, wst, DP, 3, DG, gp, a.up);
            }
#endif
            double dp64 = 0.0, dr64 = 0.0;
            if (trk) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double e = (Pd[c] + wdd[c]) - (double)TGT_POS(j, c);
                    dp64 = fma(e, e, dp64);
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double g = j == 0 ? R0d[3 * r + c] : R0d[3 * r] * Rd[c] + R0d[3 * r + 1] * Rd[3 + c] + R0d[3 * r + 2] * Rd[6 + c];
                        const double e = g - (double)TGT_ROT(j, 3 * r + c);
                        dr64 = fma(e, e, dr64);
                    }
                dp64 *= (double)wp;
                dr64 *= (double)wrr;
            }
            const double dz64 = lane < LAT ? (double)ZB[lane] - (double)zt : 0.0;
            const double sp64 = wsum_d(dp64), sr64 = wsum_d(dr64), st64 = wsum_d(dz64 * dz64);
            rep[0] = uni((float)(sp64 / (3.0 * (double)E)));
            rep[1] = uni((float)((double)a.lam_rot * (sr64 / (9.0 * (double)E))));
            rep[2] = uni((float)((double)a.lam_tmp * (st64 / 24.0)));
            wave_sync(); // (the pass's last reads before the tangents take their place back)
        }
#if DP_LM_SEQ
        if (rep0 && lane < 3) a.loss0[ft * 3 + lane] = bad_tgt ? nan : lane == 0 ? rep[0] : lane == 1 ? rep[1] : rep[2];
        if (done) { // results of the kept latent, whose pass this was, and run()'s epilogue (drag_pose.py:369-402) on them: the arithmetic and order of
                    // dp_sequence_advance_kernel, which reads them from the per-frame kernel's result arrays.  Every lane holds the same wd, d and
                    // carried gpc and computes the same new position.  (A bad target: the warm start's pose and a NaN latent, as per frame.)
            long long fo = ft; // (opaque: the step's store addresses are formed here, not hoisted into registers that live across the iteration loop)
            asm volatile("" : "+v"(fo));
            wave_sync(); // (this pass's P_j are in the wave's block for every lane)
            const float zr = bad_tgt ? nan : z;
            float gpn[3], dsp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                gpn[k] = __fadd_rn(gpc[k], wd[k]); // drag_pose.py:370
                dsp[k] = d[k];
            }
            if (a.q.adjust_joint >= 0) { // drag_pose.py:377-384, against that joint's effective target
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float tk = a.tgt_pos[(fo * NJ + a.q.adjust_target_joint) * 3 + k];
                    if (a.q.tgt_root) tk = __fadd_rn(tk, sh[k]);
                    // a difference, a product and two sums, none fused: dp_sequence_advance_kernel's v_sub, v_mul, v_add, v_add
                    const float adj = __fmul_rn(__fsub_rn(tk, PB[4 * a.q.adjust_joint + k]), a.q.adjust_weight);
                    gpn[k] = __fadd_rn(gpn[k], adj);
                    dsp[k] = __fadd_rn(dsp[k], adj);
                }
            }
            float* const o = a.q.hist + fo * (LAT + 3 + NH);
            if (lane < LAT) {
                o[lane] = zr;
                if (a.r.coeffs) { // the step's history row becomes h_1, the older rows shift: lane i on column i, read again behind the step's closing wave_sync()
                    float* const hs = hb + lane;
#pragma unroll
                    for (int k = MAX_AR_ORDER - 1; k > 0; --k)
                        if (k < a.r.order) hs[k * LAT] = hs[(k - 1) * LAT];
                    hs[0] = zr;
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o[LAT + k] = dsp[k];
                    if (a.q.pos_ret) a.q.pos_ret[fo * 3 + k] = gpn[k];
                }
                for (int h = 0; h < NH; ++h) o[LAT + 3 + h] = __fadd_rn(PB[4 * a.q.height_joints[h] + 1], gpn[1]); // y of (pos + the new global position)
            }
            if (jl) {
                if (a.pose)
#pragma unroll
                    for (int c = 0; c < 4; ++c) // the returned pose: root channels = the normalised world rotation (drag_pose.py:399-402)
                        a.pose[fo * 88 + 4 * j + c] = j == 0 ? (wr[c] - a.q.mean_q0[c]) / a.q.std_q0[c] : (qn[c] - muj[c]) / sdj[c];
                if (a.pos)
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.pos[(fo * NJ + j) * 3 + c] = P[c];
            }
            if (lane == 0) {
                if (a.world_rot)
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.world_rot[fo * 4 + c] = wr[c];
                if (a.loss) {
                    a.loss[fo * 3] = bad_tgt ? nan : rep[0]; a.loss[fo * 3 + 1] = bad_tgt ? nan : rep[1]; a.loss[fo * 3 + 2] = bad_tgt ? nan : rep[2];
                }
            }
#if DP_LM_TERMS
            if (lane < a.n_terms && a.loss_terms) a.loss_terms[fo * a.n_terms + lane] = bad_tgt ? nan : tvr;
#endif
            zc = zr;
#pragma unroll
            for (int k = 0; k < 3; ++k) gpc[k] = gpn[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) crc[k] = uni(wr[k]); // lane 0 holds the world root rotation (drag_pose.py:371)
            break;
        }
#else
        if (rep0 && lane < 3) a.loss0[f * 3 + lane] = bad_tgt ? nan : lane == 0 ? rep[0] : lane == 1 ? rep[1] : rep[2];
        if (done) { // results: all of the kept latent, whose pass this was
            if (lane < LAT) {
                if (a.z) a.z[f * LAT + lane] = bad_tgt ? nan : z;
                if (a.z_pre) a.z_pre[f * LAT + lane] = bad_tgt ? nan : z;
            }
#if DP_LM_TERMS
            if (lane < a.n_terms && a.loss_terms) a.loss_terms[f * a.n_terms + lane] = bad_tgt ? nan : tvr;
#endif
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
                    a.loss[f * 3] = bad_tgt ? nan : rep[0]; a.loss[f * 3 + 1] = bad_tgt ? nan : rep[1]; a.loss[f * 3 + 2] = bad_tgt ? nan : rep[2];
                }
            }
            break;
        }
#endif

        if (fresh) {
#include "dp_lm_frame_tangents.h" // the tangents, then J two joints at a time: na, and lr16, lk, cn, hf, dR0, dwd
#if DP_LM_TERMS
            // ---- the terms' rows (include/dragposer_lm_terms.h), into the same place and the same four tiles.  A round takes the next eight
            // active terms, four per half of the wave, each in three rows of the half's twelve: lane n < 24 forms column n of its half's terms'
            // rows, lane 24 their residuals; rows a term does not use, and the rows of a sub-slot without a term, are zero
            for (unsigned rem = tact; rem != 0u;) {
                unsigned mine = rem;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (hf != 0) mine &= mine - 1u; // (the second half skips the first half's four)
                    rem &= rem - 1u;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) rem &= rem - 1u;
#pragma unroll 1
                for (int sl = 0; sl < 4; ++sl) {
                    float r3[3] = {0.f, 0.f, 0.f};
                    if (mine != 0u && cn <= LAT) {
                        const int t = __builtin_ctz(mine);
                        term_rows(tl + TL_TBL + t * TW, RW + 4 * t, cn, PB, GB, gp, a.up, par, BONES, TB, QN, RN, RB, VB, R0, dR0, dwd, r3);
                    }
                    mine &= mine - 1u;
#pragma unroll
                    for (int e = 0; e < 3; ++e) JB[(12 * hf + 3 * sl + e) * SJ + cn] = r3[e];
                }
                wave_sync();
#pragma unroll
                for (int s = 0; s < 6; ++s) {
                    const float v0 = JB[(4 * s + lk) * SJ + lr16], v1 = JB[(4 * s + lk) * SJ + 16 + lr16];
                    na[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v0, na[0][0], 0, 0, 0);
                    na[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, v1, na[0][1], 0, 0, 0);
                    na[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v0, na[1][0], 0, 0, 0);
                    na[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, v1, na[1][1], 0, 0, 0);
                }
                wave_sync(); // (the rows' last reads before the next round's writes)
            }
#endif
#include "dp_lm_frame_close.h" // na into AB, the latent pull
        }

        // ---- the solve: H = A + mu diag(A), -g as the 25th row; Cholesky in place, lane i on row i
        float* HM = JB;
        for (int e = lane; e < 25 * 25; e += 64) {
            const int r = e / 25, c = e - 25 * r;
            float v = 0.f;
            if (r < LAT && c < LAT) v = r == c ? AB[r * SJ + c] * (1.f + mu) : AB[r * SJ + c];
            else if (r == LAT && c < LAT) v = -AB[c * SJ + LAT];
            HM[e] = v;
        }
        bool ok = true;
        float myinv = 0.f;
        // column by column, left-looking: lane i >= k forms s = H_ik - sum_(m<k) L_im L_km from its own row and row k (reads only, one store
        // per column), the pivot is lane k's s; row 24 (-g) comes out as y, L y = -g
        const int rw = lane <= LAT ? lane : LAT; // (lanes beyond the 25 rows repeat the last one and store nothing)
        for (int k = 0; k < LAT; ++k) {
            wave_sync();
            float s = HM[rw * 25 + k];
#pragma unroll 4
            for (int m = 0; m < k; ++m) s = fmaf(-HM[rw * 25 + m], HM[k * 25 + m], s);
            const float piv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), k));
            ok = ok && piv > 0.f && piv <= 3.0e38f;
            const float inv = 1.f / sqrtf(piv);
            if (lane == k) myinv = inv;
            if (lane > k && lane <= LAT) HM[lane * 25 + k] = s * inv;
        }
        wave_sync();
        float acc = lane < LAT ? HM[LAT * 25 + lane] : 0.f, dl = 0.f; // L^T delta = y: lane j reads column j of L, ends with delta_j
        for (int i = LAT - 1; i >= 0; --i) {
            const float x = acc * myinv;
            const float xi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), i));
            if (lane == i) dl = xi;
            if (lane < i) acc = fmaf(-HM[i * 25 + lane], xi, acc);
        }
        ok = uni(ok ? 1.f : 0.f) != 0.f;
        zz = ok ? z + dl : nan;
        mode = 1;
        wave_sync(); // (the solve's last reads before the pass writes the wave's block)
    }

    const bool nonfin = bad_tgt || __ballot(lane < LAT && !(fabsf(z) <= 3.0e38f)) != 0ull;
#if DP_LM_SEQ
    if (!bad_tgt) muc = mu;
    if (lane == 0) {
        long long fo = ft;
        asm volatile("" : "+v"(fo)); // (as in the epilogue)
        if (a.iters) a.iters[fo] = steps;
        if (a.n_accepted) a.n_accepted[fo] = nacc;
        if (a.mu_trace) a.mu_trace[fo] = muc;
        if (a.status) a.status[fo] = (nonfin ? DP_STATUS_NONFINITE_RESULT : 0) | (bad_tgt ? DP_STATUS_BAD_TARGETS : 0) | not_rot;
    }
    wave_sync(); // the step's closing one: the epilogue's reads of the wave's block and of the history rows before the next step's writes
    } // ---- the step loop
    // the carried state, once
    if (lane < LAT) a.z[f * LAT + lane] = zc;
    if (lane < 3) a.q.global_pos[f * 3 + lane] = lane == 0 ? gpc[0] : lane == 1 ? gpc[1] : gpc[2];
    if (lane < 4) a.q.global_rot[f * 4 + lane] = lane == 0 ? crc[0] : lane == 1 ? crc[1] : lane == 2 ? crc[2] : crc[3];
    if (lane == 0 && a.mu) a.mu[f] = muc;
#else
    if (lane == 0) {
        if (a.iters) a.iters[f] = steps;
        if (a.n_accepted) a.n_accepted[f] = nacc;
        if (a.mu && !bad_tgt) a.mu[f] = mu;
        if (a.status) a.status[f] = (nonfin ? DP_STATUS_NONFINITE_RESULT : 0) | (bad_tgt ? DP_STATUS_BAD_TARGETS : 0) | not_rot;
    }
#endif
}
#undef TGT_POS
#undef TGT_ROT
#undef BONES

