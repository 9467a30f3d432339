// dp_clip_rows_body.h -- the body of the clip solve's rows kernel, included behind the kernel's signature (its argument block is `a`, K is dpclip) with
//   DP_CLIP_SKEL 0  dp_clip_rows_kernel(K::Args): the bones are the context's, staged once per workgroup at L_OFF (dp_clip.hip)
//   DP_CLIP_SKEL 1  dp_clip_rows_skel_kernel(K::SkelArgs): the bones are those of the frame's own sequence, taken by each wave into a block of
//                   its own (dp_clip_skel.hip); everything it adds stands behind this switch, so the kernel above keeps its instructions
// What is the body's own: the sequence's word and the modes, the screening, the numbers for the decision, the results, A_t | g_t to the
// workspace.  The frame itself -- staging and BONES, a skeleton of its own, the pass's constants, the pass, the tangents with [J r]^T [J r],
// and their way into AB -- is dp_lm_frame_*.h, the text dp_lm_body.h includes too (see there); here the pass runs on `z`, once.
#define TGT_POS(jj, c) a.tgt_pos[(f * NJ + (jj)) * 3 + (c)]
#define TGT_ROT(jj, k) a.tgt_rot[(f * NJ + (jj)) * 9 + (k)]
{
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const float* __restrict__ W = a.img;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    int* par = (int*)(lds + L_PAR);
    const int* Ti = (const int*)W;
    const int mode = a.mode;

#define FRAME_SKEL DP_CLIP_SKEL
#include "dp_lm_frame_stage.h" // staging (once per workgroup): padded weight rows, sigma, the skeleton; BONES
#undef FRAME_SKEL
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
    // the skeleton of the frame's sequence: the waves of a workgroup belong to different sequences, and a component out of range refuses
    // every frame of the sequence
#define FRAME_SKEL_ROW ((long long)sq * a.skel_stride)
#include "dp_lm_frame_skel.h" // lane j: row j of that skeleton into the wave's own block; bsk
#undef FRAME_SKEL_ROW
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

#include "dp_lm_frame_consts.h" // per-lane constants of the forward pass: c0 .. muB, pj, off, sdj, muj, ct; SW

    const float z = lane < LAT ? zsrc[f * LAT + lane] : 0.f; // lane k < 24: component k of the latent this pass runs on
#define FRAME_Z z
#include "dp_lm_frame_pass.h" // decoder, kinematics, loss: q, qn, rn, R, wr, R0, d, wd, vj, P, G and lp, lr, lt
#undef FRAME_Z
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

#include "dp_lm_frame_tangents.h" // the tangents, then J two joints at a time: na, and lr16, lk
#include "dp_lm_frame_close.h" // na into AB, the latent pull
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
