// dp_cons_body.h -- the body of every kernel of the nine dp_cons*.hip units: one frame (or one sequence) per wave, optimised with Adam and
// the while-condition in one launch (dp_cons.hip's header has the phases).  Not a header in the usual sense: no include guard, it opens with
// the kernel's `{`, and a unit includes it once behind each `__global__ ... void name(Block a)` with the DP_CONS_* macros below set for that
// kernel.  It is text rather than a function the kernels call because, passed through a function, even an inlined one, the argument block is
// loaded whole at entry and the code changes (dp_cons_kernel: 78 -> 122 SGPRs, the surplus parked in VGPR lanes); included, each kernel
// reads the fields it uses where it uses them.  Every difference between two kernels is an #if on one of these macros, and a macro that is
// 0 or undefined leaves no instruction behind: a unit added with a new macro does not change the kernels of the others.  Helpers:
// dp_cons_dev.h (and hold_of, dp_cons_hold.h).
//
//   macro            1 switches                                                                      defined to 1 by (kernels)
//   DP_CONS_TABLE    the terms: a staged table of up to 16 PLANE / DISTANCE / ALIGN terms            every unit, per kernel: 0 for dp_cons_kernel,
//                    (include/dragposer_terms.h) instead of the reference's four                     dp_cons_skel_kernel, dp_cons_seq_kernel; 1 for the rest
//   DP_CONS_SKEL     the bones: each frame's own skeleton, read and screened in the prologue and     every unit but dp_cons.hip
//                    kept in the wave's block (dp_cons_skel.h) instead of L_OFF
//   DP_CONS_SEQ      a wave is a sequence: a.q.n_steps frames, each with the screening, the loop     dp_cons_seq.hip and the five units below
//                    and the results, run()'s epilogue at its `stop`; latent, global position
//                    and rotation carried in registers (dp_cons_seq.h)
//   DP_CONS_HOLD     a held term's row of the wave's block is its hold's state, updated by the       dp_cons_hold.hip (dp_terms_hold_seq_kernel) and the four
//                    epilogue (dp_cons_hold.h, include/dragposer_holds.h)                            units below
//   DP_CONS_AR       a step's z_tgt row is formed from the sequence's last history rows, kept in     dp_cons_ar.hip (dp_terms_ar_seq_kernel); the second kernel
//                    a second LDS array (dp_cons_ar.h, include/dragposer_latent_ar.h)                of dp_cons_gap.hip, dp_cons_live.hip, dp_cons_tether.hip
//   DP_CONS_GAP      `trk` is the lane's code of the step, decided from the joint's row of           dp_cons_gap.hip (dp_terms_gap_seq_kernel, dp_terms_gap_ar_seq_kernel),
//                    dp_gaps.state in global memory (dp_cons_gap.h, include/dragposer_gaps.h)        dp_cons_live.hip, dp_cons_tether.hip
//   DP_CONS_LIVE     the launch is one step and the wave appends its row to the three history        dp_cons_live.hip (dp_live_kernel, dp_live_ar_kernel)
//                    buffers itself (dp_cons_live.h, include/dragposer_live.h)
//   DP_CONS_TETHER   a tethered term's row is its tether's, rewritten at each `stop` from the        dp_cons_tether.hip (dp_terms_tether_seq_kernel,
//                    joint's new world position (dp_cons_tether.h, include/dragposer_tethers.h)      dp_terms_tether_ar_seq_kernel)
//   DP_CONS_POINTS   a PLANE or DISTANCE term's index 22 + k is point k, sum_j m_k[j] P_j: formed      dp_cons_points.hip (dp_terms_points_kernel,
//                    per iteration into the wave's block, the selectors `j == ja` replaced by the    dp_terms_points_skel_kernel, dp_terms_points_seq_kernel)
//                    lane's coefficient (dp_cons_points.h, include/dragposer_points.h)
{
    constexpr bool TBL = DP_CONS_TABLE;
#if DP_CONS_POINTS // (the table layouts with the points' area behind each wave's block and the coefficients behind the last: dp_cons_points.h)
    constexpr int N_LDS = DP_CONS_SKEL ? PT_SK_LDS_FLOATS : PT_LDS_FLOATS, W_STRIDE = DP_CONS_SKEL ? PT_SK_W_STRIDE : PT_W_STRIDE;
    constexpr int W_PT = DP_CONS_SKEL ? PT_SK_W_PT : PT_W_PT, L_COEF = DP_CONS_SKEL ? PT_SK_L_COEF : PT_L_COEF;
#if DP_CONS_SKEL
    constexpr int W_SK = W_SKEL_T;
#endif
#elif DP_CONS_SKEL
    constexpr int N_LDS = TBL ? SK_LDS_FLOATS_T : SK_LDS_FLOATS, W_STRIDE = TBL ? SK_W_FLOATS_T : SK_W_FLOATS;
    constexpr int W_SK = TBL ? W_SKEL_T : W_SKEL;
#else
    constexpr int N_LDS = TBL ? LDS_FLOATS_T : LDS_FLOATS, W_STRIDE = TBL ? W_FLOATS_T : W_FLOATS;
#endif
    __shared__ __attribute__((aligned(16))) float lds[N_LDS];
#if DP_CONS_AR
    __shared__ float arh[WPB * AR_W_FLOATS];
#endif
#if DP_CONS_TETHER && !DP_TETHER_WPREV_GLOBAL
    __shared__ float twp[WPB * TETHER_W_FLOATS];
#endif
    const float* __restrict__ W = a.img;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int* par = (int*)(lds + L_PAR);
    unsigned* sub = (unsigned*)(lds + L_SUB);
    const int* cst = (const int*)(lds + L_CST);
    const int* cls = (const int*)(lds + L_CLS);
    const int* Ti = (const int*)W;

    // ---- staging (once per workgroup): padded weight rows, skeleton tables, subtree masks
    for (int i = tid; i < H0 * LAT; i += WPB * 64) lds[L_A0 + (i / LAT) * S0 + i % LAT] = W[dpvjp::OFF_A0 + i];
    for (int i = tid; i < H1 * H0; i += WPB * 64) lds[L_A1 + (i / H0) * S1 + i % H0] = W[dpvjp::OFF_A1 + i];
    for (int i = tid; i < dpvjp::NY * H1; i += WPB * 64) lds[L_A2 + (i / H1) * S2 + i % H1] = W[dpvjp::OFF_A2 + i];
    if (tid < NJ) par[tid] = Ti[dpvjp::OFF_PARENT + tid];
    if (tid < NJ + 1) ((int*)(lds + L_CST))[tid] = Ti[dpvjp::OFF_CSTART + tid];
    if (tid < NJ) ((int*)(lds + L_CLS))[tid] = Ti[dpvjp::OFF_CLIST + tid];
#if !DP_CONS_SKEL
    if (tid < 3 * NJ) lds[L_OFF + tid] = W[dpvjp::OFF_BONE + tid];
#endif
#if DP_CONS_TABLE
    for (int i = tid; i < a.n_terms * TW; i += WPB * 64) ((unsigned*)lds)[L_TBL + i] = a.tbl[i];
#endif
#if DP_CONS_POINTS // (every row: a row beyond n_points is zero and no term names it)
    if (tid < PT_COEF_FLOATS) lds[L_COEF + tid] = a.pt.coeff[tid];
#endif
    __syncthreads();
    if (tid < NJ) { // ancestors of tid (itself included), parked in sub[] for the moment
        unsigned anc = 1u << tid;
        int c = tid;
        for (int s = 0; s < NJ && c != 0; ++s) { c = par[c]; anc |= 1u << c; } // (parents[j] < j: dp_create's check)
        sub[tid] = anc;
    }
    __syncthreads();
    unsigned mysub = 0u;
    if (tid < NJ)
        for (int d = 0; d < NJ; ++d) mysub |= ((sub[d] >> tid) & 1u) << d;
    __syncthreads();
    if (tid < NJ) sub[tid] = mysub;
    __syncthreads();

    const long long f = (long long)blockIdx.x * WPB + wv;
    if (f >= a.n_frames) return;
    float* wb = lds + (TBL ? L_WAVE0_T : L_WAVE0) + wv * W_STRIDE;
    float *ZB = wb + W_Z, *HB0 = wb + W_H0, *HB1 = wb + W_H1, *QB = wb + W_Q, *DYB = wb + W_DY, *RB = wb + W_R, *BB = wb + W_B,
          *PB = wb + W_P, *GB = wb + W_G, *GPB = wb + W_GP, *FB = wb + W_F;
    const float nan = __builtin_nanf("");
    const int j = lane; // joint of this lane (j < NJ)
    const bool jl = lane < NJ;

    // ---- screening (include/dragposer.h: DP_STATUS_*)
#if !DP_CONS_SEQ // (a sequence: per step, below the skeleton)
    float cr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cr[k] = a.cur_rot[f * 4 + k];
    float gp[3] = {0.f, 0.f, 0.f};
    if (reads_gp(a))
#pragma unroll
        for (int k = 0; k < 3; ++k) gp[k] = a.global_pos[f * 3 + k];
    const float z0 = lane < LAT ? a.z0[f * LAT + lane] : 0.f;
    const float zt = lane < LAT ? a.z_tgt[f * LAT + lane] : 0.f;
#endif
    const bool trk = jl && a.tracked[f * NJ + j] != 0;
#if DP_CONS_SKEL
    // lane j: row j of this frame's skeleton (stride 0: the launch's one) -- its bone for the whole loop, and into the wave's block for the
    // parents' child-bone loop.  Row 0 is never read.  A component out of range refuses the frame (dp_optimize_skeleton's rule).
    float off[3] = {0.f, 0.f, 0.f};
    bool bsk = false;
    if (jl && j != 0) {
        const float* __restrict__ sk = a.skel + f * (long long)a.skel_stride; // (64-bit: beyond 2^31 / 66 frames a 32-bit product wraps)
#pragma unroll
        for (int c = 0; c < 3; ++c) { off[c] = sk[3 * j + c]; bsk = bsk || refused(off[c]); }
    }
    if (jl)
#pragma unroll
        for (int c = 0; c < 3; ++c) wb[W_SK + 3 * j + c] = off[c];
#endif
#if DP_CONS_SEQ
    // what the sequence carries from step to step: the latent (lane k: component k), the global rotation and position (every lane)
    float zc = lane < LAT ? a.z0[f * LAT + lane] : 0.f, crc[4], gpc[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) crc[k] = a.cur_rot[f * 4 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) gpc[k] = a.q.global_pos[f * 3 + k]; // (the state's array, never NULL; Args::global_pos is NULL when no term reads it)
    const int NS = a.n_frames, NH = a.q.n_heights;
#if DP_CONS_HOLD // lane t, term t held and active: its row of the wave's block is the hold's state from here to the end of the launch
    if (lane < a.n_terms) {
        const int hd = hold_of(a.h.n_holds, a.h.terms, lane);
        if (hd >= 0 && lds[L_TBL + lane * TW + T_W] != 0.f)
#pragma unroll
            for (int c = 0; c < 4; ++c) wb[W_ROW + 4 * lane + c] = a.h.state[(f * a.h.n_holds + hd) * 4 + c];
    }
#endif
#if DP_CONS_TETHER // lane t, term t tethered and active: likewise its tether's row; the joint's last world position into the wave's area of twp
    if (lane < a.n_terms) {
        const int tk = hold_of(a.t.n_tethers, a.t.terms, lane);
        if (tk >= 0 && lds[L_TBL + lane * TW + T_W] != 0.f) {
            const float* const srow = a.t.state + (f * a.t.n_tethers + tk) * TETHER_ROW;
#pragma unroll
            for (int c = 0; c < 4; ++c) wb[W_ROW + 4 * lane + c] = srow[c];
#if !DP_TETHER_WPREV_GLOBAL
#pragma unroll
            for (int c = 0; c < 4; ++c) twp[wv * TETHER_W_FLOATS + 4 * tk + c] = srow[4 + c];
#endif
        }
    }
#endif
#if DP_CONS_AR // lane i: column i of the sequence's last `order` history rows, the newest (h_1) first
    float* const hb = arh + wv * AR_W_FLOATS;
    if (lane < LAT)
#pragma unroll
        for (int k = 0; k < MAX_AR_ORDER; ++k)
            if (k < a.r.order) hb[k * LAT + lane] = a.r.latent_buf[(f * a.r.history + (a.r.history - 1 - k)) * LAT + lane];
    wave_sync();
#endif
#if DP_CONS_LIVE // lane c < 27 + NH: column c of the row the step writes to hist_scratch -- NaN from a step refused as bad state
    float hnew = nan;
#endif
    for (int stp = 0; stp < a.q.n_steps; ++stp) { // ---- the step loop: frame stp of this sequence, row ft of every per-step array
    const long long ft = (long long)stp * NS + f;
    float cr[4] = {crc[0], crc[1], crc[2], crc[3]};
    float gp[3] = {0.f, 0.f, 0.f}; // (what the terms read and the screening sees: as in a per-frame launch, only when a term needs it)
    if (reads_gp(a))
#pragma unroll
        for (int k = 0; k < 3; ++k) gp[k] = gpc[k];
    const float z0 = zc;
#if DP_CONS_AR // include/dragposer_latent_ar.h, "The predictor": lane i forms component i, unfused, in the stated order
    float zt = 0.f;
    if (lane < LAT) {
        zt = a.r.bias[lane];
        for (int k = 0; k < a.r.order; ++k) {
            const float* __restrict__ Ak = a.r.coeffs + (k * LAT + lane) * LAT;
#pragma unroll
            for (int c = 0; c < LAT; ++c) zt = __fadd_rn(zt, __fmul_rn(Ak[c], hb[k * LAT + c]));
        }
    }
#else
    const float zt = lane < LAT ? a.z_tgt[(long long)stp * a.q.z_tgt_step + f * a.q.z_tgt_seq + lane] : 0.f;
#endif
    float sh[3] = {0.f, 0.f, 0.f}; // this step's target shift: tgt_root[stp] - the global position before the step
    if (a.q.tgt_root)
#pragma unroll
        for (int k = 0; k < 3; ++k) sh[k] = a.q.tgt_root[ft * 3 + k] - gpc[k];
    float tpe[3] = {0.f, 0.f, 0.f}; // lane j: joint j's effective position target of this step
#if DP_CONS_GAP // (a sample marked absent is not read)
    const bool smp = trk && !(a.g.present && a.g.present[ft * NJ + j] == 0);
    if (smp)
#else
    if (trk)
#endif
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float tk = a.tgt_pos[(ft * NJ + j) * 3 + k];
            tpe[k] = a.q.tgt_root ? tk + sh[k] : tk;
        }
#endif
    bool bs = refused(z0) || refused(cr[0]) || refused(cr[1]) || refused(cr[2]) || refused(cr[3]) || refused(gp[0]) || refused(gp[1]) ||
              refused(gp[2]);
#if DP_CONS_SKEL
    bs = bs || bsk;
#endif
#if DP_CONS_GAP
    // include/dragposer_gaps.h, "The rule": lane j decides joint j's code of this step and advances its row of the state, unless the step is
    // refused as bad state (which leaves the state as it is).  From here to the end of the step `trk` is the step's: code 1 or 2.
    const bool cfg = trk;
    float* const grow = a.g.state + (f * NJ + j) * GAP_ROW; // (dereferenced by lanes with cfg only: j < NJ)
    int code = 0;
    const bool gbad = __ballot(bs) != 0ull;
    if (cfg && !gbad) {
        bool absent = !smp;
        if (smp) {
#pragma unroll
            for (int k = 0; k < 3; ++k) absent = absent || refused(tpe[k]);
#pragma unroll
            for (int k = 0; k < 9; ++k) absent = absent || refused(a.tgt_rot[(ft * NJ + j) * 9 + k]);
        }
        if (!absent) {
            code = GAP_PRESENT;
#pragma unroll
            for (int k = 0; k < 3; ++k) grow[G_P + k] = __fadd_rn(tpe[k], gpc[k]);
#pragma unroll
            for (int k = 0; k < 9; ++k) grow[G_R + k] = a.tgt_rot[(ft * NJ + j) * 9 + k];
            grow[G_VALID] = 1.f; grow[G_AGE] = 0.f; grow[G_FACTOR] = 1.f;
        } else {
            const float age = __fadd_rn(grow[G_AGE], 1.f);
            if (grow[G_VALID] != 0.f && age <= a.g.max_hold) {
                code = GAP_HELD;
                grow[G_AGE] = age;
                grow[G_FACTOR] = __fmul_rn(grow[G_FACTOR], a.g.decay);
#pragma unroll
                for (int k = 0; k < 3; ++k) tpe[k] = __fsub_rn(grow[G_P + k], gpc[k]);
            } else {
                code = GAP_LOST;
                grow[G_VALID] = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) tpe[k] = 0.f;
            }
        }
    }
    if (jl && a.g.trace) a.g.trace[ft * NJ + j] = gbad ? 0xFF : (unsigned char)code; // (0: not tracked by configuration)
    const bool trk = code == GAP_PRESENT || code == GAP_HELD;
    const int gbits = (__ballot(code == GAP_HELD) != 0ull ? DP_STATUS_TRACKER_HELD : 0) | (__ballot(code == GAP_LOST) != 0ull ? DP_STATUS_TRACKER_LOST : 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the row's stores have left before the iteration loop reads the row
#endif
    bool bt = refused(zt);
    if (trk) {
#pragma unroll
#if DP_CONS_GAP // (the effective targets and weights: what the per-frame composition hands dp_optimize_terms)
        for (int k = 0; k < 3; ++k) bt = bt || refused(tpe[k]);
#pragma unroll
        for (int k = 0; k < 9; ++k) bt = bt || refused(grow[G_R + k]);
#elif DP_CONS_SEQ
        for (int k = 0; k < 3; ++k) bt = bt || refused(tpe[k]);
#pragma unroll
        for (int k = 0; k < 9; ++k) bt = bt || refused(a.tgt_rot[(ft * NJ + j) * 9 + k]);
#else
        for (int k = 0; k < 3; ++k) bt = bt || refused(a.tgt_pos[(f * NJ + j) * 3 + k]);
#pragma unroll
        for (int k = 0; k < 9; ++k) bt = bt || refused(a.tgt_rot[(f * NJ + j) * 9 + k]);
#endif
#if DP_CONS_GAP
        bt = bt || refused(__fmul_rn(a.w[(f * NJ + j) * 2], grow[G_FACTOR])) || refused(__fmul_rn(a.w[(f * NJ + j) * 2 + 1], grow[G_FACTOR]));
#else
        bt = bt || refused(a.w[(f * NJ + j) * 2]) || refused(a.w[(f * NJ + j) * 2 + 1]);
#endif
    }
#if DP_CONS_TABLE
    if (lane < a.n_terms) { // lane t: term t's row of this frame (the term's own vector and s_f = 1 without one) into the wave's block
        const float* tb = lds + L_TBL + lane * TW;
        const int type = __float_as_int(tb[T_TYPE]);
        const float* pf = *(const float* const*)(tb + T_ROW);
        float r[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = type == DP_TERM_ALIGN ? tb[T_DIR + c] : tb[T_PT + c];
        r[3] = 1.f;
        if (pf && tb[T_W] != 0.f) {
#pragma unroll
#if DP_CONS_SEQ // (the term's rows of this step: T_STEP floats further per step, 0 = one row held)
            for (int c = 0; c < 4; ++c) r[c] = pf[(long long)stp * __float_as_int(tb[T_STEP]) + f * 4 + c];
#else
            for (int c = 0; c < 4; ++c) r[c] = pf[f * 4 + c];
#endif
            bt = bt || refused(r[0]) || refused(r[1]) || refused(r[2]) || refused(r[3]) || r[3] < 0.f;
        }
#if DP_CONS_HOLD // (a held term has no per_frame array: its row is the state as the step before left it, screened as a per_frame row)
        if (tb[T_W] != 0.f && hold_of(a.h.n_holds, a.h.terms, lane) >= 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = wb[W_ROW + 4 * lane + c];
            bt = bt || refused(r[0]) || refused(r[1]) || refused(r[2]) || refused(r[3]) || r[3] < 0.f;
        }
#endif
#if DP_CONS_TETHER // (a tethered term likewise: its row is the tether's as the step before left it, screened as a per_frame row)
        if (tb[T_W] != 0.f && hold_of(a.t.n_tethers, a.t.terms, lane) >= 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = wb[W_ROW + 4 * lane + c];
            bt = bt || refused(r[0]) || refused(r[1]) || refused(r[2]) || refused(r[3]) || r[3] < 0.f;
        }
#endif
#pragma unroll
        for (int c = 0; c < 4; ++c) wb[W_ROW + 4 * lane + c] = r[c];
    }
#endif
    const bool bad_state = __ballot(bs) != 0ull;
    const bool bad_tgt = !bad_state && __ballot(bt) != 0ull;
#if DP_CONS_GAP // (a step without a tracker: max(E, 1), both tracker losses exactly 0, the pull and the table's terms act alone)
    const int En = __popcll(__ballot(trk));
    const int E = En > 0 ? En : 1;
#else
    const int E = __popcll(__ballot(trk));
#endif
#if DP_CONS_SEQ
    if (bad_state) { // this step's results NaN and, as the per-frame epilogue makes them from such a frame, the carried state: every later step too
        float* const o = a.q.hist + ft * (LAT + 3 + NH);
        if (lane < LAT + 3 + NH) o[lane] = nan;
        if (jl) {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (a.pose) a.pose[ft * 88 + 4 * j + c] = nan;
#pragma unroll
            for (int c = 0; c < 3; ++c) if (a.pos) a.pos[(ft * NJ + j) * 3 + c] = nan;
        }
        if (lane < 4) {
            if (a.world_rot) a.world_rot[ft * 4 + lane] = nan;
#if !DP_CONS_TABLE
            if (a.loss_extra) a.loss_extra[ft * 4 + lane] = nan;
#endif
        }
#if DP_CONS_TABLE
        if (lane < a.n_terms && a.loss_terms) a.loss_terms[ft * a.n_terms + lane] = nan;
#endif
#if DP_CONS_HOLD // (the hold's state stays as it is: the trace repeats it)
        if (lane < a.n_terms && a.h.trace) {
            const int hd = hold_of(a.h.n_holds, a.h.terms, lane);
            if (hd >= 0 && lds[L_TBL + lane * TW + T_W] != 0.f)
#pragma unroll
                for (int c = 0; c < 4; ++c) a.h.trace[(ft * a.h.n_holds + hd) * 4 + c] = wb[W_ROW + 4 * lane + c];
        }
#endif
#if DP_CONS_TETHER // (the tether's state stays as it is: the trace repeats it)
        if (lane < a.n_terms && a.t.trace) {
            const int tk = hold_of(a.t.n_tethers, a.t.terms, lane);
            if (tk >= 0 && lds[L_TBL + lane * TW + T_W] != 0.f) {
                float* const trow = a.t.trace + (ft * a.t.n_tethers + tk) * TETHER_ROW;
#if DP_TETHER_WPREV_GLOBAL
                const float* const wpv = a.t.state + (f * a.t.n_tethers + tk) * TETHER_ROW + 4;
#else
                const float* const wpv = twp + wv * TETHER_W_FLOATS + 4 * tk;
#endif
#pragma unroll
                for (int c = 0; c < 4; ++c) { trow[c] = wb[W_ROW + 4 * lane + c]; trow[4 + c] = wpv[c]; }
            }
        }
#endif
#if DP_CONS_AR // (the history stays as it is; the step used no target)
        if (lane < LAT && a.r.trace) a.r.trace[ft * LAT + lane] = nan;
#endif
        if (lane < 3) {
            if (a.q.pos_ret) a.q.pos_ret[ft * 3 + lane] = nan;
            if (a.loss) a.loss[ft * 3 + lane] = nan;
        }
        if (lane == 0) {
            if (a.iters) a.iters[ft] = a.early_stop ? 1 : a.n_iter;
            if (a.status) a.status[ft] = DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE;
        }
        zc = nan;
#pragma unroll
        for (int k = 0; k < 4; ++k) crc[k] = nan;
#pragma unroll
        for (int k = 0; k < 3; ++k) gpc[k] = nan;
        continue;
    }
#else
    if (bad_state) { // every result NaN (the reference's latent is NaN from here on); the reference's loop ends after one pass
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
        if (lane < 4) {
            if (a.world_rot) a.world_rot[f * 4 + lane] = nan;
#if !DP_CONS_TABLE
            if (a.loss_extra) a.loss_extra[f * 4 + lane] = nan;
#endif
        }
#if DP_CONS_TABLE
        if (lane < a.n_terms && a.loss_terms) a.loss_terms[f * a.n_terms + lane] = nan;
#endif
        if (lane < 3) {
            if (a.disp) a.disp[f * 3 + lane] = nan;
            if (a.world_disp) a.world_disp[f * 3 + lane] = nan;
            if (a.loss) a.loss[f * 3 + lane] = nan;
        }
        if (lane == 0) {
            if (a.iters) a.iters[f] = a.early_stop ? 1 : a.n_iter;
            if (a.status) a.status[f] = DP_STATUS_NONFINITE_RESULT | DP_STATUS_BAD_STATE;
        }
        return;
    }
#endif

#if DP_CONS_AR
    if (lane < LAT && a.r.trace) a.r.trace[ft * LAT + lane] = zt;
#endif
    // per-lane constants of the frame loop
    const float c0 = lane < H0 ? W[dpvjp::OFF_C0 + lane] : 0.f;
    const float b1 = lane < H1 ? W[dpvjp::OFF_B1 + lane] : 0.f;
    const int oB = 64 + lane; // second decoder row of lanes 0..26
    const float b2A = W[dpvjp::OFF_B2 + lane], sdA = W[dpvjp::OFF_SD + lane], muA = W[dpvjp::OFF_MU + lane];
    const float b2B = lane < NYU - 64 ? W[dpvjp::OFF_B2 + oB] : 0.f, sdB = lane < NYU - 64 ? W[dpvjp::OFF_SD + oB] : 1.f,
                muB = lane < NYU - 64 ? W[dpvjp::OFF_MU + oB] : 0.f;
    const int pj = jl ? par[j] : 0;
    const unsigned mysubj = jl ? sub[j] : 0u;
#if !DP_CONS_SKEL
    float off[3] = {0.f, 0.f, 0.f};
#endif
    float sdj[4] = {1.f, 1.f, 1.f, 1.f}, muj[4] = {0.f, 0.f, 0.f, 0.f};
    if (jl) {
#if !DP_CONS_SKEL
#pragma unroll
        for (int c = 0; c < 3; ++c) off[c] = lds[L_OFF + 3 * j + c];
#endif
#pragma unroll
        for (int c = 0; c < 4; ++c) { sdj[c] = W[dpvjp::OFF_SD + 4 * j + c]; muj[c] = W[dpvjp::OFF_MU + 4 * j + c]; }
    }
    const float cp = 2.f / (3.f * (float)E), crt = 2.f * a.lam_rot / (9.f * (float)E);
    const int up = a.up;

    float z = z0, m = 0.f, v = 0.f;
    if (lane < LAT) ZB[lane] = z;
    double b1t = 1.0, b2t = 1.0;
    float prev = 10000000.f;
    int it = 0;
    const int n_iter = bad_tgt ? 1 : a.n_iter; // (a refused target: the loss is NaN, the reference's loop ends after one pass)
    for (;; ++it) {
        wave_sync();
        // ---- decoder (autoencoder.py:224-256, folded), LeakyReLU(0.2) after layers 0 and 1
        bool pos0 = false, pos1 = false;
        if (lane < H0) {
            float s = c0;
#pragma unroll UNR
            for (int k = 0; k < LAT; ++k) s = fmaf(lds[L_A0 + lane * S0 + k], ZB[k], s);
            pos0 = s > 0.f;
            HB0[lane] = pos0 ? s : s * 0.2f;
        }
        wave_sync();
        if (lane < H1) {
            float s = b1;
#pragma unroll UNR
            for (int k = 0; k < H0; ++k) s = fmaf(lds[L_A1 + lane * S1 + k], HB0[k], s);
            pos1 = s > 0.f;
            HB1[lane] = pos1 ? s : s * 0.2f;
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
            for (int c = 0; c < 3; ++c) PB[4 * j + c] = P[c];
#pragma unroll
            for (int k = 0; k < 9; ++k) GB[9 * j + k] = G[k];
        }
        wave_sync();
#if DP_CONS_POINTS
        // the points' positions: lane 4k + c forms component c of P_(22+k) = sum_j m_k[j] P_j, one fmaf per joint in joint order from 0, so
        // that a unit point's sum is its joint's position exactly (0 + 0 P_i = 0, 0 + 1 P_j = P_j, P_j + 0 P_i = P_j)
        if (a.pt.n_points > 0) {
            if (lane < 4 * a.pt.n_points && (lane & 3) != 3) {
                const float* mk = lds + L_COEF + (lane >> 2) * PT_NJ;
                float s = 0.f;
#pragma unroll UNR
                for (int i = 0; i < NJ; ++i) s = fmaf(mk[i], PB[4 * i + (lane & 3)], s);
                wb[W_PT + lane] = s;
            }
            wave_sync();
        }
#endif

        // ---- losses and upstream gradients (drag_pose.py:115-127 and the Additional Losses block, 129-183)
        float dpj = 0.f, drj = 0.f, gPj[3] = {0.f, 0.f, 0.f}, gGj[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) gGj[k] = 0.f;
        if (trk) { // (targets re-read every iteration: not held in registers)
#if DP_CONS_GAP // (the row's factor: 1 for a present sample, and w * 1 is w)
            const float wp = __fmul_rn(a.w[(f * NJ + j) * 2], grow[G_FACTOR]), wrr = __fmul_rn(a.w[(f * NJ + j) * 2 + 1], grow[G_FACTOR]);
#else
            const float wp = a.w[(f * NJ + j) * 2], wrr = a.w[(f * NJ + j) * 2 + 1];
#endif
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#if DP_CONS_SEQ
                const float e = P[c] - tpe[c];
#else
                const float e = P[c] - a.tgt_pos[(f * NJ + j) * 3 + c];
#endif
                dpj = fmaf(e, e, dpj);
                gPj[c] = cp * wp * e;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
#if DP_CONS_GAP // (the row's rotation: the sample's own when present, the held one otherwise)
                const float e = G[k] - grow[G_R + k];
#elif DP_CONS_SEQ
                const float e = G[k] - a.tgt_rot[(ft * NJ + j) * 9 + k];
#else
                const float e = G[k] - a.tgt_rot[(f * NJ + j) * 9 + k];
#endif
                drj = fmaf(e, e, drj);
                gGj[k] = crt * wrr * e;
            }
            dpj *= wp;
            drj *= wrr;
        }
        const float dz = z - zt;
        const float dtj = lane < LAT ? dz * dz : 0.f;
        // the constraint terms: every lane evaluates them on the same LDS values; a joint's lane keeps its own gradient
        float ext[4] = {0.f, 0.f, 0.f, 0.f}; // weighted: feet_floor, head_hips_forward, head_hips_colinear, hips_feet_colinear
        float extra = 0.f, mine = 0.f;     // (table: the terms' sum in table order; lane t keeps term t's weighted value)
#if !DP_CONS_TABLE
        if (a.w_floor != 0.f) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int fj = a.floor_j[i];
                const float h = comp(gp, up) + (PB[4 * fj + up] - a.floor_level);
                float g;
                if (a.one_sided) {
                    const float r = h < 0.f ? -h : 0.f; // relu(floor_level - g_up - P_up)
                    t = fmaf(r, r, t);
                    g = -r;
                } else {
                    t = fmaf(h, h, t);
                    g = h;
                }
                if (j == fj) // d/dP_up of w * mean_i (.)^2 over the two joints
#pragma unroll
                    for (int c = 0; c < 3; ++c) gPj[c] += c == up ? a.w_floor * g : 0.f;
            }
            ext[0] = a.w_floor * (0.5f * t);
        }
        if (a.w_fwd != 0.f) {
            float av[3], bv[3];
            mv(GB + 9 * a.head, a.fwd, av);
            flatten(av, up);
            const float na = sqrtf(av[0] * av[0] + av[1] * av[1] + av[2] * av[2]);
            if (na > a.fwd_thr) {
                mv(GB + 9 * a.hips, a.fwd, bv);
                flatten(bv, up);
                const float nb = sqrtf(bv[0] * bv[0] + bv[1] * bv[1] + bv[2] * bv[2]);
                float ah[3], bh[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { ah[c] = av[c] / na; bh[c] = bv[c] / nb; }
                const float cs = ah[0] * bh[0] + ah[1] * bh[1] + ah[2] * bh[2];
                const float s = cs + a.fwd_margin;
                if (s < 1.f) {
                    const float u = 1.f - s;
                    ext[1] = a.w_fwd * (u * u);
                    const float ds = -2.f * u * a.w_fwd;
                    if (j == a.head || j == a.hips) {
                        float da[3]; // d s / d(projected axis) of this joint
#pragma unroll
                        for (int c = 0; c < 3; ++c) da[c] = j == a.head ? (bh[c] - ah[c] * cs) / na : (ah[c] - bh[c] * cs) / nb;
                        if (a.head == a.hips)
#pragma unroll
                            for (int c = 0; c < 3; ++c) da[c] = (bh[c] - ah[c] * cs) / na + (ah[c] - bh[c] * cs) / nb;
                        flatten(da, up);
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int c = 0; c < 3; ++c) gGj[3 * r + c] += ds * da[r] * a.fwd[c];
                    }
                }
            }
        }
        if (a.w_hcol != 0.f) {
            float u[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c] = PB[4 * a.head + c] - PB[4 * a.hips + c];
            flatten(u, up);
            ext[2] = a.w_hcol * (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
            const float sgn = (j == a.head ? 1.f : 0.f) - (j == a.hips ? 1.f : 0.f);
#pragma unroll
            for (int c = 0; c < 3; ++c) gPj[c] += sgn * 2.f * a.w_hcol * u[c];
        }
        if (a.w_feet != 0.f) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int fj = a.foot_j[i];
                float u[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) u[c] = PB[4 * a.hips + c] - PB[4 * fj + c];
                flatten(u, up);
                const float x = (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - a.feet_r2;
                if (x > 0.f) {
                    t += x;
                    const float sgn = (j == a.hips ? 1.f : 0.f) - (j == fj ? 1.f : 0.f);
#pragma unroll
                    for (int c = 0; c < 3; ++c) gPj[c] += sgn * 2.f * a.w_feet * u[c];
                }
            }
            ext[3] = a.w_feet * t;
        }
#else
        {
            float* const RW = wb + W_ROW;
            for (int t = 0; t < a.n_terms; ++t) {
                const float* tb = lds + L_TBL + t * TW;
                const int* ti = (const int*)tb;
                const float ws = uni(tb[T_W] * RW[4 * t + 3]); // weight * s_f
                if (ws == 0.f) continue;
                const int type = uni_i(ti[T_TYPE]), ja = uni_i(ti[T_JA]), jb = uni_i(ti[T_JB]), fl = uni_i(ti[T_FLAGS]);
                const bool drop = (fl & DP_TERM_DROP_UP) != 0;
                float val = 0.f;
#if DP_CONS_POINTS
                // An index below 22 is a joint, 22 + k is point k: its position row (the format of W_P's) and this lane's coefficient of it --
                // 1 or 0 for a joint, the other kernels' `j == ja`; m_k[j] for a point, lane j reading word j of row k.  Wave-uniform bases.
                // (ALIGN never names a point: the host refuses it.)
                const float* const PA = ja < NJ ? PB + 4 * ja : wb + W_PT + 4 * (ja - NJ);
                const float* const PBb = jb < NJ ? PB + 4 * (jb < 0 ? 0 : jb) : wb + W_PT + 4 * (jb - NJ);
                const float ca = ja < NJ ? (j == ja ? 1.f : 0.f) : (jl ? lds[L_COEF + (ja - NJ) * PT_NJ + j] : 0.f);
                const float cb = jb < NJ ? (j == jb ? 1.f : 0.f) : (jl ? lds[L_COEF + (jb - NJ) * PT_NJ + j] : 0.f);
#endif
                if (type == DP_TERM_PLANE) { // d = dir . (g + P_a - point)
                    float dd = 0.f;
#pragma unroll
#if DP_CONS_POINTS
                    for (int c = 0; c < 3; ++c) dd = fmaf(tb[T_DIR + c], (gp[c] + PA[c]) - RW[4 * t + c], dd);
#else
                    for (int c = 0; c < 3; ++c) dd = fmaf(tb[T_DIR + c], (gp[c] + PB[4 * ja + c]) - RW[4 * t + c], dd);
#endif
                    float g = dd;
                    if (fl & DP_TERM_ONE_SIDED) g = dd < 0.f ? dd : 0.f; // -relu(-d)
                    val = ws * (g * g);
#if DP_CONS_POINTS // (the factor times the coefficient: at 1 the factor itself, and the fmaf is the joint's)
                    if (ca != 0.f) {
                        const float gf = 2.f * ws * g;
#pragma unroll
                        for (int c = 0; c < 3; ++c) gPj[c] = fmaf(__fmul_rn(ca, gf), tb[T_DIR + c], gPj[c]);
                    }
#else
                    if (j == ja)
#pragma unroll
                        for (int c = 0; c < 3; ++c) gPj[c] = fmaf(2.f * ws * g, tb[T_DIR + c], gPj[c]);
#endif
                } else if (type == DP_TERM_DISTANCE) { // q = |h(P_a - P_b)|^2 or |h(g + P_a - point)|^2
                    float u[3];
                    if (jb >= 0) {
#pragma unroll
#if DP_CONS_POINTS
                        for (int c = 0; c < 3; ++c) u[c] = PA[c] - PBb[c];
#else
                        for (int c = 0; c < 3; ++c) u[c] = PB[4 * ja + c] - PB[4 * jb + c];
#endif
                    } else {
#pragma unroll
#if DP_CONS_POINTS
                        for (int c = 0; c < 3; ++c) u[c] = (gp[c] + PA[c]) - RW[4 * t + c];
#else
                        for (int c = 0; c < 3; ++c) u[c] = (gp[c] + PB[4 * ja + c]) - RW[4 * t + c];
#endif
                    }
                    if (drop) flatten(u, up);
                    const float q = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
                    const float xh = q - tb[T_P1], xl = tb[T_P0] - q; // (p0, p1 staged as lo^2, hi^2)
                    const float dq = (xh > 0.f ? ws : 0.f) - (xl > 0.f ? ws : 0.f);
                    val = ws * ((xh > 0.f ? xh : 0.f) + (xl > 0.f ? xl : 0.f));
#if DP_CONS_POINTS // (1 - 0, 0 - 1, 0 - 0 and 1 - 1 for two joints, as below; the same point twice: m - m = 0)
                    const float sgn = ca - cb;
#else
                    const float sgn = (j == ja ? 1.f : 0.f) - (j == jb ? 1.f : 0.f);
#endif
#pragma unroll
                    for (int c = 0; c < 3; ++c) gPj[c] += sgn * 2.f * dq * u[c];
                } else { // DP_TERM_ALIGN: u = h(G_a axis_a), v = h(G_b axis_b) or h(dir)
                    float av[3], bv[3], xa[3], xb[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { xa[c] = tb[T_AXA + c]; xb[c] = tb[T_AXB + c]; }
                    mv(GB + 9 * ja, xa, av);
                    if (drop) flatten(av, up);
                    const float na = sqrtf(av[0] * av[0] + av[1] * av[1] + av[2] * av[2]);
                    if (na > tb[T_P0]) {
                        if (jb >= 0) mv(GB + 9 * jb, xb, bv);
                        else
#pragma unroll
                            for (int c = 0; c < 3; ++c) bv[c] = RW[4 * t + c];
                        if (drop) flatten(bv, up);
                        const float nb = sqrtf(bv[0] * bv[0] + bv[1] * bv[1] + bv[2] * bv[2]);
                        float ah[3], bh[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) { ah[c] = av[c] / na; bh[c] = bv[c] / nb; }
                        const float cs = ah[0] * bh[0] + ah[1] * bh[1] + ah[2] * bh[2];
                        const float sc = cs + tb[T_P1];
                        if (sc < 1.f) {
                            const float w1 = 1.f - sc;
                            val = ws * (w1 * w1);
                            const float ds = -2.f * w1 * ws;
                            if (j == ja) { // d c / d u, through the projection, times the local axis
                                float da[3];
#pragma unroll
                                for (int c = 0; c < 3; ++c) da[c] = (bh[c] - ah[c] * cs) / na;
                                if (drop) flatten(da, up);
#pragma unroll
                                for (int r = 0; r < 3; ++r)
#pragma unroll
                                    for (int c = 0; c < 3; ++c) gGj[3 * r + c] += ds * da[r] * xa[c];
                            }
                            if (j == jb) {
                                float db[3];
#pragma unroll
                                for (int c = 0; c < 3; ++c) db[c] = (ah[c] - bh[c] * cs) / nb;
                                if (drop) flatten(db, up);
#pragma unroll
                                for (int r = 0; r < 3; ++r)
#pragma unroll
                                    for (int c = 0; c < 3; ++c) gGj[3 * r + c] += ds * db[r] * xb[c];
                            }
                        }
                    }
                }
                extra += val;
                mine = lane == t ? val : mine;
            }
        }
#endif
        if (jl)
#pragma unroll
            for (int c = 0; c < 3; ++c) GPB[4 * j + c] = gPj[c];
        // dL/dR_0 terms of this joint: dL/dG_j R_j^T (root: dL/dG_0) + dL/dP_j v_j^T; summed over the joints with the losses
        float red[15];
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) red[k] = gGj[k];
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) red[3 * r + c] = gGj[3 * r] * R[3 * c] + gGj[3 * r + 1] * R[3 * c + 1] + gGj[3 * r + 2] * R[3 * c + 2];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) red[3 * r + c] = fmaf(gPj[r], vj[c], red[3 * r + c]);
        if (!jl)
#pragma unroll
            for (int k = 0; k < 9; ++k) red[k] = 0.f;
        red[9] = gPj[0]; red[10] = gPj[1]; red[11] = gPj[2]; // dL/dworld_disp = sum_j dL/dP_j
        red[12] = dpj; red[13] = drj; red[14] = dtj;
#pragma unroll
        for (int k = 0; k < 15; ++k) red[k] = wsum(red[k]);
        // (every lane computed the constraint terms on the same values, lanes below 32 hold the sums: lane 0's copy makes them uniform)
        const float lp = uni(red[12]) / (3.f * (float)E), lr = a.lam_rot * (uni(red[13]) / (9.f * (float)E)), lt = a.lam_tmp * (uni(red[14]) / 24.f);
#if !DP_CONS_TABLE
#pragma unroll
        for (int k = 0; k < 4; ++k) ext[k] = uni(ext[k]);
        extra = ((ext[1] + ext[2]) + ext[0]) + ext[3]; // the reference's order (drag_pose.py:178-183)
#else
        extra = uni(extra);
#endif
        const float tot = ((lp + lr) + lt) + extra;
        const bool last = it + 1 >= n_iter;
        const bool stop = last || (a.early_stop && !((lp > a.stop_eps_pos || lr > a.stop_eps_rot) && (prev - tot > a.min_loss_incr)));
        prev = tot;
#if DP_CONS_SEQ
        if (stop) { // results of this, the step's last, forward pass, and run()'s epilogue (drag_pose.py:369-402) on them: the arithmetic and
                    // order of dp_sequence_advance_kernel, which reads them from the per-frame kernel's result arrays.  Every lane holds the
                    // same wd, d and carried gpc and computes the same new position.  (A bad target: the warm start's pose, as per frame.)
            long long fo = ft; // (opaque: the step's store addresses are formed here, not hoisted into registers that live across the iteration loop)
            asm volatile("" : "+v"(fo));
            float gpn[3], dsp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                gpn[k] = gpc[k] + wd[k]; // drag_pose.py:370
                dsp[k] = d[k];
            }
            if (a.q.adjust_joint >= 0) { // drag_pose.py:377-384
#pragma unroll
                for (int k = 0; k < 3; ++k) {
#if DP_CONS_GAP // that joint's effective target from its lane; lost or not tracked in this step: the adjusted joint's own position, adj = +0
                    float tk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tpe[k]), a.q.adjust_target_joint));
                    if (((__ballot(trk) >> a.q.adjust_target_joint) & 1ull) == 0ull) tk = PB[4 * a.q.adjust_joint + k];
#else
                    float tk = a.tgt_pos[(fo * NJ + a.q.adjust_target_joint) * 3 + k]; // (that joint's effective target: its lane's tpe)
                    if (a.q.tgt_root) tk = tk + sh[k];
#endif
                    // a difference, a product and two sums, none fused: dp_sequence_advance_kernel's v_sub, v_mul, v_add, v_add
                    const float adj = __fmul_rn(__fsub_rn(tk, PB[4 * a.q.adjust_joint + k]), a.q.adjust_weight);
                    gpn[k] = __fadd_rn(gpn[k], adj);
                    dsp[k] = __fadd_rn(dsp[k], adj);
                }
            }
#if DP_CONS_HOLD // include/dragposer_holds.h, "The update": lane t on its own row, which no lane reads again before the step's closing wave_sync()
            if (lane < a.n_terms) {
                const int hd = hold_of(a.h.n_holds, a.h.terms, lane);
                const float* tb = lds + L_TBL + lane * TW;
                if (hd >= 0 && tb[T_W] != 0.f) {
                    const int ja = __float_as_int(tb[T_JA]);
                    float* const row = wb + W_ROW + 4 * lane;
                    float wp[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) wp[k] = __fadd_rn(gpn[k], __fsub_rn(PB[4 * ja + k], PB[k])); // where a renderer puts joint a
                    const float hgt = __fsub_rn(comp(wp, up), tb[T_HLEVEL]);
                    if (row[3] == 0.f) {
                        if (hgt <= tb[T_HLO]) { row[0] = wp[0]; row[1] = wp[1]; row[2] = wp[2]; row[3] = 1.f; }
                    } else if (hgt > tb[T_HHI]) row[3] = 0.f;
                    if (a.h.trace)
#pragma unroll
                        for (int c = 0; c < 4; ++c) a.h.trace[(fo * a.h.n_holds + hd) * 4 + c] = row[c];
                }
            }
#endif
#if DP_CONS_TETHER // include/dragposer_tethers.h, "The update": lane t on its own row and its own four words of twp, which no lane reads again
                   // before the step's closing wave_sync()
            if (lane < a.n_terms) {
                const int tk = hold_of(a.t.n_tethers, a.t.terms, lane);
                const float* tb = lds + L_TBL + lane * TW;
                if (tk >= 0 && tb[T_W] != 0.f) {
                    const int ja = __float_as_int(tb[T_JA]);
                    float* const row = wb + W_ROW + 4 * lane;
#if DP_TETHER_WPREV_GLOBAL
                    float* const wpv = a.t.state + (f * a.t.n_tethers + tk) * TETHER_ROW + 4;
#else
                    float* const wpv = twp + wv * TETHER_W_FLOATS + 4 * tk;
#endif
                    float wp[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) wp[k] = __fadd_rn(gpn[k], __fsub_rn(PB[4 * ja + k], PB[k])); // where a renderer puts joint a
                    if (fabsf(wp[0]) <= DP_INPUT_LIMIT && fabsf(wp[1]) <= DP_INPUT_LIMIT && fabsf(wp[2]) <= DP_INPUT_LIMIT) {
                        const bool have = wpv[3] != 0.f;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            row[k] = have ? __fadd_rn(wp[k], __fmul_rn(tb[T_TALPHA], __fsub_rn(wp[k], wpv[k]))) : wp[k];
                            wpv[k] = wp[k];
                        }
                        row[3] = 1.f;
                        wpv[3] = 1.f;
                    }
                    if (a.t.trace) {
                        float* const trow = a.t.trace + (fo * a.t.n_tethers + tk) * TETHER_ROW;
#pragma unroll
                        for (int c = 0; c < 4; ++c) { trow[c] = row[c]; trow[4 + c] = wpv[c]; }
                    }
                }
            }
#endif
            float* const o = a.q.hist + fo * (LAT + 3 + NH);
            if (lane < LAT) o[lane] = z;
#if DP_CONS_AR // the step's history row becomes h_1, the older rows shift: lane i on column i, read again behind the step's closing wave_sync()
            if (lane < LAT) {
                float* const hs = arh + wv * AR_W_FLOATS + lane;
#pragma unroll
                for (int k = MAX_AR_ORDER - 1; k > 0; --k)
                    if (k < a.r.order) hs[k * LAT] = hs[(k - 1) * LAT];
                hs[0] = z;
            }
#endif
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o[LAT + k] = dsp[k];
                    if (a.q.pos_ret) a.q.pos_ret[fo * 3 + k] = gpn[k];
                }
                for (int h = 0; h < NH; ++h) o[LAT + 3 + h] = PB[4 * a.q.height_joints[h] + 1] + gpn[1]; // y of (pos + the new global position)
            }
#if DP_CONS_LIVE // the same row, a column per lane: lanes < 24 hold z; the displacement and the heights are lane 0's, handed over by v_readfirstlane
            hnew = z;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v = uni(dsp[k]);
                hnew = lane == LAT + k ? v : hnew;
            }
#pragma unroll
            for (int h = 0; h < DP_MAX_HEIGHT_JOINTS; ++h)
                if (h < NH) {
                    const float v = uni(PB[4 * a.q.height_joints[h] + 1] + gpn[1]);
                    hnew = lane == LAT + 3 + h ? v : hnew;
                }
#endif
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
                    a.loss[fo * 3] = bad_tgt ? nan : lp; a.loss[fo * 3 + 1] = bad_tgt ? nan : lr; a.loss[fo * 3 + 2] = bad_tgt ? nan : lt;
                }
#if !DP_CONS_TABLE
                if (a.loss_extra)
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.loss_extra[fo * 4 + c] = bad_tgt ? nan : ext[c];
#endif
            }
#if DP_CONS_TABLE
            if (lane < a.n_terms && a.loss_terms) a.loss_terms[fo * a.n_terms + lane] = bad_tgt ? nan : mine;
#endif
#pragma unroll
            for (int k = 0; k < 3; ++k) gpc[k] = gpn[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) crc[k] = uni(wr[k]); // lane 0 holds the world root rotation (drag_pose.py:371)
        }
#else
        if (stop) { // results of this, the last, forward pass (drag_pose.py:309-312)
            const bool pz = bad_tgt && !(a.early_stop || a.n_iter == 1); // (fixed count: the reference would decode the NaN latent)
            if (lane < LAT && a.z_pre) a.z_pre[f * LAT + lane] = pz ? nan : z;
            if (jl) {
                if (a.pose)
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.pose[f * 88 + 4 * j + c] = pz ? nan : (qn[c] - muj[c]) / sdj[c];
                if (a.pos)
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.pos[(f * NJ + j) * 3 + c] = pz ? nan : P[c];
                if (a.rot)
#pragma unroll
                    for (int k = 0; k < 9; ++k) a.rot[(f * NJ + j) * 9 + k] = pz ? nan : G[k];
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (a.disp) a.disp[f * 3 + c] = pz ? nan : d[c];
                    if (a.world_disp) a.world_disp[f * 3 + c] = pz ? nan : wd[c];
                }
                if (a.world_rot)
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.world_rot[f * 4 + c] = pz ? nan : wr[c];
                if (a.loss) {
                    a.loss[f * 3] = bad_tgt ? nan : lp; a.loss[f * 3 + 1] = bad_tgt ? nan : lr; a.loss[f * 3 + 2] = bad_tgt ? nan : lt;
                }
#if !DP_CONS_TABLE
                if (a.loss_extra)
#pragma unroll
                    for (int c = 0; c < 4; ++c) a.loss_extra[f * 4 + c] = bad_tgt ? nan : ext[c];
#endif
            }
#if DP_CONS_TABLE
            if (lane < a.n_terms && a.loss_terms) a.loss_terms[f * a.n_terms + lane] = bad_tgt ? nan : mine;
#endif
        }
#endif
        wave_sync();

        // ---- backward: subtree sums, per-joint rotations, root
        if (jl) {
            float F[3] = {0.f, 0.f, 0.f};
            for (int dj = 0; dj < NJ; ++dj)
                if ((mysubj >> dj) & 1u) { F[0] += GPB[4 * dj]; F[1] += GPB[4 * dj + 1]; F[2] += GPB[4 * dj + 2]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) FB[4 * j + c] = F[c];
        }
        wave_sync();
        if (jl && j != 0) {
            float M[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = gGj[k];
            for (int k = cst[j]; k < cst[j + 1]; ++k) { // child bones: M += F_c off_c^T
                const int c = cls[k];
                const float F0 = FB[4 * c], F1 = FB[4 * c + 1], F2 = FB[4 * c + 2];
#if DP_CONS_SKEL
                const float o0 = wb[W_SK + 3 * c], o1 = wb[W_SK + 3 * c + 1], o2 = wb[W_SK + 3 * c + 2];
#else
                const float o0 = lds[L_OFF + 3 * c], o1 = lds[L_OFF + 3 * c + 1], o2 = lds[L_OFF + 3 * c + 2];
#endif
                M[0] = fmaf(F0, o0, M[0]); M[1] = fmaf(F0, o1, M[1]); M[2] = fmaf(F0, o2, M[2]);
                M[3] = fmaf(F1, o0, M[3]); M[4] = fmaf(F1, o1, M[4]); M[5] = fmaf(F1, o2, M[5]);
                M[6] = fmaf(F2, o0, M[6]); M[7] = fmaf(F2, o1, M[7]); M[8] = fmaf(F2, o2, M[8]);
            }
            float dR[9], dqn[4];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) dR[3 * r + c] = R0[r] * M[c] + R0[3 + r] * M[3 + c] + R0[6 + r] * M[6 + c];
            rotmat_vjp(qn, dR, dqn);
            const float dot = qn[0] * dqn[0] + qn[1] * dqn[1] + qn[2] * dqn[2] + qn[3] * dqn[3];
#pragma unroll
            for (int c = 0; c < 4; ++c) DYB[4 * j + c] = (dqn[c] - qn[c] * dot) * rn * sdj[c];
        }
        if (lane == 0) { // root: world_rot = cur_rot (x) q_0, world_disp = R_0 d
            float dR0[9], dw[4], dq0[4];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) dR0[3 * r + c] = fmaf(red[9 + r], d[c], red[3 * r + c]);
            rotmat_vjp(wr, dR0, dw);
            dq0[0] = dw[0] * cr[0] + dw[1] * cr[1] + dw[2] * cr[2] + dw[3] * cr[3];
            dq0[1] = -dw[0] * cr[1] + dw[1] * cr[0] + dw[2] * cr[3] - dw[3] * cr[2];
            dq0[2] = -dw[0] * cr[2] - dw[1] * cr[3] + dw[2] * cr[0] + dw[3] * cr[1];
            dq0[3] = -dw[0] * cr[3] + dw[1] * cr[2] - dw[2] * cr[1] + dw[3] * cr[0];
            const float dot = qn[0] * dq0[0] + qn[1] * dq0[1] + qn[2] * dq0[2] + qn[3] * dq0[3];
#pragma unroll
            for (int c = 0; c < 4; ++c) DYB[c] = (dq0[c] - qn[c] * dot) * rn * sdj[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) // dL/dd = R_0^T dL/dworld_disp
                DYB[4 * NJ + c] = (R0[c] * red[9] + R0[3 + c] * red[10] + R0[6 + c] * red[11]) * W[dpvjp::OFF_SD + 4 * NJ + c];
        }
        wave_sync();
        // ---- decoder backward: A2^T, A1^T, A0^T with the LeakyReLU slopes of this pass
        if (lane < H1) {
            float s = 0.f;
#pragma unroll UNR
            for (int o = 0; o < NYU; ++o) s = fmaf(lds[L_A2 + o * S2 + lane], DYB[o], s);
            HB1[lane] = pos1 ? s : s * 0.2f;
        }
        wave_sync();
        if (lane < H0) {
            float s = 0.f;
#pragma unroll UNR
            for (int k = 0; k < H1; ++k) s = fmaf(lds[L_A1 + k * S1 + lane], HB1[k], s);
            HB0[lane] = pos0 ? s : s * 0.2f;
        }
        wave_sync();
        // ---- Adam (torch.optim.Adam defaults re-created per frame, drag_pose.py:218), a lane per latent component
        b1t *= a.beta1d;
        b2t *= a.beta2d;
        const float step = (float)(a.lrd / (1.0 - b1t)), rbc2s = (float)(1.0 / sqrt(1.0 - b2t));
        if (lane < LAT) {
            float s = 0.f;
#pragma unroll UNR
            for (int i = 0; i < H0; ++i) s = fmaf(lds[L_A0 + i * S0 + lane], HB0[i], s);
            const float g = fmaf(a.ctmp, dz, s);
            m = m + a.one_m_b1 * (g - m);
            v = v * a.beta2 + a.one_m_b2 * (g * g);
            const float den = sqrtf(v) * rbc2s + a.eps;
            z = z - step * (m / den);
            ZB[lane] = z;
        }
        if (stop) break;
    }
    const bool pz = bad_tgt;
#if DP_CONS_SEQ
    zc = pz ? nan : z; // the next step's warm start (a bad target: NaN, which that step's screening finds)
    const bool nonfin = pz || __ballot(lane < LAT && !(fabsf(z) <= 3.0e38f)) != 0ull;
    if (lane == 0) {
        if (a.iters) a.iters[ft] = bad_tgt && !a.early_stop ? a.n_iter : it + 1;
#if DP_CONS_GAP
        if (a.status)
            a.status[ft] = (nonfin ? DP_STATUS_NONFINITE_RESULT : 0) | (bad_tgt ? DP_STATUS_BAD_TARGETS : 0) | gbits | (En == 0 ? DP_STATUS_NO_TRACKER : 0);
#else
        if (a.status) a.status[ft] = (nonfin ? DP_STATUS_NONFINITE_RESULT : 0) | (bad_tgt ? DP_STATUS_BAD_TARGETS : 0);
#endif
    }
    wave_sync(); // (the next step's first writes into the wave's block follow this step's last reads)
    } // the step loop
#if DP_CONS_HOLD
    if (lane < a.n_terms) {
        const int hd = hold_of(a.h.n_holds, a.h.terms, lane);
        if (hd >= 0 && lds[L_TBL + lane * TW + T_W] != 0.f)
#pragma unroll
            for (int c = 0; c < 4; ++c) a.h.state[(f * a.h.n_holds + hd) * 4 + c] = wb[W_ROW + 4 * lane + c];
    }
#endif
#if DP_CONS_TETHER
    if (lane < a.n_terms) {
        const int tk = hold_of(a.t.n_tethers, a.t.terms, lane);
        if (tk >= 0 && lds[L_TBL + lane * TW + T_W] != 0.f) {
            float* const srow = a.t.state + (f * a.t.n_tethers + tk) * TETHER_ROW;
#pragma unroll
            for (int c = 0; c < 4; ++c) srow[c] = wb[W_ROW + 4 * lane + c];
#if !DP_TETHER_WPREV_GLOBAL
#pragma unroll
            for (int c = 0; c < 4; ++c) srow[4 + c] = twp[wv * TETHER_W_FLOATS + 4 * tk + c];
#endif
        }
    }
#endif
    if (lane < LAT) a.z[f * LAT + lane] = zc;
    if (lane < 3) a.q.global_pos[f * 3 + lane] = lane == 0 ? gpc[0] : lane == 1 ? gpc[1] : gpc[2];
    if (lane < 4) a.q.global_rot[f * 4 + lane] = lane == 0 ? crc[0] : lane == 1 ? crc[1] : lane == 2 ? crc[2] : crc[3];
#if DP_CONS_LIVE
    // dp_sequence_history_kernel's work for this sequence after one step: lane c moves column c of the three buffers up by one row and puts
    // the step's value in the last.  LIVE_CHUNK rows at a time, a chunk's loads before its stores; the next chunk reads only rows above every
    // row written so far.  The column is this lane's alone and the sequence this wave's: no barrier, no fence, no atomic.
    if (lane < LAT + 3 + NH) {
        const int H = a.l.history;
        float* col = a.l.latent_buf + f * H * LAT + lane;
        int stride = LAT;
        if (lane >= LAT + 3) { col = a.l.heights_buf + f * H * NH + (lane - LAT - 3); stride = NH; }
        else if (lane >= LAT) { col = a.l.disp_buf + f * H * 3 + (lane - LAT); stride = 3; }
        for (int t0 = 0; t0 + 1 < H; t0 += LIVE_CHUNK) {
            float v[LIVE_CHUNK];
#pragma unroll
            for (int i = 0; i < LIVE_CHUNK; ++i) v[i] = t0 + i + 1 < H ? col[(long long)(t0 + i + 1) * stride] : 0.f;
            asm volatile("" ::: "memory"); // (the chunk's loads are issued before its first store)
#pragma unroll
            for (int i = 0; i < LIVE_CHUNK; ++i)
                if (t0 + i + 1 < H) col[(long long)(t0 + i) * stride] = v[i];
        }
        col[(long long)(H - 1) * stride] = hnew;
    }
#endif
#else
    if (lane < LAT && a.z) a.z[f * LAT + lane] = pz ? nan : z;
    const bool nonfin = pz || __ballot(lane < LAT && !(fabsf(z) <= 3.0e38f)) != 0ull;
    if (lane == 0) {
        if (a.iters) a.iters[f] = bad_tgt && !a.early_stop ? a.n_iter : it + 1;
        if (a.status) a.status[f] = (nonfin ? DP_STATUS_NONFINITE_RESULT : 0) | (bad_tgt ? DP_STATUS_BAD_TARGETS : 0);
    }
#endif
}
