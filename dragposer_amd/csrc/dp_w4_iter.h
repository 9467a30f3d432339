// dp_w4_iter.h -- the iteration loop of the wave-private kernel: not a header of its own but a piece of W4_KERNEL's body (dp_w4_impl.h), which
// includes it where COMMON and B2MODE are in scope -- once as plain text (the general loop) and, in dp_w4_bp_lv.hip's kernels, as
// the body of the lambda that is compiled once per loop version (W4_LOOP_VERSIONS).  Everything else it names is the kernel's.
    static_assert(!COMMON || (W4_BP && !EARLY && !SEQ), "the common version belongs to the body-part fixed-count kernels");
    for (int iter = 0; iter < a.n_iter; ++iter) {
        const bool last = (iter == a.n_iter - 1);
        const f2 adam_t = *(const f2*)(lds + L_TAB + 2 * (LONG ? min(iter, MAX_ITERS - 1) : iter)); // (an LDS broadcast read, issued a whole iteration ahead of its use)
        float step = adam_t.x, rbc2s = adam_t.y;
        if constexpr (LONG) {
            if (iter >= MAX_ITERS) adam_beyond(adx, a.cont, step, rbc2s); // (uniform: beyond the argument table)
        }
        int o = lane;
        asm volatile("" : "+v"(o)); // opaque per iteration: keeps the streamed weight reads inside the loop
        // (round 5, measured and not adopted: the streamed groups from global memory instead -- the L1 / L2 path is idle in the loop and the LDS is
        //  what the four waves contend for --: +3.3 % as it stands, +4 % with every chunk requested a phase earlier; 20 KB per wave and iteration
        //  does not live in the L1, and an L2 round trip is longer than any phase ahead the registers allow)
        const f4* w2 = (const f4*)(lds + L_IMG2) + o;

        // ================= L0: a0 = lrelu(A0 z + c0)
        f4 x = PK ? xz : zD;
#ifdef W4_STAMP_L0
        { // (a scalar read of the new latent: the stamp below cannot be taken before the Adam step's last result EXISTS -- what was still in flight is slot 12's)
            int t_;
            asm volatile("v_readfirstlane_b32 %0, %1\n\ts_nop 3\n\ts_add_u32 %0, %0, 0" : "=s"(t_) : "v"(x[2]) : "scc");
        }
        STAMP(12);
#endif
        QT(x);
#ifdef W4_STAMP_L0
        { int t_; asm volatile("s_nop 3\n\tv_readfirstlane_b32 %0, %1\n\ts_nop 3\n\ts_add_u32 %0, %0, 0" : "=s"(t_) : "v"(x[3]) : "scc"); }
        STAMP(13);
#endif
        f4 acc0, acc1;
        chain_a<6, 0, 1>(acc0, acc1, x, wL0, bias0T);
        chain_end(acc0, acc1);
#ifdef W4_STAMP_L0
        STAMP(14);
#endif
        const f4 f0D = lrelu_factor(acc0 + acc1); // kept for the backward
#ifdef W4_STAMP_L0
        { int t_; asm volatile("v_readfirstlane_b32 %0, %1\n\ts_nop 3\n\ts_add_u32 %0, %0, 0" : "=s"(t_) : "v"(f0D[3]) : "scc"); }
        STAMP(15);
#else
        STAMP(0);
#endif
        // ================= L1: a1 = lrelu(A1 a0 + b1)
        x = (acc0 + acc1) * f0D;
        QT(x);
        chain_a<5, 0, 1>(acc0, acc1, x, wL1, bias1T); // the hidden layer's channels 0..19: quads 0..4,
        chain_a<5, 8>(acc0, acc1, x, wL1 + 5);  // 20..39: quads 8..12 (dp_w4.h)
        chain_end(acc0, acc1);
        const f4 f1D = lrelu_factor(acc0 + acc1);
        STAMP(1);
        // ================= L2: y = A2 a1 + b2, two 64-row blocks (channels 0, 1 | 2, 3 of both items of every quad)
        x = (acc0 + acc1) * f1D;
        QT(x);
        f4 y01, y23;
        {
            f4 pa0, pa1, pb0, pb1;
#if W4_BP
            chain_l2_bp<BP_NG_A, 0>(pa0, pa1, x, wL2A, bias2aT);
            chain_l2_bp<BP_NG_B, 1>(pb0, pb1, x, wL2B, bias2bT);
#else
            chain_a<15, 0, 1>(pa0, pa1, x, wL2A, bias2aT);
            chain_a<15, 0, 1>(pb0, pb1, x, wL2B, bias2bT);
#endif
            chain_end(pa0, pa1);
            y01 = pa0 + pa1;
            y23 = pb0 + pb1;
        }
        __builtin_amdgcn_sched_barrier(0); // (both sums first: a VALU instruction between two MFMAs of one wave costs ~14 cycles)
        quad_transpose_mfma2(y01, y23, eT); // lane (b, i): the decoder channels of my two items of frame i, side A | side B in register pairs
#if W4_BP
        { // body-part: the transposes leave side A's four channels, then side B's -- the register pairs the packed kinematics reads are moved together
            const f4 yA = y01, yB = y23;
            y01 = f4{yA[0], yB[0], yA[1], yB[1]};
            y23 = f4{yA[2], yB[2], yA[3], yB[3]};
        }
#endif
        STAMP(2);

        // ================= kinematics
        // (every instantiation takes the changes that cost it no spill, counted at compile time.  The body-part units: all three.  The dense
        //  units have 40 vector registers fewer to spare: stage T's forty operands across stage J spill 2-4 registers in the fixed-count
        //  kernels, and the late chunk 2 in the long sequence kernel -- they keep the old order there)
        constexpr int ER = W4_EARLY_READS & (W4_BP ? 7 : (EARLY ? 1 : 3));
        constexpr bool G_WAB = (ER & 1) != 0, WQ_LATE = (ER & 2) != 0, T_EARLY = (ER & 4) != 0;
        TRd trd;
#ifndef W4_ABLATE_J
        j_stage<T_EARLY>(pc, fb, y01, y23, jo, trk, trd);
#else
        jo.q[0] = f2{y01[0], y01[1]}; jo.q[1] = f2{y01[2], y01[3]}; jo.q[2] = f2{y23[0], y23[1]}; jo.q[3] = f2{y23[2], y23[3]};
        jo.u[0] = jo.q[0]; jo.u[1] = jo.q[1]; jo.u[2] = jo.q[2]; jo.inv = splat2(1.f);
        if constexpr (T_EARLY) { t_reads_q(trk, fb, trd); t_reads_bn(trk, fb, trd); }
#endif
        // (no instruction: a compiler fence between stage J's stores and the reads behind them -- the second pass's, and with T_EARLY off
        //  every read of stage T; the stores' own memory clobber is what holds the reads issued from inside stage J behind them)
        wave_sync();
        STAMP(3);
        if constexpr (!COMMON) {
            if (!optimise) break; // forward-only launch (uniform)
        }
#ifndef W4_ABLATE_T // (diagnostic builds, tools/ablate_w4.sh: a stage left out to time the rest -- results are wrong by construction)
        if constexpr (T_EARLY) t_finish<true>(trk, fb, EARLY || last, trd);
        else t_stage(trk, fb, EARLY || last);
        if constexpr (!COMMON) {
            for (int base = 16; base < Emax; base += 16) t_stage(load_tracker(a, fb, E, base + b), fb, EARLY || last); // (uniform, rare)
        }
#endif
        // bL2's weights leave LDS in three chunks (a read costs the wave its issue time wherever it stands -- the four waves of
        // a workgroup want the same LDS cycles -- so the chunks only have to be requested a phase ahead of their use, and be
        // small enough for the register file): the rest of the first 8 groups across stage G, 8 ahead of the chain, 10 behind its first chunk (each
        // pinned: the scheduler would move the reads next to their use)
        constexpr int NQ = 8 - B2_RES;
        f4 wq[NQ], wr[8], ws[10];
        // (uniform; mode 2 leaves groups 1..8 out, see bl2 below: its chain goes from group 0 straight to group 9, so groups 9.. take the
        //  first chunk's registers and its place here -- requested at the head of the chain they would come back an LDS round trip late)
        // The chunk is not needed before bL2 and reads come back in order: WQ_LATE requests it BEHIND stage G's reads (and, EARLY, the stop
        // test's), which the wave is about to wait for.
        const auto load_wq = [&] {
            if constexpr (COMMON) {
                if constexpr (B2MODE != 2) load_w<NQ>(wq, w2 + B2_RES * 64);
                else load_w<NQ>(wq, w2 + 9 * 64);
            } else {
                if (EARLY || b2_mode != 2) load_w<NQ>(wq, w2 + B2_RES * 64);
                else load_w<NQ>(wq, w2 + 9 * 64);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        if constexpr (!WQ_LATE) load_wq();
        wave_sync();
        STAMP(4);
        GRd grd;
        if constexpr (WQ_LATE) { // one group of requests: stage G's first, (EARLY: the stop test's, below,) the chunk last
#ifndef W4_ABLATE_G
            g_reads<G_WAB>(pc, fb, grd);
#endif
            if constexpr (!EARLY) load_wq();
        }
        unsigned actmask = 0xFu, stopmask = 0u; // bit r: frame f0 + r runs this iteration / stops after its step
        if (EARLY) {
            bool was_act = false, stop_now = false;
            { // the stop test of frame i, in EVERY lane of the frame's column (no branch: the reads and sums interleave with stage
              // G's; the state -- es_prev, es_act, es_iters -- is replicated over the column)
                // the loss terms of ALL ranks (zero beyond the frame's count: the set-up cleared them), read together -- a loop
                // over the frame's own count waits one LDS round trip per tracker -- and added in rank order
                float lp = 0.f, lr = 0.f, lt = 0.f;
                if (Emax <= 8) { // (uniform)
                    f4 l[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) l[k] = *(const f4*)(fb + FB_LP + 4 * k);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { lp += l[k].x; lr += l[k].y; lp += l[k].z; lr += l[k].w; }
                } else {
                    f4 l[W4_R / 2];
#pragma unroll
                    for (int k = 0; k < W4_R / 2; ++k) l[k] = *(const f4*)(fb + FB_LP + 4 * k);
#pragma unroll
                    for (int k = 0; k < W4_R / 2; ++k) { lp += l[k].x; lr += l[k].y; lp += l[k].z; lr += l[k].w; }
                }
#pragma unroll
                for (int k = 0; k < LAT; k += 4) { const f4 d = *(const f4*)(fb + FB_LT + k); lt += (d.x + d.y) + (d.z + d.w); }
                lt *= a.lam_tmp * (1.f / 24.f);
                const float tot = (lp + lr) + lt;
                const bool cont = (lp > a.stop_eps_pos || lr > a.stop_eps_rot) && (es_prev - tot > a.min_loss_incr) && !last;
                was_act = es_act;
                es_prev = es_act ? tot : es_prev;
                es_iters += es_act ? 1 : 0;
                if (es_act && b == 0) *(f4*)(fb + FB_ES) = f4{lp, lr, lt, 0.f};
                stop_now = es_act && !cont;
                es_act = es_act && cont;
            }
            actmask = (unsigned)__ballot(was_act && b == 0) & 0xFu;
            stopmask = (unsigned)__ballot(stop_now && b == 0) & 0xFu;
            if constexpr (WQ_LATE) load_wq();
        }
        f4 gyA, gyB;
#ifndef W4_ABLATE_G
        if constexpr (!WQ_LATE) g_reads<G_WAB>(pc, fb, grd);
        g_stage<G_WAB, !COMMON>(pc, fb, jo, tmask, Emax, grd, gyA, gyB);
#else
        gyA = f4{jo.q[0].x, jo.q[1].x, jo.q[2].x, jo.q[3].x}; gyB = f4{jo.q[0].y, jo.q[1].y, jo.q[2].y, jo.q[3].y};
#endif
        STAMP(5);

        // ================= bL2: d1 = (A2^T gy) * lrelu'(a1): K = 4 channels of the 16 side-A items (gyA), then of side-B
        // quads 1..10 (gyB)
        // A side-A item (= joint) whose dL/dy is exactly zero in all four frames of the wave -- neither it nor anything below its child bone
        // carries a tracker (the toes under the reference's 6 trackers; both legs under its 3- and 4-tracker sets) -- adds
        // nothing in its four K-steps: they are left out, with the read of their weights.  Which items is decided per wave in the set-up
        // (b2_mode); two patterns are compiled beside the general one, selected by a uniform branch per iteration.
        const auto bl2 = [&](auto skip_tag) {
            constexpr unsigned SK = decltype(skip_tag)::value;
            if constexpr (SK == B2_SKIP_2) { // group 0 | 9 .. 9 + NQ - 1 (in wq's registers, requested ahead of stage G) | the rest of side A | side B
                static_assert(NQ >= 1 && NQ <= 6, "mode 2 keeps groups 9.. in the first chunk's registers");
                load_w<7 - NQ>(wr, w2 + (9 + NQ) * 64);
                __builtin_amdgcn_sched_barrier(0);
                chain_begin();
                chain_b2<B2_RES_A, 0, 2, SK, true>(acc0, acc1, gyA, gyB, wB2a);
                chain_b2<NQ, 9>(acc0, acc1, gyA, gyB, wq);
                load_w<10>(ws, w2 + 16 * 64);
                __builtin_amdgcn_sched_barrier(0);
                chain_b2<7 - NQ, 9 + NQ>(acc0, acc1, gyA, gyB, wr);
            } else {
                load_w<8, 8, SK>(wr, w2 + 8 * 64);
                __builtin_amdgcn_sched_barrier(0);
                chain_begin();
                chain_b2<B2_RES_A, 0, 2, SK, true>(acc0, acc1, gyA, gyB, wB2a);
                chain_b2<B2_RES_V, B2_RES_A, 0, SK>(acc0, acc1, gyA, gyB, wB2v);
                chain_b2<NQ, B2_RES, 0, SK>(acc0, acc1, gyA, gyB, wq);
                load_w<10>(ws, w2 + 16 * 64); // (into the registers the first chunk has just released)
                __builtin_amdgcn_sched_barrier(0);
                chain_b2<8, 8, 0, SK>(acc0, acc1, gyA, gyB, wr);
            }
            chain_b2<B2_GROUPS_B, ITEMS_A>(acc0, acc1, gyA, gyB, ws);
            chain_end(acc0, acc1);
        };
        // (the early-stop and whole-sequence instantiations keep the one general chain: with their larger live state the three-way branch
        //  costs them spills inside the loop -- 3 and 39 registers, measured at compile time)
#ifdef W4_NO_B2_SKIP
        bl2(std::integral_constant<unsigned, 0u>{});
#else
        if constexpr (EARLY) bl2(std::integral_constant<unsigned, 0u>{});
        else if constexpr (COMMON) bl2(std::integral_constant<unsigned, B2MODE == 0 ? 0u : B2MODE == 1 ? B2_SKIP_1 : B2_SKIP_2>{}); // (chosen with the version)
        else {
            if (b2_mode == 0) bl2(std::integral_constant<unsigned, 0u>{});
            else if (b2_mode == 1) bl2(std::integral_constant<unsigned, B2_SKIP_1>{});
            else bl2(std::integral_constant<unsigned, B2_SKIP_2>{});
        }
#endif
        x = (acc0 + acc1) * f1D;
        QT(x);
        STAMP(6);
        // ================= bL1: d0 = (A1^T d1) * lrelu'(a0)
        chain_a<15, 0, 2>(acc0, acc1, x, wB1);
        chain_end(acc0, acc1);
        x = (acc0 + acc1) * f0D;
        QT(x);
        STAMP(7);
        // ================= bL0 + Adam (torch.optim.Adam, single-tensor form; m, v start at 0, t = iter + 1)
        chain3_v_zero<5>(acc0, acc1, x, wz); // two K-steps per instruction: lanes 0..31 | 32..63 hold the two halves of the sum
        chain_end(acc0, acc1);
        __builtin_amdgcn_sched_barrier(0); // (keeps the subtraction below out of the chains above: w4_probe, "independent v_pk_fma")
        f4 g = {0.f, 0.f, 0.f, 0.f};
        f2 gP = {0.f, 0.f};
        if constexpr (PK) gP = add_halves_packed(acc0 + acc1) + a.ctmp * (zP - ztP);
        else g = add_halves(acc0 + acc1) + a.ctmp * (zD - ztD);
        STAMP(8);
        if (!COMMON && PK && DBG_DUMP && a.dbg && iter == 0 && lane5 < LAT) { // (a launch that asks for the dump runs the general version)
            int ld = lane5;
            asm volatile("" : "+v"(ld));
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if (f0 + r + 2 * fhalf < nB) a.dbg[(size_t)(f0 + r + 2 * fhalf) * DBG_STRIDE + DBG_GZ + ld] = gP[r];
        }
        if (!PK && DBG_DUMP && a.dbg && iter == 0 && lane < LAT) {
            int ld = lane;
            asm volatile("" : "+v"(ld)); // (opaque: the four 64-bit addresses of this once-per-launch dump are not to be formed ahead of the loop and held across it)
#pragma unroll
            for (int r = 0; r < FPW; ++r)
                if (f0 + r < nB) a.dbg[(size_t)(f0 + r) * DBG_STRIDE + DBG_GZ + ld] = g[r];
        }
#ifdef W4_ABLATE_ADAM
        if constexpr (PK) { zP = zP - 1e-6f * gP; xz = unpack_frames(zP, xz); }
        else zD = zD - 1e-6f * g;
#else
        if constexpr (PK) {
            if (last && lane5 < LAT) { // (uniform) latent of this, the last, forward pass: for the epilogue
#pragma unroll
                for (int r = 0; r < 2; ++r) fb0[(r + 2 * fhalf) * FB_STRIDE + FB_ZPRE + lane5] = zP[r];
            }
            mP =mP + a.one_m_b1 * (gP - mP);
            vP = vP * a.beta2 + a.one_m_b2 * (gP * gP);
            const f2 den = f2{__builtin_amdgcn_sqrtf(vP.x), __builtin_amdgcn_sqrtf(vP.y)} * rbc2s + a.eps;
            zP = zP - step * (mP * f2{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)});
            xz = unpack_frames(zP, xz);
        } else if (!EARLY) {
            if (last && lane < LAT) { // (uniform) latent of this, the last, forward pass: for the epilogue
#pragma unroll
                for (int r = 0; r < FPW; ++r) fb0[r * FB_STRIDE + FB_ZPRE + lane] = zD[r];
            }
            mD = mD + a.one_m_b1 * (g - mD);
            vD = vD * a.beta2 + a.one_m_b2 * (g * g);
            const f4 den = f4{__builtin_amdgcn_sqrtf(vD.x), __builtin_amdgcn_sqrtf(vD.y), __builtin_amdgcn_sqrtf(vD.z),
                              __builtin_amdgcn_sqrtf(vD.w)} * rbc2s + a.eps;
            zD = zD - step * (mD * f4{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y), __builtin_amdgcn_rcpf(den.z),
                                      __builtin_amdgcn_rcpf(den.w)});
        } else {
            const f4 mN = mD + a.one_m_b1 * (g - mD);
            const f4 vN = vD * a.beta2 + a.one_m_b2 * (g * g);
            const f4 den = f4{__builtin_amdgcn_sqrtf(vN.x), __builtin_amdgcn_sqrtf(vN.y), __builtin_amdgcn_sqrtf(vN.z),
                              __builtin_amdgcn_sqrtf(vN.w)} * rbc2s + a.eps;
            const f4 zN = zD - step * (mN * f4{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y), __builtin_amdgcn_rcpf(den.z),
                                               __builtin_amdgcn_rcpf(den.w)});
#pragma unroll
            for (int r = 0; r < FPW; ++r) {
                if ((actmask >> r) & 1u) { // (uniform)
                    if ((stopmask >> r) & 1u) {
                        if (lane < LAT) fb0[r * FB_STRIDE + FB_ZPRE + lane] = zD[r]; // latent of this frame's LAST forward pass
                        zfinD[r] = zN[r]; // the frame's loop ends with this step; z, m, v stay as they are
                    } else {
                        zD[r] = zN[r]; mD[r] = mN[r]; vD[r] = vN[r];
                        const float dz = zN[r] - ztD[r];
                        if (lane < LAT) fb0[r * FB_STRIDE + FB_LT + lane] = dz * dz;
                    }
                }
            }
        }
#endif
#ifdef W4_STAMP_L0
        { int t_; asm volatile("v_readfirstlane_b32 %0, %1\n\ts_nop 3\n\ts_add_u32 %0, %0, 0" : "=s"(t_) : "v"(PK ? xz[3] : zD[3]) : "scc"); } // (Adam's slot ends when its result exists)
#endif
        STAMP(9);
#ifdef DP_PROFILE
        if (iter == 0) prof.t[18] = prof.prev - mt0;               // the first iteration (cold instruction cache)
        if (iter == 1) prof.t[19] = prof.prev - mt0 - prof.t[18];  // the second
#endif
        if (EARLY && ((unsigned)__ballot(es_act && b == 0) & 0xFu) == 0u) break; // every frame of the wave has stopped
    }
