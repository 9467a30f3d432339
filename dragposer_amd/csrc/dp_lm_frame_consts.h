// dp_lm_frame_consts.h -- a fragment of text of the LM frame (dp_lm_body.h, dp_clip_rows_body.h), included in place once per frame, behind the
// screening: the per-lane constants of the forward pass.
//   reads      W, lane, j, jl, par, BONES, SW, trk, wp, wrr, E, a.lam_rot, a.lam_tmp
//   leaves     c0, b1, oB, b2A, sdA, muA, b2B, sdB, muB (the decoder's), pj, off (the lane's bone), sdj, muj (the returned pose's), ct;
//              SW[2 j], SW[2 j + 1] written: the joint's residual scales, read by the tangents behind the pass's wave_sync()s
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
