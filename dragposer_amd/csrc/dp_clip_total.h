// dp_clip_total.h -- the body of the clip solves' per-sequence totals, included behind its signature by dp_clip.hip,
// clip_total(const dpclip::Args& a, int b, int sq, int lane, double& cp), and by dp_clip_accel.hip, clip_total(const dpclipacc::Args& aa, ...,
// double& cp, double& ap), in front of the decision kernel.
//   parameter  DP_CLIP_ACCEL  1 in the unit with the second-difference term, 0 in the other: the only switch.  ACCEL(...) is its arguments
//                             under 1 and nothing under 0
//   computes   the frames' numbers of sequence sq in buffer b, added in double in index order -> L_s; `cp`: the coupling sums'
//              part of it; under DP_CLIP_ACCEL `ap`: the second-difference sum's, read from the latent buffer b itself
//   reads      a.wloss[b], a.wcpl[b], under DP_CLIP_ACCEL a.wz[b]; the whole wave calls it (readlane, and wsum_d under DP_CLIP_ACCEL); no
//              LDS and so no wave_sync()
#if DP_CLIP_ACCEL
#define ACCEL(...) __VA_ARGS__
#else
#define ACCEL(...)
#endif
{
    ACCEL(const K::Args& a = aa.c;)
    const int S = a.n_seq, T = a.n_t;
    double tot = 0.0, cs = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const float l = t < T ? a.wloss[b][((long long)t * S + sq) * 4 + 3] : 0.f;
        const double q = t < T ? a.wcpl[b][(long long)t * S + sq] : 0.0;
        const int lo = __double2loint(q), hi = __double2hiint(q);
        const int n = T - t0 < 64 ? T - t0 : 64;
        for (int i = 0; i < n; ++i) {
            tot += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(l), i));
            cs += __hiloint2double(__builtin_amdgcn_readlane(hi, i), __builtin_amdgcn_readlane(lo, i));
        }
    }
#if DP_CLIP_ACCEL
    // |z_(t+1) - 2 z_t + z_(t-1)|^2 from the latents themselves: lane k adds component k's squares over the frames in index order, and the 24
    // sums meet once at the end (a wave sum per frame, five dependent shuffles of a double, cost 0.35 us per frame)
    double as = 0.0;
    const float* __restrict__ Z = a.wz[b];
    const int li = lane < LAT ? lane : LAT - 1;
    const auto zat = [&](int t) { return (double)Z[((long long)t * S + sq) * LAT + li]; };
    double zm = T > 2 ? zat(0) : 0.0, zc = T > 2 ? zat(1) : 0.0;
    constexpr int AHEAD = 8; // frames loaded together
    for (int t0 = 1; t0 + 1 < T; t0 += AHEAD) {
        double zn[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) zn[u] = t0 + u + 1 < T ? zat(t0 + u + 1) : 0.0;
#pragma unroll
        for (int u = 0; u < AHEAD; ++u)
            if (t0 + u + 1 < T) { // (wave-uniform)
                const double d = (zn[u] - 2.0 * zc) + zm;
                as = fma(d, d, as);
                zm = zc;
                zc = zn[u];
            }
    }
    as = wsum_d(lane < LAT ? as : 0.0);
    ap = ((double)aa.lam_accel / 24.0) * as;
#endif
    cp = ((double)a.lam_smooth / 24.0) * cs ACCEL(+ap);
    return tot + cp;
}
#undef ACCEL
