// dp_clip_decide_body.h -- the body of the clip solves' decision kernel, included behind its signature by dp_clip.hip (dpclip::Args a) and by
// dp_clip_accel.hip (dpclipacc::Args aa), behind dp_clip_total.h.  One wave per sequence.  step -1: after the pass of z0 -- is a frame refused,
// the damping the sequence starts from, L_s(Z0).  step k: trial k's decision: L_s(Z') < L_s(Z), mu, the word.  The last step's also hands the
// per-sequence outputs over.
//   parameter  DP_CLIP_ACCEL  as in dp_clip_total.h.  What stands under ACCEL(...) -- the second-difference part of the totals kept in wacc and
//                             returned in accel_loss -- is all that the two kernels differ in
//   reads      a.step; the workspace's per-frame flags, loss rows and coupling parts (and latents) through clip_total; wword, wsolved, wtot,
//              wmu, wnacc (and wacc)
//   leaves     wword, wmu, wnacc, wtot (and wacc); loss_hist's entry of the step; at step -1 of a refused sequence and at the last step the
//              caller's mu, n_accepted, clip_loss, info (and accel_loss)
//   no LDS and so no wave_sync(): lane 0 writes, every lane of the wave takes part in the ballot and in clip_total
{
#if DP_CLIP_ACCEL
#define ACCEL(...) __VA_ARGS__
#define BLOCK aa // (the unit's argument block; a is dp_clip.h's part of it)
    const K::Args& a = aa.c;
#else
#define ACCEL(...)
#define BLOCK a
#endif
    const int lane = threadIdx.x, sq = blockIdx.x, S = a.n_seq, T = a.n_t, NH = a.n_steps + 1;
    const double nan = __builtin_nan("");
    if (a.step < 0) {
        int fl = 0;
        for (int t = lane; t < T; t += 64) fl |= a.wflags[(long long)t * S + sq];
        const bool ref = __ballot(fl != 0) != 0ull;
        float mu = a.mu ? a.mu[sq] : a.mu0;
        if (!(mu >= a.mu_min && mu <= a.mu_max)) mu = a.mu0;
        double cp = nan, tot = nan;
        ACCEL(double ap = nan;)
        if (!ref) tot = clip_total(BLOCK, 0, sq, lane, cp ACCEL(, ap));
        if (lane == 0) {
            a.wword[sq] = ref ? K::W_REFUSED : 0;
            a.wmu[sq] = mu;
            a.wnacc[sq] = 0;
            a.wtot[2 * sq] = tot;
            a.wtot[2 * sq + 1] = cp;
            ACCEL(aa.wacc[sq] = ap;)
            if (a.loss_hist) a.loss_hist[(long long)sq * NH] = tot;
            if (ref) { // no step runs: what the sequence returns (mu stays as the caller holds it)
                if (a.n_accepted) a.n_accepted[sq] = 0;
                if (a.clip_loss) { a.clip_loss[2 * sq] = nan; a.clip_loss[2 * sq + 1] = nan; }
                ACCEL(if (aa.accel_loss) aa.accel_loss[sq] = nan;)
                if (a.info) a.info[sq] = DP_CLIP_REFUSED_FRAME;
            }
        }
        if (ref && a.loss_hist)
            for (int k = 1 + lane; k < NH; k += 64) a.loss_hist[(long long)sq * NH + k] = nan;
        return;
    }
    const int word = a.wword[sq];
    if ((word & K::W_REFUSED) != 0) return;
    const int cur = (word & K::W_CUR) != 0 ? 1 : 0;
    double tot = a.wtot[2 * sq], cp = a.wtot[2 * sq + 1], cpn = nan, totn = nan;
    ACCEL(double ap = aa.wacc[sq], apn = nan;)
    if (a.wsolved[sq] != 0) totn = clip_total(BLOCK, cur ^ 1, sq, lane, cpn ACCEL(, apn));
    const bool acc = totn < tot; // (a NaN rejects)
    if (lane == 0) {
        float mu = a.wmu[sq];
        int nacc = a.wnacc[sq];
        if (acc) {
            tot = totn; cp = cpn; ACCEL(ap = apn;)
            ++nacc;
            mu = fmaxf(mu * a.mu_down, a.mu_min);
            a.wword[sq] = cur ? 0 : K::W_CUR;
            a.wtot[2 * sq] = tot;
            a.wtot[2 * sq + 1] = cp;
            ACCEL(aa.wacc[sq] = ap;)
            a.wnacc[sq] = nacc;
        } else {
            mu = fminf(mu * a.mu_up, a.mu_max);
            a.wword[sq] = (cur ? K::W_CUR : 0) | K::W_REJECTED;
        }
        a.wmu[sq] = mu;
        if (a.loss_hist) a.loss_hist[(long long)sq * NH + a.step + 1] = tot;
        if (a.step == a.n_steps - 1) {
            if (a.mu) a.mu[sq] = mu;
            if (a.n_accepted) a.n_accepted[sq] = nacc;
            if (a.clip_loss) { a.clip_loss[2 * sq] = tot; a.clip_loss[2 * sq + 1] = cp; }
            ACCEL(if (aa.accel_loss) aa.accel_loss[sq] = ap;)
            if (a.info) a.info[sq] = 0;
        }
    }
#undef ACCEL
#undef BLOCK
}
