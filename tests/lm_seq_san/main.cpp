// tests/lm_seq_san/main.cpp -- dp_optimize_sequence_lm (include/dragposer_sequence_lm.h) under AddressSanitizer and UndefinedBehaviorSanitizer:
// a stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel unit) and walks the call's
// refusals, in the header's order, on a context without a device.  Every sized struct is handed over in a heap block of exactly struct_size
// bytes, so a read past what the caller owns is an error here.  Device pointers are a constant that is never dereferenced.  Built and run by
// tests/test_host_san.py; every condition is exact.
#include "../../include/dragposer_sequence_lm.h"
#include "../host_san/san_support.h"

namespace {

struct Case { // what one call is made of; the defaults are well-formed (targets from frames->z_tgt, no predictor)
    dp_lm_params p = DP_LM_PARAMS_INIT;
    unsigned results_size = sizeof(dp_seq_results), results_reserved0 = 0u, extra_size = sizeof(dp_seq_lm_extra), extra_reserved0 = 0u;
    unsigned ar_size = sizeof(dp_latent_ar), ar_reserved0 = 0u;
    bool null_latent = false, null_frames = false, null_params = false, null_state = false, null_out = false, null_extra = false, null_adjust = false;
    bool with_ar = false, with_z_tgt = true, with_outputs = true, null_scratch = false, null_tgt_rot = false, null_gpos = false, null_coeffs = false;
    int n_seq = 4, n_steps = 5, history = 4, n_heights = 6, height0 = 0, adjust_joint = 0, adjust_target = 13, order = 2;
};

int run(dp_ctx* ctx, const Case& c)
{
    dp_seq_frames f0{};
    f0.n_steps = c.n_steps;
    f0.tgt_pos = f0.tgt_root = f0.w = PTR; f0.tracked = (const unsigned char*)PTR;
    f0.tgt_rot = c.null_tgt_rot ? nullptr : PTR;
    f0.z_tgt = c.with_z_tgt ? PTR : nullptr;
    f0.z_tgt_step = 24 * c.n_seq; f0.z_tgt_seq = 24;
    dp_seq_state s0{};
    s0.global_pos = c.null_gpos ? nullptr : PTR;
    s0.global_rot = s0.latent_buf = s0.disp_buf = s0.heights_buf = PTR;
    s0.history = c.history; s0.n_heights = c.n_heights;
    for (int h = 0; h < DP_MAX_HEIGHT_JOINTS; ++h) s0.height_joints[h] = h == 0 ? c.height0 : h;
    dp_seq_step a0{};
    a0.adjust_joint = c.adjust_joint; a0.adjust_target_joint = c.adjust_target; a0.adjust_weight = 0.5f;
    dp_seq_results r0 = DP_SEQ_RESULTS_INIT;
    r0.struct_size = c.results_size; r0.reserved0 = c.results_reserved0;
    r0.hist_scratch = c.null_scratch ? nullptr : PTR;
    if (c.with_outputs) { r0.pose_ret = r0.pos_ret = r0.world_rot = r0.loss = PTR; r0.iters = r0.status = (int*)PTR; }
    dp_seq_lm_extra e0 = DP_SEQ_LM_EXTRA_INIT;
    e0.struct_size = c.extra_size; e0.reserved0 = c.extra_reserved0;
    if (c.with_outputs) { e0.mu = e0.mu_trace = e0.loss0 = e0.joint_pos = PTR; e0.n_accepted = (int*)PTR; }
    dp_latent_ar l0 = DP_LATENT_AR_INIT;
    l0.struct_size = c.ar_size; l0.reserved0 = c.ar_reserved0; l0.order = c.order;
    l0.coeffs = c.null_coeffs ? nullptr : PTR; l0.bias = PTR; l0.trace = c.with_outputs ? PTR : nullptr;
    Exact<dp_seq_frames> f(f0);
    Exact<dp_seq_state> s(s0);
    Exact<dp_seq_step> a(a0);
    Exact<dp_lm_params> p(c.p, cut<dp_lm_params>(c.p.struct_size));
    Exact<dp_seq_results> r(r0, cut<dp_seq_results>(c.results_size));
    Exact<dp_seq_lm_extra> e(e0, cut<dp_seq_lm_extra>(c.extra_size));
    Exact<dp_latent_ar> l(l0, cut<dp_latent_ar>(c.ar_size));
    return dp_optimize_sequence_lm(ctx, c.n_seq, c.null_latent ? nullptr : PTR, c.null_frames ? nullptr : f.get(), c.null_params ? nullptr : p.get(),
                                   c.with_ar ? l.get() : nullptr, c.null_state ? nullptr : s.get(), c.null_adjust ? nullptr : a.get(),
                                   c.null_out ? nullptr : r.get(), c.null_extra ? nullptr : e.get(), nullptr);
}

} // namespace

int main()
{
    Walker w("lm_seq", "dp_optimize_sequence_lm");
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    const float nan = __builtin_nanf("");
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 7; ++variant) {
        Case c;
        if (variant == 1) c.null_extra = true;
        if (variant == 2) c.with_outputs = false;                                  // every optional pointer NULL
        if (variant == 3) c.null_adjust = true;
        if (variant == 4) { c.with_ar = true; c.with_z_tgt = false; }              // the predictor is the targets' source
        if (variant == 5) { c.with_ar = true; c.with_z_tgt = false; c.order = DP_MAX_AR_ORDER; c.history = DP_MAX_AR_ORDER; c.n_heights = 0; }
        if (variant == 6) { c.adjust_joint = -1; c.adjust_target = -7; c.p.n_steps = DP_LM_MAX_STEPS; c.p.early_stop = 1; c.n_steps = 1; c.n_seq = 1; }
        w.unsupported(run(w.ctx, c), "dp_lm_seq.hip");
    }
    // the refusals in the header's order: each is reported before every later one's fault
    { Case c; c.n_seq = 0; c.p.struct_size = 4; refused(c, "n_sequences must be positive"); }
    { Case c; c.null_latent = true; c.p.n_steps = 0; refused(c, "NULL latent, frames, params, state or results"); }
    { Case c; c.null_frames = true; c.p.n_steps = 0; refused(c, "NULL latent, frames, params, state or results"); }
    { Case c; c.null_params = true; c.results_size = 8; refused(c, "NULL latent, frames, params, state or results"); }
    { Case c; c.null_state = true; c.p.n_steps = 0; refused(c, "NULL latent, frames, params, state or results"); }
    { Case c; c.null_out = true; c.p.n_steps = 0; refused(c, "NULL latent, frames, params, state or results"); }
    { Case c; c.p.struct_size = 4; c.results_size = 8; refused(c, "dp_lm_params.struct_size"); }      // a block of 4 bytes: only the size word exists
    { Case c; c.p.struct_size = 44; c.p.n_steps = 0; refused(c, "dp_lm_params.struct_size"); }
    { Case c; c.p.struct_size = 5000; refused(c, "dp_lm_params.struct_size"); }
    { Case c; c.p.n_steps = 0; c.results_size = 8; refused(c, "n_steps 0 outside"); }
    { Case c; c.p.n_steps = DP_LM_MAX_STEPS + 1; c.n_steps = 0; refused(c, "n_steps 65 outside"); }
    { Case c; c.p.lambda_tmp = -1.f; c.results_size = 8; refused(c, "lambda_rot or lambda_tmp"); }
    { Case c; c.p.mu_max = nan; c.results_size = 8; refused(c, "is not finite"); }
    { Case c; c.p.mu_down = 1.f; c.p.mu_up = 1.f; refused(c, "mu_down must lie in (0, 1)"); }
    { Case c; c.p.mu_up = 1.f; c.p.mu_min = 2.f; refused(c, "mu_up must be greater than 1"); }
    { Case c; c.p.mu_min = 0.f; c.results_size = 8; refused(c, "0 < mu_min <= mu_max"); }
    { Case c; c.p.mu0 = 1e7f; c.results_size = 8; refused(c, "mu0 outside [mu_min, mu_max]"); }
    { Case c; c.results_size = 8; c.n_steps = 0; refused(c, "dp_seq_results.struct_size"); }          // a block of 8 bytes: size word and reserved0
    { Case c; c.results_size = 5000; c.n_steps = 0; refused(c, "dp_seq_results.struct_size"); }
    { Case c; c.results_reserved0 = 3u; c.n_steps = 0; refused(c, "reserved0 3"); }
    { Case c; c.n_steps = 0; c.null_scratch = true; refused(c, "n_steps must be positive"); }
    { Case c; c.null_tgt_rot = true; c.null_scratch = true; refused(c, "NULL input array"); }
    { Case c; c.null_scratch = true; c.history = 0; refused(c, "NULL state array / hist_scratch"); }
    { Case c; c.null_gpos = true; c.history = 0; refused(c, "NULL state array / hist_scratch"); }
    { Case c; c.history = 0; c.height0 = 22; refused(c, "history / n_heights out of range"); }
    { Case c; c.n_heights = DP_MAX_HEIGHT_JOINTS + 1; refused(c, "history / n_heights out of range"); }
    { Case c; c.height0 = 22; c.adjust_joint = 22; refused(c, "bad height joint"); }
    { Case c; c.adjust_joint = 22; c.extra_size = 8; refused(c, "bad joint adjustment"); }
    { Case c; c.adjust_target = 22; c.extra_size = 8; refused(c, "bad joint adjustment"); }
    { Case c; c.extra_size = 8; c.with_z_tgt = false; refused(c, "dp_seq_lm_extra.struct_size"); }    // (a NULL z_tgt is not among the frames' refusals here)
    { Case c; c.extra_size = 40; c.with_z_tgt = false; refused(c, "dp_seq_lm_extra.struct_size"); }
    { Case c; c.extra_size = 5000; c.with_ar = true; c.ar_size = 8; refused(c, "dp_seq_lm_extra.struct_size"); }
    { Case c; c.extra_reserved0 = 9u; c.with_ar = true; c.ar_size = 8; refused(c, "reserved0 9"); }
    { Case c; c.with_ar = true; c.ar_size = 8; c.order = 0; refused(c, "dp_latent_ar.struct_size"); }
    { Case c; c.with_ar = true; c.ar_reserved0 = 1u; c.order = 0; refused(c, "reserved0 1"); }
    { Case c; c.with_ar = true; c.order = 0; c.null_coeffs = true; refused(c, "dp_latent_ar.order 0 outside"); }
    { Case c; c.with_ar = true; c.order = DP_MAX_AR_ORDER + 1; c.history = 2; refused(c, "dp_latent_ar.order 5 outside"); }
    { Case c; c.with_ar = true; c.null_coeffs = true; c.history = 1; refused(c, "coeffs or bias is NULL"); }
    { Case c; c.with_ar = true; c.order = 3; c.history = 2; refused(c, "shorter than dp_latent_ar.order 3"); }   // (with z_tgt given as well: the later fault)
    { Case c; c.with_ar = true; refused(c, "frames->z_tgt must be NULL"); }                                     // both
    { Case c; c.with_z_tgt = false; refused(c, "neither a predictor nor frames->z_tgt"); }                      // neither
    CHECK(dp_optimize_sequence_lm(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    CHECK(said(nullptr, "ctx is NULL"));
    w.done();
    return 0;
}
