// tests/lm_seq_terms_san/main.cpp -- dp_optimize_sequence_lm_terms (include/dragposer_sequence_lm_terms.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel
// unit) and walks the call's refusals, in the header's order, on a context without a device.  Every sized struct is handed over in a heap
// block of exactly struct_size bytes, and the table's 16 terms in a block of exactly 16 terms, so a read past what the caller owns is an
// error here.  Device pointers are constants that are never dereferenced.  Built and run by tests/test_host_san.py; every
// condition is exact.
#include "../../include/dragposer_sequence_lm_terms.h"
#include "../host_san/san_support.h"

namespace {

float* const GPOS = (float*)0x20000;  // ... for the state's global_pos
float* const OTHER = (float*)0x30000; // ... for a global position that is not the state's

struct Case { // what one call is made of; the defaults are well-formed: 16 terms of every type, some with per-frame rows stepped per frame
    dp_lm_params p = DP_LM_PARAMS_INIT;
    unsigned results_size = sizeof(dp_seq_results), results_reserved0 = 0u, extra_size = sizeof(dp_seq_lm_extra), extra_reserved0 = 0u,
             terms_size = sizeof(dp_terms), terms_reserved0 = 0u, tx_size = sizeof(dp_seq_extra), tx_reserved0 = 0u, ar_size = sizeof(dp_latent_ar),
             ar_reserved0 = 0u;
    bool null_latent = false, null_frames = false, null_params = false, null_terms = false, null_state = false, null_adjust = false,
         null_results = false, null_extra = false, null_tx = false, null_z_tgt = false, null_table = false, null_scratch = false, with_ar = false,
         tx_joint_pos = false, terms_loss = false;
    float* terms_gp = nullptr; // NULL or the state's
    int n_seq = 4, n_steps = 7, n_terms = DP_MAX_TERMS, up_axis = 1, bad_term = -1, bad_joint = 22, history = 4, ar_order = 2, bad_row_step = -1,
        adjust_joint = 0, height0 = 0;
    float bad_weight = 1.f;
};

int run(dp_ctx* ctx, const Case& c)
{
    dp_seq_frames f0{};
    f0.n_steps = c.n_steps;
    f0.tgt_pos = f0.tgt_rot = f0.tgt_root = f0.w = PTR; f0.tracked = (const unsigned char*)PTR;
    f0.z_tgt = c.null_z_tgt ? nullptr : PTR; f0.z_tgt_step = 96; f0.z_tgt_seq = 24;
    dp_seq_state s0{};
    s0.global_pos = GPOS; s0.global_rot = s0.latent_buf = s0.disp_buf = s0.heights_buf = PTR;
    s0.history = c.history; s0.n_heights = 2; s0.height_joints[0] = c.height0; s0.height_joints[1] = 4;
    dp_seq_step a0{};
    a0.adjust_joint = c.adjust_joint; a0.adjust_target_joint = 13; a0.adjust_weight = 0.5f;
    dp_seq_results r0 = DP_SEQ_RESULTS_INIT;
    r0.struct_size = c.results_size; r0.reserved0 = c.results_reserved0;
    r0.pose_ret = r0.pos_ret = r0.world_rot = r0.loss = PTR; r0.iters = r0.status = (int*)PTR;
    r0.hist_scratch = c.null_scratch ? nullptr : PTR;
    dp_seq_lm_extra e0 = DP_SEQ_LM_EXTRA_INIT;
    e0.struct_size = c.extra_size; e0.reserved0 = c.extra_reserved0;
    e0.mu = e0.mu_trace = e0.loss0 = e0.joint_pos = PTR; e0.n_accepted = (int*)PTR;
    dp_seq_extra x0 = DP_SEQ_EXTRA_INIT;
    x0.struct_size = c.tx_size; x0.reserved0 = c.tx_reserved0;
    x0.loss_terms = x0.loss_extra = PTR; // (loss_extra is ignored)
    x0.joint_pos = c.tx_joint_pos ? PTR : nullptr;
    for (int k = 0; k < DP_MAX_TERMS; ++k) x0.row_step[k] = k % 5 == 0 ? 16 : 0;
    if (c.bad_row_step >= 0) x0.row_step[c.bad_row_step] = -16;
    dp_latent_ar l0 = DP_LATENT_AR_INIT;
    l0.struct_size = c.ar_size; l0.reserved0 = c.ar_reserved0; l0.order = c.ar_order; l0.coeffs = l0.bias = PTR; l0.trace = PTR;
    const int n_alloc = c.n_terms > 0 && c.n_terms <= DP_MAX_TERMS ? c.n_terms : 1;
    dp_term* table = (dp_term*)std::malloc(sizeof(dp_term) * n_alloc); // exactly the terms the caller owns
    for (int k = 0; k < n_alloc; ++k) {
        dp_term t = DP_TERM_INIT;
        t.type = 1 + k % 3; t.joint_a = k; t.joint_b = t.type == DP_TERM_PLANE ? -1 : (k + 5) % 22; t.weight = 0.5f + k;
        t.flags = k % 4; t.p0 = 0.1f; t.p1 = 0.2f;
        if (k % 5 == 0) t.per_frame = PTR;
        if (k == c.bad_term) { t.joint_a = c.bad_joint; t.weight = c.bad_weight; }
        std::memcpy(table + k, &t, sizeof(t));
    }
    dp_terms t0 = DP_TERMS_INIT;
    t0.struct_size = c.terms_size; t0.reserved0 = c.terms_reserved0; t0.n_terms = c.n_terms; t0.up_axis = c.up_axis;
    t0.terms = c.null_table ? nullptr : table; t0.global_pos = c.terms_gp; t0.loss_terms = c.terms_loss ? PTR : nullptr;
    Exact<dp_seq_frames> f(f0);
    Exact<dp_seq_state> s(s0);
    Exact<dp_seq_step> a(a0);
    Exact<dp_lm_params> p(c.p, cut<dp_lm_params>(c.p.struct_size));
    Exact<dp_seq_results> r(r0, cut<dp_seq_results>(c.results_size));
    Exact<dp_seq_lm_extra> e(e0, cut<dp_seq_lm_extra>(c.extra_size));
    Exact<dp_seq_extra> x(x0, cut<dp_seq_extra>(c.tx_size));
    Exact<dp_latent_ar> l(l0, cut<dp_latent_ar>(c.ar_size));
    Exact<dp_terms> t(t0, cut<dp_terms>(c.terms_size));
    const int rc = dp_optimize_sequence_lm_terms(ctx, c.n_seq, c.null_latent ? nullptr : PTR, c.null_frames ? nullptr : f.get(), c.null_params ? nullptr : p.get(),
                                                 c.null_terms ? nullptr : t.get(), c.with_ar ? l.get() : nullptr, c.null_state ? nullptr : s.get(),
                                                 c.null_adjust ? nullptr : a.get(), c.null_results ? nullptr : r.get(), c.null_extra ? nullptr : e.get(),
                                                 c.null_tx ? nullptr : x.get(), nullptr);
    std::free(table);
    return rc;
}

} // namespace

int main()
{
    Walker w("lm_seq_terms", "dp_optimize_sequence_lm_terms");
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    const float nan = __builtin_nanf("");
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 8; ++variant) {
        Case c;
        if (variant == 1) c.null_extra = true;
        if (variant == 2) c.null_tx = true;
        if (variant == 3) { c.n_terms = 0; c.null_table = true; } // the empty table
        if (variant == 4) c.n_terms = 1;
        if (variant == 5) c.terms_gp = GPOS; // the state's own array is accepted
        if (variant == 6) { c.with_ar = true; c.null_z_tgt = true; }
        if (variant == 7) { c.null_adjust = true; c.n_seq = 1; c.n_steps = 1; }
        w.unsupported(run(w.ctx, c), "dp_lm_seq_terms.hip");
    }
    // the refusals in the header's order: each is reported before every later one's fault
    // 1. dp_optimize_sequence_lm's, up to and including dp_seq_lm_extra
    { Case c; c.n_seq = 0; c.p.struct_size = 4; refused(c, "n_sequences must be positive"); }
    { Case c; c.null_latent = true; c.p.n_steps = 0; refused(c, "NULL latent, frames, params, terms, state or results"); }
    { Case c; c.null_frames = true; c.n_terms = 17; refused(c, "NULL latent, frames, params, terms, state or results"); }
    { Case c; c.null_params = true; c.n_terms = 17; refused(c, "NULL latent, frames, params, terms, state or results"); }
    { Case c; c.null_terms = true; c.results_size = 8; refused(c, "NULL latent, frames, params, terms, state or results"); }
    { Case c; c.null_state = true; c.results_size = 8; refused(c, "NULL latent, frames, params, terms, state or results"); }
    { Case c; c.null_results = true; c.p.n_steps = 0; refused(c, "NULL latent, frames, params, terms, state or results"); }
    { Case c; c.p.struct_size = 4; c.results_size = 8; refused(c, "dp_lm_params.struct_size"); }
    { Case c; c.p.struct_size = 44; c.p.n_steps = 0; refused(c, "dp_lm_params.struct_size"); }
    { Case c; c.p.n_steps = 0; c.results_size = 8; refused(c, "n_steps 0 outside"); }
    { Case c; c.p.lambda_rot = nan; c.results_size = 8; refused(c, "lambda_rot or lambda_tmp"); }
    { Case c; c.p.mu_down = 1.f; c.results_size = 8; refused(c, "mu_down must lie in (0, 1)"); }
    { Case c; c.p.mu0 = 1e7f; c.results_size = 8; refused(c, "mu0 outside [mu_min, mu_max]"); }
    { Case c; c.results_size = 8; c.n_steps = 0; refused(c, "dp_seq_results.struct_size"); }
    { Case c; c.results_reserved0 = 2u; c.n_steps = 0; refused(c, "reserved0"); }
    { Case c; c.n_steps = 0; c.null_scratch = true; refused(c, "n_steps must be positive"); }
    { Case c; c.null_scratch = true; c.history = 0; refused(c, "NULL state array / hist_scratch"); }
    { Case c; c.history = 0; c.height0 = 22; refused(c, "history / n_heights out of range"); }
    { Case c; c.height0 = 22; c.adjust_joint = 22; refused(c, "bad height joint"); }
    { Case c; c.adjust_joint = 22; c.extra_size = 8; refused(c, "bad joint adjustment"); }
    { Case c; c.extra_size = 8; c.terms_size = 8; refused(c, "dp_seq_lm_extra.struct_size"); }
    { Case c; c.extra_size = 40; c.n_terms = 17; refused(c, "dp_seq_lm_extra.struct_size"); }
    { Case c; c.extra_reserved0 = 7u; c.n_terms = 17; refused(c, "reserved0"); }
    // 2. dp_terms and its table
    { Case c; c.terms_size = 8; c.tx_size = 8; refused(c, "dp_terms"); }
    { Case c; c.terms_size = 5000; c.tx_size = 8; refused(c, "dp_terms"); }
    { Case c; c.terms_reserved0 = 3u; c.tx_size = 8; refused(c, "reserved0"); }
    { Case c; c.terms_gp = OTHER; c.terms_loss = true; refused(c, "dp_terms.global_pos must be NULL or dp_seq_state.global_pos"); }
    { Case c; c.terms_loss = true; c.n_terms = 17; refused(c, "dp_terms.loss_terms is one row per frame; a sequence launch writes dp_seq_extra.loss_terms"); }
    { Case c; c.n_terms = 17; c.tx_size = 8; refused(c, "n_terms 17 outside 0..16"); }
    { Case c; c.n_terms = -1; c.tx_size = 8; refused(c, "n_terms -1 outside 0..16"); }
    { Case c; c.null_table = true; c.up_axis = 3; refused(c, "NULL terms with n_terms > 0"); }
    { Case c; c.up_axis = 3; c.bad_term = 0; refused(c, "up_axis outside 0..2"); }
    { Case c; c.bad_term = 15; c.bad_row_step = 0; refused(c, "term 15: joint_a 22 outside 0..21"); }
    { Case c; c.bad_term = 7; c.bad_joint = 7; c.bad_weight = nan; c.tx_joint_pos = true; refused(c, "term 7: the weight is negative or not finite"); }
    // 3. dp_seq_extra
    { Case c; c.tx_size = 8; c.with_ar = true; c.ar_size = 8; refused(c, "dp_seq_extra"); }
    { Case c; c.tx_size = 5000; c.with_ar = true; c.ar_size = 8; refused(c, "dp_seq_extra"); }
    { Case c; c.tx_reserved0 = 9u; c.with_ar = true; c.ar_order = 0; refused(c, "reserved0"); }
    { Case c; c.bad_row_step = 15; c.tx_joint_pos = true; refused(c, "dp_seq_extra.row_step[15] is negative"); }
    { Case c; c.bad_row_step = 0; c.null_z_tgt = true; refused(c, "dp_seq_extra.row_step[0] is negative"); }
    { Case c; c.tx_joint_pos = true; c.with_ar = true; c.ar_order = 0; refused(c, "dp_seq_lm_extra.joint_pos"); }
    { Case c; c.tx_joint_pos = true; c.null_z_tgt = true; refused(c, "dp_seq_extra.joint_pos must be NULL here"); }
    // 4. the predictor
    { Case c; c.with_ar = true; c.ar_size = 8; c.ar_order = 0; refused(c, "dp_latent_ar.struct_size"); }
    { Case c; c.with_ar = true; c.ar_reserved0 = 1u; c.ar_order = 0; refused(c, "reserved0"); }
    { Case c; c.with_ar = true; c.ar_order = 5; c.history = 2; refused(c, "dp_latent_ar.order 5 outside 1..4"); }
    { Case c; c.with_ar = true; c.ar_order = 3; c.history = 2; refused(c, "shorter than dp_latent_ar.order 3"); }
    { Case c; c.with_ar = true; refused(c, "frames->z_tgt must be NULL"); }          // both
    { Case c; c.null_z_tgt = true; refused(c, "neither a predictor nor frames->z_tgt"); } // neither
    CHECK(dp_optimize_sequence_lm_terms(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
