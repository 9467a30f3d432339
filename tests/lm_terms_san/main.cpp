// tests/lm_terms_san/main.cpp -- dp_optimize_lm_terms (include/dragposer_lm_terms.h) under AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel unit) and walks the call's
// refusals, in the header's order, on a context without a device.  Every sized struct is handed over in a heap block of exactly struct_size
// bytes, and the table's 16 terms in a block of exactly 16 terms, so a read past what the caller owns is an error here.  Device pointers are
// a constant that is never dereferenced.  Built and run by tests/test_host_san.py; every condition is exact.
#include "../../include/dragposer_lm_terms.h"
#include "../host_san/san_support.h"

namespace {

struct Case { // what one call is made of; the defaults are well-formed: 16 terms of every type, some with per-frame rows
    dp_lm_params p = DP_LM_PARAMS_INIT;
    unsigned result_size = sizeof(dp_result), extra_size = sizeof(dp_lm_extra), extra_reserved0 = 0u, terms_size = sizeof(dp_terms), terms_reserved0 = 0u;
    bool null_batch = false, null_params = false, null_terms = false, null_result = false, null_extra = false, null_z_tgt = false, null_table = false,
         null_gp = false;
    int n_frames = 4, n_terms = DP_MAX_TERMS, up_axis = 1, bad_term = -1, bad_joint = 22;
    float bad_weight = 1.f;
};

int run(dp_ctx* ctx, const Case& c)
{
    dp_batch b0{};
    b0.n_frames = c.n_frames;
    b0.z0 = b0.cur_rot = b0.tgt_pos = b0.tgt_rot = b0.w = PTR; b0.tracked = (const unsigned char*)PTR;
    b0.z_tgt = c.null_z_tgt ? nullptr : PTR;
    dp_result r0 = DP_RESULT_INIT;
    r0.struct_size = c.result_size;
    r0.z = r0.pose = r0.pos = r0.loss = PTR; r0.iters = r0.status = (int*)PTR;
    dp_lm_extra e0 = DP_LM_EXTRA_INIT;
    e0.struct_size = c.extra_size; e0.reserved0 = c.extra_reserved0;
    e0.mu = e0.loss0 = PTR; e0.n_accepted = (int*)PTR;
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
    t0.terms = c.null_table ? nullptr : table; t0.global_pos = c.null_gp ? nullptr : PTR; t0.loss_terms = PTR;
    Exact<dp_batch> b(b0);
    Exact<dp_lm_params> p(c.p, cut<dp_lm_params>(c.p.struct_size));
    Exact<dp_result> r(r0, cut<dp_result>(c.result_size));
    Exact<dp_lm_extra> e(e0, cut<dp_lm_extra>(c.extra_size));
    Exact<dp_terms> t(t0, cut<dp_terms>(c.terms_size));
    const int rc = dp_optimize_lm_terms(ctx, c.null_batch ? nullptr : b.get(), c.null_params ? nullptr : p.get(), c.null_terms ? nullptr : t.get(),
                                        c.null_result ? nullptr : r.get(), c.null_extra ? nullptr : e.get(), nullptr);
    std::free(table);
    return rc;
}

} // namespace

int main()
{
    Walker w("lm_terms", "dp_optimize_lm_terms");
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    const float nan = __builtin_nanf("");
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 5; ++variant) {
        Case c;
        if (variant == 1) c.null_extra = true;
        if (variant == 2) c.null_result = true;
        if (variant == 3) { c.n_terms = 0; c.null_table = true; c.null_gp = true; } // the empty table
        if (variant == 4) c.n_terms = 1;
        w.unsupported(run(w.ctx, c), "dp_lm_terms.hip");
    }
    // the refusals in the header's order: each is reported before every later one's fault
    { Case c; c.null_batch = true; c.p.n_steps = 0; refused(c, "NULL batch, params or terms"); }
    { Case c; c.null_params = true; c.n_terms = 17; refused(c, "NULL batch, params or terms"); }
    { Case c; c.null_terms = true; c.result_size = 8; refused(c, "NULL batch, params or terms"); }
    { Case c; c.p.struct_size = 4; c.result_size = 8; refused(c, "dp_lm_params.struct_size"); }
    { Case c; c.p.struct_size = 44; c.n_terms = 17; refused(c, "dp_lm_params.struct_size"); }
    { Case c; c.result_size = 8; c.extra_size = 8; refused(c, "dp_result.struct_size"); }
    { Case c; c.extra_size = 8; c.terms_size = 8; refused(c, "dp_lm_extra.struct_size"); }
    { Case c; c.extra_reserved0 = 7u; c.n_terms = 17; refused(c, "reserved0"); }
    { Case c; c.terms_size = 8; c.p.n_steps = 0; refused(c, "dp_terms"); }
    { Case c; c.terms_size = 5000; c.p.n_steps = 0; refused(c, "dp_terms"); }
    { Case c; c.terms_reserved0 = 3u; c.p.n_steps = 0; refused(c, "reserved0"); }
    { Case c; c.n_terms = 17; c.p.n_steps = 0; refused(c, "n_terms 17 outside 0..16"); }
    { Case c; c.n_terms = -1; c.p.n_steps = 0; refused(c, "n_terms -1 outside 0..16"); }
    { Case c; c.null_table = true; c.up_axis = 3; refused(c, "NULL terms with n_terms > 0"); }
    { Case c; c.up_axis = 3; c.bad_term = 0; refused(c, "up_axis outside 0..2"); }
    { Case c; c.bad_term = 15; c.p.n_steps = 0; refused(c, "term 15: joint_a 22 outside 0..21"); }
    { Case c; c.bad_term = 7; c.bad_joint = 7; c.bad_weight = nan; c.null_gp = true; refused(c, "term 7: the weight is negative or not finite"); }
    { Case c; c.null_gp = true; c.p.n_steps = 0; refused(c, "global_pos is NULL while an active PLANE"); }
    { Case c; c.p.n_steps = 0; c.n_frames = 0; refused(c, "n_steps 0 outside"); }
    { Case c; c.p.lambda_rot = nan; c.n_frames = 0; refused(c, "lambda_rot or lambda_tmp"); }
    { Case c; c.p.mu_down = 1.f; c.n_frames = 0; refused(c, "mu_down must lie in (0, 1)"); }
    { Case c; c.p.mu0 = 1e7f; c.n_frames = 0; refused(c, "mu0 outside [mu_min, mu_max]"); }
    { Case c; c.n_frames = 0; c.null_z_tgt = true; refused(c, "n_frames must be positive"); }
    { Case c; c.null_z_tgt = true; refused(c, "NULL input array"); }
    CHECK(dp_optimize_lm_terms(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
