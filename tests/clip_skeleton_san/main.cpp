// tests/clip_skeleton_san/main.cpp -- dp_optimize_clip_lm_skeleton and dp_optimize_lm_skeleton (include/dragposer_clip_skeleton.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP
// runtime, no kernel unit) and walks the two calls' refusals, in the header's order, on a context without a device.  Every sized struct is
// handed over in a heap block of exactly struct_size bytes, so a read past what the caller owns is an error here.  Device pointers are a
// constant that is never dereferenced.  Built and run by tests/test_clip_skeleton_san.py; every condition is exact.
#include "../../include/dragposer_clip_skeleton.h"
#include "../host_san/san_support.h"

namespace {

struct Case { // what one call is made of; the defaults are well-formed
    dp_clip_lm_params p = DP_CLIP_LM_PARAMS_INIT;
    dp_lm_params lp = DP_LM_PARAMS_INIT;
    dp_clip_accel_params a = DP_CLIP_ACCEL_PARAMS_INIT;
    dp_skeleton_in s = DP_SKELETON_IN_INIT;
    unsigned result_size = sizeof(dp_result), extra_size = sizeof(dp_clip_lm_extra), extra_reserved0 = 0u, lm_extra_size = sizeof(dp_lm_extra);
    bool null_batch = false, null_params = false, null_accel = false, null_skel = false, null_offsets = false, null_result = false,
         null_extra = false, with_outputs = true, null_z_tgt = false, null_workspace = false;
    int n_frames = 6, n_sequences = 2;
    long long workspace_short = 0; // bytes the workspace is short of the size function of the form chosen
    Case() { a.lambda_accel = 5.f; s.stride = DP_SKELETON_STRIDE; }
};

dp_batch batch_of(const Case& c)
{
    dp_batch b0{};
    b0.n_frames = c.n_frames;
    b0.z0 = b0.cur_rot = b0.tgt_pos = b0.tgt_rot = b0.w = PTR; b0.tracked = (const unsigned char*)PTR;
    b0.z_tgt = c.null_z_tgt ? nullptr : PTR;
    return b0;
}
dp_result result_of(const Case& c)
{
    dp_result r0 = DP_RESULT_INIT;
    r0.struct_size = c.result_size;
    if (c.with_outputs) { r0.z = r0.z_pre = r0.pose = r0.pos = r0.loss = PTR; r0.iters = r0.status = (int*)PTR; }
    return r0;
}
dp_skeleton_in skel_of(const Case& c)
{
    dp_skeleton_in s0 = c.s;
    s0.offsets = c.null_offsets ? nullptr : PTR;
    return s0;
}

int run_clip(dp_ctx* ctx, const Case& c)
{
    dp_clip_lm_extra e0 = DP_CLIP_LM_EXTRA_INIT;
    e0.struct_size = c.extra_size; e0.reserved0 = c.extra_reserved0;
    if (c.with_outputs) { e0.mu = PTR; e0.n_accepted = e0.info = (int*)PTR; e0.clip_loss = e0.loss_hist = (double*)PTR; }
    e0.workspace = c.null_workspace ? nullptr : (void*)PTR;
    const size_t need = c.null_accel ? dp_clip_lm_workspace_bytes(c.n_sequences, c.n_frames) : dp_clip_lm_accel_workspace_bytes(c.n_sequences, c.n_frames);
    e0.workspace_bytes = (size_t)((long long)need - c.workspace_short);
    dp_clip_accel_params a0 = c.a;
    if (c.with_outputs) a0.accel_loss = (double*)PTR;
    Exact<dp_batch> b(batch_of(c));
    Exact<dp_clip_lm_params> p(c.p, cut<dp_clip_lm_params>(c.p.struct_size));
    Exact<dp_clip_accel_params> a(a0, cut<dp_clip_accel_params>(c.a.struct_size));
    Exact<dp_skeleton_in> s(skel_of(c), cut<dp_skeleton_in>(c.s.struct_size));
    Exact<dp_result> r(result_of(c), cut<dp_result>(c.result_size));
    Exact<dp_clip_lm_extra> e(e0, cut<dp_clip_lm_extra>(c.extra_size));
    return dp_optimize_clip_lm_skeleton(ctx, c.null_batch ? nullptr : b.get(), c.n_sequences, c.null_params ? nullptr : p.get(), c.null_accel ? nullptr : a.get(),
                                        c.null_skel ? nullptr : s.get(), c.null_result ? nullptr : r.get(), c.null_extra ? nullptr : e.get(), nullptr);
}

int run_lm(dp_ctx* ctx, const Case& c)
{
    dp_lm_extra e0 = DP_LM_EXTRA_INIT;
    e0.struct_size = c.lm_extra_size; e0.reserved0 = c.extra_reserved0;
    if (c.with_outputs) { e0.mu = e0.loss0 = PTR; e0.n_accepted = (int*)PTR; }
    Exact<dp_batch> b(batch_of(c));
    Exact<dp_lm_params> p(c.lp, cut<dp_lm_params>(c.lp.struct_size));
    Exact<dp_skeleton_in> s(skel_of(c), cut<dp_skeleton_in>(c.s.struct_size));
    Exact<dp_result> r(result_of(c), cut<dp_result>(c.result_size));
    Exact<dp_lm_extra> e(e0, cut<dp_lm_extra>(c.lm_extra_size));
    return dp_optimize_lm_skeleton(ctx, c.null_batch ? nullptr : b.get(), c.null_params ? nullptr : p.get(), c.null_skel ? nullptr : s.get(),
                                   c.null_result ? nullptr : r.get(), c.null_extra ? nullptr : e.get(), nullptr);
}

} // namespace

int main()
{
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    {
        Walker w("clip_skeleton", "dp_optimize_clip_lm_skeleton");
        const auto refused = [&](const Case& c, const char* word) { w.refused(run_clip(w.ctx, c), word); };
        // well-formed, both forms, both strides: this link has no kernel unit, which the library says after every argument check
        for (int variant = 0; variant < 10; ++variant) {
            Case c;
            if (variant == 1) c.null_accel = true; // dp_optimize_clip_lm's problem and workspace
            if (variant == 2) { c.null_accel = true; c.s.stride = 0; }
            if (variant == 3) c.s.stride = 0;
            if (variant == 4) c.null_result = true;
            if (variant == 5) c.with_outputs = false;
            if (variant == 6) { c.n_sequences = 1; c.n_frames = 5052; }
            if (variant == 7) { c.n_sequences = 6; c.workspace_short = -4096; }
            if (variant == 8) c.a.lambda_accel = 0.f;
            if (variant == 9) { c.null_accel = true; c.p.n_steps = DP_LM_MAX_STEPS; c.p.lambda_smooth = 0.f; }
            w.unsupported(run_clip(w.ctx, c), "dp_clip_skel.hip");
        }
        // the plain calls' own refusals first, in their order, each before every later one's fault
        { Case c; c.null_batch = true; c.null_skel = true; refused(c, "NULL batch, params or extra"); }
        { Case c; c.null_params = true; c.s.struct_size = 4; refused(c, "NULL batch, params or extra"); }
        { Case c; c.null_extra = true; c.null_skel = true; refused(c, "NULL batch, params or extra"); }
        { Case c; c.p.struct_size = 4; c.s.struct_size = 4; refused(c, "dp_clip_lm_params.struct_size"); }
        { Case c; c.result_size = 8; c.null_skel = true; refused(c, "dp_result.struct_size"); }
        { Case c; c.extra_size = 8; c.null_skel = true; refused(c, "dp_clip_lm_extra.struct_size"); }
        { Case c; c.extra_reserved0 = 7u; c.s.reserved0 = 3u; refused(c, "reserved0 7"); }
        { Case c; c.p.n_steps = 0; c.null_skel = true; refused(c, "n_steps 0 outside"); }
        { Case c; c.p.lambda_rot = nan; c.s.stride = 5; refused(c, "lambda_rot or lambda_tmp"); }
        { Case c; c.p.mu0 = 1e7f; c.null_skel = true; refused(c, "mu0 outside [mu_min, mu_max]"); }
        { Case c; c.n_frames = 0; c.null_skel = true; refused(c, "n_frames must be positive"); }
        { Case c; c.null_z_tgt = true; c.null_offsets = true; refused(c, "NULL input array"); }
        { Case c; c.n_sequences = 4; c.null_skel = true; refused(c, "n_sequences 4 must be positive and divide n_frames 6"); }
        { Case c; c.p.lambda_smooth = -0.5f; c.null_skel = true; refused(c, "lambda_smooth is negative or not finite"); }
        { Case c; c.a.struct_size = 4; c.null_skel = true; refused(c, "dp_clip_accel_params.struct_size is 4"); } // a block of 4 bytes: only the size word exists
        { Case c; c.a.struct_size = 5000; c.s.struct_size = 4; refused(c, "dp_clip_accel_params.struct_size is 5000"); }
        { Case c; c.a.lambda_accel = nan; c.null_skel = true; refused(c, "lambda_accel is negative or not finite"); }
        { Case c; c.a.lambda_accel = inf; c.s.stride = 5; refused(c, "lambda_accel is negative or not finite"); }
        // ... then dp_skeleton_in's, as dp_optimize_skeleton states them, each before the workspace's
        { Case c; c.null_skel = true; c.null_workspace = true; refused(c, "the skeleton is NULL"); }
        { Case c; c.null_skel = true; c.null_accel = true; c.workspace_short = 1; refused(c, "the skeleton is NULL"); }
        { Case c; c.s.struct_size = 8; c.null_workspace = true; refused(c, "dp_skeleton_in.struct_size is 8"); } // the size word and reserved0 exist, no more
        { Case c; c.s.struct_size = 5000; c.null_offsets = true; refused(c, "dp_skeleton_in.struct_size"); }
        { Case c; c.s.reserved0 = 3u; c.null_offsets = true; refused(c, "reserved0 3"); }
        { Case c; c.null_offsets = true; c.s.stride = 5; refused(c, "dp_skeleton_in.offsets is NULL"); }
        { Case c; c.s.stride = 5; c.null_workspace = true; refused(c, "dp_skeleton_in.stride is 5"); }
        { Case c; c.s.stride = 22; c.workspace_short = 1; refused(c, "dp_skeleton_in.stride is 22"); }
        { Case c; c.s.stride = -66; c.null_accel = true; refused(c, "dp_skeleton_in.stride is -66"); }
        // ... then the workspace, against the size function of the form chosen
        { Case c; c.null_workspace = true; refused(c, "workspace is NULL"); }
        { Case c; c.workspace_short = 1; refused(c, "of dp_clip_lm_accel_workspace_bytes(2, 6)"); }
        { Case c; c.null_accel = true; c.workspace_short = 1; refused(c, "of dp_clip_lm_workspace_bytes(2, 6)"); }
        { Case c; c.workspace_short = (long long)(dp_clip_lm_accel_workspace_bytes(2, 6) - dp_clip_lm_workspace_bytes(2, 6)); refused(c, "fewer than the"); }
        { Case c; c.a.lambda_accel = 0.f; c.workspace_short = 1; refused(c, "of dp_clip_lm_accel_workspace_bytes(2, 6)"); } // (one size per form)
        { Case c; c.null_accel = true; c.workspace_short = (long long)dp_clip_lm_workspace_bytes(2, 6); refused(c, "holds 0 bytes"); }
        CHECK(dp_optimize_clip_lm_skeleton(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
        w.done();
    }
    {
        Walker w("lm_skeleton", "dp_optimize_lm_skeleton");
        const auto refused = [&](const Case& c, const char* word) { w.refused(run_lm(w.ctx, c), word); };
        for (int variant = 0; variant < 6; ++variant) {
            Case c;
            if (variant == 1) c.s.stride = 0;
            if (variant == 2) c.null_result = true;
            if (variant == 3) c.with_outputs = false;
            if (variant == 4) c.null_extra = true; // (dp_lm_extra may be NULL)
            if (variant == 5) { c.n_frames = 1; c.lp.n_steps = DP_LM_MAX_STEPS; c.lp.early_stop = 1; }
            w.unsupported(run_lm(w.ctx, c), "dp_lm_skel.hip");
        }
        // dp_optimize_lm's refusals, all of them, then dp_skeleton_in's
        { Case c; c.null_batch = true; c.null_skel = true; refused(c, "NULL batch or params"); }
        { Case c; c.null_params = true; c.null_skel = true; refused(c, "NULL batch or params"); }
        { Case c; c.lp.struct_size = 4; c.null_skel = true; refused(c, "dp_lm_params.struct_size"); } // only the size word exists
        { Case c; c.result_size = 8; c.s.struct_size = 4; refused(c, "dp_result.struct_size"); }
        { Case c; c.lm_extra_size = 8; c.null_skel = true; refused(c, "dp_lm_extra.struct_size"); }
        { Case c; c.extra_reserved0 = 7u; c.s.reserved0 = 3u; refused(c, "reserved0 7"); }
        { Case c; c.lp.n_steps = 0; c.null_skel = true; refused(c, "n_steps 0 outside"); }
        { Case c; c.lp.lambda_tmp = -1.f; c.s.stride = 5; refused(c, "lambda_rot or lambda_tmp"); }
        { Case c; c.lp.stop_eps_pos = inf; c.null_offsets = true; refused(c, "is not finite"); }
        { Case c; c.lp.mu_up = 1.f; c.null_skel = true; refused(c, "mu_up must be greater than 1"); }
        { Case c; c.n_frames = 0; c.null_skel = true; refused(c, "n_frames must be positive"); }
        { Case c; c.null_z_tgt = true; c.s.stride = 5; refused(c, "NULL input array"); }
        { Case c; c.null_skel = true; refused(c, "the skeleton is NULL"); }
        { Case c; c.s.struct_size = 8; refused(c, "dp_skeleton_in.struct_size is 8"); } // the size word and reserved0 exist, no more
        { Case c; c.s.struct_size = 5000; c.null_offsets = true; refused(c, "dp_skeleton_in.struct_size"); }
        { Case c; c.s.reserved0 = 3u; c.null_offsets = true; refused(c, "reserved0 3"); }
        { Case c; c.null_offsets = true; c.s.stride = 5; refused(c, "dp_skeleton_in.offsets is NULL"); }
        { Case c; c.s.stride = 5; refused(c, "dp_skeleton_in.stride is 5"); }
        { Case c; c.s.stride = 132; refused(c, "dp_skeleton_in.stride is 132"); }
        CHECK(dp_optimize_lm_skeleton(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
        w.done();
    }
    return 0;
}
