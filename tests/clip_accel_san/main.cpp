// tests/clip_accel_san/main.cpp -- dp_optimize_clip_lm_accel (include/dragposer_clip_accel.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel
// unit) and walks the call's refusals, in the header's order, on a context without a device.  Every sized struct is handed over in a heap
// block of exactly struct_size bytes, so a read past what the caller owns is an error here.  Device pointers are a constant that is never
// dereferenced.  Built and run by tests/test_clip_accel_san.py; every condition is exact.
#include "../../include/dragposer_clip_accel.h"
#include "../host_san/san_support.h"

namespace {

struct Case { // what one call is made of; the defaults are well-formed
    dp_clip_lm_params p = DP_CLIP_LM_PARAMS_INIT;
    dp_clip_accel_params a = DP_CLIP_ACCEL_PARAMS_INIT;
    unsigned result_size = sizeof(dp_result), extra_size = sizeof(dp_clip_lm_extra), extra_reserved0 = 0u;
    bool null_batch = false, null_params = false, null_accel = false, null_result = false, null_extra = false, with_outputs = true,
         null_z_tgt = false, null_workspace = false;
    int n_frames = 6, n_sequences = 2;
    long long workspace_short = 0; // bytes the workspace is short of dp_clip_lm_accel_workspace_bytes(n_sequences, n_frames)
    Case() { a.lambda_accel = 5.f; }
};

int run(dp_ctx* ctx, const Case& c)
{
    dp_batch b0{};
    b0.n_frames = c.n_frames;
    b0.z0 = b0.cur_rot = b0.tgt_pos = b0.tgt_rot = b0.w = PTR; b0.tracked = (const unsigned char*)PTR;
    b0.z_tgt = c.null_z_tgt ? nullptr : PTR;
    dp_result r0 = DP_RESULT_INIT;
    r0.struct_size = c.result_size;
    if (c.with_outputs) { r0.z = r0.z_pre = r0.pose = r0.pos = r0.loss = PTR; r0.iters = r0.status = (int*)PTR; }
    dp_clip_lm_extra e0 = DP_CLIP_LM_EXTRA_INIT;
    e0.struct_size = c.extra_size; e0.reserved0 = c.extra_reserved0;
    if (c.with_outputs) { e0.mu = PTR; e0.n_accepted = e0.info = (int*)PTR; e0.clip_loss = e0.loss_hist = (double*)PTR; }
    e0.workspace = c.null_workspace ? nullptr : (void*)PTR;
    e0.workspace_bytes = (size_t)((long long)dp_clip_lm_accel_workspace_bytes(c.n_sequences, c.n_frames) - c.workspace_short);
    dp_clip_accel_params a0 = c.a;
    if (c.with_outputs) a0.accel_loss = (double*)PTR;
    Exact<dp_batch> b(b0);
    Exact<dp_clip_lm_params> p(c.p, cut<dp_clip_lm_params>(c.p.struct_size));
    Exact<dp_clip_accel_params> a(a0, cut<dp_clip_accel_params>(c.a.struct_size));
    Exact<dp_result> r(r0, cut<dp_result>(c.result_size));
    Exact<dp_clip_lm_extra> e(e0, cut<dp_clip_lm_extra>(c.extra_size));
    return dp_optimize_clip_lm_accel(ctx, c.null_batch ? nullptr : b.get(), c.n_sequences, c.null_params ? nullptr : p.get(),
                                     c.null_accel ? nullptr : a.get(), c.null_result ? nullptr : r.get(), c.null_extra ? nullptr : e.get(), nullptr);
}

} // namespace

int main()
{
    Walker w("clip_accel", "dp_optimize_clip_lm_accel");
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    const auto ws = dp_clip_lm_accel_workspace_bytes;
    CHECK(ws(0, 6) == 0 && ws(2, 0) == 0 && ws(-1, -1) == 0);
    CHECK(ws(4, 6) == 0); // (4 does not divide 6)
    CHECK(ws(2, 6) > 0 && ws(2, 6) % 16 == 0);
    CHECK(ws(2, 8) > ws(2, 6) && ws(1, 5052) > ws(1, 240));
    CHECK(ws(2, 6) > dp_clip_lm_workspace_bytes(2, 6)); // (the wider factor block)
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 8; ++variant) {
        Case c;
        if (variant == 1) c.null_result = true;   // no result wanted
        if (variant == 2) c.with_outputs = false; // every optional pointer NULL
        if (variant == 3) { c.p.n_steps = DP_LM_MAX_STEPS; c.p.mu0 = c.p.mu_min; c.p.lambda_smooth = 0.f; }
        if (variant == 4) { c.p.mu_min = c.p.mu_max = c.p.mu0 = 1.f; c.p.lambda_rot = 0.f; c.p.lambda_tmp = 0.f; }
        if (variant == 5) { c.n_sequences = 1; c.n_frames = 5052; }
        if (variant == 6) { c.n_sequences = 6; c.workspace_short = -4096; } // T = 1, a workspace larger than asked for
        if (variant == 7) c.a.lambda_accel = 0.f;                           // (dp_optimize_clip_lm's train: the same unit launches it)
        w.unsupported(run(w.ctx, c), "dp_clip_accel.hip");
    }
    // the refusals in the header's order: each is reported before every later one's fault
    { Case c; c.null_batch = true; c.p.n_steps = 0; refused(c, "NULL batch, params or extra"); }
    { Case c; c.null_params = true; c.null_accel = true; refused(c, "NULL batch, params or extra"); }
    { Case c; c.null_extra = true; c.n_sequences = 0; refused(c, "NULL batch, params or extra"); }
    { Case c; c.p.struct_size = 4; c.result_size = 8; refused(c, "dp_clip_lm_params.struct_size"); } // a block of 4 bytes: only the size word exists
    { Case c; c.p.struct_size = 36; c.a.struct_size = 4; refused(c, "dp_clip_lm_params.struct_size"); }
    { Case c; c.p.struct_size = 5000; refused(c, "dp_clip_lm_params.struct_size"); }
    { Case c; c.result_size = 8; c.extra_size = 8; refused(c, "dp_result.struct_size"); }
    { Case c; c.extra_size = 8; c.p.n_steps = 0; refused(c, "dp_clip_lm_extra.struct_size"); }
    { Case c; c.extra_size = 5000; refused(c, "dp_clip_lm_extra.struct_size"); }
    { Case c; c.extra_reserved0 = 7u; c.p.n_steps = 0; refused(c, "reserved0 7"); }
    { Case c; c.p.n_steps = 0; c.p.lambda_rot = nan; refused(c, "n_steps 0 outside"); }
    { Case c; c.p.n_steps = DP_LM_MAX_STEPS + 1; c.a.lambda_accel = nan; refused(c, "n_steps 65 outside"); }
    { Case c; c.p.lambda_rot = nan; c.p.mu_down = 2.f; refused(c, "lambda_rot or lambda_tmp"); }
    { Case c; c.p.mu0 = nan; c.p.mu_down = 2.f; refused(c, "is not finite"); }
    { Case c; c.p.mu_down = 1.f; c.p.mu_up = 1.f; refused(c, "mu_down must lie in (0, 1)"); }
    { Case c; c.p.mu_up = 1.f; c.p.mu_min = 2.f; refused(c, "mu_up must be greater than 1"); }
    { Case c; c.p.mu_min = 2.f; c.p.mu_max = 1.f; c.p.mu0 = 5.f; refused(c, "0 < mu_min <= mu_max"); }
    { Case c; c.p.mu0 = 1e7f; c.n_frames = 0; refused(c, "mu0 outside [mu_min, mu_max]"); }
    { Case c; c.n_frames = 0; c.n_sequences = 0; refused(c, "n_frames must be positive"); }
    { Case c; c.null_z_tgt = true; c.n_sequences = 4; refused(c, "NULL input array"); }
    { Case c; c.n_sequences = 0; c.p.lambda_smooth = nan; refused(c, "n_sequences 0 must be positive and divide n_frames 6"); }
    { Case c; c.n_sequences = 4; c.null_accel = true; refused(c, "n_sequences 4 must be positive and divide n_frames 6"); }
    { Case c; c.p.lambda_smooth = nan; c.null_accel = true; refused(c, "lambda_smooth is negative or not finite"); }
    { Case c; c.p.lambda_smooth = -0.5f; c.a.struct_size = 4; refused(c, "lambda_smooth is negative or not finite"); }
    { Case c; c.null_accel = true; c.null_workspace = true; refused(c, "dp_clip_accel_params is NULL"); }
    { Case c; c.a.struct_size = 4; c.a.lambda_accel = nan; refused(c, "dp_clip_accel_params.struct_size is 4"); } // a block of 4 bytes: only the size word exists
    { Case c; c.a.struct_size = 8; c.workspace_short = 1; refused(c, "dp_clip_accel_params.struct_size is 8"); }
    { Case c; c.a.struct_size = 5000; refused(c, "dp_clip_accel_params.struct_size is 5000"); }
    { Case c; c.a.lambda_accel = nan; c.null_workspace = true; refused(c, "lambda_accel is negative or not finite"); }
    { Case c; c.a.lambda_accel = -0.5f; c.workspace_short = 1; refused(c, "lambda_accel is negative or not finite"); }
    { Case c; c.a.lambda_accel = inf; refused(c, "lambda_accel is negative or not finite"); }
    { Case c; c.null_workspace = true; refused(c, "workspace is NULL"); }
    { Case c; c.workspace_short = 1; refused(c, "fewer than the"); }
    { Case c; c.workspace_short = 16; c.n_sequences = 1; c.n_frames = 5052; refused(c, "of dp_clip_lm_accel_workspace_bytes(1, 5052)"); }
    { Case c; c.workspace_short = (long long)(ws(2, 6) - dp_clip_lm_workspace_bytes(2, 6)); refused(c, "fewer than the"); } // (dp_optimize_clip_lm's size is short here)
    { Case c; c.a.lambda_accel = 0.f; c.workspace_short = 1; refused(c, "fewer than the"); } // (lambda_accel 0 asks for the same workspace)
    { Case c; c.workspace_short = (long long)ws(2, 6); refused(c, "holds 0 bytes"); }
    CHECK(dp_optimize_clip_lm_accel(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
