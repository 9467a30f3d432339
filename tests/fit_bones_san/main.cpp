// tests/fit_bones_san/main.cpp -- dp_fit_bones (include/dragposer_calibration.h) under AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel unit) and walks the call's
// refusals, in the header's order, on a context without a device.  Every sized struct is handed over in a heap block of exactly struct_size
// bytes and `groups` / `base` / `prior` in blocks of exactly 22 ints / 66 floats / K floats, so a read past what the caller owns is an
// error here.  Device pointers are a constant that is never dereferenced.  Built and run by tests/test_host_san.py; every condition
// is exact.
#include "../../include/dragposer_calibration.h"
#include "../host_san/san_support.h"

namespace {

struct Case { // what one call is made of; the defaults are well-formed
    int K = 3, n_frames = 9;
    int groups[22] = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2};
    float ridge = 1.0e-3f, base_at_7 = 0.25f, prior_at_1 = 1.f;
    unsigned fit_size = sizeof(dp_bone_fit), fit_reserved0 = 0u, result_size = sizeof(dp_bone_fit_result), result_reserved0 = 0u;
    bool null_batch = false, null_fit = false, null_result = false, null_scales = false, null_groups = false, with_base = true, with_prior = true,
         with_outputs = true, null_workspace = false, null_z0 = false, null_unread = false;
    long long workspace_short = 0; // bytes the workspace is short of dp_fit_bones_workspace_bytes(n_frames)
};

int run(dp_ctx* ctx, const Case& c)
{
    dp_batch b0{};
    b0.n_frames = c.n_frames;
    b0.z0 = c.null_z0 ? nullptr : PTR;
    b0.cur_rot = b0.tgt_pos = b0.w = PTR; b0.tracked = (const unsigned char*)PTR;
    b0.z_tgt = b0.tgt_rot = c.null_unread ? nullptr : PTR; // (never read by this call)
    Block<int> groups(22);
    std::memcpy(groups.p, c.groups, sizeof(c.groups));
    Block<float> base(66), prior(c.K);
    for (int i = 0; i < 66; ++i) base.p[i] = 0.01f * (float)(i - 30);
    base.p[7] = c.base_at_7;
    for (int i = 0; i < c.K; ++i) prior.p[i] = 1.f;
    if (c.K > 1) prior.p[1] = c.prior_at_1;
    dp_bone_fit f0 = DP_BONE_FIT_INIT;
    f0.struct_size = c.fit_size; f0.reserved0 = c.fit_reserved0;
    f0.n_groups = c.K; f0.ridge = c.ridge;
    f0.groups = c.null_groups ? nullptr : groups.p;
    f0.base = c.with_base ? base.p : nullptr;
    f0.prior = c.with_prior ? prior.p : nullptr;
    f0.workspace = c.null_workspace ? nullptr : (void*)PTR;
    f0.workspace_bytes = (size_t)((long long)dp_fit_bones_workspace_bytes(c.n_frames) - c.workspace_short);
    dp_bone_fit_result r0 = DP_BONE_FIT_RESULT_INIT;
    r0.struct_size = c.result_size; r0.reserved0 = c.result_reserved0;
    r0.scales = c.null_scales ? nullptr : PTR;
    if (c.with_outputs) { r0.offsets = r0.rms = PTR; r0.normal = (double*)PTR; r0.info = r0.status = (int*)PTR; }
    Exact<dp_batch> b(b0);
    Exact<dp_bone_fit> f(f0, cut<dp_bone_fit>(c.fit_size));
    Exact<dp_bone_fit_result> r(r0, cut<dp_bone_fit_result>(c.result_size));
    return dp_fit_bones(ctx, c.null_batch ? nullptr : b.get(), c.null_fit ? nullptr : f.get(), c.null_result ? nullptr : r.get(), nullptr);
}

} // namespace

int main()
{
    Walker w("fit_bones", "dp_fit_bones");
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    CHECK(dp_fit_bones_workspace_bytes(0) == 0 && dp_fit_bones_workspace_bytes(-5) == 0);
    CHECK(dp_fit_bones_workspace_bytes(1) == dp_fit_bones_workspace_bytes(4) && dp_fit_bones_workspace_bytes(5) == 2 * dp_fit_bones_workspace_bytes(4));
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 7; ++variant) {
        Case c;
        if (variant == 1) c.with_base = false;
        if (variant == 2) c.with_prior = false;
        if (variant == 3) c.with_outputs = false; // every optional pointer NULL
        if (variant == 4) c.null_unread = true;   // z_tgt and tgt_rot are not read
        if (variant == 5) { c.K = 1; for (int j = 1; j < 22; ++j) c.groups[j] = j < 4 ? 0 : -1; c.ridge = 0.f; c.n_frames = 1; }
        if (variant == 6) { c.K = 21; for (int j = 1; j < 22; ++j) c.groups[j] = j - 1; c.groups[0] = 99; c.n_frames = 4096; } // (entry 0 is ignored)
        w.unsupported(run(w.ctx, c), "dp_fit.hip");
    }
    // the refusals in the header's order: each is reported before every later one's fault
    { Case c; c.null_batch = true; c.K = 0; refused(c, "NULL batch, fit or result"); }
    { Case c; c.null_fit = true; c.n_frames = 0; refused(c, "NULL batch, fit or result"); }
    { Case c; c.null_result = true; c.K = 99; refused(c, "NULL batch, fit or result"); }
    { Case c; c.fit_size = 8; c.result_size = 8; refused(c, "dp_bone_fit.struct_size"); } // a block of 8 bytes: only the size word and reserved0 exist
    { Case c; c.fit_size = 48; c.K = 0; refused(c, "dp_bone_fit.struct_size"); }
    { Case c; c.fit_size = 5000; refused(c, "dp_bone_fit.struct_size"); }
    { Case c; c.fit_reserved0 = 3u; c.K = 0; refused(c, "reserved0 3"); }
    { Case c; c.result_size = 8; c.K = 0; refused(c, "dp_bone_fit_result.struct_size"); }
    { Case c; c.result_size = 48; c.null_scales = true; refused(c, "dp_bone_fit_result.struct_size"); }
    { Case c; c.result_size = 5000; refused(c, "dp_bone_fit_result.struct_size"); }
    { Case c; c.result_reserved0 = 1u; c.K = 0; refused(c, "reserved0 1"); }
    { Case c; c.null_scales = true; c.K = 0; refused(c, "scales is NULL"); }
    { Case c; c.K = 0; c.groups[5] = 7; refused(c, "n_groups 0 outside 1..24"); }
    { Case c; c.K = 25; c.null_groups = true; refused(c, "n_groups 25 outside 1..24"); }
    { Case c; c.K = -1; refused(c, "n_groups -1 outside"); }
    { Case c; c.null_groups = true; c.ridge = nan; refused(c, "groups is NULL"); }
    { Case c; c.groups[5] = 3; c.groups[9] = c.groups[10] = c.groups[11] = c.groups[12] = c.groups[13] = 0; refused(c, "groups[5] is 3, outside -1..2"); }
    { Case c; c.groups[21] = -2; c.base_at_7 = nan; refused(c, "groups[21] is -2"); }
    { Case c; for (int j = 9; j < 14; ++j) c.groups[j] = 0; c.ridge = -1.f; refused(c, "group 1 owns no bone"); }
    { Case c; for (int j = 14; j < 22; ++j) c.groups[j] = -1; c.prior_at_1 = inf; refused(c, "group 2 owns no bone"); }
    { Case c; c.base_at_7 = nan; c.null_workspace = true; refused(c, "base holds a value that is not finite"); }
    { Case c; c.base_at_7 = -inf; c.prior_at_1 = nan; refused(c, "base holds"); }
    { Case c; c.prior_at_1 = nan; c.ridge = -1.f; refused(c, "prior holds a value that is not finite"); }
    { Case c; c.prior_at_1 = inf; refused(c, "prior holds"); }
    { Case c; c.ridge = -1.0e-3f; c.null_workspace = true; refused(c, "ridge is negative or not finite"); }
    { Case c; c.ridge = nan; refused(c, "ridge is negative or not finite"); }
    { Case c; c.ridge = inf; c.n_frames = 0; refused(c, "ridge is negative or not finite"); }
    { Case c; c.null_workspace = true; c.n_frames = 0; refused(c, "workspace is NULL"); }
    { Case c; c.workspace_short = 1; c.null_z0 = true; refused(c, "fewer than the"); }
    { Case c; c.n_frames = 4096; c.workspace_short = 2560; refused(c, "fewer than the"); }
    { Case c; c.n_frames = 0; c.null_z0 = true; refused(c, "n_frames must be positive"); }
    { Case c; c.n_frames = -2; refused(c, "n_frames must be positive"); }
    { Case c; c.null_z0 = true; refused(c, "NULL input array"); }
    CHECK(dp_fit_bones(nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
