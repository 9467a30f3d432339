// tests/latent_ar_san/main.cpp -- dp_optimize_sequence_ar (include/dragposer_latent_ar.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel
// unit) and walks the call's refusals, in the header's order, on a context without a device.  Every sized struct is handed over in a heap
// block of exactly struct_size bytes, the term table in one of exactly n_terms entries and the holds array in one of exactly n_holds entries,
// so a read past what the caller owns is an error here.  Device pointers are a constant that is never dereferenced.  Built and run by
// tests/test_host_san.py; every condition is exact.
#include "../../include/dragposer_latent_ar.h"
#include "../host_san/san_support.h"

namespace {

std::vector<dp_term> good_terms()
{
    dp_term plane = DP_TERM_INIT;
    plane.type = DP_TERM_PLANE; plane.joint_a = 4; plane.weight = 1.f;
    dp_term pin = DP_TERM_INIT;
    pin.type = DP_TERM_DISTANCE; pin.joint_a = 8; pin.weight = 0.8f; pin.flags = DP_TERM_DROP_UP;
    return {plane, pin};
}

struct Case { // what one call is made of; the defaults are well-formed
    std::vector<dp_term> terms = good_terms();
    std::vector<dp_hold> holds = {{1, 0.f, 0.02f, 0.05f}};
    bool null_holds_struct = false, null_ar = false, with_trace = true, with_extra = true, with_skeleton = true;
    unsigned holds_size = sizeof(dp_holds), ar_size = sizeof(dp_latent_ar), ar_reserved0 = 0u;
    int order = 2, history = 60, n_steps = 3, row_step1 = 0;
    bool null_coeffs = false, null_bias = false, z_tgt = false;
    float lr = 1e-2f;
};

int run(dp_ctx* ctx, const Case& c)
{
    SeqArgs a;
    a.frames.n_steps = c.n_steps; a.frames.z_tgt = c.z_tgt ? PTR : nullptr;
    a.params.lr = c.lr; a.params.lambda_tmp = 0.02f;
    a.state.history = c.history;
    a.extra.row_step[1] = c.row_step1;
    Array<dp_term> terms(c.terms);
    dp_terms t0 = DP_TERMS_INIT;
    t0.n_terms = (int)c.terms.size(); t0.terms = terms.p;
    Array<dp_hold> holds(c.holds);
    dp_holds h0 = DP_HOLDS_INIT;
    h0.struct_size = c.holds_size; h0.n_holds = (int)c.holds.size(); h0.holds = holds.p;
    h0.state = c.holds.empty() ? nullptr : PTR; h0.trace = nullptr;
    dp_latent_ar r0 = DP_LATENT_AR_INIT;
    r0.struct_size = c.ar_size; r0.reserved0 = c.ar_reserved0; r0.order = c.order;
    r0.coeffs = c.null_coeffs ? nullptr : PTR; r0.bias = c.null_bias ? nullptr : PTR; r0.trace = c.with_trace ? PTR : nullptr;
    SeqBlocks b(a);
    Exact<dp_terms> t(t0);
    Exact<dp_holds> h(h0, cut<dp_holds>(c.holds_size));
    Exact<dp_latent_ar> r(r0, cut<dp_latent_ar>(c.ar_size));
    return dp_optimize_sequence_ar(ctx, 4, PTR, b.frames.get(), b.params.get(), t.get(), c.null_holds_struct ? nullptr : h.get(), c.null_ar ? nullptr : r.get(),
                                   c.with_skeleton ? b.skeleton.get() : nullptr, b.state.get(), b.step.get(), b.results.get(),
                                   c.with_extra ? b.extra.get() : nullptr, nullptr);
}

} // namespace

int main()
{
    Walker w("latent_ar", "dp_optimize_sequence_ar");
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 7; ++variant) {
        Case c;
        if (variant == 1) c.null_holds_struct = true;                       // no dp_holds at all
        if (variant == 2) c.holds.clear();                                  // a dp_holds with n_holds = 0: no array, no state
        if (variant == 3) { c.terms.clear(); c.null_holds_struct = true; }  // n_terms = 0: the plain tracker loss
        if (variant == 4) { c.with_trace = false; c.with_extra = false; c.with_skeleton = false; }
        if (variant == 5) { c.order = 1; c.history = 1; }
        if (variant == 6) { c.order = DP_MAX_AR_ORDER; c.history = DP_MAX_AR_ORDER; }
        w.unsupported(run(w.ctx, c), "dp_cons_ar.hip");
    }
    // dp_latent_ar's own refusals, in the header's order: each is reported before every later one's fault
    { Case c; c.null_ar = true; refused(c, "NULL"); }
    { Case c; c.ar_size = 12; c.order = 0; refused(c, "dp_latent_ar.struct_size"); }   // a block of 12 bytes: only the size, reserved0 and order exist
    { Case c; c.ar_size = 8; refused(c, "dp_latent_ar.struct_size"); }
    { Case c; c.ar_size = 5000; refused(c, "dp_latent_ar.struct_size"); }              // (the block is sizeof(dp_latent_ar): nothing past the size word is read)
    { Case c; c.ar_reserved0 = 3u; c.order = 9; refused(c, "reserved0"); }
    { Case c; c.order = 0; c.null_coeffs = true; refused(c, "dp_latent_ar.order"); }
    { Case c; c.order = -1; refused(c, "dp_latent_ar.order"); }
    { Case c; c.order = DP_MAX_AR_ORDER + 1; c.history = 2; refused(c, "dp_latent_ar.order"); }
    { Case c; c.null_coeffs = true; c.history = 1; refused(c, "coeffs or bias is NULL"); }
    { Case c; c.null_bias = true; c.z_tgt = true; refused(c, "coeffs or bias is NULL"); }
    { Case c; c.order = 3; c.history = 2; c.z_tgt = true; refused(c, "shorter than dp_latent_ar.order"); }
    { Case c; c.z_tgt = true; refused(c, "z_tgt must be NULL"); }
    // the order around dp_latent_ar: everything dp_optimize_sequence_holds checks comes first
    { Case c; c.terms[0].joint_a = 22; c.order = 0; refused(c, "term 0"); }
    { Case c; c.holds_size = 12; c.order = 0; refused(c, "dp_holds.struct_size"); }
    { Case c; c.holds[0].term = 0; c.order = 0; refused(c, "hold 0: term 0 is not a DP_TERM_DISTANCE"); }
    { Case c; c.row_step1 = -4; c.order = 0; refused(c, "row_step[1]"); }
    { Case c; c.n_steps = 0; c.order = 0; refused(c, "n_steps must be positive"); }
    { Case c; c.history = 0; c.order = 0; refused(c, "history / n_heights"); }
    { Case c; c.lr = -1.f; c.order = 0; refused(c, "Adam"); }
    CHECK(dp_optimize_sequence_ar(nullptr, 4, PTR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
