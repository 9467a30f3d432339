// tests/tethers_san/main.cpp -- dp_optimize_sequence_tethers (include/dragposer_tethers.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel
// unit) and walks take_tethers through well-formed and malformed structs, in the header's order, on a context without a device.  Every
// sized struct is handed over in a heap block of exactly struct_size bytes, the term table in one of exactly n_terms entries, the holds and
// the tethers arrays in ones of exactly n_holds and n_tethers entries, so a read past what the caller owns is an error here.  Device
// pointers are a constant that is never dereferenced.  Built and run by tests/test_host_san.py; every condition is exact.
#include "../../include/dragposer_tethers.h"
#include "../host_san/san_support.h"

namespace {

std::vector<dp_term> good_terms()
{ // 0: a plane; 1: the held pin; 2, 3: the tethered band and pin; 4: a joint-DISTANCE term
    dp_term plane = DP_TERM_INIT;
    plane.type = DP_TERM_PLANE; plane.joint_a = 4; plane.weight = 1.f;
    dp_term pin = DP_TERM_INIT;
    pin.type = DP_TERM_DISTANCE; pin.joint_a = 8; pin.weight = 0.8f; pin.flags = DP_TERM_DROP_UP;
    dp_term band = DP_TERM_INIT;
    band.type = DP_TERM_DISTANCE; band.joint_a = 6; band.weight = 0.6f; band.p1 = 0.02f;
    dp_term damp = DP_TERM_INIT;
    damp.type = DP_TERM_DISTANCE; damp.joint_a = 19; damp.weight = 0.f; // (an inert tether is accepted like any other)
    dp_term pair = DP_TERM_INIT;
    pair.type = DP_TERM_DISTANCE; pair.joint_a = 3; pair.joint_b = 7; pair.weight = 2.f; pair.p0 = 0.1f; pair.p1 = 0.3f;
    return {plane, pin, band, damp, pair};
}

struct Case { // what one call is made of; the defaults are well-formed
    std::vector<dp_term> terms = good_terms();
    std::vector<dp_hold> holds = {{1, 0.f, 0.02f, 0.05f}};
    std::vector<dp_tether> tethers = {{2, 0.f}, {3, 1.f}};
    bool null_holds_struct = false, null_ar = false, z_tgt = false, with_extra = true, with_skeleton = true;
    bool null_tethers = false, null_tether_array = false, null_tether_state = false, with_tether_trace = true;
    unsigned tethers_size = sizeof(dp_tethers), tethers_reserved0 = 0u;
    int n_tethers = -100; // (-100: the array's length)
    int order = 2, max_hold = 3;
    float decay = 0.7f, lr = 1e-2f;
};

int run(dp_ctx* ctx, const Case& c)
{
    SeqArgs a;
    a.frames.z_tgt = c.z_tgt ? PTR : nullptr;
    a.params.lr = c.lr; a.params.lambda_tmp = 0.02f;
    Array<dp_term> terms(c.terms);
    dp_terms t0 = DP_TERMS_INIT;
    t0.n_terms = (int)c.terms.size(); t0.terms = terms.p;
    Array<dp_hold> holds(c.holds);
    dp_holds h0 = DP_HOLDS_INIT;
    h0.n_holds = (int)c.holds.size(); h0.holds = holds.p; h0.state = c.holds.empty() ? nullptr : PTR;
    dp_latent_ar r0 = DP_LATENT_AR_INIT;
    r0.order = c.order; r0.coeffs = r0.bias = PTR;
    dp_gaps g0 = DP_GAPS_INIT;
    g0.max_hold = c.max_hold; g0.decay = c.decay; g0.state = PTR;
    Array<dp_tether> tethers(c.tethers);
    dp_tethers te0 = DP_TETHERS_INIT;
    te0.struct_size = c.tethers_size; te0.reserved0 = c.tethers_reserved0;
    te0.n_tethers = c.n_tethers == -100 ? (int)c.tethers.size() : c.n_tethers;
    te0.tethers = c.null_tether_array ? nullptr : tethers.p;
    te0.state = c.null_tether_state || c.tethers.empty() ? nullptr : PTR; te0.trace = c.with_tether_trace ? PTR : nullptr;
    SeqBlocks b(a);
    Exact<dp_terms> t(t0);
    Exact<dp_holds> h(h0);
    Exact<dp_latent_ar> r(r0);
    Exact<dp_gaps> g(g0);
    Exact<dp_tethers> te(te0, cut<dp_tethers>(c.tethers_size));
    return dp_optimize_sequence_tethers(ctx, 4, PTR, b.frames.get(), b.params.get(), t.get(), c.null_holds_struct ? nullptr : h.get(), c.null_ar ? nullptr : r.get(),
                                        g.get(), c.null_tethers ? nullptr : te.get(), c.with_skeleton ? b.skeleton.get() : nullptr, b.state.get(), b.step.get(),
                                        b.results.get(), c.with_extra ? b.extra.get() : nullptr, nullptr);
}

} // namespace

int main()
{
    Walker w("tethers", "dp_optimize_sequence_tethers");
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 9; ++variant) {
        Case c;
        if (variant == 1) c.null_holds_struct = true;                        // no dp_holds at all
        if (variant == 2) { c.null_ar = true; c.z_tgt = true; }              // no predictor: the targets are frames->z_tgt
        if (variant == 3) c.tethers.clear();                                 // n_tethers = 0: NULL tethers and state are accepted
        if (variant == 4) { c.with_tether_trace = false; c.with_extra = false; c.with_skeleton = false; }
        if (variant == 5) c.tethers = {{2, 0.5f}};                           // one tether, of an array of exactly one
        if (variant == 6) { c.null_holds_struct = true; c.tethers = {{1, 1.f}, {2, 0.f}, {3, 0.25f}}; } // the pin is free to be tethered without its hold
        if (variant == 7) { c.holds.clear(); c.tethers = {{3, 0.f}, {1, 1.f}, {2, 1.f}}; c.null_ar = true; c.z_tgt = true; }
        if (variant == 8) { c.tethers = {{3, 0.f}}; c.terms.resize(4); }     // the table's last term, of a table of exactly four
        w.unsupported(run(w.ctx, c), "dp_cons_tether.hip");
    }
    // dp_tethers' own refusals, in the header's order: each is reported before every later one's fault
    { Case c; c.null_tethers = true; refused(c, "NULL"); }
    { Case c; c.tethers_size = 16; c.n_tethers = -1; refused(c, "dp_tethers.struct_size"); }  // a block of 16 bytes: only the size, reserved0 and n_tethers exist
    { Case c; c.tethers_size = 8; refused(c, "dp_tethers.struct_size"); }
    { Case c; c.tethers_size = 5000; refused(c, "dp_tethers.struct_size"); }                  // (the block is sizeof(dp_tethers): nothing past the size word is read)
    { Case c; c.tethers_reserved0 = 3u; c.n_tethers = -1; refused(c, "reserved0"); }
    { Case c; c.n_tethers = -1; c.null_tether_array = true; refused(c, "dp_tethers.n_tethers -1"); }
    { Case c; c.n_tethers = DP_MAX_TETHERS + 1; c.null_tether_state = true; refused(c, "dp_tethers.n_tethers 5"); } // (the array of two is not read)
    { Case c; c.null_tether_array = true; c.null_tether_state = true; refused(c, "dp_tethers.tethers is NULL"); }
    { Case c; c.null_tether_state = true; c.tethers[0].alpha = 2.f; refused(c, "dp_tethers.state is NULL"); }
    { Case c; c.tethers[0].term = -1; c.tethers[0].alpha = 2.f; refused(c, "tether 0: term -1 outside the table of 5"); }
    { Case c; c.tethers[1].term = 5; c.tethers[1].alpha = nan; refused(c, "tether 1: term 5 outside the table of 5"); }
    { Case c; c.tethers[0].term = 0; c.tethers[0].alpha = 2.f; refused(c, "tether 0: term 0 is not a DP_TERM_DISTANCE term"); }
    { Case c; c.tethers[1].term = 4; c.tethers[1].alpha = 2.f; refused(c, "tether 1: term 4 has a joint_b"); }
    { Case c; c.terms[2].per_frame = PTR; c.tethers[0].alpha = 2.f; refused(c, "tether 0: term 2 has a per_frame array"); }
    { Case c; c.tethers[1].term = 2; c.tethers[1].alpha = 2.f; refused(c, "tether 1: term 2 is already tethered by tether 0"); }
    { Case c; c.tethers[1].term = 1; c.tethers[1].alpha = 2.f; refused(c, "tether 1: term 1 is held by hold 0"); }
    { Case c; c.tethers[0].alpha = -0.25f; refused(c, "tether 0: alpha"); }
    { Case c; c.tethers[1].alpha = 1.0000001f; refused(c, "tether 1: alpha"); }
    { Case c; c.tethers[0].alpha = nan; refused(c, "tether 0: alpha"); }
    { Case c; c.tethers[1].alpha = inf; refused(c, "tether 1: alpha"); }
    { Case c; c.tethers[1].alpha = -inf; refused(c, "tether 1: alpha"); }
    // the order around dp_tethers: everything dp_optimize_sequence_gaps checks comes first
    { Case c; c.terms[0].joint_a = 22; c.n_tethers = -1; refused(c, "term 0"); }
    { Case c; c.holds[0].term = 9; c.n_tethers = -1; refused(c, "hold 0"); }
    { Case c; c.lr = -1.f; c.n_tethers = -1; refused(c, "Adam"); }
    { Case c; c.order = 0; c.n_tethers = -1; refused(c, "dp_latent_ar.order"); }
    { Case c; c.z_tgt = true; c.n_tethers = -1; refused(c, "z_tgt must be NULL"); }
    { Case c; c.null_ar = true; c.n_tethers = -1; refused(c, "NULL input array"); }  // without a predictor frames->z_tgt is required
    { Case c; c.max_hold = -1; c.n_tethers = -1; refused(c, "dp_gaps.max_hold"); }
    { Case c; c.decay = 0.f; c.tethers[0].alpha = 2.f; refused(c, "dp_gaps.decay"); }
    { Case c; c.null_ar = true; c.z_tgt = true; c.n_tethers = -1; refused(c, "dp_tethers.n_tethers"); }
    CHECK(dp_optimize_sequence_tethers(nullptr, 4, PTR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
