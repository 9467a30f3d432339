// tests/holds_san/main.cpp -- dp_optimize_sequence_holds (include/dragposer_holds.h) under AddressSanitizer and UndefinedBehaviorSanitizer:
// a stand-alone program that links dp_host.cpp against tests/host_san/fake_hip.cpp (no HIP runtime, no kernel unit) and walks the call's
// refusals on a context without a device.  Every sized struct is handed over in a heap block of exactly struct_size bytes, the term table in
// one of exactly n_terms entries and the holds array in one of exactly n_holds entries, so a read past what the caller owns is an error here.
// Device pointers are a constant that is never dereferenced.  Built and run by tests/test_host_san.py; every condition is exact.
#include <limits>

#include "../../include/dragposer_holds.h"
#include "../host_san/san_support.h"

namespace {

dp_term point_term(int joint, float weight)
{
    dp_term t = DP_TERM_INIT;
    t.type = DP_TERM_DISTANCE; t.joint_a = joint; t.weight = weight; t.flags = DP_TERM_DROP_UP;
    return t;
}

std::vector<dp_term> good_terms()
{
    dp_term plane = DP_TERM_INIT;
    plane.type = DP_TERM_PLANE; plane.joint_a = 4; plane.weight = 1.f;
    dp_term joints = DP_TERM_INIT;
    joints.type = DP_TERM_DISTANCE; joints.joint_a = 3; joints.joint_b = 7; joints.weight = 2.f; joints.p0 = 0.1f; joints.p1 = 0.3f;
    return {plane, point_term(4, 0.8f), joints, point_term(8, 0.f)};
}

struct Case { // what one call is made of; the defaults are well-formed
    std::vector<dp_term> terms = good_terms();
    std::vector<dp_hold> holds = {{1, 0.f, 0.02f, 0.05f}, {3, -0.9f, 0.05f, 0.05f}};
    int n_holds = -100;               // (-100: holds.size())
    unsigned holds_size = sizeof(dp_holds), holds_reserved0 = 0u;
    bool null_holds_struct = false, null_state = false, with_trace = true, with_extra = true, with_skeleton = true;
    float lr = 1e-2f;
    int n_steps = 3, row_step3 = 0;
};

int run(dp_ctx* ctx, const Case& c)
{
    SeqArgs a;
    a.frames.n_steps = c.n_steps; a.frames.z_tgt = PTR; a.frames.z_tgt_seq = 24;
    a.params.lr = c.lr;
    a.extra.row_step[3] = c.row_step3;
    Array<dp_term> terms(c.terms);
    dp_terms t0 = DP_TERMS_INIT;
    t0.n_terms = (int)c.terms.size(); t0.terms = terms.p;
    Array<dp_hold> holds(c.holds);
    dp_holds h0 = DP_HOLDS_INIT;
    h0.struct_size = c.holds_size; h0.reserved0 = c.holds_reserved0;
    h0.n_holds = c.n_holds == -100 ? (int)c.holds.size() : c.n_holds; h0.holds = holds.p;
    h0.state = c.null_state ? nullptr : PTR; h0.trace = c.with_trace ? PTR : nullptr;
    SeqBlocks b(a);
    Exact<dp_terms> t(t0);
    Exact<dp_holds> h(h0, cut<dp_holds>(c.holds_size));
    return dp_optimize_sequence_holds(ctx, 4, PTR, b.frames.get(), b.params.get(), t.get(), c.null_holds_struct ? nullptr : h.get(),
                                      c.with_skeleton ? b.skeleton.get() : nullptr, b.state.get(), b.step.get(), b.results.get(),
                                      c.with_extra ? b.extra.get() : nullptr, nullptr);
}

} // namespace

int main()
{
    Walker w("holds", "dp_optimize_sequence_holds");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const auto refused = [&](const Case& c, const char* word) { w.refused(run(w.ctx, c), word); };
    // well-formed: this link has no kernel unit, which the library says after every argument check
    for (int variant = 0; variant < 5; ++variant) {
        Case c;
        if (variant == 1) { c.holds.clear(); c.null_state = true; c.with_trace = false; } // no hold at all: no array, no state
        if (variant == 2) c.with_trace = false;
        if (variant == 3) { c.with_extra = false; c.with_skeleton = false; }
        if (variant == 4) { c.terms.push_back(point_term(3, 1.f)); c.terms.push_back(point_term(7, 1.f)); c.holds.push_back({4, 0.f, 0.f, 0.f}); c.holds.push_back({5, 1.f, -1.f, 1.f}); }
        w.unsupported(run(w.ctx, c), "dp_cons_hold.hip");
    }
    { Case c; c.null_holds_struct = true; refused(c, "NULL"); }
    { Case c; c.holds_size = 12; refused(c, "dp_holds.struct_size"); }       // a block of 12 bytes: only the size, reserved0 and n_holds exist
    { Case c; c.holds_size = 8; refused(c, "dp_holds.struct_size"); }
    { Case c; c.holds_size = 5000; refused(c, "dp_holds.struct_size"); }     // (the block is sizeof(dp_holds): nothing past the size word is read)
    { Case c; c.holds_reserved0 = 3u; refused(c, "reserved0"); }
    { Case c; c.n_holds = -1; refused(c, "n_holds"); }
    { Case c; c.n_holds = DP_MAX_HOLDS + 1; refused(c, "n_holds"); }          // (refused before the array of 2 is read as 5)
    { Case c; c.holds.clear(); c.n_holds = 2; refused(c, "dp_holds.holds is NULL"); }
    { Case c; c.null_state = true; refused(c, "dp_holds.state is NULL"); }
    { Case c; c.holds[1].term = 4; refused(c, "outside the table"); }        // (one past the table of exactly 4 entries: not read)
    { Case c; c.holds[0].term = -1; refused(c, "outside the table"); }
    { Case c; c.holds[1].term = 0; refused(c, "hold 1: term 0 is not a DP_TERM_DISTANCE"); }
    { Case c; c.holds[0].term = 2; refused(c, "hold 0: term 2 has a joint_b"); }
    { Case c; c.terms[3].per_frame = PTR; refused(c, "hold 1: term 3 has a per_frame"); }
    { Case c; c.holds[1].term = 1; refused(c, "already held by hold 0"); }
    { Case c; c.holds[0].level = nan; refused(c, "non-finite"); }
    { Case c; c.holds[1].contact_lo = -inf; refused(c, "non-finite"); }
    { Case c; c.holds[1].contact_hi = inf; refused(c, "non-finite"); }
    { Case c; c.holds[0].contact_lo = 0.06f; refused(c, "contact_lo is above contact_hi"); }
    // the order around dp_holds: the table's faults before, dp_seq_extra's and everything later after
    { Case c; c.terms[0].joint_a = 22; c.holds[0].term = 9; refused(c, "term 0"); }
    { Case c; c.holds[0].term = 9; c.row_step3 = -4; refused(c, "outside the table"); }
    { Case c; c.row_step3 = -4; refused(c, "row_step[3]"); }
    { Case c; c.n_steps = 0; refused(c, "n_steps must be positive"); }
    { Case c; c.lr = -1.f; refused(c, "Adam"); }
    CHECK(dp_optimize_sequence_holds(nullptr, 4, PTR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
