// tests/points_san/main.cpp -- dp_optimize_terms_points, dp_optimize_terms_points_skeleton and dp_optimize_sequence_terms_points
// (include/dragposer_points.h) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program that links dp_host.cpp against
// tests/host_san/fake_hip.cpp (no HIP runtime, no kernel unit) and walks take_points through well-formed and malformed structs, in the
// header's order, on a context without a device.  dp_points is handed over in a heap block of exactly struct_size bytes, its coefficients
// in one of exactly n_points * 22 floats and the term table in one of exactly n_terms entries, so a read past what the caller owns is an
// error here.  Device pointers are a constant that is never dereferenced.  Built and run by tests/test_host_san.py; every condition is
// exact.
#include "../../include/dragposer_points.h"
#include "../host_san/san_support.h"

namespace {

std::vector<dp_term> good_terms()
{ // 0: a plane on point 1; 1: the balance band, point 0 against point 1; 2: point 2 pinned; 3: a point against a member joint; 4: an ALIGN of joints
    dp_term plane = DP_TERM_INIT;
    plane.type = DP_TERM_PLANE; plane.joint_a = 23; plane.weight = 1.f; plane.flags = DP_TERM_ONE_SIDED;
    dp_term band = DP_TERM_INIT;
    band.type = DP_TERM_DISTANCE; band.joint_a = 22; band.joint_b = 23; band.weight = 2.f; band.p1 = 0.1f; band.flags = DP_TERM_DROP_UP;
    dp_term pin = DP_TERM_INIT;
    pin.type = DP_TERM_DISTANCE; pin.joint_a = 24; pin.weight = 0.5f;
    dp_term member = DP_TERM_INIT;
    member.type = DP_TERM_DISTANCE; member.joint_a = 4; member.joint_b = 23; member.weight = 1.f; member.p0 = 0.05f; member.p1 = 0.2f;
    dp_term align = DP_TERM_INIT;
    align.type = DP_TERM_ALIGN; align.joint_a = 13; align.joint_b = 0; align.weight = 1.f;
    return {plane, band, pin, member, align};
}

std::vector<float> good_coeff()
{ // point 0: the centroid; 1: the midpoint of the feet; 2: the midpoint of the hands
    std::vector<float> m(3 * 22, 0.f);
    for (int j = 0; j < 22; ++j) m[j] = 1.f / 22.f;
    m[22 + 4] = m[22 + 8] = 0.5f;
    m[44 + 17] = m[44 + 21] = 0.5f;
    return m;
}

enum Which { FRAME, SKEL, SEQ };

struct Case { // what one call is made of; the defaults are well-formed
    std::vector<dp_term> terms = good_terms();
    std::vector<float> coeff = good_coeff();
    Which which = FRAME;
    bool null_points = false, null_coeff = false, with_extra = true, with_skeleton = true;
    unsigned points_size = sizeof(dp_points), reserved0 = 0u;
    int reserved1 = 0;
    int n_points = -100; // (-100: the array's rows)
    int skel_stride = DP_SKELETON_STRIDE;
    float lr = 1e-2f;
};

const char* const NAMES[3] = {"dp_optimize_terms_points", "dp_optimize_terms_points_skeleton", "dp_optimize_sequence_terms_points"};

int run(dp_ctx* ctx, const Case& c)
{
    SeqArgs a; // (the params and the skeleton serve the per-frame calls as well)
    a.frames.z_tgt = PTR;
    a.params.lr = c.lr; a.params.lambda_tmp = 0.02f;
    a.skeleton.stride = c.skel_stride;
    Array<dp_term> terms(c.terms);
    dp_terms t0 = DP_TERMS_INIT;
    t0.n_terms = (int)c.terms.size(); t0.terms = terms.p;
    t0.global_pos = PTR;
    Array<float> coeff(c.coeff);
    dp_points q0 = DP_POINTS_INIT;
    q0.struct_size = c.points_size; q0.reserved0 = c.reserved0; q0.reserved1 = c.reserved1;
    q0.n_points = c.n_points == -100 ? (int)c.coeff.size() / 22 : c.n_points;
    q0.coeff = c.null_coeff ? nullptr : coeff.p;
    SeqBlocks s(a);
    Exact<dp_terms> t(t0);
    Exact<dp_points> q(q0, cut<dp_points>(c.points_size));
    const dp_points* qp = c.null_points ? nullptr : q.get();
    if (c.which != SEQ) {
        dp_batch b0{};
        b0.n_frames = 4; b0.z0 = b0.z_tgt = b0.cur_rot = b0.tgt_pos = b0.tgt_rot = b0.w = PTR; b0.tracked = (const unsigned char*)PTR;
        dp_result r0 = DP_RESULT_INIT;
        r0.z = r0.pos = PTR;
        Exact<dp_batch> b(b0);
        Exact<dp_result> r(r0);
        if (c.which == FRAME) return dp_optimize_terms_points(ctx, b.get(), s.params.get(), t.get(), qp, r.get(), nullptr);
        return dp_optimize_terms_points_skeleton(ctx, b.get(), s.params.get(), t.get(), qp, s.skeleton.get(), r.get(), nullptr);
    }
    t0.global_pos = nullptr; // (a sequence reads the state's own)
    Exact<dp_terms> ts(t0);
    return dp_optimize_sequence_terms_points(ctx, 4, PTR, s.frames.get(), s.params.get(), ts.get(), qp, c.with_skeleton ? s.skeleton.get() : nullptr, s.state.get(),
                                             s.step.get(), s.results.get(), c.with_extra ? s.extra.get() : nullptr, nullptr);
}

} // namespace

int main()
{
    Walker w("points", NAMES[FRAME]);
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    for (const Which which : {FRAME, SKEL, SEQ}) {
        w.entry_point = NAMES[which];
        const auto refused = [&](Case c, const char* word) {
            c.which = which;
            w.refused(run(w.ctx, c), word);
        };
        // well-formed: this link has no kernel unit, which the library says after every argument check
        for (int variant = 0; variant < 6; ++variant) {
            Case c;
            c.which = which;
            if (variant == 1) { c.coeff.clear(); c.terms = {good_terms()[4]}; }                // n_points = 0, a NULL coeff, a table of joints
            if (variant == 2) { c.coeff.clear(); c.terms.clear(); }                            // ... and no table either
            if (variant == 3) {                                                                // n_points = 4: index 25 in use, a unit point
                c.coeff.resize(4 * 22, 0.f);
                c.coeff[66 + 13] = 1.f;
                c.terms[2].joint_a = 25;
                c.terms[1].joint_b = 25;
            }
            if (variant == 4) { c.with_extra = false; c.with_skeleton = false; c.skel_stride = 0; }
            if (variant == 5) { c.terms[1].joint_b = 22; c.coeff[0] += 5e-5f; }                // the same point twice; a sum within the tolerance
            w.unsupported(run(w.ctx, c), "dp_cons_points.hip");
            CHECK(said(w.ctx, NAMES[which]));
        }
        // dp_points' own refusals, in the header's order: each is reported with every later one's fault present as well
        { Case c; c.null_points = true; refused(c, "NULL"); }
        { Case c; c.points_size = 16; c.n_points = -1; refused(c, "dp_points.struct_size"); }  // a block of 16 bytes: no coeff word exists
        { Case c; c.points_size = 8; refused(c, "dp_points.struct_size"); }
        { Case c; c.points_size = 5000; refused(c, "dp_points.struct_size"); }                 // (the block is sizeof(dp_points): nothing past it is read)
        { Case c; c.reserved0 = 3u; c.n_points = -1; refused(c, "reserved0"); }
        { Case c; c.reserved1 = 7; c.n_points = -1; refused(c, "dp_points.reserved1"); }
        { Case c; c.n_points = -1; c.null_coeff = true; refused(c, "dp_points.n_points -1 outside 0..4"); }
        { Case c; c.n_points = DP_MAX_POINTS + 1; c.coeff[3] = nan; refused(c, "dp_points.n_points 5 outside 0..4"); } // (the three rows are not read)
        { Case c; c.null_coeff = true; c.terms[2].joint_a = 25; refused(c, "dp_points.coeff is NULL"); }
        { Case c; c.coeff[22 + 7] = nan; c.coeff[0] = 2.f; refused(c, "point 1: the coefficient of joint 7 is not finite"); }
        { Case c; c.coeff[44 + 21] = inf; c.terms[2].joint_a = 25; refused(c, "point 2: the coefficient of joint 21 is not finite"); }
        { Case c; c.coeff[44] = -inf; refused(c, "point 2: the coefficient of joint 0 is not finite"); }
        { Case c; c.coeff[22 + 4] = 0.6f; c.terms[2].joint_a = 25; refused(c, "point 1: the coefficients sum to"); }
        { Case c; c.coeff[44 + 17] = 0.4997f; c.terms[4].joint_a = 22; refused(c, "point 2: the coefficients sum to"); }
        { Case c; for (int j = 0; j < 22; ++j) c.coeff[j] = 0.f; refused(c, "point 0: the coefficients sum to"); }
        { Case c; c.terms[2].joint_a = 25; c.terms[4].joint_a = 22; refused(c, "term 2: index 25 names a point, and dp_points has 3"); }
        { Case c; c.terms[3].joint_b = 25; refused(c, "term 3: index 25 names a point"); }
        { Case c; c.coeff.resize(22); c.terms[1].joint_b = 22; c.terms[2].joint_a = 22; refused(c, "term 0: index 23 names a point, and dp_points has 1"); }
        { Case c; c.coeff.clear(); refused(c, "term 0: index 23 names a point, and dp_points has 0"); }
        { Case c; c.terms[4].joint_a = 22; refused(c, "term 4: an ALIGN term names a point"); }
        { Case c; c.terms[4].joint_b = 24; refused(c, "term 4: an ALIGN term names a point"); }
        // the order around dp_points: what dp_terms refuses comes first, the skeleton struct, the batch or the frames and Adam after
        { Case c; c.terms[0].joint_a = 26; c.n_points = -1; refused(c, "term 0: joint_a 26 outside 0..25"); }
        { Case c; c.terms[1].joint_b = 26; c.n_points = -1; refused(c, "term 1: joint_b 26 outside -1..25"); }
        { Case c; c.terms[0].joint_b = 22; c.n_points = -1; refused(c, "a PLANE has no second joint"); }
        { Case c; c.terms[2].weight = -1.f; c.reserved1 = 1; refused(c, "term 2"); }
        if (which != FRAME) { Case c; c.skel_stride = 5; c.n_points = -1; refused(c, "dp_points.n_points"); }
        if (which != FRAME) { Case c; c.skel_stride = 5; refused(c, "dp_skeleton_in.stride"); }
        { Case c; c.lr = -1.f; c.terms[4].joint_a = 22; refused(c, "an ALIGN term names a point"); }
        { Case c; c.lr = -1.f; refused(c, "Adam"); }
    }
    CHECK(dp_optimize_terms_points(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    CHECK(dp_optimize_terms_points_skeleton(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    CHECK(dp_optimize_sequence_terms_points(nullptr, 4, PTR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DP_ERR_INVALID);
    w.done();
    return 0;
}
