// tests/unity_san/main.cpp -- the plug-in's additions (include/dragposer_unity.h) under AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program that links dp_unity.cpp and the library's host files against tests/host_san/fake_hip.cpp (one malloc-backed device, no
// HIP runtime, no kernel unit).  Every array a caller hands over lives in a heap block of exactly its size -- the term table, the holds, the
// coefficients and the bias, the targets, `present` and the results -- and every device block is a malloc of exactly what the plug-in asked
// for, so a read or write past either is an error here.  Built and run by tests/test_host_san.py, which passes: the BVH clip, a model
// folder without temporal.bin, one with it, and a folder to write the latent_ar.bin variants into.  Every condition is exact.
#include <fstream>

#include "../../include/dragposer_unity.h"
#include "../host_san/san_support.h"

void fake_hip_mode(bool fake); // tests/host_san/fake_hip.cpp
int fake_hip_outstanding();

namespace {

int n_checks = 0;

void said(DragPoser* h, const char* word)
{
    const std::string msg = drag_poser_last_error(h);
    if (msg.find(word) == std::string::npos) { std::fprintf(stderr, "expected '%s' in: %s\n", word, msg.c_str()); std::exit(1); }
    ++n_checks;
}
void fine(DragPoser* h)
{
    const std::string msg = drag_poser_last_error(h);
    if (!msg.empty()) { std::fprintf(stderr, "unexpected failure: %s\n", msg.c_str()); std::exit(1); }
    ++n_checks;
}

std::vector<dp_term> table(int n)
{
    dp_term plane = DP_TERM_INIT;
    plane.type = DP_TERM_PLANE; plane.joint_a = 4; plane.weight = 1.f;
    dp_term pin = DP_TERM_INIT;
    pin.type = DP_TERM_DISTANCE; pin.joint_a = 8; pin.weight = 0.8f; pin.flags = DP_TERM_DROP_UP;
    std::vector<dp_term> t;
    for (int k = 0; k < n; ++k) t.push_back(k % 2 ? pin : plane);
    return t;
}

// a DPM1 file (tools/export_model_bin.py) of the given tensors; name_len overrides the first tensor's stated name length, cut the file's length
struct Spec { std::string name; std::vector<unsigned> dims; };
std::string write_bin(const std::string& path, const std::vector<Spec>& ts, long long cut = -1, unsigned name_len = 0)
{
    std::string s = "DPM1";
    const auto put = [&](unsigned v) { s.append((const char*)&v, 4); };
    put((unsigned)ts.size());
    for (size_t i = 0; i < ts.size(); ++i) {
        put(i == 0 && name_len ? name_len : (unsigned)ts[i].name.size());
        s += ts[i].name;
        put((unsigned)ts[i].dims.size());
        double n = 1;
        for (unsigned d : ts[i].dims) { put(d); n *= d; }
        for (size_t k = 0; n < 1e6 && k < (size_t)n; ++k) { // (dims beyond any file: no data follows)
            const float v = 0.001f * (float)(k % 97);
            s.append((const char*)&v, 4);
        }
    }
    if (cut >= 0) s.resize((size_t)cut);
    std::ofstream(path, std::ios::binary).write(s.data(), (std::streamsize)s.size());
    return path;
}

void setters_before_load_models(DragPoser* h)
{
    { Array<dp_term> t(table(17)); drag_poser_set_terms(h, 17, t.p, 1); said(h, "nTerms 17 outside 0..16"); }
    { Array<dp_term> t(table(2)); drag_poser_set_terms(h, 2, t.p, 3); said(h, "upAxis 3 outside 0..2"); }
    { Array<dp_term> t(table(2)); drag_poser_set_terms(h, -1, t.p, 1); said(h, "nTerms -1"); }
    { drag_poser_set_terms(h, 2, nullptr, 1); said(h, "NULL terms"); }
    {
        std::vector<dp_term> v = table(3);
        v[2].per_frame = PTR;
        Array<dp_term> t(v);
        drag_poser_set_terms(h, 3, t.p, 1);
        said(h, "term 2: per_frame must be NULL");
    }
    { Array<dp_term> t(table(2)); drag_poser_set_terms(h, 2, t.p, 1); said(h, "drag_poser_set_terms: call load_models first"); }
    { Array<dp_hold> b(std::vector<dp_hold>(1, dp_hold{1, 0.f, 0.f, 0.1f})); drag_poser_set_holds(h, 1, b.p); said(h, "drag_poser_set_holds: call load_models first"); }
    drag_poser_set_gaps(h, 5, 0.9f); said(h, "drag_poser_set_gaps: call load_models first");
    {
        Array<float> A(std::vector<float>(24 * 24, 0.f)), c(std::vector<float>(24, 0.f));
        drag_poser_set_latent_ar(h, 1, A.p, c.p);
        said(h, "drag_poser_set_latent_ar: call load_models first");
    }
}

void setters(DragPoser* h)
{
    // terms: the table is copied out of a block of exactly nTerms entries
    { Array<dp_term> t(table(16)); drag_poser_set_terms(h, 16, t.p, 2); fine(h); }
    { Array<dp_term> t(table(17)); drag_poser_set_terms(h, 17, t.p, 1); said(h, "nTerms 17"); }
    { Array<dp_term> t(table(2)); drag_poser_set_terms(h, 2, t.p, 1); fine(h); }
    // holds
    { Array<dp_hold> b(std::vector<dp_hold>(5, dp_hold{1, 0.f, 0.f, 0.1f})); drag_poser_set_holds(h, 5, b.p); said(h, "nHolds 5 outside 0..4"); }
    drag_poser_set_holds(h, -1, nullptr); said(h, "nHolds -1");
    drag_poser_set_holds(h, 2, nullptr); said(h, "NULL holds");
    { Array<dp_hold> b(std::vector<dp_hold>(1, dp_hold{2, 0.f, 0.f, 0.1f})); drag_poser_set_holds(h, 1, b.p); said(h, "term 2 outside the table of 2"); }
    { Array<dp_hold> b(std::vector<dp_hold>(1, dp_hold{-1, 0.f, 0.f, 0.1f})); drag_poser_set_holds(h, 1, b.p); said(h, "term -1 outside"); }
    { Array<dp_hold> b(std::vector<dp_hold>(1, dp_hold{1, 0.f, 0.f, 0.1f})); drag_poser_set_holds(h, 1, b.p); fine(h); }
    { Array<dp_term> t(table(1)); drag_poser_set_terms(h, 1, t.p, 1); said(h, "a hold refers to term 1"); } // (the table may not shrink under a hold)
    // gaps
    drag_poser_set_gaps(h, -1, 0.9f); said(h, "maxHold -1 outside 0..65535");
    drag_poser_set_gaps(h, 65536, 0.9f); said(h, "maxHold 65536");
    drag_poser_set_gaps(h, 3, 0.f); said(h, "decay");
    drag_poser_set_gaps(h, 3, 1.5f); said(h, "decay");
    drag_poser_set_gaps(h, 3, __builtin_nanf("")); said(h, "decay");
    drag_poser_set_gaps(h, 3, __builtin_inff()); said(h, "decay");
    drag_poser_set_gaps(h, 5, 0.9f); fine(h);
    // the predictor: coeffs in a block of exactly order * 576 floats, the bias in one of 24
    {
        Array<float> A(std::vector<float>(4 * 576, 0.01f)), c(std::vector<float>(24, 0.f));
        drag_poser_set_latent_ar(h, 5, A.p, c.p); said(h, "order 5 outside 0..4");
        drag_poser_set_latent_ar(h, -1, A.p, c.p); said(h, "order -1");
        drag_poser_set_latent_ar(h, 2, nullptr, c.p); said(h, "NULL coeffs or bias");
        drag_poser_set_latent_ar(h, 2, A.p, nullptr); said(h, "NULL coeffs or bias");
        drag_poser_set_latent_ar(h, 4, A.p, c.p); fine(h);
    }
    { Array<float> A(std::vector<float>(1 * 576, 0.01f)), c(std::vector<float>(24, 0.f)); drag_poser_set_latent_ar(h, 1, A.p, c.p); fine(h); }
    drag_poser_set_latent_ar(h, 0, nullptr, nullptr); fine(h); // off
}

void latent_ar_files(DragPoser* h, const std::string& dir)
{
    const auto load = [&](const std::string& path) { std::vector<char> p(path.begin(), path.end()); p.push_back('\0'); drag_poser_load_latent_ar(h, p.data()); };
    const std::vector<Spec> good = {{"coeffs", {2, 24, 24}}, {"bias", {24}}};
    load(write_bin(dir + "/good.bin", good)); fine(h);
    load(dir + "/absent.bin"); said(h, "cannot open");
    load(write_bin(dir + "/cut_data.bin", good, 4 + 4 + 4 + 6 + 4 + 12 + 100)); said(h, "truncated");
    load(write_bin(dir + "/cut_dims.bin", good, 4 + 4 + 4 + 6 + 4 + 5)); said(h, "truncated");
    load(write_bin(dir + "/cut_head.bin", good, 6)); said(h, "not a DPM1");
    load(write_bin(dir + "/rank.bin", {{"coeffs", {2, 576}}, {"bias", {24}}})); said(h, "rank");
    load(write_bin(dir + "/rank0.bin", {{"coeffs", {2, 24, 24}}, {"bias", {}}})); said(h, "rank");
    load(write_bin(dir + "/dims.bin", {{"coeffs", {2, 24, 23}}, {"bias", {24}}})); said(h, "[order][24][24]");
    load(write_bin(dir + "/dims_bias.bin", {{"coeffs", {2, 24, 24}}, {"bias", {25}}})); said(h, "[order][24][24]");
    load(write_bin(dir + "/order5.bin", {{"coeffs", {5, 24, 24}}, {"bias", {24}}})); said(h, "order 5 outside 1..4");
    load(write_bin(dir + "/order0.bin", {{"coeffs", {0, 24, 24}}, {"bias", {24}}})); said(h, "order 0 outside 1..4");
    load(write_bin(dir + "/count.bin", {{"coeffs", {1, 24, 24}}, {"bias", {24}}, {"extra", {1}}})); said(h, "expected the two tensors");
    load(write_bin(dir + "/names.bin", {{"coeffs", {1, 24, 24}}, {"bios", {24}}})); said(h, "expected the two tensors");
    load(write_bin(dir + "/name_len.bin", good, -1, 0xFFFFFFF0u)); said(h, "truncated");
    load(write_bin(dir + "/huge_dims.bin", {{"coeffs", {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}}}, 4 + 4 + 4 + 6 + 4 + 12)); said(h, "truncated");
    load(write_bin(dir + "/good4.bin", {{"coeffs", {4, 24, 24}}, {"bias", {24}}})); fine(h); // (the last accepted model stays)
}

// one well-formed frame with `present`: this link has no kernel unit, so the frame fails and must leave the handle as it was
void a_frame(DragPoser* h, int nEE)
{
    float before[24], after[24];
    drag_poser_get_latent(h, before);
    const int iters = drag_poser_last_iterations(h), status = drag_poser_last_status(h);
    std::vector<dp_float3> tp((size_t)nEE, dp_float3{0.1f, 0.9f, 0.2f});
    tp[1].y = __builtin_nanf(""); // (a sample lost through NaN travels as it is)
    Array<dp_float3> P(tp);
    Array<dp_quaternion> Q(std::vector<dp_quaternion>((size_t)nEE, dp_quaternion{0.5f, 0.5f, -0.5f, 0.5f}));
    std::vector<unsigned char> pr((size_t)nEE, 1);
    pr[nEE - 1] = 0;
    Array<unsigned char> present(pr);
    Array<dp_quaternion> pose(std::vector<dp_quaternion>(22, dp_quaternion{9.f, 9.f, 9.f, 9.f}));
    Array<dp_float3> pos(std::vector<dp_float3>(1, dp_float3{9.f, 9.f, 9.f}));
    drag_pose_present(h, nEE, P.p, Q.p, present.p, pose.p, pos.p);
    said(h, "dp_cons_live.hip"); // "this library was linked without ..."
    drag_pose_present(h, nEE, P.p, Q.p, nullptr, pose.p, pos.p);
    said(h, "dp_cons_live.hip");
    drag_pose_present(h, nEE - 1, P.p, Q.p, present.p, pose.p, pos.p);
    said(h, "nEndEffectors differs");
    drag_poser_get_latent(h, after);
    CHECK(std::memcmp(before, after, sizeof(before)) == 0);
    CHECK(drag_poser_last_iterations(h) == iters && drag_poser_last_status(h) == status);
    CHECK(pose.p[0].w == 9.f && pose.p[21].z == 9.f && pos.p[0].x == 9.f); // nothing was returned
    unsigned char codes[22];
    std::memset(codes, 7, sizeof(codes));
    drag_poser_get_gap_codes(h, codes);
    for (int j = 0; j < 22; ++j) CHECK(codes[j] == 0);
    Array<float> rows(std::vector<float>(4, 7.f)); // one hold: exactly [1][4]
    drag_poser_get_hold_state(h, rows.p);
    for (int c = 0; c < 4; ++c) CHECK(rows.p[c] == 0.f);
    n_checks += 3;
}

} // namespace

int main(int argc, char** argv)
{
    CHECK(argc == 5);
    const std::string scratch = argv[4];
    DragPoser* h = init_drag_poser();
    CHECK(h);
    setters_before_load_models(h);
    fake_hip_mode(true);
    set_reference_skeleton(h, argv[1]); fine(h);
    load_models(h, argv[2]); fine(h);
    CHECK(drag_poser_has_temporal(h) == 0);
    float mask[22] = {0.f};
    dp_float2 w[22];
    const int tracked[6] = {0, 4, 8, 13, 17, 21};
    for (int j = 0; j < 22; ++j) w[j] = dp_float2{1.f, 1.f};
    for (int j : tracked) mask[j] = 1.f;
    set_mask_and_weights(h, mask, w);
    set_optim_params(h, 1e-4f, 1e-2f, 10, 1e-2f);
    init_drag_model(h, dp_float3{0.1f, 0.2f, 0.3f}, dp_quaternion{1.f, 0.f, 0.f, 0.f}); fine(h);
    {   // nothing configured yet: `present` has nothing to belong to
        Array<dp_float3> P(std::vector<dp_float3>(6, dp_float3{0.f, 1.f, 0.f}));
        Array<dp_quaternion> Q(std::vector<dp_quaternion>(6, dp_quaternion{1.f, 0.f, 0.f, 0.f}));
        Array<unsigned char> present(std::vector<unsigned char>(6, 1));
        Array<dp_quaternion> pose(std::vector<dp_quaternion>(22, dp_quaternion{9.f, 9.f, 9.f, 9.f}));
        Array<dp_float3> pos(std::vector<dp_float3>(1, dp_float3{9.f, 9.f, 9.f}));
        drag_pose_present(h, 6, P.p, Q.p, present.p, pose.p, pos.p);
        said(h, "`present` belongs to the gaps");
    }
    setters(h);
    latent_ar_files(h, scratch);
    set_lambdas(h, 1.f, 0.02f, 0); fine(h); // a predictor is configured: nothing to report
    a_frame(h, 6);
    // both states are zeroed where the header says so, on blocks of exactly their size
    float z[24];
    drag_poser_get_latent(h, z);
    drag_poser_set_latent(h, z); // (it reports through the same message but does not clear it: as before)
    init_drag_model(h, dp_float3{0.f, 0.f, 0.f}, dp_quaternion{1.f, 0.f, 0.f, 0.f}); fine(h);
    load_models(h, argv[2]); fine(h); // again: the device blocks are replaced and the additions forgotten
    { Array<dp_hold> b(std::vector<dp_hold>(1, dp_hold{0, 0.f, 0.f, 0.1f})); drag_poser_set_holds(h, 1, b.p); said(h, "term 0 outside the table of 0"); }
    destroy_drag_poser(h);

    // beside a loaded temporal model the predictor is refused: the targets have one source
    DragPoser* g = init_drag_poser();
    set_reference_skeleton(g, argv[1]); fine(g);
    load_models(g, argv[3]); fine(g);
    CHECK(drag_poser_has_temporal(g) == 1);
    {
        Array<float> A(std::vector<float>(2 * 576, 0.01f)), c(std::vector<float>(24, 0.f));
        drag_poser_set_latent_ar(g, 2, A.p, c.p);
        said(g, "the targets have one source");
        drag_poser_set_latent_ar(g, 0, A.p, c.p); fine(g);
    }
    {
        const std::string good = scratch + "/good.bin";
        std::vector<char> p(good.begin(), good.end());
        p.push_back('\0');
        drag_poser_load_latent_ar(g, p.data());
        said(g, "the targets have one source");
    }
    destroy_drag_poser(g);
    CHECK(fake_hip_outstanding() == 0);
    std::printf("unity live: %d checks, all checks held\n", n_checks);
    return 0;
}
