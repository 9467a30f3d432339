// main.cpp -- a stand-alone program that drives the library's host code (dp_host.cpp, dp_w16_host.cpp, dp_encoder_host.cpp,
// dp_temporal_host.cpp) under AddressSanitizer / UndefinedBehaviorSanitizer with fake_hip.cpp in place of the HIP runtime and the kernel units.
// tests/test_host_san.py builds and runs it; it needs no GPU and is linked into nothing else.  Exit status 0: every check held (and the
// sanitizers, LeakSanitizer at exit included, stayed silent).
//
// Every buffer the library reads or writes is a heap block of EXACTLY the documented size (std::vector / malloc), so that one element too many
// is a sanitizer report.  Strict part: any runtime call aborts.  Fake part: create / destroy of the three handles with every allocation failing
// in turn.
#include <new>
#include <random>
#include <stdexcept>

#include "../../include/dragposer.h"
#include "../../include/dragposer_constraints.h"
#include "../../include/dragposer_encoder.h"
#include "../../include/dragposer_grad.h"
#include "../../include/dragposer_skeleton.h"
#include "../../include/dragposer_terms.h"
#include "../../dragposer_amd/csrc/dp_host_rt.h"
#include "../../dragposer_amd/csrc/dp_kernel.h"
#include "san_support.h"

// fake_hip.cpp's controls
void fake_hip_mode(bool fake);
void fake_hip_fail_allocation(int k); // the k-th allocation from now fails (0: none); restarts the count
int fake_hip_allocations();
int fake_hip_outstanding();
int fake_hip_current_device();
void fake_hip_set_current_device(int d);

// the library's private hooks
extern "C" {
int dp_debug_pack(const dp_folded*, const int*, float*, float*, unsigned*);
int dp_debug_pack_w4(const dp_folded*, const dp_model*, float*, float*);
int dp_debug_pack_w4_bp(const dp_folded*, const dp_model*, float*, float*);
int dp_debug_pairs_w4(const dp_model*, void*);
int dp_debug_pairs_w4_bp(const dp_model*, void*);
int dp_debug_items(const dp_model*, void*);
int dp_debug_encoder_image(const dp_encoder_folded*, float*, int*, int);
int dp_temporal_debug_pack(const dp_temporal_model*, float*, int);
}

namespace {

std::mt19937 g_rng(1234);
std::vector<float> randv(size_t n, float lo = -0.5f, float hi = 0.5f)
{
    std::uniform_real_distribution<float> d(lo, hi);
    std::vector<float> v(n);
    for (float& x : v) x = d(g_rng);
    return v;
}
bool has(const char* msg, const char* part) { return msg && std::strstr(msg, part) != nullptr; }

// ---------------------------------------------------------------------------------------------- the exception shell
struct Handle { int device = -1; std::string err; };

void test_shell()
{
    Handle h, *none = nullptr;
    for (int kind = 0; kind < 3; ++kind) {
        const auto body = [&]() -> int {
            if (kind == 0) throw std::bad_alloc();
            if (kind == 1) throw std::runtime_error("boom");
            throw 7;
        };
        h.err = "before";
        CHECK(dprt::shell(&h, "entry_point", body) == DP_ERR_INVALID);
        CHECK(h.err == "entry_point: host-side failure");
        dprt::fail(none, DP_OK, "before");
        CHECK(dprt::shell(none, "a_create", body) == DP_ERR_INVALID);
        CHECK(std::string(dprt::last_error(none)) == "a_create: host-side failure");
        CHECK(h.err == "entry_point: host-side failure"); // (the two slots are apart)
    }
    CHECK(dprt::shell(&h, "entry_point", [] { return 5; }) == 5 && h.err == "entry_point: host-side failure"); // (no exception: nothing written)
}

// ---------------------------------------------------------------------------------------------- decoder packers
const int XSENS[22] = {0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 12, 11, 14, 15, 16, 11, 18, 19, 20};
const int TWO_LEVELS[22] = {0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 12, 10, 14, 15, 16, 9, 18, 19, 20};   // tests/test_hip_topology.py
const int FOUR_LIMBS[22] = {0, 0, 1, 2, 3, 4, 3, 6, 3, 8, 3, 10, 0, 12, 13, 14, 15, 16, 17, 0, 19, 20};    // tests/test_hip_topology.py
const int PARENT_NOT_BELOW[22] = {0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 12, 11, 15, 15, 16, 11, 18, 19, 20}; // parents[15] = 15
const int FOUR_ROOT_CHILDREN[22] = {0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 12, 11, 14, 15, 16, 0, 18, 19, 20};
const int CHAIN_OF_EIGHT[22] = {0, 0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 12, 11, 14, 15, 16, 11, 18, 19, 20}; // bones 1 .. 8 in a row

struct Model { // a synthetic decoder: random weights, masks of ones; every tensor a heap block of its documented size
    std::vector<float> fw, fb, up[3], cw[3], cm[3], cb[3], mq, sq, md, sd, off;
    std::vector<int> par;
    dp_model m{};
    explicit Model(const int* parents)
    {
        const int d[4] = {24, 40, 60, 92};
        fw = randv(24 * 24); fb = randv(24);
        for (int l = 0; l < 3; ++l) {
            up[l] = randv((size_t)d[l + 1] * d[l]); cw[l] = randv((size_t)d[l + 1] * d[l + 1]);
            cm[l].assign((size_t)d[l + 1] * d[l + 1], 1.f); cb[l] = randv(d[l + 1]);
            m.unpool_w[l] = up[l].data(); m.conv_w[l] = cw[l].data(); m.conv_mask[l] = cm[l].data(); m.conv_b[l] = cb[l].data();
        }
        mq = randv(88); sq = randv(88, 0.1f, 1.f); md = randv(3); sd = randv(3, 0.1f, 1.f); off = randv(66);
        par.assign(parents, parents + 22);
        m.f_latent_w = fw.data(); m.f_latent_b = fb.data(); m.mean_q = mq.data(); m.std_q = sq.data(); m.mean_disp = md.data();
        m.std_disp = sd.data(); m.parents = par.data(); m.offsets = off.data(); m.weight_dtype = DP_WEIGHTS_FP32;
    }
};

// every packer on one tree: `expect` for the calls that depend on the tree, `w16` for dp_debug_pack_w16 (the Xsens tree only)
void test_decoder_packers(const int* parents, int expect, int expect_items, int w16)
{
    Model M(parents);
    std::vector<dp_folded> f(1);
    CHECK(dp_fold_decoder(&M.m, f.data()) == DP_OK);
    std::vector<float> wfrag((size_t)dpl::NWAVE * dpl::W_REGS * 64), bias(128);
    std::vector<unsigned> smask((size_t)dpl::NWAVE * dpl::NGEMM);
    CHECK(dp_debug_pack(f.data(), M.m.parents, wfrag.data(), bias.data(), smask.data()) == expect);
    std::vector<float> img(dpw4::IMG_FLOATS), b4(dpw4::BIAS_FLOATS);
    CHECK(dp_debug_pack_w4(f.data(), &M.m, img.data(), b4.data()) == expect);
    const int bp = dp_debug_pack_w4_bp(f.data(), &M.m, img.data(), b4.data()); // (dense random weights do not fit the body-part layout)
    CHECK(bp == (expect == DP_OK ? (int)DP_ERR_UNSUPPORTED : expect));
    std::vector<dpl::ItemConst> items(32);
    CHECK(dp_debug_items(&M.m, items.data()) == expect_items);
    std::vector<dpw4::Pair> pairs(16);
    CHECK(dp_debug_pairs_w4(&M.m, pairs.data()) == expect_items);
    CHECK(dp_debug_pairs_w4_bp(&M.m, pairs.data()) == expect_items);
    std::vector<unsigned> img16(dpw16::IMG_U32);
    std::vector<float> b16(dpw16::BIAS_FLOATS);
    std::vector<dpw16::SlotConst> slots((size_t)dpw16::NTY * 4);
    CHECK(dp_debug_pack_w16(f.data(), &M.m, img16.data(), b16.data(), slots.data()) == w16);
    if (expect != DP_OK) CHECK(dp_last_error(nullptr)[0] != '\0');
}

// ---------------------------------------------------------------------------------------------- encoder
struct EncModel {
    std::vector<float> cw[3], cm[3], cb[3], pw[3], mw, mb, lw, lb;
    dp_encoder_model m = DP_ENCODER_MODEL_INIT;
    EncModel()
    {
        const int mid[3] = {176, 112, 72}, rows[3] = {112, 72, 48};
        for (int l = 0; l < 3; ++l) {
            cw[l] = randv((size_t)mid[l] * mid[l]); cm[l].assign((size_t)mid[l] * mid[l], 1.f); cb[l] = randv(mid[l]);
            pw[l] = randv((size_t)rows[l] * mid[l]);
            m.conv_w[l] = cw[l].data(); m.conv_mask[l] = cm[l].data(); m.conv_b[l] = cb[l].data(); m.pool_w[l] = pw[l].data();
        }
        mw = randv(24 * 48); mb = randv(24); lw = randv(24 * 48); lb = randv(24);
        m.f_mu_w = mw.data(); m.f_mu_b = mb.data(); m.f_logvar_w = lw.data(); m.f_logvar_b = lb.data();
    }
};

void test_encoder()
{
    EncModel E;
    std::vector<dp_encoder_folded> f(1);
    CHECK(dp_fold_encoder(&E.m, f.data()) == DP_OK);
    const int words = dp_debug_encoder_image(f.data(), nullptr, nullptr, 0);
    CHECK(words > 0);
    std::vector<float> image(words);
    std::vector<int> table((size_t)3 * words);
    CHECK(dp_debug_encoder_image(f.data(), image.data(), table.data(), words) == words);
    std::vector<float> shorter(words - 1);
    CHECK(dp_debug_encoder_image(f.data(), shorter.data(), nullptr, words - 1) == DP_ERR_INVALID);
    CHECK(has(dp_encoder_last_error(nullptr), "capacity below"));
}

// ---------------------------------------------------------------------------------------------- predictor
struct TemporalModel {
    std::vector<std::vector<float>> store; // every tensor a block of its documented size
    std::vector<dp_temporal_layer> enc, dec;
    dp_temporal_model m{};
    const float* t(size_t n) { store.push_back(randv(n)); return store.back().data(); }
    TemporalModel(int n_enc, int n_dec, int F, int nh)
    {
        const int D = DP_TEMPORAL_D_MODEL;
        m.n_heights = nh; m.dim_feedforward = F; m.n_encoder_layers = n_enc; m.n_decoder_layers = n_dec; m.max_len = 64; m.sample_step = 4;
        m.in_proj_encoder_w = t((size_t)D * (24 + 3 + nh)); m.in_proj_encoder_b = t(D);
        m.in_proj_decoder_w = t(D * 24); m.in_proj_decoder_b = t(D);
        m.out_proj_w = t(24 * D); m.out_proj_b = t(24);
        m.pos_encoding = t((size_t)m.max_len * D);
        m.enc_norm_w = t(D); m.enc_norm_b = t(D); m.dec_norm_w = t(D); m.dec_norm_b = t(D);
        m.means_latent = t(24); m.stds_latent = t(24);
        const auto layer = [&](bool is_dec) {
            dp_temporal_layer L{};
            L.sa_in_w = t(3 * D * D); L.sa_in_b = t(3 * D); L.sa_out_w = t(D * D); L.sa_out_b = t(D);
            if (is_dec) { L.ca_in_w = t(3 * D * D); L.ca_in_b = t(3 * D); L.ca_out_w = t(D * D); L.ca_out_b = t(D); L.norm3_w = t(D); L.norm3_b = t(D); }
            L.lin1_w = t((size_t)F * D); L.lin1_b = t(F); L.lin2_w = t((size_t)D * F); L.lin2_b = t(D);
            L.norm1_w = t(D); L.norm1_b = t(D); L.norm2_w = t(D); L.norm2_b = t(D);
            return L;
        };
        for (int l = 0; l < n_enc; ++l) enc.push_back(layer(false));
        for (int l = 0; l < n_dec; ++l) dec.push_back(layer(true));
        m.enc = enc.data(); m.dec = dec.data();
    }
};

void test_temporal_pack(int n_enc, int n_dec, int F, int nh)
{
    TemporalModel T(n_enc, n_dec, F, nh);
    const int n = dp_temporal_debug_pack(&T.m, nullptr, 0);
    CHECK(n > 0);
    std::vector<float> image(n);
    CHECK(dp_temporal_debug_pack(&T.m, image.data(), n) == n);
    CHECK(dp_temporal_debug_pack(&T.m, image.data(), n - 1) == DP_ERR_INVALID);
    T.dec.back().norm3_b = nullptr; // a NULL tensor
    CHECK(dp_temporal_debug_pack(&T.m, image.data(), n) == DP_ERR_INVALID);
    CHECK(has(dp_temporal_last_error(nullptr), "NULL tensor"));
}

// ---------------------------------------------------------------------------------------------- sized structs
// A T as a caller built from another header would hand it over: `size` bytes in a heap block of exactly that size (zero beyond the fields
// this header knows), struct_size = size.
template <class T>
struct Sized {
    void* block;
    Sized(const T& init, unsigned size) : block(std::calloc(1, size))
    {
        std::memcpy(block, &init, size < sizeof(T) ? size : sizeof(T));
        std::memcpy(block, &size, sizeof(size));
    }
    ~Sized() { std::free(block); }
    Sized(const Sized&) = delete;
    const T* get() const { return (const T*)block; }
};

struct Call { // the well-formed arguments of every entry point, and the sizes of this call's sized structs (0: sizeof)
    unsigned params = 0, result = 0, seq_results = 0, skel = 0, grad = 0, cons = 0, terms = 0;
    int n_terms = 1;
    bool pre05_params = false; // dp_params as a 0.4 caller has it: 52 bytes that start with n_iter = 100 and lr
};

// one entry point (by index) with the structs at the sizes `c` asks for; returns its code
int call(dp_ctx* ctx, int ep, const Call& c)
{
    dp_batch b{4, PTR, PTR, PTR, PTR, PTR, PTR, (const unsigned char*)PTR};
    dp_params p0 = DP_PARAMS_INIT;
    p0.n_iter = 10; p0.lr = 1e-2f; p0.beta1 = 0.9f; p0.beta2 = 0.999f; p0.eps = 1e-8f; p0.lambda_rot = 1.f; p0.lambda_tmp = 0.02f;
    dp_result r0 = DP_RESULT_INIT;
    r0.z = r0.z_pre = r0.pose = r0.disp = r0.world_disp = r0.world_rot = r0.pos = r0.rot = r0.loss = PTR;
    dp_seq_results q0 = DP_SEQ_RESULTS_INIT;
    q0.pose_ret = q0.pos_ret = q0.world_rot = q0.loss = q0.hist_scratch = PTR;
    dp_skeleton_in s0 = DP_SKELETON_IN_INIT;
    s0.offsets = PTR; s0.stride = DP_SKELETON_STRIDE;
    dp_grad_in g0 = DP_GRAD_IN_INIT;
    g0.pos = PTR;
    dp_constraints c0 = DP_CONSTRAINTS_INIT;
    c0.loss_extra = PTR;
    std::vector<dp_term> table(c.n_terms, dp_term DP_TERM_INIT); // (a block of exactly n_terms terms)
    for (dp_term& t : table) { t.type = DP_TERM_PLANE; t.joint_a = 3; t.weight = 1.f; }
    dp_terms t0 = DP_TERMS_INIT;
    t0.n_terms = c.n_terms; t0.terms = table.data(); t0.global_pos = PTR; t0.loss_terms = PTR;
    Sized<dp_params> p(p0, c.params ? c.params : sizeof(p0));
    if (c.pre05_params) {
        const struct { int n_iter; float lr; float rest[11]; } old{100, 1e-2f, {}};
        static_assert(sizeof(old) == 52, "the 0.4 layout");
        std::free(p.block);
        p.block = std::malloc(52);
        std::memcpy(p.block, &old, 52);
    }
    const Sized<dp_result> r(r0, c.result ? c.result : sizeof(r0));
    const Sized<dp_seq_results> q(q0, c.seq_results ? c.seq_results : sizeof(q0));
    const Sized<dp_skeleton_in> s(s0, c.skel ? c.skel : sizeof(s0));
    const Sized<dp_grad_in> g(g0, c.grad ? c.grad : sizeof(g0));
    const Sized<dp_constraints> cs(c0, c.cons ? c.cons : sizeof(c0));
    const Sized<dp_terms> ts(t0, c.terms ? c.terms : sizeof(t0));
    dp_seq_frames fr{};
    fr.n_steps = 3; fr.tgt_pos = fr.tgt_rot = fr.tgt_root = fr.w = fr.z_tgt = PTR; fr.tracked = (const unsigned char*)PTR; fr.z_tgt_step = 24;
    dp_seq_state st{PTR, PTR, PTR, PTR, PTR, 4, 2, {4, 8}};
    dp_seq_step adj{};
    adj.adjust_joint = -1;
    switch (ep) {
    case 0: return dp_optimize(ctx, &b, p.get(), r.get(), nullptr);
    case 1: return dp_optimize_skeleton(ctx, &b, p.get(), s.get(), r.get(), nullptr);
    case 2: return dp_forward(ctx, 4, PTR, PTR, r.get(), nullptr);
    case 3: return dp_forward_skeleton(ctx, 4, PTR, PTR, s.get(), r.get(), nullptr);
    case 4: return dp_optimize_sequence(ctx, 2, PTR, &fr, p.get(), &st, &adj, q.get(), nullptr);
    case 5: return dp_optimize_sequence_skeleton(ctx, 2, PTR, &fr, p.get(), s.get(), &st, &adj, q.get(), nullptr);
    case 6: return dp_forward_vjp(ctx, 4, PTR, PTR, g.get(), PTR, PTR, nullptr, nullptr);
    case 7: return dp_forward_vjp_skeleton(ctx, 4, PTR, PTR, s.get(), g.get(), PTR, PTR, PTR, nullptr, nullptr);
    case 8: return dp_optimize_constrained(ctx, &b, p.get(), cs.get(), r.get(), nullptr);
    case 9: return dp_optimize_constrained_skeleton(ctx, &b, p.get(), cs.get(), s.get(), r.get(), nullptr);
    case 10: return dp_optimize_terms(ctx, &b, p.get(), ts.get(), r.get(), nullptr);
    default: return dp_optimize_terms_skeleton(ctx, &b, p.get(), ts.get(), s.get(), r.get(), nullptr);
    }
}
constexpr int N_EP = 12;
// which sized structs an entry point takes: bit 0 params, 1 result, 2 seq_results, 3 skeleton, 4 grad_in, 5 constraints, 6 terms
const unsigned TAKES[N_EP] = {3, 3 | 8, 2, 2 | 8, 1 | 4, 1 | 4 | 8, 16, 16 | 8, 3 | 32, 3 | 32 | 8, 3 | 64, 3 | 64 | 8};

void test_sized_structs()
{
    dp_ctx* ctx = nullptr;
    CHECK(dp_debug_host_ctx(&ctx) == DP_OK && ctx);
    // (each struct's minimum: its first version ends with the named field)
    const unsigned mins[7] = {offsetof(dp_params, kernel) + sizeof(int), offsetof(dp_result, clock) + sizeof(void*),
                              offsetof(dp_seq_results, status) + sizeof(void*), offsetof(dp_skeleton_in, stride) + sizeof(int),
                              offsetof(dp_grad_in, rot) + sizeof(void*), offsetof(dp_constraints, loss_extra) + sizeof(void*),
                              offsetof(dp_terms, loss_terms) + sizeof(void*)};
    const unsigned sizeofs[7] = {sizeof(dp_params), sizeof(dp_result), sizeof(dp_seq_results), sizeof(dp_skeleton_in), sizeof(dp_grad_in),
                                 sizeof(dp_constraints), sizeof(dp_terms)};
    unsigned Call::* const field[7] = {&Call::params, &Call::result, &Call::seq_results, &Call::skel, &Call::grad, &Call::cons, &Call::terms};
    for (int ep = 0; ep < N_EP; ++ep) {
        CHECK(call(ctx, ep, Call{}) == DP_ERR_DEVICE); // well-formed: refused for the missing device image, after every check
        CHECK(has(dp_last_error(ctx), "no device image"));
        for (int k = 0; k < 7; ++k) {
            if (!(TAKES[ep] >> k & 1)) continue;
            const struct { unsigned size; int expect; } tries[5] = {{mins[k], DP_ERR_DEVICE}, {sizeofs[k], DP_ERR_DEVICE}, {mins[k] - 1, DP_ERR_INVALID},
                                                                    {4096, DP_ERR_DEVICE}, {4097, DP_ERR_INVALID}};
            for (const auto& t : tries) {
                Call c;
                c.*field[k] = t.size;
                CHECK(call(ctx, ep, c) == t.expect);
                if (t.expect == DP_ERR_INVALID) CHECK(has(dp_last_error(ctx), "struct_size"));
            }
        }
        if (TAKES[ep] & 1) { // refused on the struct's first two words: nothing beyond byte 52 is read
            Call c;
            c.pre05_params = true;
            CHECK(call(ctx, ep, c) == DP_ERR_INVALID && has(dp_last_error(ctx), "pre-0.5"));
        }
        if (TAKES[ep] & 64) {
            Call c;
            c.n_terms = 16;
            CHECK(call(ctx, ep, c) == DP_ERR_DEVICE);
            c.n_terms = 17;
            CHECK(call(ctx, ep, c) == DP_ERR_INVALID && has(dp_last_error(ctx), "n_terms"));
        }
    }
    CHECK(dp_destroy(ctx) == DP_OK); // (a context without a device: no runtime call, or strict mode would have aborted)
}

// ---------------------------------------------------------------------------------------------- fake mode: create / destroy
// create(&handle) with the k-th allocation failing, k = 1 .. n_alloc: DP_ERR_DEVICE, *out NULL, nothing left allocated, the current device kept
template <class H, class Create, class Destroy>
void test_create(const char* who, int n_alloc, Create create, Destroy destroy, const char* (*last_error)(const H*))
{
    for (int current = 0; current < 2; ++current) { // the handle goes on device 0; the thread's current device is 0, then 1
        fake_hip_set_current_device(current);
        fake_hip_fail_allocation(0);
        H* h = nullptr;
        CHECK(create(&h) == DP_OK && h);
        CHECK(fake_hip_allocations() == n_alloc && fake_hip_outstanding() == n_alloc && fake_hip_current_device() == current);
        CHECK(destroy(h) == DP_OK);
        CHECK(fake_hip_outstanding() == 0 && fake_hip_current_device() == current);
        for (int k = 1; k <= n_alloc; ++k) {
            fake_hip_fail_allocation(k);
            h = (H*)PTR;
            CHECK(create(&h) == DP_ERR_DEVICE);
            CHECK(h == nullptr && fake_hip_outstanding() == 0 && fake_hip_current_device() == current);
            CHECK(has(last_error(nullptr), who));
        }
    }
    fake_hip_fail_allocation(0);
}

} // namespace

int main()
{
    // ---- strict: no runtime call
    test_shell();
    test_decoder_packers(XSENS, DP_OK, DP_OK, DP_OK);
    test_decoder_packers(TWO_LEVELS, DP_OK, DP_OK, DP_ERR_UNSUPPORTED);
    test_decoder_packers(FOUR_LIMBS, DP_OK, DP_OK, DP_ERR_UNSUPPORTED);
    test_decoder_packers(PARENT_NOT_BELOW, DP_ERR_INVALID, DP_ERR_INVALID, DP_ERR_UNSUPPORTED);
    test_decoder_packers(FOUR_ROOT_CHILDREN, DP_ERR_UNSUPPORTED, DP_ERR_UNSUPPORTED, DP_ERR_UNSUPPORTED);
    test_decoder_packers(CHAIN_OF_EIGHT, DP_OK, DP_ERR_UNSUPPORTED, DP_ERR_UNSUPPORTED); // (the chain's depth is the items' limit, not the packers')
    test_encoder();
    test_temporal_pack(3, 3, 2048, 6); // the reference architecture
    test_temporal_pack(3, 3, 40, 6);   // F no multiple of 32
    test_temporal_pack(3, 3, 2048, 0);
    test_temporal_pack(3, 3, 2048, 8);
    test_temporal_pack(1, 1, 2048, 6);
    test_temporal_pack(8, 8, 2048, 6);
    test_sized_structs();

    // ---- fake: one gfx950 device
    fake_hip_mode(true);
    {
        Model M(XSENS);
        test_create<dp_ctx>("dp_create", 10, [&](dp_ctx** out) { return dp_create(out, &M.m, 0); }, dp_destroy, dp_last_error);
        Model M2(FOUR_LIMBS); // (no dp_w16 image: seven allocations)
        test_create<dp_ctx>("dp_create", 7, [&](dp_ctx** out) { return dp_create(out, &M2.m, 0); }, dp_destroy, dp_last_error);
    }
    {
        TemporalModel T(3, 3, 2048, 6);
        test_create<dp_temporal>("dp_temporal_create", 3, [&](dp_temporal** out) { return dp_temporal_create(out, &T.m, 0); }, dp_temporal_destroy,
                                 dp_temporal_last_error);
    }
    {
        EncModel E;
        test_create<dp_encoder>("dp_encoder_create", 1, [&](dp_encoder** out) { return dp_encoder_create(out, &E.m, 0); }, dp_encoder_destroy,
                                dp_encoder_last_error);
    }
    std::puts("host_san: all checks held");
    return 0;
}
