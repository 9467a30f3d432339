// dp_temporal_host.cpp -- host side of the temporal predictor (include/dragposer.h: dp_temporal_*): the handle, the packer of the kernel's
// weight image (layout: dp_temporal.h and the comments at its readers in dp_temporal.hip), the choice of the kernel variant, the private
// test hooks that are host arithmetic.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dragposer.h"
#include "dp_host_rt.h"
#include "dp_temporal.h"

using namespace dpt;
using dprt::fail;
using dprt::shell;

struct dp_temporal {
    int device = -1, n_cu = 256;
    int forced_variant = 0; // dp_temporal_debug_force_variant (private test hook, below): 21, 41 or 42 (waves per SIMD, sequences
                            // per workgroup) = that kernel variant whatever the batch; 0 = chosen from the batch (the product)
    dprt::DeviceBuf<float> d_w;
    dprt::DeviceBuf<unsigned char> d_xch; // the teams' exchange area: [n_cu / 2 teams][2][XCH_GRANULES][XCH_GMAX] granules, the teams' tag counters, the status word
    size_t xch_granule_bytes = 0;
    dprt::MappedWord h_status; // page-locked host mirror of the status word (written by the device on a team time-out, read here without a synchronise)
    int status_seen = 0;     // DP_TEMPORAL_* bits ever seen in it (sticky)
    bool teams_off = false;  // no team launches any more: a time-out was reported, or the TEAM kernel does not fit a CU of this device
    int poll_limit = XCH_POLL_LIMIT, dbg_skip_team = -1, dbg_skip_member = -1; // dp_temporal_debug_team_fault (private test hook)
    TArgs args{};
    std::string err;
};
constexpr dp_temporal* NO_HANDLE = nullptr; // (its messages go to the thread-local slot: dp_temporal_last_error(NULL))

// float -> three bf16 terms with x = t0 + t1 + t2 exactly: the host's copy of the device's split_pair (round to nearest even at every stage, what
// v_cvt_pk_bf16_f32 does; the remainders are exact fp32 differences).  Weights are finite.
static unsigned host_bf16_rne(float x)
{
    unsigned u;
    std::memcpy(&u, &x, 4);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
static float host_bf16_val(unsigned h)
{
    const unsigned u = h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static void host_split3(float x, unsigned (&t)[3])
{
    t[0] = host_bf16_rne(x);
    const float r = x - host_bf16_val(t[0]);
    t[1] = host_bf16_rne(r);
    const float q = r - host_bf16_val(t[1]);
    t[2] = host_bf16_rne(q);
}
// private test hook (host arithmetic only; a CPU test holds it to numpy): the three bf16 terms of x as 16-bit patterns
extern "C" void dp_temporal_debug_split3(float x, unsigned short* out3)
{
    unsigned t[3];
    host_split3(x, t);
    for (int k = 0; k < 3; ++k) out3[k] = (unsigned short)t[k];
}

extern "C" const char* dp_temporal_last_error(const dp_temporal* t) { return dprt::last_error(t); }

// The weight image of `m` (every tensor copied or packed into one float buffer) and the offsets into it (a: everything but w and the per-call
// fields).  DP_ERR_INVALID with a message in the thread-local slot for an architecture out of range or a NULL tensor.
static int pack_model(const dp_temporal_model* m, std::vector<float>& buf, TArgs& a)
{
    if (!m) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_temporal_create: model is NULL");
    if (m->n_heights < 0 || m->n_heights > DP_MAX_HEIGHT_JOINTS || m->dim_feedforward < 1 || m->sample_step < 1 || m->max_len < 1 ||
        m->n_encoder_layers < 1 || m->n_encoder_layers > MAXL || m->n_decoder_layers < 1 || m->n_decoder_layers > MAXL)
        return fail(NO_HANDLE, DP_ERR_INVALID, "dp_temporal_create: architecture out of range (layers 1..8, heights <= 8)");
    const int n_in = LAT + 3 + m->n_heights, F = m->dim_feedforward;
    buf.clear();
    bool null_seen = false;
    auto put = [&](const float* p, size_t n) { // plain copy
        const int off = (int)buf.size();
        if (!p) { null_seen = true; buf.resize(buf.size() + n, 0.f); return off; }
        buf.insert(buf.end(), p, p + n);
        return off;
    };
    auto putT = [&](const float* p, int rows_out, int cols_in, int ldk = 0) { // Linear.weight [out][in] as it is, rows padded with zeros to a multiple of 4 (or to ldk)
        while (buf.size() % 4) buf.push_back(0.f);               // floats and 16-byte aligned (lin: a lane reads KS consecutive floats of a row)
        const int off = (int)buf.size();
        if (ldk == 0) ldk = (cols_in + 3) / 4 * 4;
        buf.resize(buf.size() + (size_t)rows_out * ldk, 0.f);
        if (!p) { null_seen = true; return off; }
        for (int r = 0; r < rows_out; ++r)
            for (int c = 0; c < cols_in; ++c) buf[off + (size_t)r * ldk + c] = p[(size_t)r * cols_in + c];
        return off;
    };
    // feed-forward image (split precision: the comment above ffn_tile), per tile of 32 hidden units and lane (l16 = lane & 15, g = lane >> 4),
    // FFN_IMG_V 16-byte words of eight bf16 each (element j in bits 16 (j & 1) of word j >> 1), three words per operand = its hi / mid / lo terms:
    //   v = (t 2) 3 + term:           W1[32 nt + 16 t + l16][8 g + j]                                  (A of product 1: M-tile t, channels 0 .. 31)
    //   v = (t 2 + 1) 3 + {0, 1, 2}:  [hi | hi], [mid | mid], [lo | hi] of W1[32 nt + 16 t + l16][32 + 8 (g & 1) + j]: the first term in lanes g < 2,
    //                                 the second in lanes g >= 2                                       (channels 32 .. 47: two term pairs per MFMA)
    //   v = 12 + ct 3 + term:         W2[16 ct + l16][32 nt + 16 (j >> 2) + 4 g + (j & 3)]             (B of product 2: column tile ct)
    //   v = 21 + t (four floats):     bias1[32 nt + 16 t + 4 g + r]
    // hidden units beyond F and input channels beyond 47 are zeros (ReLU(0) = 0 contributes nothing)
    auto split3 = [&](float x, unsigned (&t)[3]) { host_split3(x, t); };
    auto pack_ffn = [&](const float* w1, const float* b1, const float* w2) {
        while (buf.size() % 4) buf.push_back(0.f); // 16-byte alignment of the image
        const int off = (int)buf.size(), ntiles = (F + FT - 1) / FT;
        buf.resize(buf.size() + (size_t)ntiles * FFN_TILE_FLOATS, 0.f);
        if (!w1 || !b1 || !w2) { null_seen = true; return off; }
        for (int nt = 0; nt < ntiles; ++nt)
            for (int lane = 0; lane < 64; ++lane) {
                const int l16 = lane & 15, g = lane >> 4;
                float* dst = buf.data() + off + (size_t)nt * FFN_TILE_FLOATS;
                auto put8 = [&](int v0, const float (&val)[8]) { // eight values -> the words v0 (hi), v0 + 1 (mid), v0 + 2 (lo) of this lane
                    unsigned words[3][4] = {};
                    for (int j = 0; j < 8; ++j) {
                        unsigned t[3];
                        split3(val[j], t);
                        for (int k = 0; k < 3; ++k) words[k][j >> 1] |= t[k] << (16 * (j & 1));
                    }
                    for (int k = 0; k < 3; ++k) std::memcpy(dst + ((v0 + k) * 64 + lane) * 4, words[k], 16);
                };
                for (int t = 0; t < 2; ++t) {
                    float val[8];
                    const int h = FT * nt + 16 * t + l16;
                    for (int j = 0; j < 8; ++j) val[j] = h < F ? w1[(size_t)h * D + 8 * g + j] : 0.f;
                    put8((t * 2) * 3, val);
                    // channels 32 .. 47: which TERM a lane holds depends on its half of the K-block
                    unsigned words[3][4] = {};
                    for (int j = 0; j < 8; ++j) {
                        unsigned tm[3];
                        split3(h < F ? w1[(size_t)h * D + 32 + 8 * (g & 1) + j] : 0.f, tm);
                        const unsigned pick[3] = {tm[0], tm[1], g < 2 ? tm[2] : tm[0]}; // [hi | hi], [mid | mid], [lo | hi]
                        for (int k = 0; k < 3; ++k) words[k][j >> 1] |= pick[k] << (16 * (j & 1));
                    }
                    for (int k = 0; k < 3; ++k) std::memcpy(dst + (((t * 2 + 1) * 3 + k) * 64 + lane) * 4, words[k], 16);
                }
                for (int ct = 0; ct < 3; ++ct) {
                    float val[8];
                    for (int j = 0; j < 8; ++j) {
                        const int h = FT * nt + 16 * (j >> 2) + 4 * g + (j & 3);
                        val[j] = h < F ? w2[(size_t)(16 * ct + l16) * F + h] : 0.f;
                    }
                    put8(12 + ct * 3, val);
                }
                for (int t = 0; t < 2; ++t)
                    for (int r = 0; r < 4; ++r) {
                        const int h = FT * nt + 16 * t + 4 * g + r;
                        dst[((21 + t) * 64 + lane) * 4 + r] = h < F ? b1[h] : 0.f;
                    }
            }
        return off;
    };
    std::vector<float> lnbuf; // the LayerNorm rows, appended to buf as one block below (offsets are relative until then)
    auto put_ln = [&](const float* p) {
        const int off = (int)lnbuf.size();
        if (!p) { null_seen = true; lnbuf.resize(lnbuf.size() + D, 0.f); return off; }
        lnbuf.insert(lnbuf.end(), p, p + D);
        return off;
    };
    a = TArgs{};
    a.n_enc = m->n_encoder_layers; a.n_dec = m->n_decoder_layers; a.ff = F; a.n_in = n_in; a.nh = m->n_heights;
    a.max_len = m->max_len; a.step = m->sample_step;
    a.ipe_wT = putT(m->in_proj_encoder_w, D, n_in, MAX_IN); a.ipe_b = put(m->in_proj_encoder_b, D); // (the kernel's K-steps cover MAX_IN inputs)
    a.ipd_wT = putT(m->in_proj_decoder_w, D, LAT); a.ipd_b = put(m->in_proj_decoder_b, D);
    a.op_wT = putT(m->out_proj_w, LAT, D); a.op_b = put(m->out_proj_b, LAT);
    a.pe = put(m->pos_encoding, (size_t)m->max_len * D);
    a.encn_w = put_ln(m->enc_norm_w); a.encn_b = put_ln(m->enc_norm_b);
    a.decn_w = put_ln(m->dec_norm_w); a.decn_b = put_ln(m->dec_norm_b);
    a.mean = put(m->means_latent, LAT); a.stdv = put(m->stds_latent, LAT);
    if (!m->enc || !m->dec) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_temporal_create: NULL layer array");
    auto layer = [&](const dp_temporal_layer& L, bool dec) {
        TLayer o{};
        o.sa_in_wT = putT(L.sa_in_w, 3 * D, D); o.sa_in_b = put(L.sa_in_b, 3 * D);
        o.sa_out_wT = putT(L.sa_out_w, D, D); o.sa_out_b = put(L.sa_out_b, D);
        if (dec) {
            o.ca_in_wT = putT(L.ca_in_w, 3 * D, D); o.ca_in_b = put(L.ca_in_b, 3 * D);
            o.ca_out_wT = putT(L.ca_out_w, D, D); o.ca_out_b = put(L.ca_out_b, D);
        }
        o.ffn_pack = pack_ffn(L.lin1_w, L.lin1_b, L.lin2_w);
        o.lin2_b = put(L.lin2_b, D);
        o.n1w = put_ln(L.norm1_w); o.n1b = put_ln(L.norm1_b);
        o.n2w = put_ln(L.norm2_w); o.n2b = put_ln(L.norm2_b);
        if (dec) { o.n3w = put_ln(L.norm3_w); o.n3b = put_ln(L.norm3_b); }
        return o;
    };
    std::vector<TLayer> tabs;
    for (int l = 0; l < a.n_enc; ++l) tabs.push_back(layer(m->enc[l], false));
    for (int l = 0; l < a.n_dec; ++l) tabs.push_back(layer(m->dec[l], true));
    while (buf.size() % 4) buf.push_back(0.f);
    a.ln0 = (int)buf.size(); a.ln_len = (int)lnbuf.size();
    buf.insert(buf.end(), lnbuf.begin(), lnbuf.end());
    for (TLayer& t : tabs) { t.n1w += a.ln0; t.n1b += a.ln0; t.n2w += a.ln0; t.n2b += a.ln0; t.n3w += a.ln0; t.n3b += a.ln0; } // (n3*: decoder layers only; unused otherwise)
    a.encn_w += a.ln0; a.encn_b += a.ln0; a.decn_w += a.ln0; a.decn_b += a.ln0;
    static_assert(sizeof(TLayer) % sizeof(float) == 0, "layer tables live in the float buffer");
    a.enc_tab = (int)buf.size();
    a.dec_tab = a.enc_tab + a.n_enc * (int)(sizeof(TLayer) / sizeof(float));
    buf.resize(buf.size() + tabs.size() * sizeof(TLayer) / sizeof(float));
    std::memcpy(buf.data() + a.enc_tab, tabs.data(), tabs.size() * sizeof(TLayer));
    if (null_seen) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_temporal_create: NULL tensor pointer in model");
    return DP_OK;
}

// private test hook (host only): the image pack_model builds, so that a CPU program reaches the packer -- returns its size in floats (out may be
// NULL to ask for it), DP_ERR_INVALID when `capacity_floats` is below it
extern "C" int dp_temporal_debug_pack(const dp_temporal_model* m, float* out, int capacity_floats)
{
    return shell(NO_HANDLE, "dp_temporal_debug_pack", [&]() -> int {
        std::vector<float> buf;
        TArgs a;
        if (int rc = pack_model(m, buf, a)) return rc;
        if (out && (size_t)capacity_floats < buf.size())
            return fail(NO_HANDLE, DP_ERR_INVALID, "dp_temporal_debug_pack: capacity below " + std::to_string(buf.size()) + " floats");
        if (out) std::memcpy(out, buf.data(), buf.size() * sizeof(float));
        return (int)buf.size();
    });
}

static int max_teams(const dp_temporal* t) { return t->n_cu / 2 > 0 ? t->n_cu / 2 : 1; }

static int create_impl(dp_temporal** out, const dp_temporal_model* m, int device)
{
    std::vector<float> buf;
    std::unique_ptr<dp_temporal> t(new dp_temporal);
    if (int rc = pack_model(m, buf, t->args)) return rc;
    if (int rc = dprt::open_device<dp_temporal>("dp_temporal_create", device, &t->n_cu)) return rc;
    t->device = device;
    dprt::DeviceGuard guard(device);
    hipError_t e = guard.ok ? t->d_w.upload(buf) : hipErrorInvalidDevice;
    t->xch_granule_bytes = (size_t)max_teams(t.get()) * 2 * XCH_GRANULES * XCH_GMAX * XCH_GRANULE_BYTES;
    if (e == hipSuccess) e = t->d_xch.alloc_zeroed(t->xch_granule_bytes + (size_t)max_teams(t.get()) * sizeof(unsigned) + 16); // (tag 0 = never written; a team's first exchange carries tag 1)
    if (e == hipSuccess) e = t->h_status.alloc();
    if (e != hipSuccess) {
        t.reset(); // (under the guard)
        return fail(NO_HANDLE, DP_ERR_DEVICE, std::string("dp_temporal_create: ") + hipGetErrorString(e));
    }
    t->teams_off = dp_temporal_team_blocks_per_cu() < 1;
    t->args.w = t->d_w.get();
    *out = t.release();
    return DP_OK;
}

extern "C" int dp_temporal_create(dp_temporal** out, const dp_temporal_model* m, int device)
{
    if (!out) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_temporal_create: out is NULL");
    *out = nullptr;
    return shell(NO_HANDLE, "dp_temporal_create", [&] { return create_impl(out, m, device); });
}

extern "C" int dp_temporal_destroy(dp_temporal* t)
{
    if (!t) return DP_ERR_INVALID;
    dprt::DeviceGuard guard(t->device);
    delete t;
    return DP_OK;
}

// private test hook (not in include/dragposer.h; the product reads no environment variable): pin the kernel variant of later predictions
extern "C" int dp_temporal_debug_force_variant(dp_temporal* t, int variant)
{
    // (102, 104, 108, 116: a team of 2 / 4 / 8 / 16 workgroups per sequence where the launch fits the device, else as 0)
    if (!t || (variant != 0 && variant != 21 && variant != 41 && variant != 42 && variant != 44 && variant != 102 && variant != 104 && variant != 108 && variant != 116)) return DP_ERR_INVALID;
    t->forced_variant = variant;
    return DP_OK;
}

// The team size the library picks for n_seq sequences on a device of n_cu usable CUs (1: no teams).  Host arithmetic only (a CPU test holds it): the
// largest power of two up to 16 with every workgroup on a CU of its own (team members wait for each other: all of them must be resident, and the
// TEAM kernel's 86 KB of LDS allow one workgroup per CU), ALL TEAMS TOGETHER ON AT MOST HALF THE CUs (round 6: the other half is what keeps a second
// handle's teams, or another stream's kernel, from starving a member -- a launch that filled the device left no slack at all) and at least one
// feed-forward tile per wave; 16 pays with a quarter of the device at most (profiles/r05_team_latency.txt), 8 beyond.
extern "C" int dp_temporal_debug_team_size(int n_cu, int n_seq, int dim_feedforward)
{
    if (n_cu <= 0 || n_seq <= 0 || dim_feedforward <= 0) return 1;
    int G = 1;
    while (G < 16 && n_seq * (2 * G) <= n_cu / 2 && (dim_feedforward + FT - 1) / FT >= 2 * G * NWV) G *= 2;
    if (G == 16 && n_seq * 64 > n_cu) G = 8;
    return G;
}

// private test hook: make the team exchange fail on purpose -- member `member` of sequence `team`'s team never publishes its partial sums (-1: nobody),
// and a member gives up after `poll_limit` re-reads instead of ~1 s (0: the default).  What the product promises then is in dp_temporal.hip, "time-out".
extern "C" int dp_temporal_debug_team_fault(dp_temporal* t, int team, int member, int poll_limit)
{
    if (!t) return DP_ERR_INVALID;
    t->dbg_skip_team = team; t->dbg_skip_member = member;
    t->poll_limit = poll_limit > 0 ? poll_limit : XCH_POLL_LIMIT;
    return DP_OK;
}

// Health of the handle, WITHOUT a synchronise: DP_TEMPORAL_TEAM_TIMEOUT once a team member of an earlier launch has given up waiting (the device
// writes the word into page-locked host memory the moment it happens; sticky).  The targets of that launch's affected sequences are NaN.
extern "C" int dp_temporal_status(const dp_temporal* t)
{
    if (!t) return DP_ERR_INVALID;
    return t->h_status.read() != 0 ? t->status_seen | DP_TEMPORAL_TEAM_TIMEOUT : t->status_seen;
}

// private test hook: the teams' status word (0: every exchange completed; 1: a workgroup waited XCH_POLL_LIMIT reads for its team -- the launch's
// predictions are garbage); synchronises the device
extern "C" int dp_temporal_debug_team_status(dp_temporal* t)
{
    if (!t || !t->d_xch.get()) return -1;
    dprt::DeviceGuard guard(t->device);
    int v = -1;
    if (!guard.ok || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(&v, t->d_xch.get() + t->xch_granule_bytes + (size_t)max_teams(t) * sizeof(unsigned), sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

static int predict_impl(dp_temporal* t, int n_seq, const dp_seq_state* st, int window, float* target_buf, void* stream)
{
    if (n_seq <= 0 || !st || !target_buf) return fail(t, DP_ERR_INVALID, "dp_temporal_predict: bad arguments");
    if (!st->latent_buf || !st->disp_buf || !st->heights_buf) return fail(t, DP_ERR_INVALID, "dp_temporal_predict: NULL history buffer");
    const TArgs& m = t->args;
    if (st->n_heights != m.nh) return fail(t, DP_ERR_INVALID, "dp_temporal_predict: state.n_heights differs from the model's");
    if (window < 0 || window % m.step != 0) return fail(t, DP_ERR_INVALID, "dp_temporal_predict: window must be a non-negative multiple of sample_step");
    const int n_past = (st->history + m.step - 1) / m.step, n_steps = window / m.step + 1;
    if (st->history < 2 * m.step || n_past - 1 > MAXT || n_steps > MAXT || n_past - 1 > m.max_len || n_steps > m.max_len)
        return fail(t, DP_ERR_UNSUPPORTED, "dp_temporal_predict: more than 32 encoder or decoder tokens (or more than max_len positions)");
    if (!t->teams_off && t->h_status.read() != 0) { // a team member of an EARLIER launch gave up waiting (dp_temporal.hip, "time-out")
        t->teams_off = true;
        t->status_seen |= DP_TEMPORAL_TEAM_TIMEOUT;
        return fail(t, DP_ERR_TIMEOUT, "dp_temporal_predict: a team of workgroups of an earlier launch of this handle timed out waiting for a member that was not "
                                        "resident (another stream's kernel or a CU mask held its CUs?); that launch wrote NaN into the targets of the affected "
                                        "sequences.  Nothing was launched now; the handle runs one workgroup per sequence from here on -- call again");
    }
    dprt::DeviceGuard guard(t->device);
    if (!guard.ok) return fail(t, DP_ERR_DEVICE, "cannot select the predictor's device");
    TArgs a = m;
    a.latent_buf = st->latent_buf; a.disp_buf = st->disp_buf; a.heights_buf = st->heights_buf;
    a.H = st->history; a.n_seq = n_seq; a.window = window; a.target = target_buf;
    // variant: few sequences -> latency (one workgroup per CU, prefetch); many -> two workgroups per CU, and two sequences per
    // workgroup when each has at most 16 tokens (every weight fetch then serves both)
    const bool pair_ok = n_past - 1 <= 16 && n_steps <= 16;
    // (44 = PAIR, one 1024-thread workgroup of two NS = 2 halves per CU that share the weight fetches of the feed-forward layers in calls over at
    //  most 8 tokens.  Measured at 1024 / 4096 sequences, profiles/r06_temporal_pair_ab.txt: window 16 (five decoder calls of 1 .. 5 tokens) -12.8 %
    //  / -12.8 %; window 0 -3.1 % / -1.2 %; window 60 -2.7 % / -2.4 % -- there most of what the shared fetches save is given back by the halves'
    //  lock-step: two independent workgroups on a CU drift apart and run one's small phases under the other's tile loop.  Taken wherever variant 42
    //  would put two workgroups on a CU anyway.)
    int variant = n_seq <= t->n_cu ? 21 : (pair_ok ? (n_seq > 2 * t->n_cu ? 44 : 42) : 41);
    // few sequences: a TEAM of G workgroups per sequence (the largest power of two up to 16 with every workgroup on a CU of its own -- they wait for
    // each other, so all of them must be resident -- and at least one feed-forward tile per wave)
    const int n_cu = dp_temporal_stream_cus((hipStream_t)stream, t->n_cu); // (the CUs this launch may use: a stream may carry a CU mask)
    int G = t->teams_off ? 1 : dp_temporal_debug_team_size(n_cu, n_seq, m.ff);
    if (t->forced_variant >= 100 && !t->teams_off) { // (a forced size: the largest the launch fits -- here the whole device may be used --, whatever pays)
        G = 1;
        while (G < 16 && n_seq * (2 * G) <= n_cu && (m.ff + FT - 1) / FT >= 2 * G * NWV) G *= 2;
        const int want = t->forced_variant - 100;
        G = G >= want ? want : 1;
    }
    if (G >= 2 && (t->forced_variant == 0 || t->forced_variant >= 100)) variant = 100 + G;
    if (t->forced_variant == 21 || t->forced_variant == 41 || ((t->forced_variant == 42 || t->forced_variant == 44) && pair_ok)) variant = t->forced_variant;
    if (variant >= 100) {
        a.G = G; a.xch = (float*)t->d_xch.get(); a.epochs = (unsigned*)(t->d_xch.get() + t->xch_granule_bytes); a.tstatus = (int*)(a.epochs + max_teams(t));
        a.hstatus = t->h_status.get(); a.poll_limit = t->poll_limit; a.dbg_skip_team = t->dbg_skip_team; a.dbg_skip_member = t->dbg_skip_member;
    }
    const hipError_t e = dp_launch_temporal(variant, n_seq, G, a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(t, DP_ERR_LAUNCH, std::string("dp_temporal_predict: ") + hipGetErrorString(e));
    return DP_OK;
}

extern "C" int dp_temporal_predict(dp_temporal* t, int n_seq, const dp_seq_state* st, int window, float* target_buf, void* stream)
{
    if (!t) return DP_ERR_INVALID;
    return shell(t, "dp_temporal_predict", [&] { return predict_impl(t, n_seq, st, window, target_buf, stream); });
}
