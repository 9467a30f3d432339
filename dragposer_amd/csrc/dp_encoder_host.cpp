// dp_encoder_host.cpp -- host side of the pose encoder (include/dragposer_encoder.h): folding, the packer of the kernel's weight
// image (layout: dp_encoder.h), the handle and the C entry points.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dragposer_encoder.h"
#include "dp_encoder.h"
#include "dp_host_rt.h"

using namespace dpenc;
using dprt::fail;
using dprt::shell;

struct dp_encoder {
    int device = -1, n_cu = 256;
    dprt::DeviceBuf<float> d_image;
    std::string err;
};
constexpr dp_encoder* NO_HANDLE = nullptr; // (its messages go to the thread-local slot: dp_encoder_last_error(NULL))

extern "C" const char* dp_encoder_last_error(const dp_encoder* e) { return dprt::last_error(e); }

// the first missing pointer of the model by name, or NULL
static const char* missing_pointer(const dp_encoder_model* m)
{
    static const char* const names[4][3] = {{"conv_w[0]", "conv_w[1]", "conv_w[2]"}, {"conv_mask[0]", "conv_mask[1]", "conv_mask[2]"},
                                            {"conv_b[0]", "conv_b[1]", "conv_b[2]"}, {"pool_w[0]", "pool_w[1]", "pool_w[2]"}};
    for (int l = 0; l < 3; ++l) {
        if (!m->conv_w[l]) return names[0][l];
        if (!m->conv_mask[l]) return names[1][l];
        if (!m->conv_b[l]) return names[2][l];
        if (!m->pool_w[l]) return names[3][l];
    }
    if (!m->f_mu_w) return "f_mu_w";
    if (!m->f_mu_b) return "f_mu_b";
    if (!m->f_logvar_w) return "f_logvar_w";
    if (!m->f_logvar_b) return "f_logvar_b";
    return nullptr;
}

static int check_model(const char* who, const dp_encoder_model* m)
{
    if (!m) return fail(NO_HANDLE, DP_ERR_INVALID, std::string(who) + ": model is NULL");
    if (m->struct_size != sizeof(dp_encoder_model))
        return fail(NO_HANDLE, DP_ERR_INVALID, std::string(who) + ": dp_encoder_model.struct_size is " + std::to_string(m->struct_size) + ", this library's is " +
                                                  std::to_string(sizeof(dp_encoder_model)) + " (use DP_ENCODER_MODEL_INIT)");
    if (const char* name = missing_pointer(m)) return fail(NO_HANDLE, DP_ERR_INVALID, std::string(who) + ": model." + name + " is NULL");
    return DP_OK;
}

// A_l = P_l (W_l * M_l), c_l = P_l b_l (reference: skeleton.py:120 then the pool matmul, nothing non-linear in between): summed
// in double in the order of the middle index, rounded to fp32 once
static int fold_encoder(const dp_encoder_model* m, dp_encoder_folded* out)
{
    if (int rc = check_model("dp_fold_encoder", m)) return rc;
    if (!out) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_fold_encoder: out is NULL");
    float* const A[3] = {out->A0, out->A1, out->A2};
    float* const c[3] = {out->c0, out->c1, out->c2};
    for (int l = 0; l < 3; ++l) {
        const int rows = enc_rows(l), mid = enc_cols(l); // the conv is square: [mid][mid]; the pool [rows][mid]
        const float *W = m->conv_w[l], *M = m->conv_mask[l], *b = m->conv_b[l], *P = m->pool_w[l];
        std::vector<double> acc(mid);
        for (int i = 0; i < rows; ++i) {
            std::fill(acc.begin(), acc.end(), 0.0);
            double cb = 0.0;
            for (int j = 0; j < mid; ++j) {
                const double p = (double)P[i * mid + j];
                for (int k = 0; k < mid; ++k) acc[k] += p * ((double)W[j * mid + k] * (double)M[j * mid + k]);
                cb += p * (double)b[j];
            }
            for (int k = 0; k < mid; ++k) A[l][i * mid + k] = (float)acc[k];
            c[l][i] = (float)cb;
        }
    }
    std::memcpy(out->Ah, m->f_mu_w, sizeof(float) * LAT * 48);
    std::memcpy(out->Ah + LAT * 48, m->f_logvar_w, sizeof(float) * LAT * 48);
    std::memcpy(out->ch, m->f_mu_b, sizeof(float) * LAT);
    std::memcpy(out->ch + LAT, m->f_logvar_b, sizeof(float) * LAT);
    return DP_OK;
}
extern "C" int dp_fold_encoder(const dp_encoder_model* m, dp_encoder_folded* out)
{
    return shell(NO_HANDLE, "dp_fold_encoder", [&] { return fold_encoder(m, out); });
}

// the kernel's image of `f` and, per word, what it holds: (layer, row, column), column -1 = bias, layer -1 = padding
static void pack_image(const dp_encoder_folded& f, float* image, int* table)
{
    const float* const A[NL] = {f.A0, f.A1, f.A2, f.Ah};
    const float* const c[NL] = {f.c0, f.c1, f.c2, f.ch};
    auto put = [&](int word, int l, int row, int col, float v) {
        if (image) image[word] = v;
        if (table) { table[3 * word] = l; table[3 * word + 1] = row; table[3 * word + 2] = col; }
    };
    for (int w = 0; w < IMG_WORDS; ++w) put(w, -1, 0, 0, 0.f);
    for (int l = 0; l < NL; ++l) {
        const int rows = enc_rows(l), cols = enc_cols(l);
        for (int T = 0; T < enc_tiles(l); ++T)
            for (int s = 0; s < enc_steps(l); ++s)
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = 16 * T + (lane & 15), k = enc_channel(s, lane >> 4);
                    if (i < rows && k < cols) {
                        const int row = enc_image_row(l, i);
                        put(enc_w_word(l, T, s, lane), l, row, k, A[l][row * cols + k]);
                    }
                }
        for (int i = 0; i < rows; ++i) put(enc_b_off(l) + i, l, enc_image_row(l, i), -1, c[l][enc_image_row(l, i)]);
    }
}

extern "C" int dp_debug_encoder_image(const dp_encoder_folded* folded, float* image, int* table, int capacity_words)
{
    return shell(NO_HANDLE, "dp_debug_encoder_image", [&] {
        if (!folded) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_debug_encoder_image: folded is NULL");
        if ((image || table) && capacity_words < IMG_WORDS)
            return fail(NO_HANDLE, DP_ERR_INVALID, "dp_debug_encoder_image: capacity below " + std::to_string(IMG_WORDS) + " words");
        pack_image(*folded, image, table);
        return IMG_WORDS;
    });
}

static int create_impl(dp_encoder** out, const dp_encoder_model* m, int device)
{
    std::vector<dp_encoder_folded> folded(1); // (167 KB: not on the stack)
    if (int rc = check_model("dp_encoder_create", m)) return rc;
    if (int rc = fold_encoder(m, folded.data())) return rc;
    std::vector<float> image(IMG_WORDS);
    pack_image(folded[0], image.data(), nullptr);
    std::unique_ptr<dp_encoder> e(new dp_encoder);
    if (int rc = dprt::open_device<dp_encoder>("dp_encoder_create", device, &e->n_cu)) return rc;
    e->device = device;
    dprt::DeviceGuard guard(device);
    const hipError_t rc = guard.ok ? e->d_image.upload(image) : hipErrorInvalidDevice;
    if (rc != hipSuccess) {
        e.reset(); // (under the guard)
        return fail(NO_HANDLE, DP_ERR_DEVICE, std::string("dp_encoder_create: ") + hipGetErrorString(rc));
    }
    *out = e.release();
    return DP_OK;
}

extern "C" int dp_encoder_create(dp_encoder** out, const dp_encoder_model* m, int device)
{
    if (!out) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_encoder_create: out is NULL");
    *out = nullptr;
    return shell(NO_HANDLE, "dp_encoder_create", [&] { return create_impl(out, m, device); });
}

extern "C" int dp_encoder_destroy(dp_encoder* e)
{
    if (!e) return DP_ERR_INVALID;
    dprt::DeviceGuard guard(e->device);
    delete e;
    return DP_OK;
}

extern "C" int dp_encoder_geometry(const dp_encoder* e, int* poses_per_wave, int* waves_per_block, int* max_blocks)
{
    if (!e) return shell(NO_HANDLE, "dp_encoder_geometry", [&] { return fail(NO_HANDLE, DP_ERR_INVALID, "dp_encoder_geometry: handle is NULL"); });
    if (poses_per_wave) *poses_per_wave = POSES;
    if (waves_per_block) *waves_per_block = WAVES;
    if (max_blocks) *max_blocks = e->n_cu;
    return DP_OK;
}

static bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

// the checks dp_encode and dp_sequence_begin share, then the launch on the handle's device
static int run(const char* who, dp_encoder* e, EncArgs& a, void* stream)
{
    const std::string w(who);
    if (a.n < 0) return fail(e, DP_ERR_INVALID, w + ": n is negative");
    if (a.n > 0 && !a.pose) return fail(e, DP_ERR_INVALID, w + ": pose is NULL");
    if (misaligned(a.pose) || misaligned(a.eps) || misaligned(a.mu) || misaligned(a.logvar) || misaligned(a.latent) || misaligned(a.latent_buf))
        return fail(e, DP_ERR_INVALID, w + ": pose, eps, mu, logvar, latent and latent_buf must be 16-byte aligned");
    if (!e) return fail(NO_HANDLE, DP_ERR_INVALID, w + ": handle is NULL");
    if (a.n == 0) return DP_OK;
    if (a.n > (1 << 27)) return fail(e, DP_ERR_INVALID, w + ": n is beyond 2^27 poses");
    a.image = e->d_image.get();
    a.n_tiles = (a.n + POSES - 1) / POSES;
    a.limit = DP_INPUT_LIMIT;
    dprt::DeviceGuard guard(e->device);
    if (!guard.ok) return fail(e, DP_ERR_DEVICE, w + ": cannot select the handle's device");
    const int rc = launch_encoder(a, e->n_cu, stream);
    if (rc != (int)hipSuccess) return fail(e, DP_ERR_LAUNCH, w + ": " + hipGetErrorString((hipError_t)rc));
    return DP_OK;
}

extern "C" int dp_encode(dp_encoder* e, int n, const float* pose, const float* eps, float* mu, float* logvar, float* latent, int* status,
                         void* hip_stream)
{
    EncArgs a{};
    a.n = n; a.pose = pose; a.eps = eps; a.mu = mu; a.logvar = logvar; a.latent = latent; a.status = status;
    return shell(e, "dp_encode", [&] { return run("dp_encode", e, a, hip_stream); });
}

extern "C" int dp_sequence_begin(dp_encoder* e, int n_seq, const float* pose, const float* eps, const float* init_global_pos,
                                 const float* init_global_rot, const float* init_heights, const dp_seq_state* st, float* latent, int* status,
                                 void* hip_stream)
{
    const char* who = "dp_sequence_begin";
    return shell(e, who, [&]() -> int {
        if (!st) return fail(e, DP_ERR_INVALID, std::string(who) + ": state is NULL");
        if (st->n_heights < 0 || st->n_heights > DP_MAX_HEIGHT_JOINTS)
            return fail(e, DP_ERR_INVALID, std::string(who) + ": state->n_heights is " + std::to_string(st->n_heights) + ", must be 0 .. DP_MAX_HEIGHT_JOINTS");
        if (st->history < 1) return fail(e, DP_ERR_INVALID, std::string(who) + ": state->history is " + std::to_string(st->history) + ", must be >= 1");
        if (n_seq > 0) {
            if (!init_global_pos) return fail(e, DP_ERR_INVALID, std::string(who) + ": init_global_pos is NULL");
            if (!init_global_rot) return fail(e, DP_ERR_INVALID, std::string(who) + ": init_global_rot is NULL");
            if (!init_heights && st->n_heights > 0) return fail(e, DP_ERR_INVALID, std::string(who) + ": init_heights is NULL");
            if (!latent) return fail(e, DP_ERR_INVALID, std::string(who) + ": latent is NULL");
            if (!st->global_pos || !st->global_rot || !st->latent_buf || !st->disp_buf || (!st->heights_buf && st->n_heights > 0))
                return fail(e, DP_ERR_INVALID, std::string(who) + ": NULL pointer in state");
        }
        EncArgs a{};
        a.n = n_seq; a.pose = pose; a.eps = eps; a.latent = latent; a.status = status;
        a.begin = 1; a.history = st->history; a.n_heights = st->n_heights;
        a.init_pos = init_global_pos; a.init_rot = init_global_rot; a.init_heights = init_heights;
        a.global_pos = st->global_pos; a.global_rot = st->global_rot; a.latent_buf = st->latent_buf; a.disp_buf = st->disp_buf; a.heights_buf = st->heights_buf;
        return run(who, e, a, hip_stream);
    });
}
