// dp_host.cpp -- host side of libdragposer_hip.so: decoder folding, MFMA fragment packing,
// skeleton tables, context management and the C ABI declared in include/dragposer.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dragposer.h"
#include "../../include/dragposer_grad.h"
#include "../../include/dragposer_constraints.h"
#include "../../include/dragposer_terms.h"
#include "../../include/dragposer_skeleton.h"
#include "../../include/dragposer_sequence_constraints.h"
#include "../../include/dragposer_holds.h"
#include "../../include/dragposer_latent_ar.h"
#include "../../include/dragposer_gaps.h"
#include "../../include/dragposer_live.h"
#include "../../include/dragposer_tethers.h"
#include "../../include/dragposer_points.h"
#include "../../include/dragposer_lm.h"
#include "../../include/dragposer_sequence_lm.h"
#include "../../include/dragposer_lm_terms.h"
#include "../../include/dragposer_sequence_lm_terms.h"
#include "../../include/dragposer_calibration.h"
#include "../../include/dragposer_clip_accel.h"
#include "../../include/dragposer_clip_lm.h"
#include "../../include/dragposer_clip_skeleton.h"
#include "dp_clip.h"
#include "dp_clip_accel.h"
#include "dp_clip_skel.h"
#include "dp_cons_live.h"
#include "dp_cons_tether.h"
#include "dp_cons_points.h"
#include "dp_fit.h"
#include "dp_host_rt.h"
#include "dp_lm_seq.h"
#include "dp_lm_seq_terms.h"
#include "dp_lm_terms.h"
#include "dp_kernel.h"
#include "dp_sequence.h"
#include "dp_vjp.h"
#include "dp_w4.h"

using namespace dpl;
using dprt::DeviceBuf;
using dprt::DeviceGuard;
using dprt::fail;

struct dp_ctx {
    int device = -1;
    int n_cu = 256;
    std::string err;
    // device memory (DeviceBuf: get() is NULL until uploaded -- a dp_debug_host_ctx context has none)
    DeviceBuf<float> d_wfrag, d_bias, d_w4img, d_w4bias;
    DeviceBuf<dpw4::Pair> d_w4pairs;
    bool w4_bp = false; // the w4 image / pairs are in the body-part layout (dp_w4_bp.hip), not the dense one (dp_w4.hip)
    std::vector<float> w4img_h[2], w4bias_h[2]; // host copies of both layouts [dense, body-part] (empty: the model does not fit it),
    std::vector<dpw4::Pair> w4pairs_h[2];       // for dp_debug_set_w4_layout
    DeviceBuf<unsigned> d_w16img; // 16-frames-per-wave kernel (dp_w16.hip); NULL when the skeleton is not the one its slot map is for
    DeviceBuf<float> d_w16bias;
    DeviceBuf<dpw16::SlotConst> d_w16slots;
    DeviceBuf<float> d_vjpimg; // dp_forward_vjp's image (dp_vjp.h): folded decoder, de-normalisation, bones, skeleton walk
    int weight_dtype = DP_WEIGHTS_FP32;
    DeviceBuf<ItemConst> d_items;
    dp_folded folded;
    std::vector<unsigned> smask;
    float mean_q0[4] = {0, 0, 0, 0}, std_q0[4] = {1, 1, 1, 1}; // root quaternion channels (sequence epilogue)
    int last_kernel = 0;   // what the last launch used: 4 = dp_w4.hip (8 in the test-only library, below)
    LaunchPick last_pick{}; // the instantiation the last launch ran, as its launcher recorded it (dp_debug_last_launch)
};

// The product library has two optimise kernels: dp_w4.hip (4 frames per wave, fp32 MFMA) and dp_w16*.hip (16 frames per wave, bf16
// MFMA in split precision, for batches beyond one round of the former): include/dragposer.h, DP_KERNEL_*.  Round 1's 8-wave kernel (dp_kernel.hip: the reference's matrix
// chain taken literally, 16x16x4 tiles) survives as an independent second implementation for cross-checks in a TEST-ONLY
// library, libdragposer_hip_ref8.so = this file compiled with -DDP_REF8_BUILD + dp_kernel.o; no environment variable is read.
#ifdef DP_REF8_BUILD
constexpr int KERNEL_CHOICE = 8;
#else
constexpr int KERNEL_CHOICE = 4;
#endif

constexpr dp_ctx* NO_HANDLE = nullptr; // (its messages go to the thread-local slot: dp_last_error(NULL))

#define DEVICE_GUARD(ctx)                                                                        \
    DeviceGuard guard_((ctx)->device);                                                           \
    if (!guard_.ok) return fail(ctx, DP_ERR_DEVICE, "cannot select the context's device")

extern "C" int dp_version(void) { return DP_VERSION; }

extern "C" const char* dp_last_error(const dp_ctx* ctx) { return dprt::last_error(ctx); }

// ------------------------------------------------------------------------------------------------
static float round_bf16(float x)
{ // nearest-even; NaN/Inf do not occur in checkpoint weights
    unsigned u;
    std::memcpy(&u, &x, 4);
    u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
    std::memcpy(&x, &u, 4);
    return x;
}

static bool model_ptrs_ok(const dp_model* m)
{
    if (!m || !m->f_latent_w || !m->f_latent_b || !m->mean_q || !m->std_q || !m->mean_disp || !m->std_disp ||
        !m->parents || !m->offsets)
        return false;
    for (int l = 0; l < 3; ++l)
        if (!m->unpool_w[l] || !m->conv_w[l] || !m->conv_mask[l] || !m->conv_b[l]) return false;
    return true;
}

// A0 = (W0*M0) U0 Wf, c0 = (W0*M0) U0 bf + b0, A1 = (W1*M1) U1, A2 = (W2*M2) U2
// (reference: autoencoder.py:228-234, skeleton.py:120,245 -- no non-linearity between these steps)
static int fold_decoder(const dp_model* m, dp_folded* out)
{
    if (!model_ptrs_ok(m) || !out) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_fold_decoder: NULL pointer in model");
    const int dims[4] = {24, 40, 60, 92};
    const bool bf = m->weight_dtype == DP_WEIGHTS_BF16;
    if (m->weight_dtype != DP_WEIGHTS_FP32 && !bf) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_fold_decoder: unknown weight_dtype");
    auto wq = [&](float x) { return bf ? round_bf16(x) : x; };
    // T = U0 Wf (40x24), tb = U0 bf
    std::vector<double> T(40 * 24), tb(40);
    for (int i = 0; i < 40; ++i) {
        for (int k = 0; k < 24; ++k) {
            double s = 0;
            for (int j = 0; j < 24; ++j) s += (double)m->unpool_w[0][i * 24 + j] * (double)wq(m->f_latent_w[j * 24 + k]);
            T[i * 24 + k] = s;
        }
        double s = 0;
        for (int j = 0; j < 24; ++j) s += (double)m->unpool_w[0][i * 24 + j] * (double)m->f_latent_b[j];
        tb[i] = s;
    }
    auto wm = [&](int l, int i, int j) { return (double)(wq(m->conv_w[l][i * dims[l + 1] + j]) * m->conv_mask[l][i * dims[l + 1] + j]); };
    for (int i = 0; i < 40; ++i) {
        for (int k = 0; k < 24; ++k) {
            double s = 0;
            for (int j = 0; j < 40; ++j) s += wm(0, i, j) * T[j * 24 + k];
            out->A0[i * 24 + k] = (float)s;
        }
        double s = m->conv_b[0][i];
        for (int j = 0; j < 40; ++j) s += wm(0, i, j) * tb[j];
        out->c0[i] = (float)s;
    }
    for (int i = 0; i < 60; ++i) {
        for (int k = 0; k < 40; ++k) {
            double s = 0;
            for (int j = 0; j < 60; ++j) s += wm(1, i, j) * (double)m->unpool_w[1][j * 40 + k];
            out->A1[i * 40 + k] = (float)s;
        }
        out->b1[i] = m->conv_b[1][i];
    }
    for (int i = 0; i < 92; ++i) {
        for (int k = 0; k < 60; ++k) {
            double s = 0;
            for (int j = 0; j < 92; ++j) s += wm(2, i, j) * (double)m->unpool_w[2][j * 60 + k];
            out->A2[i * 60 + k] = (float)s;
        }
        out->b2[i] = m->conv_b[2][i];
    }
    return DP_OK;
}
// (every exported function whose body can allocate runs inside dprt::shell: nothing is thrown across the C ABI)
extern "C" int dp_fold_decoder(const dp_model* m, dp_folded* out) { return dprt::shell(NO_HANDLE, "dp_fold_decoder", [&] { return fold_decoder(m, out); }); }

// ------------------------------------------------------------------------------------------------
// Skeleton-derived layout of the P3 items (see dp_layout.h)
struct ItemPlan {
    int nvirt = 0;
    int virt_parent[MAX_VIRT] = {0, 0, 0}; // joint whose quad virtual item v copies
    int virt_child[MAX_VIRT] = {0, 0, 0};  // the extra child bone it handles
    int first_child[NJ];                   // child handled by the joint's own item (-1: leaf)
    int root_child[MAX_ROOT_CH] = {-1, -1, -1};
};

static int plan_items(const int* par, ItemPlan& pl, std::string& err)
{
    if (par[0] != 0) { err = "parents[0] must be 0"; return DP_ERR_INVALID; }
    for (int j = 1; j < NJ; ++j)
        if (par[j] < 0 || par[j] >= j) { err = "parents must be topologically ordered (parents[j] < j)"; return DP_ERR_INVALID; }
    for (int j = 0; j < NJ; ++j) pl.first_child[j] = -1;
    int nroot = 0;
    for (int k = 1; k < NJ; ++k) {
        const int p = par[k];
        if (p == 0) {
            if (nroot == MAX_ROOT_CH) { err = "root has more than 3 children"; return DP_ERR_UNSUPPORTED; }
            pl.root_child[nroot++] = k;
        } else if (pl.first_child[p] < 0) {
            pl.first_child[p] = k;
        } else {
            if (pl.nvirt == MAX_VIRT) { err = "more than 3 extra child bones on non-root joints"; return DP_ERR_UNSUPPORTED; }
            pl.virt_parent[pl.nvirt] = p;
            pl.virt_child[pl.nvirt] = k;
            ++pl.nvirt;
        }
    }
    return DP_OK;
}

// weight of product g at (output row, input column); zero outside the real matrix
static float gemm_w(const dp_folded& f, const ItemPlan& pl, int g, int row, int col)
{
    if (row >= G_ROWS[g]) return 0.f;
    if (g == G_L2 && col == L2_ONE_COL) return f.b2[row]; // bias rides on the constant-1 column
    if (g == G_B2 && col >= 4 * ITEM_VIRT0) {             // duplicated rows for the virtual quads
        const int v = (col - 4 * ITEM_VIRT0) / 4;
        if (v >= pl.nvirt) return 0.f;
        return f.A2[(4 * pl.virt_parent[v] + (col & 3)) * 60 + row];
    }
    if (col >= G_KREAL[g]) return 0.f;
    switch (g) {
    case G_L0: return f.A0[row * 24 + col];
    case G_L1: return f.A1[row * 40 + col];
    case G_L2: return f.A2[row * 60 + col];
    case G_B2: return (col == 91) ? 0.f : f.A2[col * 60 + row]; // A2^T; channel 91 is unused padding
    case G_B1: return f.A1[col * 40 + row]; // A1^T
    case G_B0: return f.A0[col * 24 + row]; // A0^T
    }
    return 0.f;
}

static float gemm_bias(const dp_folded& f, int g, int row)
{
    if (row >= G_ROWS[g]) return 0.f;
    switch (g) {
    case G_L0: return f.c0[row];
    case G_L1: return f.b1[row];
    }
    return 0.f;
}

// host-only, exported for the CPU tests: per-wave/per-lane MFMA operand images
//   wfrag [NWAVE][W_REGS][64], bias [2][64] (rows of c0 / b1, zero padded; b1 row 60 = 1 feeds the
//   constant-1 column that carries b2), smask [NWAVE][NGEMM] (bit i: step i of the wave's chain is non-zero)
static int pack_frags(const dp_folded* f, const int* parents, float* wfrag, float* bias, unsigned* smask)
{
    if (!f || !parents || !wfrag || !bias || !smask) return DP_ERR_INVALID;
    ItemPlan pl;
    std::string err;
    int rc = plan_items(parents, pl, err);
    if (rc != DP_OK) return fail(NO_HANDLE, rc, err);
    std::memset(wfrag, 0, sizeof(float) * NWAVE * W_REGS * 64);
    std::memset(smask, 0, sizeof(unsigned) * NWAVE * NGEMM);
    for (int r = 0; r < 64; ++r) { bias[r] = gemm_bias(*f, G_L0, r); bias[64 + r] = gemm_bias(*f, G_L1, r); }
    bias[64 + L2_ONE_COL] = 1.0f; // lrelu(1) = 1: a1[:, 60] == 1
    const int woff[NGEMM] = {W_OFF_L0, W_OFF_L1, W_OFF_L2, W_OFF_B2, W_OFF_B1, W_OFF_B0};
    for (int w = 0; w < NWAVE; ++w) {
        for (int g = 0; g < NGEMM; ++g) {
            const int tile = wave_tile(g, w), s0 = wave_step0(g, w), n = wave_nsteps(g, w);
            if (tile < 0) continue;
            for (int i = 0; i < n; ++i) {
                bool any = false;
                for (int l = 0; l < 64; ++l) {
                    const float v = gemm_w(*f, pl, g, 16 * tile + (l & 15), 4 * (s0 + i) + (l >> 4));
                    wfrag[(w * W_REGS + woff[g] + i) * 64 + l] = v;
                    any = any || v != 0.f;
                }
                if (any) smask[w * NGEMM + g] |= 1u << i;
            }
        }
    }
    return DP_OK;
}
extern "C" int dp_debug_pack(const dp_folded* f, const int* parents, float* wfrag, float* bias, unsigned* smask) { return dprt::shell(NO_HANDLE, "dp_debug_pack", [&] { return pack_frags(f, parents, wfrag, bias, smask); }); }

// host-only, exported for the CPU tests: weight image of the wave-private kernel (dp_w4.h)
//   img [N_GROUPS][64][4]: step s = 4 g + m of lane l at img[(g * 64 + l) * 4 + m];  bias [4][64]
// Rows of layer 2 / columns of its transpose are indexed by P3 item: row 4 * item + c is channel c of joint `item`
// (items 0..21), of the root displacement (22) or of a virtual copy of a joint with a second / third child (23..25).
static int w4_src_row(const ItemPlan& pl, int item, int c)
{ // row of A2 that feeds channel c of `item`, or -1
    if (item < 0) return -1;
    if (item < NJ) return 4 * item + c;
    if (item == ITEM_DISP) return 4 * ITEM_DISP + c; // 88..91 (91: the decoder's unused fourth displacement channel)
    const int v = item - ITEM_VIRT0;
    if (v >= 0 && v < pl.nvirt) return 4 * pl.virt_parent[v] + c;
    return -1;
}

// The body-part layout (dp_w4.h) runs only some K-groups of layer 2 per block; it is packed only when every weight it leaves out is
// exactly zero (else DP_ERR_UNSUPPORTED, and dp_create keeps the dense layout).
static int pack_w4(const dp_folded* f, const dp_model* m, float* img, float* bias, bool bp)
{
    if (!f || !model_ptrs_ok(m) || !img || !bias) return DP_ERR_INVALID;
    ItemPlan pl;
    std::string err;
    int rc = plan_items(m->parents, pl, err);
    if (rc != DP_OK) return fail(NO_HANDLE, rc, err);
    std::memset(img, 0, sizeof(float) * dpw4::IMG_FLOATS);
    std::memset(bias, 0, sizeof(float) * dpw4::BIAS_FLOATS);
    auto put = [&](int step, int lane, float v) { img[((step >> 2) * 64 + lane) * 4 + (step & 3)] = v; };
    // The de-normalisation of the decoder's last layer (drag_pose.py:84-85: r = y * sigma + mu) is folded into it:
    // rows of A2 scaled by sigma, bias sigma * b2 + mu; its transpose carries the same scaling (dL/dy = sigma * dL/dr).
    auto sd_of = [&](int item, int c) -> double {
        if (item == ITEM_DISP) return c < 3 ? (double)m->std_disp[c] : 0.0;
        const int r = w4_src_row(pl, item, c);
        return r >= 0 ? (double)m->std_q[r] : 0.0;
    };
    auto mu_of = [&](int item, int c) -> double {
        if (item == ITEM_DISP) return c < 3 ? (double)m->mean_disp[c] : 0.0;
        const int r = w4_src_row(pl, item, c);
        return r >= 0 ? (double)m->mean_q[r] : (c == 0 ? 1.0 : 0.0); // idle rows decode to the unit quaternion
    };
    for (int l = 0; l < 64; ++l) {
        const int c0ch = dpw4::h0_channel(l); // the first hidden layer's channel in row l (dp_w4.h), or -1
        for (int k = 0; k < 24; ++k) put(dpw4::S_L0 + k, l, c0ch >= 0 ? f->A0[c0ch * 24 + k] : 0.f);
        for (int k = 0; k < 40; ++k) put(dpw4::S_L1 + k, l, l < 60 ? f->A1[l * 40 + k] : 0.f); // (K-step k = channel k: quads 0..4, 8..12)
        // layer 2, dense: row l of block blk = channel l2_channel(blk, l & 3) of the side-l2_side(l & 3) item of quad l >> 2;
        // body-part: channel l & 3 of the side-blk item of quad l >> 2, K-groups BP_GROUPS_A / _B of the block only (dp_w4.h)
        int it2b[2], ch2[2];
        for (int blk = 0; blk < 2; ++blk) {
            it2b[blk] = bp ? dpw4::bp_item_of(blk, l >> 2) : dpw4::item_of(dpw4::l2_side(l & 3), l >> 2);
            ch2[blk] = bp ? (l & 3) : dpw4::l2_channel(blk, l & 3);
        }
        const int r2[2] = {w4_src_row(pl, it2b[0], ch2[0]), w4_src_row(pl, it2b[1], ch2[1])};
        for (int blk = 0; blk < 2; ++blk) {
            const int s0 = blk ? dpw4::S_L2B : dpw4::S_L2A;
            int kept = 0; // (body-part: K-steps packed so far)
            for (int k = 0; k < 60; ++k) {
                const float v = r2[blk] >= 0 ? (float)(sd_of(it2b[blk], ch2[blk]) * (double)f->A2[r2[blk] * 60 + k]) : 0.f;
                if (!bp) { put(s0 + k, l, v); continue; }
                bool run = false;
                for (int g = 0; g < (blk ? dpw4::BP_NG_B : dpw4::BP_NG_A); ++g) run = run || (blk ? dpw4::BP_GROUPS_B[g] : dpw4::BP_GROUPS_A[g]) == k / 4;
                if (run) put(s0 + kept++, l, v);
                else if (v != 0.f)
                    return fail(NO_HANDLE, DP_ERR_UNSUPPORTED, "w4 body-part layout: K-group " + std::to_string(k / 4) + " of item " +
                                                                 std::to_string(it2b[blk]) + " is not zero");
            }
        }
        for (int k = 0; k < 104; ++k) { // column k = channel k & 3 of an item of dL/dr (side A quads 0..15, then side B quads 1..10)
            const int item = k < 64 ? dpw4::item_of(0, k >> 2) : dpw4::item_of(1, dpw4::B2_ABID0_B + ((k - 64) >> 2));
            const int r = w4_src_row(pl, item, k & 3);
            put(dpw4::S_B2 + k, l, (l < 60 && r >= 0) ? (float)(sd_of(item, k & 3) * (double)f->A2[r * 60 + l]) : 0.f);
        }
        for (int k = 0; k < 60; ++k) put(dpw4::S_B1 + k, l, c0ch >= 0 ? f->A1[k * 40 + c0ch] : 0.f);
        for (int k = 0; k < 20; ++k) // bL0, K split: lanes 0..31 carry K-step k, lanes 32..63 K-step 20 + k, of rows l & 31
            put(dpw4::S_B0 + k, l, (l & 31) < 24 ? f->A0[((l < 32 ? 0 : 20) + k) * 24 + (l & 31)] : 0.f);
        bias[l] = c0ch >= 0 ? f->c0[c0ch] : 0.f;
        bias[64 + l] = l < 60 ? f->b1[l] : 0.f;
        for (int blk = 0; blk < 2; ++blk) // (idle items: sigma 0, mu (1, 0, 0, 0) -- they decode to the unit quaternion)
            bias[128 + 64 * blk + l] = (float)(sd_of(it2b[blk], ch2[blk]) * (r2[blk] >= 0 ? (double)f->b2[r2[blk]] : 0.0) + mu_of(it2b[blk], ch2[blk]));
    }
    return DP_OK;
}

extern "C" int dp_debug_pack_w4(const dp_folded* f, const dp_model* m, float* img, float* bias) { return dprt::shell(NO_HANDLE, "dp_debug_pack_w4", [&] { return pack_w4(f, m, img, bias, false); }); }
extern "C" int dp_debug_pack_w4_bp(const dp_folded* f, const dp_model* m, float* img, float* bias) { return dprt::shell(NO_HANDLE, "dp_debug_pack_w4_bp", [&] { return pack_w4(f, m, img, bias, true); }); }

// host-only, exported for the CPU tests: the body-part placement (dp_w4.h) -- items [2][16] (side, quad; -1 idle), the K-groups of layer 2
// each block runs [2][15] (-1 beyond BP_NG_A / BP_NG_B)
extern "C" int dp_debug_w4_bp_layout(int* items, int* groups)
{
    if (!items || !groups) return DP_ERR_INVALID;
    for (int s = 0; s < 2; ++s)
        for (int b = 0; b < 16; ++b) items[16 * s + b] = dpw4::bp_item_of(s, b);
    for (int g = 0; g < 15; ++g) {
        groups[g] = g < dpw4::BP_NG_A ? dpw4::BP_GROUPS_A[g] : -1;
        groups[15 + g] = g < dpw4::BP_NG_B ? dpw4::BP_GROUPS_B[g] : -1;
    }
    return DP_OK;
}

static int items_of(const dp_model* m, void* out_items);

// host-only, exported for the CPU tests: kinematics constants of the wave-private kernel, one dpw4::Pair per lane quad
static int pairs_w4(const dp_model* m, void* out_pairs, bool bp)
{
    if (!model_ptrs_ok(m) || !out_pairs) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_debug_pairs_w4: NULL pointer");
    std::vector<ItemConst> items(32);
    int rc = items_of(m, items.data());
    if (rc != DP_OK) return rc;
    dpw4::Pair* pr = (dpw4::Pair*)out_pairs;
    std::memset(pr, 0, sizeof(dpw4::Pair) * 16);
    for (int b = 0; b < 16; ++b)
        for (int s = 0; s < 2; ++s) {
            dpw4::Pair& p = pr[b];
            const int item = bp ? dpw4::bp_item_of(s, b) : dpw4::item_of(s, b);
            p.item[s] = item;
            p.kind[s] = KIND_IDLE;
            p.mu[0][s] = 1.f; // idle: a unit quaternion, whatever the (zero) decoder channels say
            p.sgn[s] = 1.f;
            p.bone_slot[s] = SLOT_TRASH + ((2 * b + s) & 7);
            if (item < 0) continue;
            const ItemConst& c = items[item];
            p.kind[s] = c.kind;
            if (c.kind == KIND_IDLE) continue;
            for (int k = 0; k < 4; ++k) { p.sd[k][s] = c.sd[k]; p.mu[k][s] = c.mu[k]; }
            for (int k = 0; k < 3; ++k) p.off[k][s] = c.ch_off[k];
            p.bone_slot[s] = c.ch_id;
            p.ch_sub[s] = c.ch_sub;
            if (c.kind == KIND_ROOT) { p.sgn[s] = -1.f; p.rho[s] = 1.f; p.ch_sub[s] = (1u << NJ) - 1u; }
        }
    return DP_OK;
}
extern "C" int dp_debug_pairs_w4(const dp_model* m, void* out_pairs /* 16 x 144 B */) { return dprt::shell(NO_HANDLE, "dp_debug_pairs_w4", [&] { return pairs_w4(m, out_pairs, false); }); }
extern "C" int dp_debug_pairs_w4_bp(const dp_model* m, void* out_pairs /* 16 x 144 B */) { return dprt::shell(NO_HANDLE, "dp_debug_pairs_w4_bp", [&] { return pairs_w4(m, out_pairs, true); }); }

// host-only, exported for the CPU tests: P3 per-item constants [32]
static int items_of(const dp_model* m, void* out_items /* 32 x 128 B */)
{
    if (!model_ptrs_ok(m) || !out_items) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_debug_items: NULL pointer");
    ItemConst* it = (ItemConst*)out_items;
    std::memset(it, 0, sizeof(ItemConst) * 32);
    const int* par = m->parents;
    ItemPlan pl;
    std::string err;
    int rc = plan_items(par, pl, err);
    if (rc != DP_OK) return fail(NO_HANDLE, rc, err);
    unsigned sub[NJ]; // subtree masks
    for (int j = 0; j < NJ; ++j) sub[j] = 1u << j;
    for (int j = NJ - 1; j >= 1; --j) sub[par[j]] |= sub[j];
    auto set_child = [&](ItemConst& c, int k) {
        c.ch_id = k;
        c.ch_sub = sub[k];
        for (int a = 0; a < 3; ++a) c.ch_off[a] = m->offsets[3 * k + a];
    };
    for (int id = 0; id < 32; ++id) {
        ItemConst& c = it[id];
        c.kind = KIND_IDLE;
        c.ch_id = SLOT_TRASH + (id & 7);
        c.init_id = SLOT_TRASH + (id & 7);
        c.src_quad = ITEM_VIRT0; // a quad layer 2 always writes as zeros (channels 92..95)
        c.dst_quad = (id < NQUAD_GY) ? id : -1;
        unsigned long long path = 0;
        for (int i = 0; i < MAX_PATH; ++i) path |= (unsigned long long)SLOT_ZERO << (5 * i);
        if (id < NJ) {
            c.kind = id == 0 ? KIND_ROOT : KIND_JOINT;
            c.src_quad = id;
            for (int k = 0; k < 4; ++k) { c.sd[k] = m->std_q[4 * id + k]; c.mu[k] = m->mean_q[4 * id + k]; }
            if (id > 0 && pl.first_child[id] >= 0) set_child(c, pl.first_child[id]);
            int chain[NJ], n = 0; // bones on the path root -> id (joint ids, root excluded)
            for (int k = id; k != 0; k = par[k]) chain[n++] = k;
            if (n > MAX_PATH) return fail(NO_HANDLE, DP_ERR_UNSUPPORTED, "kinematic chain deeper than 7 bones");
            path = 0;
            for (int i = 0; i < MAX_PATH; ++i) path |= (unsigned long long)(i < n ? chain[i] : SLOT_ZERO) << (5 * i);
        } else if (id == ITEM_DISP) {
            c.kind = KIND_DISP;
            c.src_quad = ITEM_DISP;
            for (int k = 0; k < 3; ++k) { c.sd[k] = m->std_disp[k]; c.mu[k] = m->mean_disp[k]; }
            c.ch_sub = (1u << NJ) - 1u; // the displacement's "subtree" is every joint
        } else if (id - ITEM_VIRT0 < pl.nvirt) {
            const int v = id - ITEM_VIRT0, j = pl.virt_parent[v];
            c.kind = KIND_VIRT;
            c.src_quad = j;
            for (int k = 0; k < 4; ++k) { c.sd[k] = m->std_q[4 * j + k]; c.mu[k] = m->mean_q[4 * j + k]; }
            set_child(c, pl.virt_child[v]);
        }
        if (id < MAX_ROOT_CH && pl.root_child[id] >= 0) {
            c.init_id = pl.root_child[id];
            for (int a = 0; a < 3; ++a) c.init_off[a] = m->offsets[3 * pl.root_child[id] + a];
        }
        c.path_lo = (unsigned)(path & 0x3FFFFFFFull);
        c.path_hi = (unsigned)(path >> 30);
    }
    return DP_OK;
}
extern "C" int dp_debug_items(const dp_model* m, void* out_items) { return dprt::shell(NO_HANDLE, "dp_debug_items", [&] { return items_of(m, out_items); }); }

// dp_forward_vjp's image (dp_vjp.h), from the context's folded decoder
static void pack_vjp(const dp_folded& fd, const dp_model* m, std::vector<float>& img)
{
    using dpvjp::NY; using dpvjp::OFF_A0; using dpvjp::OFF_C0; using dpvjp::OFF_A1; using dpvjp::OFF_B1; using dpvjp::OFF_A2;
    using dpvjp::OFF_B2; using dpvjp::OFF_SD; using dpvjp::OFF_MU; using dpvjp::OFF_BONE; using dpvjp::OFF_PARENT;
    img.assign(dpvjp::IMG_WORDS, 0.f);
    std::memcpy(&img[OFF_A0], fd.A0, sizeof(fd.A0));
    std::memcpy(&img[OFF_C0], fd.c0, sizeof(fd.c0));
    std::memcpy(&img[OFF_A1], fd.A1, sizeof(fd.A1));
    std::memcpy(&img[OFF_B1], fd.b1, sizeof(fd.b1));
    std::memcpy(&img[OFF_A2], fd.A2, sizeof(fd.A2));
    std::memcpy(&img[OFF_B2], fd.b2, sizeof(fd.b2));
    for (int o = 0; o < NY; ++o) {
        img[OFF_SD + o] = o < 4 * NJ ? m->std_q[o] : o < 4 * NJ + 3 ? m->std_disp[o - 4 * NJ] : 1.f;
        img[OFF_MU + o] = o < 4 * NJ ? m->mean_q[o] : o < 4 * NJ + 3 ? m->mean_disp[o - 4 * NJ] : 0.f;
    }
    for (int k = 0; k < 3 * NJ; ++k) img[OFF_BONE + k] = m->offsets[k];
    int walk[NJ + 1 + 2 * NJ]; // parent | cstart | clist (children in increasing order)
    int* parent = walk;
    int* cstart = walk + NJ;
    int* clist = walk + 2 * NJ + 1;
    int n = 0;
    for (int p = 0; p < NJ; ++p) {
        parent[p] = m->parents[p];
        cstart[p] = n;
        for (int c = 1; c < NJ; ++c)
            if (m->parents[c] == p) clist[n++] = c;
    }
    cstart[NJ] = n;
    for (int k = n; k < NJ; ++k) clist[k] = 0;
    std::memcpy(&img[OFF_PARENT], walk, sizeof(walk));
}

// ------------------------------------------------------------------------------------------------
#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(ctx, DP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// dp_create behind the exception shell.  Order: the arguments, the device (queries only), everything built on the host -- all that can throw --,
// and only then the device's memory: a flat list of uploads into a context that a unique_ptr owns until *out has it.
static int create_impl(dp_ctx** out, const dp_model* model, int device)
{
    if (!model_ptrs_ok(model)) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_create: NULL pointer in model");
    int n_cu = 256;
    if (int rc = dprt::open_device<dp_ctx>("dp_create", device, &n_cu)) return rc;
    std::unique_ptr<dp_ctx> ctx(new dp_ctx());
    ctx->n_cu = n_cu;
    for (int k = 0; k < 4; ++k) { ctx->mean_q0[k] = model->mean_q[k]; ctx->std_q0[k] = model->std_q[k]; }
    int rc = fold_decoder(model, &ctx->folded);
    std::vector<float> wfrag(NWAVE * W_REGS * 64), bfrag(128);
    ctx->smask.assign(NWAVE * NGEMM, 0u);
    std::vector<ItemConst> items(32);
    if (rc == DP_OK) rc = pack_frags(&ctx->folded, model->parents, wfrag.data(), bfrag.data(), ctx->smask.data());
    // the w4 family: the body-part layout when the decoder's block sparsity fits it (every K-group it leaves out exactly zero), else dense.
    // Both are packed and kept on the host (dp_debug_set_w4_layout switches between them).
    for (int bp = 0; bp < 2 && rc == DP_OK; ++bp) {
        std::vector<float> img(dpw4::IMG_FLOATS), bias(dpw4::BIAS_FLOATS);
        const std::string prev_err = dprt::null_slot<dp_ctx>(); // (a model the body-part layout does not fit is no error)
        const int prc = pack_w4(&ctx->folded, model, img.data(), bias.data(), bp == 1);
        if (prc != DP_OK && bp == 1) { dprt::null_slot<dp_ctx>() = prev_err; continue; }
        rc = prc;
        std::vector<dpw4::Pair> pairs(16);
        if (rc == DP_OK) rc = pairs_w4(model, pairs.data(), bp == 1);
        ctx->w4img_h[bp].swap(img); ctx->w4bias_h[bp].swap(bias); ctx->w4pairs_h[bp].swap(pairs);
    }
    ctx->w4_bp = rc == DP_OK && !ctx->w4img_h[1].empty();
    if (rc == DP_OK) rc = items_of(model, items.data());
    const bool w16 = rc == DP_OK && dp_w16_supported(model);
    std::vector<unsigned> w16img(w16 ? dpw16::IMG_U32 : 0);
    std::vector<float> w16bias(dpw16::BIAS_FLOATS);
    std::vector<dpw16::SlotConst> w16slots(dpw16::NTY * 4);
    if (w16) rc = dp_debug_pack_w16(&ctx->folded, model, w16img.data(), w16bias.data(), w16slots.data());
    ctx->weight_dtype = model->weight_dtype;
    if (rc != DP_OK) return rc;
    std::vector<float> vjpimg;
    pack_vjp(ctx->folded, model, vjpimg); // (the skeleton passed plan_items' checks above: parents[j] < j)

    ctx->device = device;
    DeviceGuard guard(device); // (declared before nothing that owns device memory but `ctx`, which a failure below frees first)
    hipError_t e = guard.ok ? hipSuccess : hipErrorInvalidDevice;
    const auto up = [&e](auto& buf, const auto& v) { if (e == hipSuccess) e = buf.upload(v); };
    up(ctx->d_wfrag, wfrag);
    up(ctx->d_bias, bfrag);
    up(ctx->d_items, items);
    up(ctx->d_w4img, ctx->w4img_h[ctx->w4_bp]);
    up(ctx->d_w4bias, ctx->w4bias_h[ctx->w4_bp]);
    up(ctx->d_w4pairs, ctx->w4pairs_h[ctx->w4_bp]);
    up(ctx->d_vjpimg, vjpimg);
    if (w16) {
        up(ctx->d_w16img, w16img);
        up(ctx->d_w16bias, w16bias);
        up(ctx->d_w16slots, w16slots);
    }
    if (e != hipSuccess) {
        ctx.reset(); // (under the guard)
        return fail(NO_HANDLE, DP_ERR_DEVICE, std::string("dp_create: ") + hipGetErrorString(e));
    }
    *out = ctx.release();
    return DP_OK;
}

extern "C" int dp_create(dp_ctx** out, const dp_model* model, int device)
{
    if (!out) return fail(NO_HANDLE, DP_ERR_INVALID, "dp_create: out is NULL");
    *out = nullptr;
    return dprt::shell(NO_HANDLE, "dp_create", [&] { return create_impl(out, model, device); });
}

extern "C" int dp_destroy(dp_ctx* ctx)
{
    if (!ctx) return DP_ERR_INVALID;
    DeviceGuard guard(ctx->device);
    delete ctx;
    return DP_OK;
}

// The dp_io_* helpers: one runtime call each, on the context's device
template <class Call>
static int io_call(dp_ctx* ctx, bool args_ok, const char* who, Call call)
{
    if (!ctx || !args_ok) return DP_ERR_INVALID;
    return dprt::shell(ctx, who, [&] {
        DEVICE_GUARD(ctx);
        const hipError_t e = call();
        return e == hipSuccess ? (int)DP_OK : fail(ctx, DP_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    });
}
extern "C" int dp_io_alloc(dp_ctx* ctx, unsigned long long bytes, void** dev_ptr)
{
    return io_call(ctx, dev_ptr, "dp_io_alloc", [&] { const hipError_t e = dprt::device_alloc(dev_ptr, bytes); return e != hipSuccess ? e : hipMemset(*dev_ptr, 0, bytes); });
}
extern "C" int dp_io_free(dp_ctx* ctx, void* dev_ptr) { return io_call(ctx, true, "dp_io_free", [&] { return dprt::device_free(dev_ptr); }); }
extern "C" int dp_io_upload(dp_ctx* ctx, void* dev_dst, const void* host_src, unsigned long long bytes, void* stream)
{
    return io_call(ctx, dev_dst && host_src, "dp_io_upload", [&] { return hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream); });
}
extern "C" int dp_io_download(dp_ctx* ctx, void* host_dst, const void* dev_src, unsigned long long bytes, void* stream)
{
    return io_call(ctx, host_dst && dev_src, "dp_io_download", [&] { return hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream); });
}
extern "C" int dp_io_alloc_host(dp_ctx* ctx, unsigned long long bytes, void** host_ptr)
{
    return io_call(ctx, host_ptr, "dp_io_alloc_host", [&] {
        const hipError_t e = dprt::pinned_alloc(host_ptr, bytes);
        if (e == hipSuccess) std::memset(*host_ptr, 0, bytes);
        return e;
    });
}
extern "C" int dp_io_free_host(dp_ctx* ctx, void* host_ptr) { return io_call(ctx, true, "dp_io_free_host", [&] { return dprt::pinned_free(host_ptr); }); }
extern "C" int dp_stream_sync(dp_ctx* ctx, void* stream) { return io_call(ctx, true, "dp_stream_sync", [&] { return hipStreamSynchronize((hipStream_t)stream); }); }

extern "C" int dp_kernel_geometry(const dp_ctx* ctx, int* frames_per_block, int* threads_per_block, int* lds_bytes)
{ // of the kernel the context's launches use
    (void)ctx;
#ifdef DP_REF8_BUILD
    if (frames_per_block) *frames_per_block = FPB;
    if (threads_per_block) *threads_per_block = NTHREADS;
    if (lds_bytes) *lds_bytes = dp_kernel_lds_bytes();
#else
    const int w16w = ctx && ctx->last_kernel >= 16 ? ctx->last_kernel / 4 : 0; // waves per workgroup of the last dp_w16 launch
    const bool k16 = w16w != 0;
    if (frames_per_block) *frames_per_block = k16 ? w16w * dp_w16_frames_per_wave() : dp_w4_frames_per_block();
    if (threads_per_block) *threads_per_block = k16 ? w16w * 64 : 256;
    if (lds_bytes) *lds_bytes = k16 ? dp_w16_lds_bytes() : dp_w4_lds_bytes();
#endif
    return DP_OK;
}

static void fill_model_args(const dp_ctx* ctx, KArgs& k)
{
    std::memset(&k, 0, sizeof(k));
    k.wfrag = ctx->d_wfrag.get();
    k.bias = ctx->d_bias.get();
    k.items = ctx->d_items.get();
    k.w4img = ctx->d_w4img.get();
    k.w4bias = ctx->d_w4bias.get();
    k.w4pairs = ctx->d_w4pairs.get();
    k.w16img = ctx->d_w16img.get();
    k.w16bias = ctx->d_w16bias.get();
    k.w16slots = ctx->d_w16slots.get();
    std::memcpy(k.smask, ctx->smask.data(), sizeof(k.smask));
}

// A sized struct as the caller compiled it (include/dragposer.h: struct_size) -- the library's defence against a caller built from another header.
// check_sized: the size word must lie in [min_size, 4096] and reserved0 (every sized struct but dp_params has it) must be 0.  copy_sized: a copy
// of the first struct_size bytes over a zeroed struct of THIS build -- a field the caller's header did not have reads as its default.
//   name, init: the struct's name and its *_INIT hint, for the message;  pre05: the struct existed before 0.5 without its size word
//   (dp_params, dp_result, dp_seq_results), so a small size is most likely a caller compiled against that header, and the message says so
struct Sized {
    const char *name, *init;
    unsigned min_size;
    bool pre05;
};
template <class T>
static int check_sized(dp_ctx* ctx, const T* in, const Sized& s, const char* who)
{
    unsigned reserved0 = 0u;
    constexpr bool has_reserved0 = !std::is_same<T, dp_params>::value;
    if constexpr (has_reserved0) reserved0 = in->reserved0;
    if (in->struct_size < s.min_size || in->struct_size > 4096u || reserved0 != 0u)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": " + s.name + ".struct_size is " + std::to_string(in->struct_size) +
                                             (has_reserved0 ? " (reserved0 " + std::to_string(reserved0) + ")" : "") + ", this library" +
                                             (s.pre05 ? " (DP_VERSION " + std::to_string(DP_VERSION) + ")" : "") + " expects at least " +
                                             std::to_string(s.min_size) + (has_reserved0 ? " and reserved0 = 0" : "") +
                                             (s.pre05 ? " -- was the caller compiled against a pre-0.5 dragposer.h?" : "") + "  (" + s.init + ")");
    return DP_OK;
}
template <class T>
static void copy_sized(const T* in, T& o)
{
    std::memset(&o, 0, sizeof(o));
    std::memcpy(&o, in, std::min<size_t>(in->struct_size, sizeof(o)));
}
template <class T>
static int take_sized(dp_ctx* ctx, const T* in, T& o, const Sized& s, const char* who)
{
    if (int rc = check_sized(ctx, in, s, who)) return rc;
    copy_sized(in, o);
    return DP_OK;
}
// (each struct's minimum: its first version, up to the named field)
constexpr Sized PARAMS_V500 = {"dp_params", "dp_params p = DP_PARAMS_INIT;", offsetof(dp_params, kernel) + sizeof(int), true};
constexpr Sized RESULT_V500 = {"dp_result", "dp_result r = DP_RESULT_INIT;", offsetof(dp_result, clock) + sizeof(void*), true};
constexpr Sized SEQ_RESULTS_V500 = {"dp_seq_results", "dp_seq_results r = DP_SEQ_RESULTS_INIT;", offsetof(dp_seq_results, status) + sizeof(void*), true};
constexpr Sized SKEL_IN_V510 = {"dp_skeleton_in", "dp_skeleton_in s = DP_SKELETON_IN_INIT;", offsetof(dp_skeleton_in, stride) + sizeof(int), false};
constexpr Sized GRAD_IN_V510 = {"dp_grad_in", "dp_grad_in g = DP_GRAD_IN_INIT;", offsetof(dp_grad_in, rot) + sizeof(void*), false};
constexpr Sized CONS_V510 = {"dp_constraints", "dp_constraints c = DP_CONSTRAINTS_INIT;", offsetof(dp_constraints, loss_extra) + sizeof(void*), false};
constexpr Sized TERMS_V510 = {"dp_terms", "dp_terms t = DP_TERMS_INIT;", offsetof(dp_terms, loss_terms) + sizeof(void*), false};
constexpr Sized HOLDS_V530 = {"dp_holds", "dp_holds h = DP_HOLDS_INIT;", offsetof(dp_holds, trace) + sizeof(void*), false};
constexpr Sized LATENT_AR_V540 = {"dp_latent_ar", "dp_latent_ar r = DP_LATENT_AR_INIT;", offsetof(dp_latent_ar, trace) + sizeof(void*), false};
constexpr Sized GAPS_V550 = {"dp_gaps", "dp_gaps g = DP_GAPS_INIT;", offsetof(dp_gaps, trace) + sizeof(void*), false};
constexpr Sized TETHERS_V570 = {"dp_tethers", "dp_tethers t = DP_TETHERS_INIT;", offsetof(dp_tethers, trace) + sizeof(void*), false};
constexpr Sized POINTS_V580 = {"dp_points", "dp_points p = DP_POINTS_INIT;", offsetof(dp_points, coeff) + sizeof(void*), false};
constexpr Sized LM_PARAMS_V590 = {"dp_lm_params", "dp_lm_params p = DP_LM_PARAMS_INIT;", offsetof(dp_lm_params, stop_eps_rot) + sizeof(float), false};
constexpr Sized LM_EXTRA_V590 = {"dp_lm_extra", "dp_lm_extra e = DP_LM_EXTRA_INIT;", offsetof(dp_lm_extra, loss0) + sizeof(void*), false};
constexpr Sized SEQ_LM_EXTRA_V600 = {"dp_seq_lm_extra", "dp_seq_lm_extra e = DP_SEQ_LM_EXTRA_INIT;", offsetof(dp_seq_lm_extra, joint_pos) + sizeof(void*), false};
constexpr Sized BONE_FIT_V510 = {"dp_bone_fit", "dp_bone_fit f = DP_BONE_FIT_INIT;", offsetof(dp_bone_fit, workspace_bytes) + sizeof(size_t), false};
constexpr Sized BONE_FIT_RESULT_V510 = {"dp_bone_fit_result", "dp_bone_fit_result r = DP_BONE_FIT_RESULT_INIT;", offsetof(dp_bone_fit_result, status) + sizeof(void*), false};
constexpr Sized CLIP_LM_EXTRA_V510 = {"dp_clip_lm_extra", "dp_clip_lm_extra e = DP_CLIP_LM_EXTRA_INIT;", offsetof(dp_clip_lm_extra, workspace_bytes) + sizeof(size_t), false};
constexpr Sized SEQ_EXTRA_V520 = {"dp_seq_extra", "dp_seq_extra e = DP_SEQ_EXTRA_INIT;", offsetof(dp_seq_extra, row_step) + sizeof(int) * DP_MAX_TERMS, false};

static int take_params(dp_ctx* ctx, const dp_params* p, dp_params& o, const char* who)
{
    if (int rc = check_sized(ctx, p, PARAMS_V500, who)) return rc;
    // A 0.4 caller's struct is 52 bytes and starts with n_iter: one that asks for 56 ... 4096 iterations passes the size test above.  Its SECOND word is
    // `lr`, whose bits read as an iteration count are beyond DP_MAX_ITERS for any learning rate above 1.4e-39 -- tested HERE, on the two words every
    // layout has, before anything is copied: the 52-byte struct is never read past.
    if (p->n_iter < 1 || p->n_iter > DP_MAX_ITERS)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": n_iter " + std::to_string(p->n_iter) + " out of range [1, DP_MAX_ITERS] (dp_params.struct_size " +
                                             std::to_string(p->struct_size) + ": if that is the iteration count you meant, the caller was compiled against a pre-0.5 "
                                             "dragposer.h, whose dp_params starts with n_iter; dp_params p = DP_PARAMS_INIT;)");
    copy_sized(p, o);
    return DP_OK;
}
static int take_result(dp_ctx* ctx, const dp_result* r, dp_result& o, const char* who)
{
    std::memset(&o, 0, sizeof(o)); // (NULL: no result is wanted)
    return r ? take_sized(ctx, r, o, RESULT_V500, who) : DP_OK;
}

// Adam's per-iteration scalars, as torch computes them in Python doubles: a table for the first MAX_ITERS iterations (in the kernel arguments), and
// what the kernels need to continue the two products on the device beyond it (dp_kernel.h: AdamCont)
static void fill_adam(KArgs& k, const dp_params& p)
{
    double b1t = 1.0, b2t = 1.0;
    for (int t = 0; t < MAX_ITERS; ++t) {
        b1t *= (double)p.beta1;
        b2t *= (double)p.beta2;
        if (t < p.n_iter) {
            k.tab.step[t] = (float)((double)p.lr / (1.0 - b1t));
            k.tab.bc2s[t] = (float)(1.0 / std::sqrt(1.0 - b2t));
        }
    }
    k.cont.beta1 = (double)p.beta1; k.cont.beta2 = (double)p.beta2; k.cont.lr = (double)p.lr;
    k.cont.b1t = b1t; k.cont.b2t = b2t;
}

// The three parts every optimise kernel's argument block has under the same field names (KArgs: dp_kernel.h; dpcons::Args, dpcons::TermArgs: dp_cons.h)
template <class A>
static void fill_batch(A& a, const dp_batch& in)
{
    a.z0 = in.z0; a.z_tgt = in.z_tgt; a.cur_rot = in.cur_rot; a.tgt_pos = in.tgt_pos; a.tgt_rot = in.tgt_rot; a.w = in.w; a.tracked = in.tracked;
    a.n_frames = in.n_frames;
}
template <class A>
static void fill_results(A& a, const dp_result& out)
{ // (dp_result.clock: KArgs only, set where it is used)
    a.z = out.z; a.z_pre = out.z_pre; a.pose = out.pose; a.disp = out.disp; a.world_disp = out.world_disp;
    a.world_rot = out.world_rot; a.pos = out.pos; a.rot = out.rot; a.loss = out.loss; a.iters = out.iters; a.status = out.status;
}
template <class A>
static void fill_loop(A& a, const dp_params& p, bool early_stop)
{
    a.n_iter = p.n_iter;
    a.lam_rot = p.lambda_rot; a.lam_tmp = p.lambda_tmp; a.ctmp = 2.f * p.lambda_tmp / 24.f;
    // torch passes (1-beta) as Python doubles into fp32 tensor ops
    a.beta2 = p.beta2; a.one_m_b1 = (float)(1.0 - (double)p.beta1); a.one_m_b2 = (float)(1.0 - (double)p.beta2);
    a.eps = p.eps;
    a.early_stop = early_stop ? 1 : 0;
    a.stop_eps_pos = p.stop_eps_pos; a.stop_eps_rot = p.stop_eps_rot; a.min_loss_incr = p.min_loss_incr;
}

// What every optimise entry point asks of its batch and of Adam's hyper-parameters
static int check_batch(dp_ctx* ctx, const dp_batch* in, const char* who)
{
    if (in->n_frames <= 0) return fail(ctx, DP_ERR_INVALID, std::string(who) + ": n_frames must be positive");
    if (!in->z0 || !in->z_tgt || !in->cur_rot || !in->tgt_pos || !in->tgt_rot || !in->w || !in->tracked)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": NULL input array");
    return DP_OK;
}
static int check_adam(dp_ctx* ctx, const dp_params& p, const char* who)
{
    if (!(p.lr > 0.f) || !(p.beta1 >= 0.f && p.beta1 < 1.f) || !(p.beta2 >= 0.f && p.beta2 < 1.f))
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": bad Adam hyper-parameters");
    if (!(p.eps > 0.f)) return fail(ctx, DP_ERR_INVALID, std::string(who) + ": Adam eps must be > 0 (include/dragposer.h: dp_params.eps)");
    return DP_OK;
}

// The shell of an entry point that reports a NULL context in words: the refusal, then dprt::shell
template <class Body>
static int entry(dp_ctx* ctx, const char* who, Body body)
{
    if (!ctx) return dprt::shell(NO_HANDLE, who, [&] { return fail(NO_HANDLE, DP_ERR_INVALID, std::string(who) + ": ctx is NULL"); });
    return dprt::shell(ctx, who, body);
}
// ... and of the entry points older than that, which refuse a NULL context by the code alone
template <class Body>
static int entry_quiet(dp_ctx* ctx, const char* who, Body body)
{
    return ctx ? dprt::shell(ctx, who, body) : (int)DP_ERR_INVALID;
}

// The test-only library (DP_REF8_BUILD) has the round-1 kernel behind dp_optimize and dp_forward only: every other launch is refused, after its
// argument checks (dp_optimize_sequence: before them).  A context without device memory (dp_debug_host_ctx) is refused by every launch, after
// everything else, before anything of the image is read.
constexpr bool REF8_BUILD = KERNEL_CHOICE == 8;
static int refuse_ref8(dp_ctx* ctx, const char* who) { return fail(ctx, DP_ERR_UNSUPPORTED, std::string(who) + ": not part of the test-only library"); }
static int refuse_no_image(dp_ctx* ctx, const char* who) { return fail(ctx, DP_ERR_DEVICE, std::string(who) + ": the context has no device image"); }

// Which kernel runs a launch: the wave-private kernel of dp_w4.hip (4 frames per wave, no workgroup barrier in the
// loop); in the test-only library the previous decomposition (dp_kernel.hip: 16 frames per 8-wave workgroup).  Both
// implement the same operator within the tolerance of tests/test_hip_w4.py.
// skel: the per-frame skeleton units of the same layout (dp_w4_skel.hip, dp_w4_bp_skel.hip: include/dragposer_skeleton.h), never with DP_KERNEL_W16
static int launch(dp_ctx* ctx, KArgs& k, void* stream, int kernel = DP_KERNEL_W4, bool skel = false)
{
    DEVICE_GUARD(ctx);
    ctx->last_kernel = KERNEL_CHOICE;
    ctx->last_pick = LaunchPick{};
#ifdef DP_REF8_BUILD
    (void)kernel; (void)skel;
    hipError_t e = dp_launch_optimize(&k, (hipStream_t)stream);
#else
    // dp_w16: one wave per SIMD (4 waves, 64 frames per workgroup) until every SIMD of the chip has a wave; beyond that two
    // (8 waves, 128 frames per workgroup): one wave's matrix phases under the other's vector phases
    const int w16_waves = k.n_frames > ctx->n_cu * 4 * dp_w16_frames_per_wave() ? 8 : 4;
    if (kernel == DP_KERNEL_W16) ctx->last_kernel = 16 * (w16_waves / 4);
    LaunchPick* pick = &ctx->last_pick;
    hipError_t e = kernel == DP_KERNEL_W16 ? dp_launch_w16(&k, (hipStream_t)stream, w16_waves, pick)
                   : skel                  ? (ctx->w4_bp ? dp_launch_w4sk_bp(&k, (hipStream_t)stream, pick) : dp_launch_w4sk(&k, (hipStream_t)stream, pick))
                   : ctx->w4_bp            ? dp_launch_w4_bp(&k, (hipStream_t)stream, pick)
                                           : dp_launch_w4(&k, (hipStream_t)stream, pick);
#endif
    if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string("kernel launch: ") + hipGetErrorString(e));
    return DP_OK;
}

// host-only, exported for the tests: the instantiation the context's last dp_optimize / dp_forward / dp_optimize_sequence launched, as the
// launcher recorded it -- out[5] = unit (1 dp_w4.hip, 2 dp_w4_bp.hip, 3 dp_w16*.hip, 4 dp_w4_skel.hip, 5 dp_w4_bp_skel.hip, 6 dp_w4_bp_lv.hip -- the body-part
// layout's fixed-count optimising launches without the debug dump; 0: none yet, or the test-only library), waves per workgroup, and the EARLY, SEQ and
// LONG template flags
extern "C" int dp_debug_last_launch(const dp_ctx* ctx, int* out)
{
    if (!ctx || !out) return DP_ERR_INVALID;
    const LaunchPick& p = ctx->last_pick;
    out[0] = p.unit; out[1] = p.waves; out[2] = p.early; out[3] = p.seq; out[4] = p.lng;
    return DP_OK;
}

// host-only, exported for the tests: upload the w4 image, bias rows and pairs in the dense (bp = 0) or the body-part (bp = 1) layout, so that
// one model runs through both units; bp = -1 only queries.  Returns the layout now in place, or DP_ERR_UNSUPPORTED when the model does not fit
// the body-part layout (dp_create found a left-out weight that is not zero).  The caller has no launch of the context in flight.
extern "C" int dp_debug_set_w4_layout(dp_ctx* ctx, int bp)
{
    if (!ctx || bp < -1 || bp > 1) return DP_ERR_INVALID;
    if (bp < 0) return ctx->w4_bp ? 1 : 0;
    return dprt::shell(ctx, "dp_debug_set_w4_layout", [&] {
        if (ctx->w4img_h[bp].empty()) return fail(ctx, DP_ERR_UNSUPPORTED, "dp_debug_set_w4_layout: the model does not fit the body-part layout");
        DEVICE_GUARD(ctx);
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipMemcpy(ctx->d_w4img.get(), ctx->w4img_h[bp].data(), ctx->w4img_h[bp].size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->d_w4bias.get(), ctx->w4bias_h[bp].data(), ctx->w4bias_h[bp].size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->d_w4pairs.get(), ctx->w4pairs_h[bp].data(), ctx->w4pairs_h[bp].size() * sizeof(dpw4::Pair), hipMemcpyHostToDevice));
        ctx->w4_bp = bp == 1;
        return bp;
    });
}

// include/dragposer_skeleton.h: dp_skeleton_in as the caller compiled it (the entry point has refused a NULL one) -> what goes into
// KArgs::skel / skel_stride
static int take_skeleton(dp_ctx* ctx, const dp_skeleton_in* s, const float*& off, int& stride, const char* who)
{
    dp_skeleton_in sv;
    if (int rc = take_sized(ctx, s, sv, SKEL_IN_V510, who)) return rc;
    if (!sv.offsets) return fail(ctx, DP_ERR_INVALID, std::string(who) + ": dp_skeleton_in.offsets is NULL");
    if (sv.stride != 0 && sv.stride != DP_SKELETON_STRIDE)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": dp_skeleton_in.stride is " + std::to_string(sv.stride) +
                                             ", expected 66 (one [22][3] skeleton per frame / sequence) or 0 (one for the launch)");
    off = sv.offsets;
    stride = sv.stride;
    return DP_OK;
}
static int refuse_null_skeleton(dp_ctx* ctx, const char* who) { return fail(ctx, DP_ERR_INVALID, std::string(who) + ": the skeleton is NULL"); }
static int refuse_w16_skeleton(dp_ctx* ctx, const char* who)
{
    return fail(ctx, DP_ERR_UNSUPPORTED, std::string(who) + ": DP_KERNEL_W16 keeps the bone offsets in per-slot constants; per-frame skeletons run on "
                                                            "DP_KERNEL_W4 (DP_KERNEL_AUTO takes it)");
}

// dp_optimize (sk = NULL) and dp_optimize_skeleton (who names the caller in the messages)
static int optimize_impl(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_result* out_in, float* dbg, void* stream,
                         const dp_skeleton_in* sk, const char* who)
{
    if (!in || !p_in) return fail(ctx, DP_ERR_INVALID, std::string(who) + ": NULL batch/params");
    dp_params p; dp_result out;
    if (int rc = take_params(ctx, p_in, p, who)) return rc;
    if (int rc = take_result(ctx, out_in, out, who)) return rc;
    if (int rc = check_batch(ctx, in, who)) return rc;
    if (REF8_BUILD && p.n_iter > MAX_ITERS)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": n_iter out of range [1,256] (the test-only kernel reads the argument table only)");
    if (int rc = check_adam(ctx, p, who)) return rc;
    const float* sk_off = nullptr;
    int sk_stride = 0;
    if (sk) // (include/dragposer_skeleton.h: the dp_w4sk units, at every batch size)
        if (int rc = take_skeleton(ctx, sk, sk_off, sk_stride, who)) return rc;
    // which kernel (include/dragposer.h: DP_KERNEL_*)
    if (p.kernel != DP_KERNEL_AUTO && p.kernel != DP_KERNEL_W4 && p.kernel != DP_KERNEL_W16)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": unknown kernel selector");
    if (sk && p.kernel == DP_KERNEL_W16) return refuse_w16_skeleton(ctx, who);
    if (sk && REF8_BUILD) return refuse_ref8(ctx, who);
    if (!ctx->d_w4img.get()) return refuse_no_image(ctx, who);
    KArgs k;
    fill_model_args(ctx, k);
    fill_batch(k, *in);
    fill_results(k, out);
    k.clk = out.clock;
    k.dbg = dbg;
    k.mode = 0;
    fill_loop(k, p, p.early_stop != 0);
    fill_adam(k, p);
    k.skel = sk_off; k.skel_stride = sk_stride;
    if (sk) return launch(ctx, k, stream, DP_KERNEL_W4, true);
    if (p.kernel == DP_KERNEL_W16 && !ctx->d_w16img.get())
        return fail(ctx, DP_ERR_UNSUPPORTED, "dp_optimize: DP_KERNEL_W16 is laid out for the reference's 22-joint skeleton only");
    // (beyond the argument table of Adam scalars, n_iter > 256, both kernels have LONG instantiations that continue them on the device)
    return launch(ctx, k, stream, p.kernel == DP_KERNEL_AUTO ? dp_auto_kernel(ctx, in->n_frames) : p.kernel);
}

// private extension used by the tests: same as dp_optimize, plus an optional debug dump
// [B][240] = y(104) | dL/dy(104) | dL/dz(24) | pad, all of iteration 0.
extern "C" int dp_optimize_debug(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_result* out_in, float* dbg, void* stream)
{
    return entry_quiet(ctx, "dp_optimize", [&] { return optimize_impl(ctx, in, p_in, out_in, dbg, stream, nullptr, "dp_optimize"); });
}

extern "C" int dp_auto_kernel(const dp_ctx* ctx, int n_frames)
{
    if (!ctx || n_frames <= 0) return DP_ERR_INVALID;
#ifdef DP_REF8_BUILD
    return DP_KERNEL_W4;
#else
    // more than TWO rounds of dp_w4's 16 frames per CU: dp_w16 (where its slot map fits the skeleton).  Up to two rounds dp_w4 is the faster one
    // since round 5 (its waves' staggered start: 0.252 ms for 8192 frames against dp_w16's 0.273 at the steady clock, 0.251 against 0.274 at 6144,
    // profiles/r05_batch_sweep.txt; equal from an idle GPU); from three rounds on dp_w16 wins by 1.3x and more
    return ctx->d_w16img.get() != nullptr && n_frames > ctx->n_cu * 32 ? DP_KERNEL_W16 : DP_KERNEL_W4;
#endif
}

extern "C" int dp_optimize(dp_ctx* ctx, const dp_batch* in, const dp_params* p, const dp_result* out, void* stream)
{
    return dp_optimize_debug(ctx, in, p, out, nullptr, stream);
}

static int forward_impl(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_skeleton_in* sk, const dp_result* out_in, void* stream,
                        const char* who)
{
    if (n_frames <= 0 || !z || !cur_rot || !out_in) return fail(ctx, DP_ERR_INVALID, std::string(who) + ": bad arguments");
    dp_result out;
    if (int rc = take_result(ctx, out_in, out, who)) return rc;
    const float* sk_off = nullptr;
    int sk_stride = 0;
    if (sk) {
        if (int rc = take_skeleton(ctx, sk, sk_off, sk_stride, who)) return rc;
        if (REF8_BUILD) return refuse_ref8(ctx, who);
    }
    if (!ctx->d_w4img.get()) return refuse_no_image(ctx, who);
    KArgs k;
    fill_model_args(ctx, k);
    k.skel = sk_off; k.skel_stride = sk_stride;
    k.z0 = z; k.cur_rot = cur_rot;
    fill_results(k, out);
    k.z = nullptr; k.z_pre = nullptr; k.loss = nullptr; k.iters = nullptr;
    k.n_frames = n_frames; k.n_iter = 1; k.mode = 1;
    return launch(ctx, k, stream, DP_KERNEL_W4, sk != nullptr);
}

extern "C" int dp_forward(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_result* out, void* stream)
{
    return entry_quiet(ctx, "dp_forward", [&] { return forward_impl(ctx, n_frames, z, cur_rot, nullptr, out, stream, "dp_forward"); });
}

// host-only, exported for the CPU tests: a context with no device and no device memory -- argument checks run on it, every launch is
// refused (DP_ERR_DEVICE); dp_destroy frees it
extern "C" int dp_debug_host_ctx(dp_ctx** out)
{
    if (!out) return DP_ERR_INVALID;
    *out = new (std::nothrow) dp_ctx();
    return *out ? DP_OK : DP_ERR_DEVICE;
}

// include/dragposer_grad.h: dp_forward_vjp (sk = NULL, dp_vjp.hip) and dp_forward_vjp_skeleton (dp_vjp_skel.hip; who names the caller in the messages)
static int vjp_impl(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_skeleton_in* sk, const dp_grad_in* g, float* dz,
                    float* dcur_rot, float* doffsets, int* status, void* stream, const char* who)
{
    const std::string w = who;
    if (n_frames <= 0) return fail(ctx, DP_ERR_INVALID, w + ": n_frames must be positive");
    if (!z || !cur_rot || !g || !dz) return fail(ctx, DP_ERR_INVALID, w + ": NULL z, cur_rot, g or dz");
    dp_grad_in gv;
    if (int rc = take_sized(ctx, g, gv, GRAD_IN_V510, who)) return rc;
    const float* sk_off = nullptr;
    int sk_stride = 0;
    if (sk)
        if (int rc = take_skeleton(ctx, sk, sk_off, sk_stride, who)) return rc;
    if (REF8_BUILD) return refuse_ref8(ctx, who);
    if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
    DEVICE_GUARD(ctx);
    dpvjp::SkelArgs a;
    a.img = ctx->d_vjpimg.get();
    a.z = z; a.cur_rot = cur_rot;
    a.g_pose = gv.pose; a.g_disp = gv.disp; a.g_wdisp = gv.world_disp; a.g_wrot = gv.world_rot; a.g_pos = gv.pos; a.g_rot = gv.rot;
    a.dz = dz; a.dcur = dcur_rot; a.status = status;
    a.n_frames = n_frames;
    a.skel = sk_off; a.skel_stride = sk_stride; a.doff = doffsets;
    const hipError_t e = sk ? dp_launch_vjp_skel(&a, (hipStream_t)stream) : dp_launch_vjp(&a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, w + ": kernel launch: " + hipGetErrorString(e));
    return DP_OK;
}

extern "C" int dp_forward_vjp(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_grad_in* g, float* dz, float* dcur_rot,
                              int* status, void* stream)
{
    const char* who = "dp_forward_vjp";
    return entry(ctx, who, [&] { return vjp_impl(ctx, n_frames, z, cur_rot, nullptr, g, dz, dcur_rot, nullptr, status, stream, who); });
}

extern "C" int dp_forward_vjp_skeleton(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_skeleton_in* skel,
                                       const dp_grad_in* g, float* dz, float* dcur_rot, float* doffsets, int* status, void* stream)
{
    const char* who = "dp_forward_vjp_skeleton";
    return entry(ctx, who, [&] {
        if (!skel) return refuse_null_skeleton(ctx, who);
        return vjp_impl(ctx, n_frames, z, cur_rot, skel, g, dz, dcur_rot, doffsets, status, stream, who);
    });
}

// dp_optimize_constrained (A = dpcons::Args), dp_optimize_terms (dpcons::TermArgs) and their per-frame-skeleton forms (dpcons::SkelArgs,
// dpcons::TermSkelArgs: dp_cons_skel.h), whose callers have refused a NULL argument: everything but the entry point's own structs.  own(a) validates that struct and writes its fields into the zeroed argument block -- between the checks of
// params / result and those of the batch, which is the order the refusals have.
static_assert(DP_MAX_TERMS == dpcons::MAX_TERMS, "dp_cons.h's table holds DP_MAX_TERMS terms");
template <class A, class Own>
static int constrained_impl(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_result* out_in, void* stream, const char* who, Own own,
                            hipError_t (*launch_fn)(const A*, hipStream_t))
{
    dp_params p; dp_result out;
    if (int rc = take_params(ctx, p_in, p, who)) return rc;
    if (int rc = take_result(ctx, out_in, out, who)) return rc;
    A a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = own(a)) return rc;
    if (int rc = check_batch(ctx, in, who)) return rc;
    if (int rc = check_adam(ctx, p, who)) return rc;
    if (REF8_BUILD) return refuse_ref8(ctx, who);
    if (!launch_fn) return fail(ctx, DP_ERR_UNSUPPORTED, std::string(who) + ": this library was linked without dp_cons_points.hip"); // (the one weak per-frame unit)
    if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
    DEVICE_GUARD(ctx);
    a.img = ctx->d_vjpimg.get();
    fill_batch(a, *in);
    fill_results(a, out);
    fill_loop(a, p, p.early_stop != 0);
    a.beta1d = p.beta1; a.beta2d = p.beta2; a.lrd = p.lr; // (Adam's bias corrections are Python doubles in torch: fill_adam for dp_optimize)
    const hipError_t e = launch_fn(&a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string(who) + ": kernel launch: " + hipGetErrorString(e));
    return DP_OK;
}

// What a sequence launch (include/dragposer_sequence_constraints.h) asks of the two per-frame pointers of dp_constraints / dp_terms: the terms
// read the state's own global position step after step, so `global_pos` is NULL or that array, and the per-frame output is dp_seq_extra's
static int seq_pointers(dp_ctx* ctx, const float*& global_pos, const float* per_frame_out, const dp_seq_state* seq, const std::string& w, const char* strct,
                        const char* out_name)
{
    if (global_pos && global_pos != seq->global_pos)
        return fail(ctx, DP_ERR_INVALID, w + ": " + strct + ".global_pos must be NULL or dp_seq_state.global_pos (the terms read the sequence's own position)");
    if (per_frame_out)
        return fail(ctx, DP_ERR_INVALID, w + ": " + strct + "." + out_name + " is one row per frame; a sequence launch writes dp_seq_extra." + out_name);
    global_pos = seq->global_pos;
    return DP_OK;
}

// include/dragposer_constraints.h: dp_constraints validated and written into the argument block (constrained_impl's own(a)), for
// dp_optimize_constrained, dp_optimize_constrained_skeleton and, with `seq` (the launch's state), dp_optimize_sequence_constrained (who names
// the caller in the messages)
static int take_constraints(dp_ctx* ctx, const dp_constraints* c_in, dpcons::Args& a, const char* who, const dp_seq_state* seq = nullptr)
{
    const std::string w = who;
    dp_constraints c;
    if (int rc = take_sized(ctx, c_in, c, CONS_V510, who)) return rc;
    if (seq)
        if (int rc = seq_pointers(ctx, c.global_pos, c.loss_extra, seq, w, "dp_constraints", "loss_extra")) return rc;
    const float wts[4] = {c.w_feet_floor, c.w_head_hips_forward, c.w_head_hips_colinear, c.w_hips_feet_colinear};
    for (float x : wts)
        if (!(x >= 0.f && x <= 3.0e38f)) return fail(ctx, DP_ERR_INVALID, w + ": a weight is negative or not finite");
    const int joints[6] = {c.floor_joints[0], c.floor_joints[1], c.foot_joints[0], c.foot_joints[1], c.head_joint, c.hips_joint};
    for (int jj : joints)
        if (jj < 0 || jj >= NJ) return fail(ctx, DP_ERR_INVALID, w + ": joint index " + std::to_string(jj) + " outside 0..21");
    if (c.up_axis < 0 || c.up_axis > 2) return fail(ctx, DP_ERR_INVALID, w + ": up_axis outside 0..2");
    const float rest[7] = {c.floor_level, c.fwd_axis[0], c.fwd_axis[1], c.fwd_axis[2], c.fwd_threshold, c.fwd_margin, c.feet_radius};
    for (float x : rest)
        if (!(std::fabs(x) <= 3.0e38f)) return fail(ctx, DP_ERR_INVALID, w + ": a constraint parameter is not finite");
    if (!seq && c.w_feet_floor != 0.f && !c.global_pos) return fail(ctx, DP_ERR_INVALID, w + ": global_pos is NULL while feet_floor is on");
    a.global_pos = c.global_pos;
    a.loss_extra = c.loss_extra;
    a.w_floor = c.w_feet_floor; a.w_fwd = c.w_head_hips_forward; a.w_hcol = c.w_head_hips_colinear; a.w_feet = c.w_hips_feet_colinear;
    a.floor_j[0] = c.floor_joints[0]; a.floor_j[1] = c.floor_joints[1]; a.foot_j[0] = c.foot_joints[0]; a.foot_j[1] = c.foot_joints[1];
    a.head = c.head_joint; a.hips = c.hips_joint; a.up = c.up_axis; a.one_sided = c.floor_one_sided ? 1 : 0;
    a.floor_level = c.floor_level;
    a.fwd[0] = c.fwd_axis[0]; a.fwd[1] = c.fwd_axis[1]; a.fwd[2] = c.fwd_axis[2];
    a.fwd_thr = c.fwd_threshold; a.fwd_margin = c.fwd_margin;
    a.feet_r2 = c.feet_radius * c.feet_radius; // (the reference: a Python float subtracted from a float32 tensor)
    return DP_OK;
}

extern "C" int dp_optimize_constrained(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_constraints* c_in, const dp_result* out_in,
                                       void* stream)
{
    const char* who = "dp_optimize_constrained";
    const auto own = [&](dpcons::Args& a) -> int { return take_constraints(ctx, c_in, a, who); };
    return entry(ctx, who, [&] {
        if (!in || !p_in || !c_in || !out_in) return fail(ctx, DP_ERR_INVALID, "dp_optimize_constrained: NULL batch, params, constraints or result");
        return constrained_impl<dpcons::Args>(ctx, in, p_in, out_in, stream, who, own, dp_launch_cons);
    });
}

// the same on dp_cons_skel.hip: the skeleton struct is checked after dp_constraints and before the batch
extern "C" int dp_optimize_constrained_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_constraints* c_in,
                                                const dp_skeleton_in* skel, const dp_result* out_in, void* stream)
{
    const char* who = "dp_optimize_constrained_skeleton";
    const auto own = [&](dpcons::SkelArgs& a) -> int {
        if (int rc = take_constraints(ctx, c_in, a, who)) return rc;
        return take_skeleton(ctx, skel, a.skel, a.skel_stride, who);
    };
    return entry(ctx, who, [&] {
        if (!in || !p_in || !c_in || !out_in)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_constrained_skeleton: NULL batch, params, constraints or result");
        if (!skel) return refuse_null_skeleton(ctx, who);
        return constrained_impl<dpcons::SkelArgs>(ctx, in, p_in, out_in, stream, who, own, dp_launch_cons_skel);
    });
}

// one term of the table: "" when it is well-formed, otherwise what is wrong with it (n_idx: the indices a term may name, 22 joints and,
// through the entry points of include/dragposer_points.h, up to DP_MAX_POINTS points behind them -- take_points narrows that to the call's)
static std::string check_term(const dp_term& t, int n_idx)
{
    const auto fin = [](float x) { return std::fabs(x) <= 3.0e38f; };
    const auto unit = [](const float* v) {
        const double n = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
        return std::fabs(n - 1.0) <= 1e-4;
    };
    const auto zero = [](const float* v) { return v[0] == 0.f && v[1] == 0.f && v[2] == 0.f; };
    if (t.type != DP_TERM_PLANE && t.type != DP_TERM_DISTANCE && t.type != DP_TERM_ALIGN) return "unknown type " + std::to_string(t.type);
    if (t.flags & ~(DP_TERM_ONE_SIDED | DP_TERM_DROP_UP)) return "unknown flag bits " + std::to_string(t.flags);
    if (t.joint_a < 0 || t.joint_a >= n_idx) return "joint_a " + std::to_string(t.joint_a) + " outside 0.." + std::to_string(n_idx - 1);
    if (t.joint_b < -1 || t.joint_b >= n_idx) return "joint_b " + std::to_string(t.joint_b) + " outside -1.." + std::to_string(n_idx - 1);
    if (t.type == DP_TERM_PLANE && t.joint_b != -1) return "a PLANE has no second joint (joint_b must be -1)";
    if (!(t.weight >= 0.f && t.weight <= 3.0e38f)) return "the weight is negative or not finite";
    for (int c = 0; c < 3; ++c)
        if (!fin(t.point[c]) || !fin(t.dir[c]) || !fin(t.axis_a[c]) || !fin(t.axis_b[c])) return "a point, dir or axis is not finite";
    if (!fin(t.p0) || !fin(t.p1)) return "p0 or p1 is not finite";
    if (t.type == DP_TERM_PLANE && !unit(t.dir)) return "the plane's normal (dir) is not unit length";
    if (t.type == DP_TERM_DISTANCE && !(t.p0 >= 0.f && t.p0 <= t.p1)) return "DISTANCE needs 0 <= lo (p0) <= hi (p1)";
    if (t.type == DP_TERM_ALIGN) {
        if (!(t.p0 >= 0.f)) return "ALIGN's threshold (p0) is negative";
        if (zero(t.axis_a) || (t.joint_b >= 0 && zero(t.axis_b))) return "ALIGN's axis is zero";
        if (t.joint_b < 0 && !t.per_frame && !unit(t.dir)) return "ALIGN's world direction (dir) is not unit length";
    }
    return "";
}

// include/dragposer_terms.h: dp_terms validated and written into the argument block (constrained_impl's own(a)), for dp_optimize_terms,
// dp_optimize_terms_skeleton and, with `seq` (the launch's state), dp_optimize_sequence_terms (who names the caller in the messages).
// A: dpcons::TermArgs or one derived from it, or dplm::TermArgs (dp_optimize_lm_terms), which carries the same fields under the same names
template <class A>
static int take_terms(dp_ctx* ctx, const dp_terms* t_in, A& a, const char* who, const dp_seq_state* seq = nullptr, int n_idx = NJ)
{
    static_assert(sizeof(a.tbl) == sizeof(unsigned) * DP_MAX_TERMS * dpcons::TW, "the staged table of dp_cons.h's layout");
    const std::string nm = who;
    dp_terms ts;
    if (int rc = take_sized(ctx, t_in, ts, TERMS_V510, who)) return rc;
    if (seq)
        if (int rc = seq_pointers(ctx, ts.global_pos, ts.loss_terms, seq, nm, "dp_terms", "loss_terms")) return rc;
    if (ts.n_terms < 0 || ts.n_terms > DP_MAX_TERMS)
        return fail(ctx, DP_ERR_INVALID, nm + ": n_terms " + std::to_string(ts.n_terms) + " outside 0..16");
    if (ts.n_terms > 0 && !ts.terms) return fail(ctx, DP_ERR_INVALID, nm + ": NULL terms with n_terms > 0");
    if (ts.up_axis < 0 || ts.up_axis > 2) return fail(ctx, DP_ERR_INVALID, nm + ": up_axis outside 0..2");
    bool need_gp = false;
    for (int k = 0; k < ts.n_terms; ++k) {
        const dp_term& t = ts.terms[k];
        const std::string why = check_term(t, n_idx);
        if (!why.empty()) return fail(ctx, DP_ERR_INVALID, nm + ": term " + std::to_string(k) + ": " + why);
        need_gp = need_gp || (t.weight != 0.f && (t.type == DP_TERM_PLANE || (t.type == DP_TERM_DISTANCE && t.joint_b < 0)));
    }
    if (!seq && need_gp && !ts.global_pos)
        return fail(ctx, DP_ERR_INVALID, nm + ": global_pos is NULL while an active PLANE or point-DISTANCE term needs it");
    a.global_pos = need_gp ? ts.global_pos : nullptr;
    a.up = ts.up_axis;
    a.n_terms = ts.n_terms; a.need_gp = need_gp ? 1 : 0; a.loss_terms = ts.loss_terms;
    for (int k = 0; k < ts.n_terms; ++k) { // dp_cons.h's T_* layout
        const dp_term& t = ts.terms[k];
        unsigned* w = a.tbl + k * dpcons::TW;
        float* wf = (float*)w;
        w[dpcons::T_TYPE] = (unsigned)t.type; w[dpcons::T_JA] = (unsigned)t.joint_a; w[dpcons::T_JB] = (unsigned)t.joint_b;
        w[dpcons::T_FLAGS] = (unsigned)t.flags;
        wf[dpcons::T_W] = t.weight;
        for (int c = 0; c < 3; ++c) {
            wf[dpcons::T_PT + c] = t.point[c]; wf[dpcons::T_DIR + c] = t.dir[c];
            wf[dpcons::T_AXA + c] = t.axis_a[c]; wf[dpcons::T_AXB + c] = t.axis_b[c];
        }
        // DISTANCE: lo^2, hi^2 (float products, as the reference's feet_radius ** 2 meets a float32 tensor)
        wf[dpcons::T_P0] = t.type == DP_TERM_DISTANCE ? t.p0 * t.p0 : t.p0;
        wf[dpcons::T_P1] = t.type == DP_TERM_DISTANCE ? t.p1 * t.p1 : t.p1;
        const float* pf = t.per_frame;
        std::memcpy(w + dpcons::T_ROW, &pf, sizeof(pf));
    }
    return DP_OK;
}

extern "C" int dp_optimize_terms(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_terms* t_in, const dp_result* out_in, void* stream)
{
    const char* who = "dp_optimize_terms";
    const auto own = [&](dpcons::TermArgs& a) -> int { return take_terms(ctx, t_in, a, who); };
    return entry(ctx, who, [&] {
        if (!in || !p_in || !t_in || !out_in) return fail(ctx, DP_ERR_INVALID, "dp_optimize_terms: NULL batch, params, terms or result");
        return constrained_impl<dpcons::TermArgs>(ctx, in, p_in, out_in, stream, who, own, dp_launch_terms);
    });
}

extern "C" int dp_optimize_terms_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_terms* t_in, const dp_skeleton_in* skel,
                                          const dp_result* out_in, void* stream)
{
    const char* who = "dp_optimize_terms_skeleton";
    const auto own = [&](dpcons::TermSkelArgs& a) -> int {
        if (int rc = take_terms(ctx, t_in, a, who)) return rc;
        return take_skeleton(ctx, skel, a.skel, a.skel_stride, who);
    };
    return entry(ctx, who, [&] {
        if (!in || !p_in || !t_in || !out_in) return fail(ctx, DP_ERR_INVALID, "dp_optimize_terms_skeleton: NULL batch, params, terms or result");
        if (!skel) return refuse_null_skeleton(ctx, who);
        return constrained_impl<dpcons::TermSkelArgs>(ctx, in, p_in, out_in, stream, who, own, dp_launch_terms_skel);
    });
}

// include/dragposer_lm.h: dp_lm_params and dp_lm_extra validated and written into the kernel's argument block, in the header's order of
// refusals (dp_lm_params has no reserved0: its size word alone is checked, like dp_params')
// (its launcher is a weak reference, like those of the sequence units below: a library linked without dp_lm.hip refuses the call)
hipError_t dp_launch_lm(const dplm::Args* args, hipStream_t stream) __attribute__((weak));
static int check_lm_params_size(dp_ctx* ctx, const dp_lm_params* p_in, const char* who)
{
    if (p_in->struct_size < LM_PARAMS_V590.min_size || p_in->struct_size > 4096u)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": dp_lm_params.struct_size is " + std::to_string(p_in->struct_size) + ", this library expects at least " +
                                             std::to_string(LM_PARAMS_V590.min_size) + "  (" + LM_PARAMS_V590.init + ")");
    return DP_OK;
}
// ... the values of a dp_lm_params whose size word has passed (dp_optimize_lm, dp_optimize_sequence_lm)
static int take_lm_params(dp_ctx* ctx, const dp_lm_params* p_in, dplm::Args& a, const char* who)
{
    const std::string w = who;
    dp_lm_params p;
    copy_sized(p_in, p);
    if (p.n_steps < 1 || p.n_steps > DP_LM_MAX_STEPS)
        return fail(ctx, DP_ERR_INVALID, w + ": n_steps " + std::to_string(p.n_steps) + " outside 1.." + std::to_string(DP_LM_MAX_STEPS));
    const auto fin = [](float x) { return std::fabs(x) <= 3.0e38f; };
    if (!(p.lambda_rot >= 0.f && fin(p.lambda_rot)) || !(p.lambda_tmp >= 0.f && fin(p.lambda_tmp)))
        return fail(ctx, DP_ERR_INVALID, w + ": lambda_rot or lambda_tmp is negative or not finite");
    const float rest[7] = {p.mu0, p.mu_up, p.mu_down, p.mu_min, p.mu_max, p.stop_eps_pos, p.stop_eps_rot};
    for (float x : rest)
        if (!fin(x)) return fail(ctx, DP_ERR_INVALID, w + ": mu0, mu_up, mu_down, mu_min, mu_max or a stop threshold is not finite");
    if (!(p.mu_down > 0.f && p.mu_down < 1.f)) return fail(ctx, DP_ERR_INVALID, w + ": mu_down must lie in (0, 1)");
    if (!(p.mu_up > 1.f)) return fail(ctx, DP_ERR_INVALID, w + ": mu_up must be greater than 1");
    if (!(p.mu_min > 0.f) || p.mu_min > p.mu_max) return fail(ctx, DP_ERR_INVALID, w + ": need 0 < mu_min <= mu_max");
    if (p.mu0 < p.mu_min || p.mu0 > p.mu_max) return fail(ctx, DP_ERR_INVALID, w + ": mu0 outside [mu_min, mu_max]");
    a.n_steps = p.n_steps; a.early_stop = p.early_stop ? 1 : 0;
    a.lam_rot = p.lambda_rot; a.lam_tmp = p.lambda_tmp;
    a.mu0 = p.mu0; a.mu_up = p.mu_up; a.mu_down = p.mu_down; a.mu_min = p.mu_min; a.mu_max = p.mu_max;
    a.stop_eps_pos = p.stop_eps_pos; a.stop_eps_rot = p.stop_eps_rot;
    return DP_OK;
}
static int take_lm(dp_ctx* ctx, const dp_lm_params* p_in, const dp_lm_extra* e_in, dplm::Args& a, const char* who)
{
    dp_lm_extra e;
    std::memset(&e, 0, sizeof(e));
    if (e_in)
        if (int rc = take_sized(ctx, e_in, e, LM_EXTRA_V590, who)) return rc;
    if (int rc = take_lm_params(ctx, p_in, a, who)) return rc;
    a.mu = e.mu; a.n_accepted = e.n_accepted; a.loss0 = e.loss0;
    return DP_OK;
}

// (A: dplm::Args or what a unit derives from it; own(a): that unit's refusals and fields, behind dp_optimize_lm's own; unit: its file, for the message)
template <class A, class Own>
static int lm_impl(dp_ctx* ctx, const dp_batch* in, const dp_lm_params* p_in, const dp_result* out_in, const dp_lm_extra* e_in, void* stream,
                   const char* who, const Own& own, hipError_t (*launch)(const A*, hipStream_t), const char* unit)
{
    return entry(ctx, who, [&] {
        if (!in || !p_in) return fail(ctx, DP_ERR_INVALID, std::string(who) + ": NULL batch or params");
        if (int rc = check_lm_params_size(ctx, p_in, who)) return rc;
        dp_result out;
        if (int rc = take_result(ctx, out_in, out, who)) return rc;
        A a;
        std::memset(&a, 0, sizeof(a));
        if (int rc = take_lm(ctx, p_in, e_in, a, who)) return rc;
        if (int rc = check_batch(ctx, in, who)) return rc;
        if (int rc = own(a)) return rc;
        if (REF8_BUILD) return refuse_ref8(ctx, who);
        if (!launch) return fail(ctx, DP_ERR_UNSUPPORTED, std::string(who) + ": this library was linked without " + unit);
        if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
        DEVICE_GUARD(ctx);
        a.img = ctx->d_vjpimg.get();
        fill_batch(a, *in);
        fill_results(a, out);
        const hipError_t e = launch(&a, (hipStream_t)stream);
        if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string(who) + ": kernel launch: " + hipGetErrorString(e));
        return (int)DP_OK;
    });
}
extern "C" int dp_optimize_lm(dp_ctx* ctx, const dp_batch* in, const dp_lm_params* p_in, const dp_result* out_in, const dp_lm_extra* e_in, void* stream)
{
    return lm_impl<dplm::Args>(ctx, in, p_in, out_in, e_in, stream, "dp_optimize_lm", [](dplm::Args&) { return (int)DP_OK; }, dp_launch_lm, "dp_lm.hip");
}

// include/dragposer_clip_skeleton.h: dp_optimize_lm with the bones of each frame's own skeleton -- dp_optimize_lm's refusals, all of them, then
// dp_skeleton_in's.  (Its launcher is a weak reference, like dp_launch_lm.)
hipError_t dp_launch_lm_skel(const dplm::SkelArgs* args, hipStream_t stream) __attribute__((weak));
extern "C" int dp_optimize_lm_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_lm_params* p_in, const dp_skeleton_in* skel, const dp_result* out_in,
                                       const dp_lm_extra* e_in, void* stream)
{
    const char* who = "dp_optimize_lm_skeleton";
    const auto own = [&](dplm::SkelArgs& a) -> int {
        if (!skel) return refuse_null_skeleton(ctx, who);
        return take_skeleton(ctx, skel, a.skel, a.skel_stride, who);
    };
    return lm_impl<dplm::SkelArgs>(ctx, in, p_in, out_in, e_in, stream, who, own, dp_launch_lm_skel, "dp_lm_skel.hip");
}

// include/dragposer_lm_terms.h: dp_optimize_lm with a term table in its loss, in the header's order of refusals -- dp_optimize_lm's up to and
// including dp_lm_extra, what take_terms refuses, the LM parameters' values, the batch.  (Its launcher is a weak reference, like dp_launch_lm.)
hipError_t dp_launch_lm_terms(const dplm::TermArgs* args, hipStream_t stream) __attribute__((weak));
extern "C" int dp_optimize_lm_terms(dp_ctx* ctx, const dp_batch* in, const dp_lm_params* p_in, const dp_terms* t_in, const dp_result* out_in,
                                    const dp_lm_extra* e_in, void* stream)
{
    const char* who = "dp_optimize_lm_terms";
    return entry(ctx, who, [&] {
        if (!in || !p_in || !t_in) return fail(ctx, DP_ERR_INVALID, "dp_optimize_lm_terms: NULL batch, params or terms");
        if (int rc = check_lm_params_size(ctx, p_in, who)) return rc;
        dp_result out;
        if (int rc = take_result(ctx, out_in, out, who)) return rc;
        dp_lm_extra e;
        std::memset(&e, 0, sizeof(e));
        if (e_in)
            if (int rc = take_sized(ctx, e_in, e, LM_EXTRA_V590, who)) return rc;
        dplm::TermArgs a;
        std::memset(&a, 0, sizeof(a));
        if (int rc = take_terms(ctx, t_in, a, who)) return rc;
        if (int rc = take_lm_params(ctx, p_in, a, who)) return rc;
        a.mu = e.mu; a.n_accepted = e.n_accepted; a.loss0 = e.loss0;
        if (int rc = check_batch(ctx, in, who)) return rc;
        if (REF8_BUILD) return refuse_ref8(ctx, who);
        if (!dp_launch_lm_terms) return fail(ctx, DP_ERR_UNSUPPORTED, std::string(who) + ": this library was linked without dp_lm_terms.hip");
        if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
        DEVICE_GUARD(ctx);
        a.img = ctx->d_vjpimg.get();
        fill_batch(a, *in);
        fill_results(a, out);
        const hipError_t err = dp_launch_lm_terms(&a, (hipStream_t)stream);
        if (err != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string(who) + ": kernel launch: " + hipGetErrorString(err));
        return (int)DP_OK;
    });
}

// include/dragposer_calibration.h: dp_fit_bones, in the header's order of refusals.  Everything the HOST arrays hold goes into the kernels'
// argument block here, so the call copies nothing to the device.  (Its launcher is a weak reference, like dp_launch_lm.)
hipError_t dp_launch_fit(const dpfit::Args* args, hipStream_t stream) __attribute__((weak));
static_assert(DP_FIT_MAX_GROUPS == dpfit::MAXK, "dp_fit.h's matrix holds DP_FIT_MAX_GROUPS scales");
extern "C" size_t dp_fit_bones_workspace_bytes(int n_frames)
{
    return n_frames > 0 ? (size_t)dpfit::parts_of(n_frames) * dpfit::PART_FLOATS * sizeof(float) : 0;
}
extern "C" int dp_fit_bones(dp_ctx* ctx, const dp_batch* in, const dp_bone_fit* f_in, const dp_bone_fit_result* r_in, void* stream)
{
    const char* who = "dp_fit_bones";
    return entry(ctx, who, [&] {
        const std::string w = who;
        if (!in || !f_in || !r_in) return fail(ctx, DP_ERR_INVALID, w + ": NULL batch, fit or result");
        dp_bone_fit ft;
        if (int rc = take_sized(ctx, f_in, ft, BONE_FIT_V510, who)) return rc;
        dp_bone_fit_result out;
        if (int rc = take_sized(ctx, r_in, out, BONE_FIT_RESULT_V510, who)) return rc;
        if (!out.scales) return fail(ctx, DP_ERR_INVALID, w + ": dp_bone_fit_result.scales is NULL");
        const int K = ft.n_groups;
        if (K < 1 || K > DP_FIT_MAX_GROUPS) return fail(ctx, DP_ERR_INVALID, w + ": n_groups " + std::to_string(K) + " outside 1.." + std::to_string(DP_FIT_MAX_GROUPS));
        if (!ft.groups) return fail(ctx, DP_ERR_INVALID, w + ": dp_bone_fit.groups is NULL");
        dpfit::Args a;
        std::memset(&a, 0, sizeof(a));
        bool owns[DP_FIT_MAX_GROUPS] = {};
        a.grp[0] = -1;
        for (int j = 1; j < NJ; ++j) {
            const int g = ft.groups[j];
            if (g < -1 || g >= K)
                return fail(ctx, DP_ERR_INVALID, w + ": groups[" + std::to_string(j) + "] is " + std::to_string(g) + ", outside -1.." + std::to_string(K - 1));
            if (g >= 0) owns[g] = true;
            a.grp[j] = g;
        }
        for (int g = 0; g < K; ++g)
            if (!owns[g]) return fail(ctx, DP_ERR_INVALID, w + ": group " + std::to_string(g) + " owns no bone");
        const auto fin = [](float x) { return std::fabs(x) <= 3.0e38f; };
        if (ft.base)
            for (int i = 0; i < 3 * NJ; ++i) {
                if (!fin(ft.base[i])) return fail(ctx, DP_ERR_INVALID, w + ": base holds a value that is not finite");
                a.base[i] = ft.base[i];
            }
        for (int g = 0; g < K; ++g) {
            a.prior[g] = ft.prior ? ft.prior[g] : 1.f;
            if (!fin(a.prior[g])) return fail(ctx, DP_ERR_INVALID, w + ": prior holds a value that is not finite");
        }
        if (!(ft.ridge >= 0.f && fin(ft.ridge))) return fail(ctx, DP_ERR_INVALID, w + ": ridge is negative or not finite");
        const size_t need = dp_fit_bones_workspace_bytes(in->n_frames);
        if (!ft.workspace || ft.workspace_bytes < need)
            return fail(ctx, DP_ERR_INVALID, w + ": the workspace is NULL or holds " + std::to_string(ft.workspace_bytes) + " bytes, fewer than the " +
                                                 std::to_string(need) + " of dp_fit_bones_workspace_bytes(" + std::to_string(in->n_frames) + ")");
        if (in->n_frames <= 0) return fail(ctx, DP_ERR_INVALID, w + ": n_frames must be positive");
        if (!in->z0 || !in->cur_rot || !in->tgt_pos || !in->w || !in->tracked) return fail(ctx, DP_ERR_INVALID, w + ": NULL input array");
        if (REF8_BUILD) return refuse_ref8(ctx, who);
        if (!dp_launch_fit) return fail(ctx, DP_ERR_UNSUPPORTED, w + ": this library was linked without dp_fit.hip");
        if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
        DEVICE_GUARD(ctx);
        a.img = ctx->d_vjpimg.get();
        a.z0 = in->z0; a.cur_rot = in->cur_rot; a.tgt_pos = in->tgt_pos; a.w = in->w; a.tracked = in->tracked;
        a.n_frames = in->n_frames; a.n_parts = dpfit::parts_of(in->n_frames);
        a.K = K; a.has_base = ft.base ? 1 : 0; a.ridge = ft.ridge;
        a.workspace = (float*)ft.workspace;
        a.scales = out.scales; a.offsets = out.offsets; a.normal = out.normal; a.rms = out.rms; a.info = out.info; a.status = out.status;
        const hipError_t e = dp_launch_fit(&a, (hipStream_t)stream);
        if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, w + ": kernel launch: " + hipGetErrorString(e));
        return (int)DP_OK;
    });
}

// include/dragposer_clip_lm.h, dragposer_clip_accel.h, dragposer_clip_skeleton.h: dp_optimize_clip_lm, dp_optimize_clip_lm_accel (the same call
// with one more struct, a wider workspace and its own chain and decision) and dp_optimize_clip_lm_skeleton (either, with the bones of each
// sequence's own skeleton in the rows pass) are one path, clip_impl, in the headers' order of refusals: take_clip; take_clip_accel where the
// call has the struct; the skeleton's; the workspace; the test-only library; the missing unit; the missing image.  dp_clip_lm_params has
// dp_lm_params' fields without the early stop and lambda_smooth among them: its values pass through take_lm_params as a dp_lm_params, so the
// calls refuse as dp_optimize_lm does.  (The launchers are weak references, like dp_launch_lm.)
hipError_t dp_launch_clip(const dpclip::Args* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_clip_accel(const dpclipacc::Args* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_clip_train(const dpclip::Args* args, const dpclip::Rows* rows, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_clip_accel_train(const dpclipacc::Args* args, const dpclip::Rows* rows, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_clip_rows_skel(const dpclip::Args* args, int mode, const void* own, hipStream_t stream) __attribute__((weak));
struct ClipCall {
    dp_result out;
    dp_clip_lm_extra e;
    dp_clip_lm_params p;
    dplm::Args la;
};
static int take_clip(dp_ctx* ctx, const dp_batch* in, int n_seq, const dp_clip_lm_params* p_in, const dp_result* out_in, const dp_clip_lm_extra* e_in,
                     ClipCall& c, const char* who)
{
    const std::string w = who;
    if (!in || !p_in || !e_in) return fail(ctx, DP_ERR_INVALID, w + ": NULL batch, params or extra");
    constexpr unsigned min_size = (unsigned)(offsetof(dp_clip_lm_params, mu_max) + sizeof(float));
    if (p_in->struct_size < min_size || p_in->struct_size > 4096u)
        return fail(ctx, DP_ERR_INVALID, w + ": dp_clip_lm_params.struct_size is " + std::to_string(p_in->struct_size) + ", this library expects at least " +
                                             std::to_string(min_size) + "  (dp_clip_lm_params p = DP_CLIP_LM_PARAMS_INIT;)");
    if (int rc = take_result(ctx, out_in, c.out, who)) return rc;
    if (int rc = take_sized(ctx, e_in, c.e, CLIP_LM_EXTRA_V510, who)) return rc;
    copy_sized(p_in, c.p);
    dp_lm_params lp = DP_LM_PARAMS_INIT;
    lp.n_steps = c.p.n_steps; lp.lambda_rot = c.p.lambda_rot; lp.lambda_tmp = c.p.lambda_tmp;
    lp.mu0 = c.p.mu0; lp.mu_up = c.p.mu_up; lp.mu_down = c.p.mu_down; lp.mu_min = c.p.mu_min; lp.mu_max = c.p.mu_max;
    std::memset(&c.la, 0, sizeof(c.la));
    if (int rc = take_lm_params(ctx, &lp, c.la, who)) return rc;
    if (int rc = check_batch(ctx, in, who)) return rc;
    if (n_seq <= 0 || in->n_frames % n_seq != 0)
        return fail(ctx, DP_ERR_INVALID, w + ": n_sequences " + std::to_string(n_seq) + " must be positive and divide n_frames " + std::to_string(in->n_frames));
    if (!(c.p.lambda_smooth >= 0.f && std::fabs(c.p.lambda_smooth) <= 3.0e38f)) return fail(ctx, DP_ERR_INVALID, w + ": lambda_smooth is negative or not finite");
    return DP_OK;
}
// dp_clip_accel_params as the caller compiled it: NULL or a bad size word, then lambda_accel
static int take_clip_accel(dp_ctx* ctx, const dp_clip_accel_params* a_in, dp_clip_accel_params& ap, const char* who)
{
    const std::string w = who;
    constexpr unsigned min_size = (unsigned)(offsetof(dp_clip_accel_params, accel_loss) + sizeof(double*));
    if (!a_in || a_in->struct_size < min_size || a_in->struct_size > 4096u)
        return fail(ctx, DP_ERR_INVALID, w + (a_in ? ": dp_clip_accel_params.struct_size is " + std::to_string(a_in->struct_size) : ": dp_clip_accel_params is NULL") +
                                             ", this library expects at least " + std::to_string(min_size) + "  (dp_clip_accel_params a = DP_CLIP_ACCEL_PARAMS_INIT;)");
    copy_sized(a_in, ap);
    if (!(ap.lambda_accel >= 0.f && std::fabs(ap.lambda_accel) <= 3.0e38f)) return fail(ctx, DP_ERR_INVALID, w + ": lambda_accel is negative or not finite");
    return DP_OK;
}
// the workspace of either problem (dp_clip.h's one list): with the acceleration term the factor block is wider and `acc` exists
static dpclip::Layout clip_layout(int n_seq, int n_frames, bool accel)
{
    return accel ? dpclip::layout(n_seq, n_frames, dpclipacc::LF_FLOATS, true) : dpclip::layout(n_seq, n_frames);
}
static size_t clip_workspace_bytes(int n_sequences, int n_frames, bool accel)
{
    if (n_sequences <= 0 || n_frames <= 0 || n_frames % n_sequences != 0) return 0;
    return clip_layout(n_sequences, n_frames, accel).bytes;
}
extern "C" size_t dp_clip_lm_workspace_bytes(int n_sequences, int n_frames) { return clip_workspace_bytes(n_sequences, n_frames, false); }
extern "C" size_t dp_clip_lm_accel_workspace_bytes(int n_sequences, int n_frames) { return clip_workspace_bytes(n_sequences, n_frames, true); }
static void fill_clip(dpclip::Args& a, const dp_ctx* ctx, const dp_batch* in, int n_seq, const ClipCall& c, const dpclip::Layout& l)
{
    std::memset(&a, 0, sizeof(a));
    a.img = ctx->d_vjpimg.get();
    fill_batch(a, *in);
    fill_results(a, c.out);
    const dp_clip_lm_extra& e = c.e;
    a.mu = e.mu; a.n_accepted = e.n_accepted; a.clip_loss = e.clip_loss; a.loss_hist = e.loss_hist; a.info = e.info;
    char* const ws = (char*)e.workspace;
    for (int i = 0; i < 2; ++i) {
        a.wz[i] = (float*)(ws + l.z[i]); a.wloss[i] = (float*)(ws + l.loss[i]); a.wcpl[i] = (double*)(ws + l.cpl[i]);
    }
    a.wag = (float*)(ws + l.ag); a.wli = (float*)(ws + l.li); a.wflags = (int*)(ws + l.flags); a.wtot = (double*)(ws + l.tot);
    a.wword = (int*)(ws + l.word); a.wsolved = (int*)(ws + l.solved); a.wmu = (float*)(ws + l.mu); a.wnacc = (int*)(ws + l.nacc);
    a.n_seq = n_seq; a.n_t = in->n_frames / n_seq; a.n_steps = c.la.n_steps;
    a.lam_rot = c.la.lam_rot; a.lam_tmp = c.la.lam_tmp; a.lam_smooth = c.p.lambda_smooth;
    a.mu0 = c.la.mu0; a.mu_up = c.la.mu_up; a.mu_down = c.la.mu_down; a.mu_min = c.la.mu_min; a.mu_max = c.la.mu_max;
}
// accel: the call has a dp_clip_accel_params and solves its problem on its workspace (a_in NULL is then take_clip_accel's refusal).
// skeleton: the call has a dp_skeleton_in, and the launch trains run with dp_clip_skel.hip's rows kernel as their rows pass.
static int clip_impl(dp_ctx* ctx, const char* who, const dp_batch* in, int n_seq, const dp_clip_lm_params* p_in, bool accel, const dp_clip_accel_params* a_in,
                     bool skeleton, const dp_skeleton_in* skel, const dp_result* out_in, const dp_clip_lm_extra* e_in, void* stream)
{
    return entry(ctx, who, [&] {
        const std::string w = who;
        ClipCall c;
        if (int rc = take_clip(ctx, in, n_seq, p_in, out_in, e_in, c, who)) return rc;
        dp_clip_accel_params ap = DP_CLIP_ACCEL_PARAMS_INIT;
        if (accel)
            if (int rc = take_clip_accel(ctx, a_in, ap, who)) return rc;
        dpclip::SkelOwn own;
        if (skeleton) {
            if (!skel) return refuse_null_skeleton(ctx, who);
            if (int rc = take_skeleton(ctx, skel, own.skel, own.skel_stride, who)) return rc;
        }
        const dpclip::Layout l = clip_layout(n_seq, in->n_frames, accel);
        if (!c.e.workspace || c.e.workspace_bytes < l.bytes)
            return fail(ctx, DP_ERR_INVALID, w + ": the workspace is NULL or holds " + std::to_string(c.e.workspace_bytes) + " bytes, fewer than the " +
                                                 std::to_string(l.bytes) + " of " + (accel ? "dp_clip_lm_accel_workspace_bytes" : "dp_clip_lm_workspace_bytes") + "(" +
                                                 std::to_string(n_seq) + ", " + std::to_string(in->n_frames) + ")");
        if (REF8_BUILD) return refuse_ref8(ctx, who);
        if (skeleton ? !dp_launch_clip_rows_skel || !dp_launch_clip_train || !dp_launch_clip_accel_train : accel ? !dp_launch_clip_accel : !dp_launch_clip)
            return fail(ctx, DP_ERR_UNSUPPORTED, w + ": this library was linked without " +
                                                     (skeleton ? "dp_clip_skel.hip, dp_clip.hip or dp_clip_accel.hip" : accel ? "dp_clip_accel.hip" : "dp_clip.hip"));
        if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
        DEVICE_GUARD(ctx);
        dpclipacc::Args a; // (without the acceleration term only its dp_clip.h part is filled and launched)
        fill_clip(a.c, ctx, in, n_seq, c, l);
        if (accel) {
            a.lam_accel = ap.lambda_accel;
            a.accel_loss = ap.accel_loss;
            a.wacc = (double*)((char*)c.e.workspace + l.acc);
        }
        const dpclip::Rows rows = {dp_launch_clip_rows_skel, &own};
        const hipStream_t s = (hipStream_t)stream;
        const hipError_t err = skeleton ? (accel ? dp_launch_clip_accel_train(&a, &rows, s) : dp_launch_clip_train(&a.c, &rows, s))
                                        : (accel ? dp_launch_clip_accel(&a, s) : dp_launch_clip(&a.c, s));
        if (err != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, w + ": kernel launch: " + hipGetErrorString(err));
        return (int)DP_OK;
    });
}
extern "C" int dp_optimize_clip_lm(dp_ctx* ctx, const dp_batch* in, int n_seq, const dp_clip_lm_params* p_in, const dp_result* out_in,
                                   const dp_clip_lm_extra* e_in, void* stream)
{
    return clip_impl(ctx, "dp_optimize_clip_lm", in, n_seq, p_in, false, nullptr, false, nullptr, out_in, e_in, stream);
}
extern "C" int dp_optimize_clip_lm_accel(dp_ctx* ctx, const dp_batch* in, int n_seq, const dp_clip_lm_params* p_in, const dp_clip_accel_params* a_in,
                                         const dp_result* out_in, const dp_clip_lm_extra* e_in, void* stream)
{
    return clip_impl(ctx, "dp_optimize_clip_lm_accel", in, n_seq, p_in, true, a_in, false, nullptr, out_in, e_in, stream);
}
// (a_in NULL: dp_optimize_clip_lm's problem and workspace)
extern "C" int dp_optimize_clip_lm_skeleton(dp_ctx* ctx, const dp_batch* in, int n_seq, const dp_clip_lm_params* p_in, const dp_clip_accel_params* a_in,
                                            const dp_skeleton_in* skel, const dp_result* out_in, const dp_clip_lm_extra* e_in, void* stream)
{
    return clip_impl(ctx, "dp_optimize_clip_lm_skeleton", in, n_seq, p_in, a_in != nullptr, a_in, true, skel, out_in, e_in, stream);
}

// ------------------------------------------------------------------------------------------------
// What every whole-sequence launch asks of its frames, state, scratch and joint adjustment (who names the caller in the messages)
// (own_z_tgt: the launch forms its targets itself, include/dragposer_latent_ar.h, and frames->z_tgt is its own check's business)
static int check_sequence(dp_ctx* ctx, const dp_seq_frames* fr, const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results& out, const std::string& who,
                          bool own_z_tgt = false)
{
    if (fr->n_steps <= 0 || !fr->tgt_pos || !fr->tgt_rot || !fr->w || !fr->tracked || (!own_z_tgt && !fr->z_tgt))
        return fail(ctx, DP_ERR_INVALID, who + ": NULL input array / n_steps must be positive");
    if (!st->global_pos || !st->global_rot || !st->latent_buf || !st->disp_buf || !st->heights_buf || !out.hist_scratch)
        return fail(ctx, DP_ERR_INVALID, who + ": NULL state array / hist_scratch");
    if (st->history < 1 || st->n_heights < 0 || st->n_heights > DP_MAX_HEIGHT_JOINTS)
        return fail(ctx, DP_ERR_INVALID, who + ": history / n_heights out of range");
    for (int h = 0; h < st->n_heights; ++h)
        if (st->height_joints[h] < 0 || st->height_joints[h] >= NJ) return fail(ctx, DP_ERR_INVALID, who + ": bad height joint");
    if (adj && (adj->adjust_joint >= NJ || (adj->adjust_joint >= 0 && (adj->adjust_target_joint < 0 || adj->adjust_target_joint >= NJ))))
        return fail(ctx, DP_ERR_INVALID, who + ": bad joint adjustment");
    return DP_OK;
}

// ... the step loop's part of the argument block (Q: dp_kernel.h's SeqK, dp_cons_seq.h's SeqFields -- the same field names)
template <class Q>
static void fill_sequence(Q& q, const dp_ctx* ctx, const dp_seq_frames* fr, const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results& out)
{
    q.n_steps = fr->n_steps; q.z_tgt_step = fr->z_tgt_step; q.z_tgt_seq = fr->z_tgt_seq; q.tgt_root = fr->tgt_root;
    q.global_pos = st->global_pos; q.global_rot = st->global_rot; q.hist = out.hist_scratch; q.pos_ret = out.pos_ret;
    q.n_heights = st->n_heights;
    for (int h = 0; h < st->n_heights; ++h) q.height_joints[h] = st->height_joints[h];
    q.adjust_joint = adj ? adj->adjust_joint : -1;
    q.adjust_target_joint = adj ? adj->adjust_target_joint : -1;
    q.adjust_weight = adj ? adj->adjust_weight : 0.f;
    for (int c = 0; c < 4; ++c) { q.mean_q0[c] = ctx->mean_q0[c]; q.std_q0[c] = ctx->std_q0[c]; }
}

// ... and its second launch: the steps' rows appended to the three history buffers
static int append_history(dp_ctx* ctx, int n_seq, const dp_seq_frames* fr, const dp_seq_state* st, const dp_seq_results& out, void* stream)
{
    DEVICE_GUARD(ctx);
    HistArgs h;
    h.n_seq = n_seq; h.n_steps = fr->n_steps; h.history = st->history; h.n_heights = st->n_heights;
    h.scratch = out.hist_scratch; h.latent_buf = st->latent_buf; h.disp_buf = st->disp_buf; h.heights_buf = st->heights_buf;
    hipError_t e = dp_launch_sequence_history(&h, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string("history launch: ") + hipGetErrorString(e));
    return DP_OK;
}

// n_steps frames of S sequences in one launch (+ one for the history buffers), see include/dragposer.h
static int sequence_impl(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_skeleton_in* sk,
                         const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out_in, void* stream)
{
    const char* who = "dp_optimize_sequence"; // (in every message but the skeleton's own)
    if (REF8_BUILD) return refuse_ref8(ctx, who);
    if (n_seq <= 0 || !latent || !fr || !p_in || !st || !out_in) return fail(ctx, DP_ERR_INVALID, "dp_optimize_sequence: bad arguments");
    dp_params p;
    if (int rc = take_params(ctx, p_in, p, who)) return rc;
    dp_seq_results out;
    if (int rc = take_sized(ctx, out_in, out, SEQ_RESULTS_V500, who)) return rc;
    if (int rc = check_sequence(ctx, fr, st, adj, out, who)) return rc;
    if (int rc = check_adam(ctx, p, who)) return rc;
    const float* sk_off = nullptr;
    int sk_stride = 0;
    if (sk) {
        who = "dp_optimize_sequence_skeleton";
        if (int rc = take_skeleton(ctx, sk, sk_off, sk_stride, who)) return rc;
        if (p.kernel == DP_KERNEL_W16) return refuse_w16_skeleton(ctx, who);
    }
    if (!ctx->d_w4img.get()) return refuse_no_image(ctx, who);
    KArgs k;
    fill_model_args(ctx, k);
    k.skel = sk_off; k.skel_stride = sk_stride;
    k.z0 = latent; k.z_tgt = fr->z_tgt; k.cur_rot = st->global_rot; k.tgt_pos = fr->tgt_pos; k.tgt_rot = fr->tgt_rot; k.w = fr->w; k.tracked = fr->tracked;
    k.z = latent; k.pose = out.pose_ret; k.world_rot = out.world_rot; k.iters = out.iters; k.loss = out.loss; k.status = out.status;
    k.n_frames = n_seq; k.mode = 0;
    fill_loop(k, p, true);
    fill_adam(k, p);
    fill_sequence(k.seq, ctx, fr, st, adj, out);
    int rc = launch(ctx, k, stream, DP_KERNEL_W4, sk != nullptr);
    if (rc != DP_OK) return rc;
    return append_history(ctx, n_seq, fr, st, out, stream);
}

extern "C" int dp_optimize_sequence(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_seq_state* st,
                                    const dp_seq_step* adj, const dp_seq_results* out, void* stream)
{
    return entry_quiet(ctx, "dp_optimize_sequence", [&] { return sequence_impl(ctx, n_seq, latent, fr, p_in, nullptr, st, adj, out, stream); });
}

// ------------------------------------------------------------------------------------------------
// include/dragposer_skeleton.h: the three calls above with per-frame (per-sequence) bone offsets, on the dp_w4sk units
extern "C" int dp_optimize_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* p, const dp_skeleton_in* skel, const dp_result* out, void* stream)
{
    const char* who = "dp_optimize_skeleton";
    return entry(ctx, who, [&] {
        if (!skel) return refuse_null_skeleton(ctx, who);
        return optimize_impl(ctx, in, p, out, nullptr, stream, skel, who);
    });
}

extern "C" int dp_forward_skeleton(dp_ctx* ctx, int n_frames, const float* z, const float* cur_rot, const dp_skeleton_in* skel, const dp_result* out,
                                   void* stream)
{
    const char* who = "dp_forward_skeleton";
    return entry(ctx, who, [&] {
        if (!skel) return refuse_null_skeleton(ctx, who);
        return forward_impl(ctx, n_frames, z, cur_rot, skel, out, stream, who);
    });
}

extern "C" int dp_optimize_sequence_skeleton(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p, const dp_skeleton_in* skel,
                                             const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out, void* stream)
{
    const char* who = "dp_optimize_sequence_skeleton";
    return entry(ctx, who, [&] {
        if (!skel) return refuse_null_skeleton(ctx, who);
        return sequence_impl(ctx, n_seq, latent, fr, p, skel, st, adj, out, stream);
    });
}

// ------------------------------------------------------------------------------------------------
// include/dragposer_sequence_constraints.h: dp_optimize_sequence_constrained (A = dpcons::SeqConsArgs) and dp_optimize_sequence_terms
// (dpcons::SeqTermArgs), whose callers have refused a NULL argument -- constrained_impl's order of refusals with sequence_impl's frames and
// state in the batch's place: params, results, own(a) (dp_constraints / dp_terms, then dp_seq_extra), the skeleton (NULL: the context's own
// bones, one for the launch), frames / state, Adam.
static int take_seq_extra(dp_ctx* ctx, const dp_seq_extra* e_in, dp_seq_extra& e, const char* who)
{
    std::memset(&e, 0, sizeof(e)); // (NULL: no per-step output of the terms, every per_frame array one row per sequence)
    if (!e_in) return DP_OK;
    if (int rc = take_sized(ctx, e_in, e, SEQ_EXTRA_V520, who)) return rc;
    for (int k = 0; k < DP_MAX_TERMS; ++k)
        if (e.row_step[k] < 0) return fail(ctx, DP_ERR_INVALID, std::string(who) + ": dp_seq_extra.row_step[" + std::to_string(k) + "] is negative");
    return DP_OK;
}

// The sequence units are units a link of the host code may leave out (a host-only program without the kernel units, the plug-in without
// dp_cons_tether.hip): their launchers are weak references here, and a library without one refuses the call with DP_ERR_UNSUPPORTED, as
// the headers state.
hipError_t dp_launch_cons_seq(const dpcons::SeqConsArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_seq(const dpcons::SeqTermArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_hold_seq(const dpcons::HoldSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_ar_seq(const dpcons::ArSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_gap_seq(const dpcons::GapSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_gap_ar_seq(const dpcons::GapArSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_live(const dpcons::LiveSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_live_ar(const dpcons::LiveArSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_tether_seq(const dpcons::TetherSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_tether_ar_seq(const dpcons::TetherArSeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_points(const dpcons::PointTermArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_points_skel(const dpcons::PointTermSkelArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_terms_points_seq(const dpcons::PointSeqTermArgs* args, hipStream_t stream) __attribute__((weak));

// One description per argument block of sequence_constrained_impl -- a new variant is a row here and its entry point.  Which optional parts a
// block has (a.h, a.r, a.g, a.t, a.l) is read off the block itself (has_h .. has_l below).
template <class A>
struct SeqVariant {
    hipError_t (*launch)(const A*, hipStream_t); // NULL: the link left the unit out
    const char* unit;                            // ... and the refusal names it
    bool appends_history;                        // the kernel appends the step's row itself: no second launch
};
template <class A> static SeqVariant<A> seq_variant();
template <> SeqVariant<dpcons::SeqConsArgs> seq_variant() { return {dp_launch_cons_seq, "dp_cons_seq.hip", false}; }
template <> SeqVariant<dpcons::SeqTermArgs> seq_variant() { return {dp_launch_terms_seq, "dp_cons_seq.hip", false}; }
template <> SeqVariant<dpcons::HoldSeqArgs> seq_variant() { return {dp_launch_terms_hold_seq, "dp_cons_hold.hip", false}; }
template <> SeqVariant<dpcons::ArSeqArgs> seq_variant() { return {dp_launch_terms_ar_seq, "dp_cons_ar.hip", false}; }
template <> SeqVariant<dpcons::GapSeqArgs> seq_variant() { return {dp_launch_terms_gap_seq, "dp_cons_gap.hip", false}; }
template <> SeqVariant<dpcons::GapArSeqArgs> seq_variant() { return {dp_launch_terms_gap_ar_seq, "dp_cons_gap.hip", false}; }
template <> SeqVariant<dpcons::LiveSeqArgs> seq_variant() { return {dp_launch_live, "dp_cons_live.hip", true}; }
template <> SeqVariant<dpcons::LiveArSeqArgs> seq_variant() { return {dp_launch_live_ar, "dp_cons_live.hip", true}; }
template <> SeqVariant<dpcons::TetherSeqArgs> seq_variant() { return {dp_launch_terms_tether_seq, "dp_cons_tether.hip", false}; }
template <> SeqVariant<dpcons::TetherArSeqArgs> seq_variant() { return {dp_launch_terms_tether_ar_seq, "dp_cons_tether.hip", false}; }
template <> SeqVariant<dpcons::PointSeqTermArgs> seq_variant() { return {dp_launch_terms_points_seq, "dp_cons_points.hip", false}; }

#define DP_HAS_MEMBER(m)                                                   \
    template <class A, class = void> struct has_##m : std::false_type {}; \
    template <class A> struct has_##m<A, std::void_t<decltype(&A::m)>> : std::true_type {}
DP_HAS_MEMBER(h); DP_HAS_MEMBER(r); DP_HAS_MEMBER(g); DP_HAS_MEMBER(t); DP_HAS_MEMBER(l); // HoldFields, ArFields, GapFields, TetherFields, LiveFields
DP_HAS_MEMBER(pt);                                                                        // PointFields
#undef DP_HAS_MEMBER

// What a call with a term table brought beyond its frames and state, NULL where it has none (dp_optimize_sequence_constrained: all of it)
struct SeqParts {
    const dp_terms* terms = nullptr;
    const dp_holds* holds = nullptr;
    const dp_latent_ar* ar = nullptr;
    const dp_gaps* gaps = nullptr;
    const dp_tethers* tethers = nullptr;
    const dp_points* points = nullptr;
};

// include/dragposer_latent_ar.h: dp_latent_ar checked, after everything dp_optimize_sequence_holds checks, against the launch's frames and
// state, and written into the argument block
// (R: dp_cons_ar.h's ArFields or dp_lm_seq.h's -- the same field names)
template <class R>
static int take_latent_ar(dp_ctx* ctx, const dp_latent_ar* r_in, const dp_seq_frames* fr, const dp_seq_state* st, R& r, const char* who)
{
    const std::string nm = who;
    dp_latent_ar ar;
    if (int rc = take_sized(ctx, r_in, ar, LATENT_AR_V540, who)) return rc;
    if (ar.order < 1 || ar.order > DP_MAX_AR_ORDER)
        return fail(ctx, DP_ERR_INVALID, nm + ": dp_latent_ar.order " + std::to_string(ar.order) + " outside 1.." + std::to_string(DP_MAX_AR_ORDER));
    if (!ar.coeffs || !ar.bias) return fail(ctx, DP_ERR_INVALID, nm + ": dp_latent_ar.coeffs or bias is NULL");
    if (st->history < ar.order)
        return fail(ctx, DP_ERR_INVALID, nm + ": the state's history of " + std::to_string(st->history) + " rows is shorter than dp_latent_ar.order " +
                                             std::to_string(ar.order));
    if (fr->z_tgt) return fail(ctx, DP_ERR_INVALID, nm + ": frames->z_tgt must be NULL (the predictor is the targets' one source)");
    r.coeffs = ar.coeffs; r.bias = ar.bias; r.trace = ar.trace; r.latent_buf = st->latent_buf; r.order = ar.order; r.history = st->history;
    return DP_OK;
}

// include/dragposer_gaps.h: dp_gaps checked, after everything dp_optimize_sequence_ar checks, and written into the argument block
static int take_gaps(dp_ctx* ctx, const dp_gaps* g_in, dpcons::GapFields& g, const char* who)
{
    const std::string nm = who;
    dp_gaps gs;
    if (int rc = take_sized(ctx, g_in, gs, GAPS_V550, who)) return rc;
    if (gs.max_hold < 0 || gs.max_hold > DP_GAP_MAX_HOLD)
        return fail(ctx, DP_ERR_INVALID, nm + ": dp_gaps.max_hold " + std::to_string(gs.max_hold) + " outside 0.." + std::to_string(DP_GAP_MAX_HOLD));
    if (!(gs.decay > 0.f && gs.decay <= 1.f)) return fail(ctx, DP_ERR_INVALID, nm + ": dp_gaps.decay must be a finite number in (0, 1]");
    if (!gs.state) return fail(ctx, DP_ERR_INVALID, nm + ": dp_gaps.state is NULL");
    g.state = gs.state; g.present = gs.present; g.trace = gs.trace; g.decay = gs.decay; g.max_hold = (float)gs.max_hold;
    return DP_OK;
}

// include/dragposer_points.h: dp_points checked after take_terms has accepted the table t_in (with indices up to 21 + DP_MAX_POINTS), against
// it, and the coefficients written into the argument block (rows beyond n_points stay zero)
static_assert(DP_MAX_POINTS == dpcons::MAX_POINTS && NJ == dpcons::PT_NJ, "dp_cons_points.h's table holds DP_MAX_POINTS rows of a coefficient per joint");
static int take_points(dp_ctx* ctx, const dp_points* q_in, const dp_terms* t_in, dpcons::PointFields& pt, const char* who)
{
    const std::string nm = who;
    dp_points ps;
    if (int rc = take_sized(ctx, q_in, ps, POINTS_V580, who)) return rc;
    if (ps.reserved1 != 0) return fail(ctx, DP_ERR_INVALID, nm + ": dp_points.reserved1 is " + std::to_string(ps.reserved1) + ", must be 0");
    if (ps.n_points < 0 || ps.n_points > DP_MAX_POINTS)
        return fail(ctx, DP_ERR_INVALID, nm + ": dp_points.n_points " + std::to_string(ps.n_points) + " outside 0.." + std::to_string(DP_MAX_POINTS));
    if (ps.n_points > 0 && !ps.coeff) return fail(ctx, DP_ERR_INVALID, nm + ": dp_points.coeff is NULL with n_points > 0");
    for (int k = 0; k < ps.n_points; ++k)
        for (int j = 0; j < NJ; ++j)
            if (!(std::fabs(ps.coeff[k * NJ + j]) <= 3.0e38f))
                return fail(ctx, DP_ERR_INVALID, nm + ": point " + std::to_string(k) + ": the coefficient of joint " + std::to_string(j) + " is not finite");
    for (int k = 0; k < ps.n_points; ++k) {
        double sum = 0.0;
        for (int j = 0; j < NJ; ++j) sum += (double)ps.coeff[k * NJ + j];
        if (!(std::fabs(sum - 1.0) <= 1e-4))
            return fail(ctx, DP_ERR_INVALID, nm + ": point " + std::to_string(k) + ": the coefficients sum to " + std::to_string(sum) + ", not to 1 within 1e-4");
    }
    dp_terms ts;
    copy_sized(t_in, ts);
    for (int k = 0; k < ts.n_terms; ++k) {
        const dp_term& t = ts.terms[k];
        const int hi = std::max(t.joint_a, t.joint_b);
        if (hi >= NJ + ps.n_points)
            return fail(ctx, DP_ERR_INVALID, nm + ": term " + std::to_string(k) + ": index " + std::to_string(hi) + " names a point, and dp_points has " +
                                                 std::to_string(ps.n_points) + " (indices up to " + std::to_string(NJ + ps.n_points - 1) + ")");
    }
    for (int k = 0; k < ts.n_terms; ++k) {
        const dp_term& t = ts.terms[k];
        if (t.type == DP_TERM_ALIGN && std::max(t.joint_a, t.joint_b) >= NJ)
            return fail(ctx, DP_ERR_INVALID, nm + ": term " + std::to_string(k) + ": an ALIGN term names a point, and a point has no rotation");
    }
    pt.n_points = ps.n_points;
    for (int i = 0; i < ps.n_points * NJ; ++i) pt.coeff[i] = ps.coeff[i];
    return DP_OK;
}

// What entry k of a call's holds or tethers (E: dp_hold, dp_tether) may refer to: a point-DISTANCE term of the accepted table without a
// per_frame array, which no earlier entry refers to.  "" or what is wrong with it (noun, verb: "hold", "held" / "tether", "tethered")
template <class E>
static std::string check_term_ref(const dp_terms& ts, const E* entries, int k, const std::string& noun, const char* verb)
{
    const int term = entries[k].term;
    const std::string tn = "term " + std::to_string(term);
    if (term < 0 || term >= ts.n_terms) return tn + " outside the table of " + std::to_string(ts.n_terms);
    const dp_term& t = ts.terms[term];
    if (t.type != DP_TERM_DISTANCE) return tn + " is not a DP_TERM_DISTANCE term";
    if (t.joint_b != -1) return tn + " has a joint_b (a " + noun + " needs a point-DISTANCE term)";
    if (t.per_frame) return tn + " has a per_frame array (the " + noun + "'s state is its row)";
    for (int g = 0; g < k; ++g)
        if (entries[g].term == term) return tn + " is already " + verb + " by " + noun + " " + std::to_string(g);
    return "";
}

// include/dragposer_holds.h: dp_holds checked after take_terms has accepted the table t_in, against it; each hold's level and thresholds go
// into its term's staged axis_a words (a point-DISTANCE term never reads them) and the hold-to-term map is filled (dp_cons_hold.h).
static int take_holds(dp_ctx* ctx, const dp_holds* h_in, const dp_terms* t_in, dpcons::HoldSeqArgs& a, const char* who)
{
    const std::string nm = who;
    dp_holds hs;
    if (int rc = take_sized(ctx, h_in, hs, HOLDS_V530, who)) return rc;
    dp_terms ts;
    copy_sized(t_in, ts);
    if (hs.n_holds < 0 || hs.n_holds > DP_MAX_HOLDS)
        return fail(ctx, DP_ERR_INVALID, nm + ": dp_holds.n_holds " + std::to_string(hs.n_holds) + " outside 0.." + std::to_string(DP_MAX_HOLDS));
    if (hs.n_holds > 0 && !hs.holds) return fail(ctx, DP_ERR_INVALID, nm + ": dp_holds.holds is NULL with n_holds > 0");
    if (hs.n_holds > 0 && !hs.state) return fail(ctx, DP_ERR_INVALID, nm + ": dp_holds.state is NULL with n_holds > 0");
    a.h.state = hs.state; a.h.trace = hs.trace; a.h.n_holds = hs.n_holds; a.h.terms = 0u;
    for (int h = 0; h < hs.n_holds; ++h) {
        const dp_hold& hd = hs.holds[h];
        const std::string hn = nm + ": hold " + std::to_string(h) + ": ";
        const std::string why = check_term_ref(ts, hs.holds, h, "hold", "held");
        if (!why.empty()) return fail(ctx, DP_ERR_INVALID, hn + why);
        if (!std::isfinite(hd.level) || !std::isfinite(hd.contact_lo) || !std::isfinite(hd.contact_hi))
            return fail(ctx, DP_ERR_INVALID, hn + "non-finite level, contact_lo or contact_hi");
        if (hd.contact_lo > hd.contact_hi) return fail(ctx, DP_ERR_INVALID, hn + "contact_lo is above contact_hi");
        float* wf = (float*)(a.tbl + hd.term * dpcons::TW);
        wf[dpcons::T_HLEVEL] = hd.level; wf[dpcons::T_HLO] = hd.contact_lo; wf[dpcons::T_HHI] = hd.contact_hi;
        a.h.terms |= (unsigned)hd.term << (8 * h);
    }
    return DP_OK;
}

// include/dragposer_tethers.h: dp_tethers checked, after everything dp_optimize_sequence_gaps checks, against the table and the holds the
// call was given (both accepted by then); each tether's alpha goes into its term's first staged axis_a word (a point-DISTANCE term never
// reads it, and no hold has put its level there: a tethered term is not held) and the tether-to-term map is filled (dp_cons_tether.h)
static int take_tethers(dp_ctx* ctx, const SeqParts& in, unsigned* tbl, dpcons::TetherFields& tf, const char* who)
{
    const std::string nm = who;
    dp_tethers ts;
    if (int rc = take_sized(ctx, in.tethers, ts, TETHERS_V570, who)) return rc;
    dp_terms tt;
    copy_sized(in.terms, tt);
    dp_holds hs;
    std::memset(&hs, 0, sizeof(hs));
    if (in.holds) copy_sized(in.holds, hs);
    if (ts.n_tethers < 0 || ts.n_tethers > DP_MAX_TETHERS)
        return fail(ctx, DP_ERR_INVALID, nm + ": dp_tethers.n_tethers " + std::to_string(ts.n_tethers) + " outside 0.." + std::to_string(DP_MAX_TETHERS));
    if (ts.n_tethers > 0 && !ts.tethers) return fail(ctx, DP_ERR_INVALID, nm + ": dp_tethers.tethers is NULL with n_tethers > 0");
    if (ts.n_tethers > 0 && !ts.state) return fail(ctx, DP_ERR_INVALID, nm + ": dp_tethers.state is NULL with n_tethers > 0");
    tf.state = ts.state; tf.trace = ts.trace; tf.n_tethers = ts.n_tethers; tf.terms = 0u;
    for (int k = 0; k < ts.n_tethers; ++k) {
        const dp_tether& te = ts.tethers[k];
        const std::string tn = nm + ": tether " + std::to_string(k) + ": ";
        const std::string why = check_term_ref(tt, ts.tethers, k, "tether", "tethered");
        if (!why.empty()) return fail(ctx, DP_ERR_INVALID, tn + why);
        for (int h = 0; h < hs.n_holds; ++h)
            if (hs.holds[h].term == te.term)
                return fail(ctx, DP_ERR_INVALID, tn + "term " + std::to_string(te.term) + " is held by hold " + std::to_string(h));
        if (!(te.alpha >= 0.f && te.alpha <= 1.f)) return fail(ctx, DP_ERR_INVALID, tn + "alpha must be a finite number in [0, 1]");
        ((float*)(tbl + te.term * dpcons::TW))[dpcons::T_TALPHA] = te.alpha;
        tf.terms |= (unsigned)te.term << (8 * k);
    }
    return DP_OK;
}

// Every whole-sequence launch of dp_cons_body.h's kernels (A: a block with a seq_variant row), whose caller has refused a NULL argument.
// own(a) validates the entry point's own structs and writes them into the zeroed block; the parts a block has beyond them are checked
// after Adam in the order the layers were stacked: dp_latent_ar, dp_gaps, dp_tethers.
template <class A, class Own>
static int sequence_constrained_impl(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_skeleton_in* sk,
                                     const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out_in, void* stream, const char* who, Own own,
                                     const SeqParts& parts)
{
    const SeqVariant<A> v = seq_variant<A>();
    dp_params p;
    if (int rc = take_params(ctx, p_in, p, who)) return rc;
    dp_seq_results out;
    if (int rc = take_sized(ctx, out_in, out, SEQ_RESULTS_V500, who)) return rc;
    A a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = own(a)) return rc;
    if (sk)
        if (int rc = take_skeleton(ctx, sk, a.skel, a.skel_stride, who)) return rc;
    if (int rc = check_sequence(ctx, fr, st, adj, out, who, has_r<A>::value)) return rc;
    if (int rc = check_adam(ctx, p, who)) return rc;
    if constexpr (has_r<A>::value)
        if (int rc = take_latent_ar(ctx, parts.ar, fr, st, a.r, who)) return rc;
    if constexpr (has_g<A>::value)
        if (int rc = take_gaps(ctx, parts.gaps, a.g, who)) return rc;
    if constexpr (has_t<A>::value)
        if (int rc = take_tethers(ctx, parts, a.tbl, a.t, who)) return rc;
    if (REF8_BUILD) return refuse_ref8(ctx, who);
    if (!v.launch) return fail(ctx, DP_ERR_UNSUPPORTED, std::string(who) + ": this library was linked without " + v.unit);
    if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
    a.img = ctx->d_vjpimg.get();
    if (!sk) { a.skel = ctx->d_vjpimg.get() + dpvjp::OFF_BONE; a.skel_stride = 0; } // (the image's bone rows: what the per-frame kernels stage)
    a.z0 = latent; a.z = latent; a.z_tgt = fr->z_tgt; a.cur_rot = st->global_rot; a.tgt_pos = fr->tgt_pos; a.tgt_rot = fr->tgt_rot; a.w = fr->w;
    a.tracked = fr->tracked; a.n_frames = n_seq;
    a.pose = out.pose_ret; a.world_rot = out.world_rot; a.iters = out.iters; a.loss = out.loss; a.status = out.status;
    fill_loop(a, p, true);
    a.beta1d = p.beta1; a.beta2d = p.beta2; a.lrd = p.lr;
    fill_sequence(a.q, ctx, fr, st, adj, out);
    if constexpr (has_l<A>::value) {
        a.l.latent_buf = st->latent_buf; a.l.disp_buf = st->disp_buf; a.l.heights_buf = st->heights_buf; a.l.history = st->history;
    }
    {
        DEVICE_GUARD(ctx);
        const hipError_t e = v.launch(&a, (hipStream_t)stream);
        if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string(who) + ": kernel launch: " + hipGetErrorString(e));
    }
    if (v.appends_history) return DP_OK;
    return append_history(ctx, n_seq, fr, st, out, stream);
}

// ... with a term table (every entry point but dp_optimize_sequence_constrained): own(a) is the table, the holds if the call has any,
// dp_seq_extra, then each term's step between rows (dp_cons_seq.h)
template <class A>
static int sequence_terms_impl(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_skeleton_in* sk,
                               const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out, const dp_seq_extra* extra, void* stream,
                               const char* who, const SeqParts& parts)
{
    const auto own = [&](A& a) -> int {
        if (int rc = take_terms(ctx, parts.terms, a, who, st, has_pt<A>::value ? NJ + DP_MAX_POINTS : NJ)) return rc;
        if constexpr (has_pt<A>::value)
            if (int rc = take_points(ctx, parts.points, parts.terms, a.pt, who)) return rc;
        if constexpr (has_h<A>::value)
            if (parts.holds)
                if (int rc = take_holds(ctx, parts.holds, parts.terms, a, who)) return rc;
        dp_seq_extra e;
        if (int rc = take_seq_extra(ctx, extra, e, who)) return rc;
        a.loss_terms = e.loss_terms; a.pos = e.joint_pos;
        for (int k = 0; k < a.n_terms; ++k) a.tbl[k * dpcons::TW + dpcons::T_STEP] = (unsigned)e.row_step[k];
        return DP_OK;
    };
    return sequence_constrained_impl<A>(ctx, n_seq, latent, fr, p_in, sk, st, adj, out, stream, who, own, parts);
}

extern "C" int dp_optimize_sequence_constrained(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in,
                                                const dp_constraints* c_in, const dp_skeleton_in* skel, const dp_seq_state* st, const dp_seq_step* adj,
                                                const dp_seq_results* out, const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_optimize_sequence_constrained";
    const auto own = [&](dpcons::SeqConsArgs& a) -> int {
        if (int rc = take_constraints(ctx, c_in, a, who, st)) return rc;
        dp_seq_extra e;
        if (int rc = take_seq_extra(ctx, extra, e, who)) return rc;
        a.loss_extra = e.loss_extra; a.pos = e.joint_pos;
        return DP_OK;
    };
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !c_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_sequence_constrained: n_sequences must be positive; NULL latent, frames, params, constraints, state or results");
        return sequence_constrained_impl<dpcons::SeqConsArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, stream, who, own, SeqParts{});
    });
}

extern "C" int dp_optimize_sequence_terms(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_terms* t_in,
                                          const dp_skeleton_in* skel, const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out,
                                          const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_optimize_sequence_terms";
    SeqParts parts;
    parts.terms = t_in;
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_sequence_terms: n_sequences must be positive; NULL latent, frames, params, terms, state or results");
        return sequence_terms_impl<dpcons::SeqTermArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
    });
}

// include/dragposer_points.h: dp_optimize_terms, dp_optimize_terms_skeleton and dp_optimize_sequence_terms with points (A = dpcons::PointTermArgs,
// PointTermSkelArgs, PointSeqTermArgs); dp_points is checked behind the table (take_points)
extern "C" int dp_optimize_terms_points(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_terms* t_in, const dp_points* q_in,
                                        const dp_result* out_in, void* stream)
{
    const char* who = "dp_optimize_terms_points";
    const auto own = [&](dpcons::PointTermArgs& a) -> int {
        if (int rc = take_terms(ctx, t_in, a, who, nullptr, NJ + DP_MAX_POINTS)) return rc;
        return take_points(ctx, q_in, t_in, a.pt, who);
    };
    return entry(ctx, who, [&] {
        if (!in || !p_in || !t_in || !q_in || !out_in) return fail(ctx, DP_ERR_INVALID, "dp_optimize_terms_points: NULL batch, params, terms, points or result");
        return constrained_impl<dpcons::PointTermArgs>(ctx, in, p_in, out_in, stream, who, own, dp_launch_terms_points);
    });
}

extern "C" int dp_optimize_terms_points_skeleton(dp_ctx* ctx, const dp_batch* in, const dp_params* p_in, const dp_terms* t_in, const dp_points* q_in,
                                                 const dp_skeleton_in* skel, const dp_result* out_in, void* stream)
{
    const char* who = "dp_optimize_terms_points_skeleton";
    const auto own = [&](dpcons::PointTermSkelArgs& a) -> int {
        if (int rc = take_terms(ctx, t_in, a, who, nullptr, NJ + DP_MAX_POINTS)) return rc;
        if (int rc = take_points(ctx, q_in, t_in, a.pt, who)) return rc;
        return take_skeleton(ctx, skel, a.skel, a.skel_stride, who);
    };
    return entry(ctx, who, [&] {
        if (!in || !p_in || !t_in || !q_in || !out_in)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_terms_points_skeleton: NULL batch, params, terms, points or result");
        if (!skel) return refuse_null_skeleton(ctx, who);
        return constrained_impl<dpcons::PointTermSkelArgs>(ctx, in, p_in, out_in, stream, who, own, dp_launch_terms_points_skel);
    });
}

extern "C" int dp_optimize_sequence_terms_points(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_terms* t_in,
                                                 const dp_points* q_in, const dp_skeleton_in* skel, const dp_seq_state* st, const dp_seq_step* adj,
                                                 const dp_seq_results* out, const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_optimize_sequence_terms_points";
    SeqParts parts;
    parts.terms = t_in; parts.points = q_in;
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !q_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID,
                        "dp_optimize_sequence_terms_points: n_sequences must be positive; NULL latent, frames, params, terms, points, state or results");
        return sequence_terms_impl<dpcons::PointSeqTermArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
    });
}

// include/dragposer_holds.h: dp_optimize_sequence_terms with holds (A = dpcons::HoldSeqArgs)
extern "C" int dp_optimize_sequence_holds(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_terms* t_in,
                                          const dp_holds* h_in, const dp_skeleton_in* skel, const dp_seq_state* st, const dp_seq_step* adj,
                                          const dp_seq_results* out, const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_optimize_sequence_holds";
    SeqParts parts;
    parts.terms = t_in; parts.holds = h_in;
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !h_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_sequence_holds: n_sequences must be positive; NULL latent, frames, params, terms, holds, state or results");
        return sequence_terms_impl<dpcons::HoldSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
    });
}

// include/dragposer_latent_ar.h: dp_optimize_sequence_holds with the step's z_tgt formed in the launch (A = dpcons::ArSeqArgs); `holds` may be
// NULL, and dp_latent_ar is checked last (take_latent_ar, from sequence_constrained_impl)
extern "C" int dp_optimize_sequence_ar(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_terms* t_in,
                                       const dp_holds* h_in, const dp_latent_ar* r_in, const dp_skeleton_in* skel, const dp_seq_state* st,
                                       const dp_seq_step* adj, const dp_seq_results* out, const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_optimize_sequence_ar";
    SeqParts parts;
    parts.terms = t_in; parts.holds = h_in; parts.ar = r_in;
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !r_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_sequence_ar: n_sequences must be positive; NULL latent, frames, params, terms, ar, state or results");
        return sequence_terms_impl<dpcons::ArSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
    });
}

// include/dragposer_gaps.h: dp_optimize_sequence_ar with a tracker set decided per step (A = dpcons::GapArSeqArgs; `ar` NULL:
// dpcons::GapSeqArgs, dp_optimize_sequence_holds' frames->z_tgt); dp_gaps is checked last (take_gaps, from sequence_constrained_impl)
extern "C" int dp_optimize_sequence_gaps(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_terms* t_in,
                                         const dp_holds* h_in, const dp_latent_ar* r_in, const dp_gaps* g_in, const dp_skeleton_in* skel,
                                         const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out, const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_optimize_sequence_gaps";
    SeqParts parts;
    parts.terms = t_in; parts.holds = h_in; parts.ar = r_in; parts.gaps = g_in;
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !g_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_sequence_gaps: n_sequences must be positive; NULL latent, frames, params, terms, gaps, state or results");
        if (r_in) return sequence_terms_impl<dpcons::GapArSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
        return sequence_terms_impl<dpcons::GapSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
    });
}

// include/dragposer_tethers.h: dp_optimize_sequence_gaps with tethers (A = dpcons::TetherArSeqArgs; `ar` NULL: dpcons::TetherSeqArgs);
// dp_tethers is checked last (take_tethers, from sequence_constrained_impl)
extern "C" int dp_optimize_sequence_tethers(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_terms* t_in,
                                            const dp_holds* h_in, const dp_latent_ar* r_in, const dp_gaps* g_in, const dp_tethers* te_in,
                                            const dp_skeleton_in* skel, const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out,
                                            const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_optimize_sequence_tethers";
    SeqParts parts;
    parts.terms = t_in; parts.holds = h_in; parts.ar = r_in; parts.gaps = g_in; parts.tethers = te_in;
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !g_in || !te_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID,
                        "dp_optimize_sequence_tethers: n_sequences must be positive; NULL latent, frames, params, terms, gaps, tethers, state or results");
        if (r_in) return sequence_terms_impl<dpcons::TetherArSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
        return sequence_terms_impl<dpcons::TetherSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
    });
}

// include/dragposer_live.h: dp_optimize_sequence_gaps for one step, in one launch (A = dpcons::LiveArSeqArgs; `ar` NULL: dpcons::LiveSeqArgs)
extern "C" int dp_live_step(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_params* p_in, const dp_terms* t_in,
                            const dp_holds* h_in, const dp_latent_ar* r_in, const dp_gaps* g_in, const dp_skeleton_in* skel, const dp_seq_state* st,
                            const dp_seq_step* adj, const dp_seq_results* out, const dp_seq_extra* extra, void* stream)
{
    const char* who = "dp_live_step";
    SeqParts parts;
    parts.terms = t_in; parts.holds = h_in; parts.ar = r_in; parts.gaps = g_in;
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !g_in || !st || !out)
            return fail(ctx, DP_ERR_INVALID, "dp_live_step: n_sequences must be positive; NULL latent, frames, params, terms, gaps, state or results");
        if (fr->n_steps != 1) return fail(ctx, DP_ERR_INVALID, "dp_live_step: frames->n_steps is " + std::to_string(fr->n_steps) + ", a live step is one frame");
        if (r_in) return sequence_terms_impl<dpcons::LiveArSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
        return sequence_terms_impl<dpcons::LiveSeqArgs>(ctx, n_seq, latent, fr, p_in, skel, st, adj, out, extra, stream, who, parts);
    });
}

// ------------------------------------------------------------------------------------------------
// per-frame epilogue of S sequences (reference drag_pose.py:369-402), see include/dragposer.h
// include/dragposer_sequence_lm.h and include/dragposer_sequence_lm_terms.h: dp_optimize_lm's frame for n_steps frames of S sequences in one launch
// (+ one for the history buffers), in the headers' order of refusals.  A: dplm::SeqArgs or dplm::SeqTermArgs; own(a) validates what the entry
// point brought beyond dp_seq_lm_extra (the table and dp_seq_extra) and stands between that struct and the predictor.  (The launchers are weak
// references, like dp_launch_lm; the caller has refused a NULL argument.)
hipError_t dp_launch_lm_seq(const dplm::SeqArgs* args, hipStream_t stream) __attribute__((weak));
hipError_t dp_launch_lm_seq_terms(const dplm::SeqTermArgs* args, hipStream_t stream) __attribute__((weak));
template <class A, class Own>
static int sequence_lm_impl(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_lm_params* p_in, const dp_latent_ar* ar,
                            const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out_in, const dp_seq_lm_extra* e_in, void* stream,
                            const char* who, Own own, hipError_t (*launch)(const A*, hipStream_t), const char* unit)
{
    if (int rc = check_lm_params_size(ctx, p_in, who)) return rc;
    A a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = take_lm_params(ctx, p_in, a, who)) return rc;
    dp_seq_results out;
    if (int rc = take_sized(ctx, out_in, out, SEQ_RESULTS_V500, who)) return rc;
    if (int rc = check_sequence(ctx, fr, st, adj, out, who, true)) return rc;
    dp_seq_lm_extra e;
    std::memset(&e, 0, sizeof(e));
    if (e_in)
        if (int rc = take_sized(ctx, e_in, e, SEQ_LM_EXTRA_V600, who)) return rc;
    if (int rc = own(a)) return rc;
    if (ar) {
        if (int rc = take_latent_ar(ctx, ar, fr, st, a.r, who)) return rc;
    } else if (!fr->z_tgt)
        return fail(ctx, DP_ERR_INVALID, std::string(who) + ": neither a predictor nor frames->z_tgt: the pull term's targets have no source");
    if (REF8_BUILD) return refuse_ref8(ctx, who);
    if (!launch) return fail(ctx, DP_ERR_UNSUPPORTED, std::string(who) + ": this library was linked without " + unit);
    if (!ctx->d_vjpimg.get()) return refuse_no_image(ctx, who);
    a.img = ctx->d_vjpimg.get();
    a.z0 = latent; a.z = latent; a.z_tgt = fr->z_tgt; a.cur_rot = st->global_rot; a.tgt_pos = fr->tgt_pos; a.tgt_rot = fr->tgt_rot; a.w = fr->w;
    a.tracked = fr->tracked; a.n_frames = n_seq;
    a.pose = out.pose_ret; a.world_rot = out.world_rot; a.iters = out.iters; a.loss = out.loss; a.status = out.status;
    a.mu = e.mu; a.mu_trace = e.mu_trace; a.n_accepted = e.n_accepted; a.loss0 = e.loss0; a.pos = e.joint_pos;
    fill_sequence(a.q, ctx, fr, st, adj, out);
    {
        DEVICE_GUARD(ctx);
        const hipError_t err = launch(&a, (hipStream_t)stream);
        if (err != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string(who) + ": kernel launch: " + hipGetErrorString(err));
    }
    return append_history(ctx, n_seq, fr, st, out, stream);
}

extern "C" int dp_optimize_sequence_lm(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_lm_params* p_in, const dp_latent_ar* ar,
                                       const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out_in, const dp_seq_lm_extra* e_in, void* stream)
{
    const char* who = "dp_optimize_sequence_lm";
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !st || !out_in)
            return fail(ctx, DP_ERR_INVALID, "dp_optimize_sequence_lm: n_sequences must be positive; NULL latent, frames, params, state or results");
        return sequence_lm_impl<dplm::SeqArgs>(ctx, n_seq, latent, fr, p_in, ar, st, adj, out_in, e_in, stream, who, [](dplm::SeqArgs&) { return (int)DP_OK; },
                                               dp_launch_lm_seq, "dp_lm_seq.hip");
    });
}

// ... with a term table in the loss: the table as dp_optimize_sequence_terms takes it (take_terms' `seq` form), then dp_seq_extra, whose
// joint_pos is refused here (dp_seq_lm_extra.joint_pos is this call's array of joint positions), then each term's step between rows
extern "C" int dp_optimize_sequence_lm_terms(dp_ctx* ctx, int n_seq, float* latent, const dp_seq_frames* fr, const dp_lm_params* p_in, const dp_terms* t_in,
                                             const dp_latent_ar* ar, const dp_seq_state* st, const dp_seq_step* adj, const dp_seq_results* out_in,
                                             const dp_seq_lm_extra* e_in, const dp_seq_extra* term_extra, void* stream)
{
    const char* who = "dp_optimize_sequence_lm_terms";
    const auto own = [&](dplm::SeqTermArgs& a) -> int {
        if (int rc = take_terms(ctx, t_in, a, who, st)) return rc;
        dp_seq_extra x;
        if (int rc = take_seq_extra(ctx, term_extra, x, who)) return rc;
        if (x.joint_pos)
            return fail(ctx, DP_ERR_INVALID, std::string(who) + ": dp_seq_extra.joint_pos must be NULL here; the joint positions of every step go to dp_seq_lm_extra.joint_pos");
        a.loss_terms = x.loss_terms;
        for (int k = 0; k < a.n_terms; ++k) a.tbl[k * dpcons::TW + dpcons::T_STEP] = (unsigned)x.row_step[k];
        return DP_OK;
    };
    return entry(ctx, who, [&] {
        if (n_seq <= 0 || !latent || !fr || !p_in || !t_in || !st || !out_in)
            return fail(ctx, DP_ERR_INVALID,
                        "dp_optimize_sequence_lm_terms: n_sequences must be positive; NULL latent, frames, params, terms, state or results");
        return sequence_lm_impl<dplm::SeqTermArgs>(ctx, n_seq, latent, fr, p_in, ar, st, adj, out_in, e_in, stream, who, own, dp_launch_lm_seq_terms,
                                                   "dp_lm_seq_terms.hip");
    });
}

static int advance_impl(dp_ctx* ctx, int n_seq, const dp_result* res, const dp_seq_state* st, const dp_seq_step* step, void* stream)
{
    if (n_seq <= 0 || !res || !st || !step) return fail(ctx, DP_ERR_INVALID, "dp_sequence_advance: bad arguments");
    dp_result rv;
    if (int rc = take_result(ctx, res, rv, "dp_sequence_advance")) return rc;
    res = &rv;
    if (!res->z_pre || !res->pose || !res->disp || !res->world_disp || !res->world_rot || !res->pos)
        return fail(ctx, DP_ERR_INVALID, "dp_sequence_advance: the frame result needs z_pre, pose, disp, world_disp, world_rot and pos");
    if (!st->global_pos || !st->global_rot || !st->latent_buf || !st->disp_buf || !st->heights_buf)
        return fail(ctx, DP_ERR_INVALID, "dp_sequence_advance: NULL state array");
    if (st->history < 1 || st->n_heights < 0 || st->n_heights > DP_MAX_HEIGHT_JOINTS)
        return fail(ctx, DP_ERR_INVALID, "dp_sequence_advance: history / n_heights out of range");
    for (int h = 0; h < st->n_heights; ++h)
        if (st->height_joints[h] < 0 || st->height_joints[h] >= NJ) return fail(ctx, DP_ERR_INVALID, "dp_sequence_advance: bad height joint");
    if (step->adjust_joint >= NJ || (step->adjust_joint >= 0 && (step->adjust_target_joint < 0 || step->adjust_target_joint >= NJ || !step->tgt_pos)))
        return fail(ctx, DP_ERR_INVALID, "dp_sequence_advance: bad joint adjustment");
    SeqArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_seq = n_seq; a.history = st->history; a.n_heights = st->n_heights;
    for (int h = 0; h < st->n_heights; ++h) a.height_joints[h] = st->height_joints[h];
    a.adjust_joint = step->adjust_joint < 0 ? -1 : step->adjust_joint;
    a.adjust_target_joint = step->adjust_target_joint; a.adjust_weight = step->adjust_weight;
    for (int k = 0; k < 4; ++k) { a.mean_q0[k] = ctx->mean_q0[k]; a.std_q0[k] = ctx->std_q0[k]; }
    a.z_pre = res->z_pre; a.pose = res->pose; a.disp = res->disp; a.world_disp = res->world_disp; a.world_rot = res->world_rot; a.pos = res->pos;
    a.tgt_pos = step->tgt_pos;
    a.global_pos = st->global_pos; a.global_rot = st->global_rot; a.latent_buf = st->latent_buf; a.disp_buf = st->disp_buf;
    a.heights_buf = st->heights_buf; a.pose_ret = step->pose_ret; a.pos_ret = step->pos_ret;
    DEVICE_GUARD(ctx);
    hipError_t e = dp_launch_sequence_advance(&a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, DP_ERR_LAUNCH, std::string("sequence kernel launch: ") + hipGetErrorString(e));
    return DP_OK;
}

extern "C" int dp_sequence_advance(dp_ctx* ctx, int n_seq, const dp_result* res, const dp_seq_state* st, const dp_seq_step* step, void* stream)
{
    return entry_quiet(ctx, "dp_sequence_advance", [&] { return advance_impl(ctx, n_seq, res, st, step, stream); });
}
