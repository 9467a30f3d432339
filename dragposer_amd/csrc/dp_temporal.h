// dp_temporal.h -- what the temporal predictor's host side (dp_temporal_host.cpp: the handle, the packer of the weight image, the variant
// choice) shares with its device unit (dp_temporal.hip: the kernels and their launcher): the sizes the image is laid out by, the argument
// block, the launcher's interface.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dragposer.h"

namespace dpt {

constexpr int D = DP_TEMPORAL_D_MODEL, LAT = 24;
constexpr int MAXT = DP_TEMPORAL_MAX_TOKENS, MAXL = DP_TEMPORAL_MAX_LAYERS;
constexpr int NT = 512, NWV = NT / 64;              // threads / waves per workgroup (two waves per SIMD)
constexpr int MAX_IN = 36;                          // 24 + 3 + 8 heights, padded to a multiple of 4 (K-steps)
constexpr int FT = 32;                              // hidden units per feed-forward tile (the K of one v_mfma_f32_16x16x32_bf16)
constexpr int FFN_IMG_V = 12 + 9 + 2;               // 16-byte words per lane of a tile's image: W1 [2 M-tiles][2 K-blocks][3 terms], W2 [3 column tiles][3 terms], bias1 [2]
constexpr int FFN_TILE_FLOATS = FFN_IMG_V * 64 * 4; // ... in 32-bit words

// the TEAM exchange area (dp_temporal.hip, "the TEAM exchange"): granules of 16 bytes, [team][2 slots][XCH_GRANULES][XCH_GMAX]
constexpr int XCH_GRANULES = 2 * 16 * D / 3;          // two token tiles of 16 x 48 partial sums, three per granule
constexpr int XCH_GMAX = 16;                          // the largest team; slots per granule in the layout
constexpr int XCH_POLL_LIMIT = 1 << 19;               // (~1 s: then the member gives up -- dp_temporal.hip, "time-out")
constexpr int XCH_GRANULE_BYTES = 16;

struct TLayer { // offsets (in floats) into the device weight buffer
    int sa_in_wT, sa_in_b, sa_out_wT, sa_out_b, ca_in_wT, ca_in_b, ca_out_wT, ca_out_b;
    int ffn_pack, lin2_b, n1w, n1b, n2w, n2b, n3w, n3b; // ffn_pack: [ceil(F / 16)][7][64 lanes][4] (dp_temporal_host.cpp: pack_model)
};
struct TArgs {
    const float* w;
    int enc_tab, dec_tab; // offsets of the TLayer tables inside the weight buffer (a kernel-argument array indexed by the
                          // layer loop would be copied into registers: 288 SGPRs)
    int n_enc, n_dec, ff, n_in, nh, max_len, step;
    int ipe_wT, ipe_b, ipd_wT, ipd_b, op_wT, op_b, pe, encn_w, encn_b, decn_w, decn_b, mean, stdv;
    int ln0, ln_len; // all LayerNorm rows (the layers' and the two final ones) are one block: the TEAM kernel keeps it in LDS
    // per call
    const float *latent_buf, *disp_buf, *heights_buf;
    float* target;
    int H, n_seq, window;
    // a TEAM of G workgroups per sequence (few sequences: latency; below): the exchange area of the handle, the tag base of this launch
    float* xch;
    unsigned* epochs; // one word per team: the tag of the team's last exchange (device-resident, so that a captured launch can be replayed)
    int* tstatus;     // the handle's status word in DEVICE memory: what every team launch checks at entry and while it waits
    int* hstatus;     // ... and its mirror in page-locked HOST memory: what dp_temporal_status / the next dp_temporal_predict read without a synchronise
    int G;
    int poll_limit;   // re-reads of a granule set before a member gives up (XCH_POLL_LIMIT; the debug hook shortens it)
    int dbg_skip_team, dbg_skip_member; // private test hook: that member of that team never publishes (-1: nobody)
};

// variant: 21 / 41 = one sequence per workgroup at 2 / 4 waves per SIMD, 42 = two sequences per workgroup, 44 = PAIR (four per 1024-thread
// workgroup), >= 100 = a TEAM of G workgroups per sequence (a.xch ... a.dbg_skip_member filled in).  Returns the launch's error.
hipError_t dp_launch_temporal(int variant, int n_seq, int G, const TArgs& a, hipStream_t stream);
// workgroups of the TEAM kernel that fit one CU by the runtime's occupancy query (< 1: it does not fit, or the query failed)
int dp_temporal_team_blocks_per_cu();
// the CUs a launch on `stream` may use: n_cu, or fewer when the stream carries a CU mask
int dp_temporal_stream_cus(hipStream_t stream, int n_cu);

} // namespace dpt
