// dp_encoder.h -- the weight image of dp_encoder.hip, shared by the packer (dp_encoder_host.cpp) and the device code so that the two
// cannot disagree (as dp_layout.h does for the round-1 kernel), and the launcher's interface.
//
// The folded encoder is four dense layers y = A x + c (include/dragposer_encoder.h: dp_encoder_folded).  One wavefront owns 16 poses
// and runs every product on v_mfma_f32_16x16x4_f32 with the weights as A (M = 16 output rows, K = 4) and the poses as B (N = 16):
//   A operand   lane l supplies A[row l & 15][k = l >> 4]
//   B operand   lane l supplies B[k = l >> 4][pose l & 15]
//   C / D       register r of lane l is row 4 (l >> 4) + r of pose l & 15
// so output tile t leaves channel 16 t + 4 g + r of pose n in register r on lane 16 g + n -- and a B operand wants lane 16 g + n to
// supply ONE channel of pose n.  THE K-ORDER RULE: K step s = (t, r) = (s >> 2, s & 3) of every layer reads input channel
//   enc_channel(s, g) = 16 t + 4 g + r                                                 from lane group g,
// which makes register r of the previous layer's tile t the B operand of step s as it stands: activations never leave the register
// file.  Layer 0 follows the same rule with "tile t" = the t-th 16-byte load of the pose row (lane group g loads channels
// 16 t + 4 g .. + 3).
//
// Image (fp32 words), staged into LDS once per workgroup:
//   weights of layer l at enc_w_off(l):  word (((T * S/4 + s/4) * 64 + lane) * 4 + s % 4) = A_l[image row 16 T + (lane & 15)][enc_channel(s, lane >> 4)]
//                                        -- one 16-byte LDS read per lane feeds four K steps of tile T
//   biases of layer l at enc_b_off(l):   word (image row); a lane's C operand of tile T is the 16 bytes at row 16 T + 4 g
// Rows and channels beyond the layer's size are padding (zero words): layer 1 has 72 rows in 5 tiles, so layer 2 reads 80 channels
// of which the last 8 are LeakyReLU(0) = 0 against zero weights.
// The head's image rows are permuted (enc_head_row) so that a lane holds mu[k] and logvar[k] of the SAME k: tile 0 = mu[0..15],
// tile 1 = logvar[0..15], tile 2 = lane group g even: mu[16 + 2 g + r], g odd: logvar[16 + 2 (g - 1) + r] (partners 16 lanes apart).
#pragma once

namespace dpenc {

constexpr int NL = 4;             // A0, A1, A2, Ah
constexpr int POSES = 16;         // poses per wavefront (N of the MFMA)
constexpr int WAVES = 8;          // wavefronts per workgroup (two per SIMD; 140 KB of LDS: one workgroup per CU)
constexpr int THREADS = WAVES * 64;
constexpr int IN_CH = 176, LAT = 24;
constexpr float SLOPE = 0.2f;

constexpr int enc_rows(int l) { return l == 0 ? 112 : l == 1 ? 72 : 48; }          // rows of the folded matrix
constexpr int enc_cols(int l) { return l == 0 ? 176 : l == 1 ? 112 : l == 2 ? 72 : 48; }
constexpr int enc_tiles(int l) { return (enc_rows(l) + 15) / 16; }                 // 7, 5, 3, 3
constexpr int enc_steps(int l) { return l == 0 ? 44 : 4 * enc_tiles(l - 1); }      // 44, 28, 20, 12 K steps (a multiple of 4)
constexpr int enc_channel(int s, int g) { return 16 * (s >> 2) + 4 * g + (s & 3); }
constexpr int enc_w_words(int l) { return enc_tiles(l) * enc_steps(l) * 64; }
constexpr int enc_w_off(int l) { return l == 0 ? 0 : enc_w_off(l - 1) + enc_w_words(l - 1); }
constexpr int enc_b_off(int l) { return l == 0 ? enc_w_off(NL - 1) + enc_w_words(NL - 1) : enc_b_off(l - 1) + 16 * enc_tiles(l - 1); }
constexpr int IMG_WORDS = enc_b_off(NL - 1) + 16 * enc_tiles(NL - 1);              // 34 816 weights + 288 biases = 140 416 bytes
constexpr int enc_w_word(int l, int T, int s, int lane) { return enc_w_off(l) + ((T * (enc_steps(l) / 4) + (s >> 2)) * 64 + lane) * 4 + (s & 3); }
// image row i of the head -> row of Ah / ch (0..23 mu, 24..47 logvar)
constexpr int enc_head_row(int i)
{
    return i < 16 ? i : i < 32 ? LAT + (i - 16) : ((((i - 32) >> 2) & 1) ? LAT : 0) + 16 + 4 * ((i - 32) >> 3) + (i & 3);
}
constexpr int enc_image_row(int l, int i) { return l == 3 ? enc_head_row(i) : i; }
static_assert(IMG_WORDS == 35104 && IMG_WORDS % 4 == 0, "image size");
static_assert(IMG_WORDS * 4 <= 160 * 1024, "the image must fit one CU's LDS");
static_assert(enc_head_row(32) == 16 && enc_head_row(36) == 40 && enc_head_row(43) == 23 && enc_head_row(47) == 47, "head permutation");

// device pointers; the begin form (dp_sequence_begin) when `begin` is set
struct EncArgs {
    const float* image;
    int n, n_tiles;
    const float *pose, *eps;
    float *mu, *logvar, *latent;
    int* status;
    int begin, history, n_heights;
    const float *init_pos, *init_rot, *init_heights;
    float *global_pos, *global_rot, *latent_buf, *disp_buf, *heights_buf;
    float limit;
};

// the workgroups of a launch of n_tiles tiles on a device of n_cu CUs: a tile per SIMD (four per workgroup) until every CU has a
// workgroup, then a persistent loop.  A pose's arithmetic does not depend on it.
constexpr int enc_grid(int n_tiles, int n_cu)
{
    return (n_tiles + 3) / 4 < 1 ? 1 : (n_tiles + 3) / 4 < n_cu ? (n_tiles + 3) / 4 : n_cu;
}

int launch_encoder(const EncArgs& a, int n_cu, void* stream); // dp_encoder.hip; a hipError_t as int

} // namespace dpenc
