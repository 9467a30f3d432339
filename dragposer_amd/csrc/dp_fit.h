// dp_fit.h -- argument block and LDS layout of dp_fit_bones' two kernels (dp_fit.hip), shared with the host side (dp_host.cpp).
//
// dp_fit_rows_kernel: one frame per wave, WPB waves per workgroup; the folded decoder staged once per workgroup from the context's
// dp_forward_vjp image in dp_lm.h's places (weights, sigma, parents, bones -- here `base`), then a block per wave: the forward pass's state,
// 24 design rows at a time, and the frame's [A b]^T [A b].  After ONE workgroup barrier the waves' matrices are added in wave order and
// written as the workgroup's partial sum.  dp_fit_solve_kernel: one workgroup that adds the partial sums in index order in double and
// solves.  Reference of what is computed: include/dragposer_calibration.h.
#pragma once
#include <hip/hip_runtime.h>

#include "dp_lm.h"

namespace dpfit {

constexpr int WPB = 4;      // waves (= frames in flight) per workgroup: 69 KB of LDS, two workgroups per CU
constexpr int MAXK = 24;    // DP_FIT_MAX_GROUPS
constexpr int MS = MAXK + 1; // rows and columns of a matrix as it is stored, whatever K is (what lies beyond K is zero)

// LDS (floats): dp_lm.h's weight part up to its first wave's block, the bones' groups, then a block per wave
constexpr int L_GRP = dplm::L_WAVE0;      // int group[22] (+2 pad)
constexpr int L_WAVE0 = L_GRP + 24;
constexpr int W_Z = 0;          // [24] the latent
constexpr int W_H0 = 24;        // [40] h0
constexpr int W_H1 = 64;        // [60] h1
constexpr int W_Q = 124;        // [92] de-normalised decoder output
constexpr int W_R = 216;        // [22][9] R_j (root: R_0, the world root rotation)
constexpr int W_B = 414;        // [22][4] bone b_j = R_p base_j (root frame)
constexpr int W_SW = 502;       // [22] sqrt(w_pos / 3E) (+2 pad)
constexpr int SJ = 32;          // row stride of the design rows and of the matrix
constexpr int W_J = 528;        // [24][SJ] the rows of up to eight tracked joints: columns 0..K-1 of A, column K of b
constexpr int W_A = W_J + 24 * SJ; // [MS][SJ] the frame's [A b]^T [A b]
constexpr int W_N = W_A + MS * SJ; // [1] 1.0: the frame was used (+3 pad)
constexpr int W_FLOATS = W_N + 4;
constexpr int LDS_FLOATS = L_WAVE0 + WPB * W_FLOATS;
constexpr int LDS_BYTES = 4 * LDS_FLOATS;
static_assert(WPB == 4 && LDS_BYTES == 70704 && 2 * LDS_BYTES <= 160 * 1024, "the LDS budget stated in DESIGN.md section 17");

// a workgroup's partial sum in the workspace (floats): the matrix [MS][MS], the frames used, padding to a multiple of 64 bytes
constexpr int PART_COUNT = MS * MS;
constexpr int PART_FLOATS = 640;
static_assert(PART_COUNT + 1 <= PART_FLOATS, "a partial sum holds the matrix and the count");
constexpr int SOLVE_THREADS = PART_FLOATS; // dp_fit_solve_kernel: a thread per element of a partial sum

struct Args {
    const float* img; // dp_vjp.h image (IMG_WORDS)
    const float *z0, *cur_rot, *tgt_pos, *w;
    const unsigned char* tracked;
    float* workspace; // [n_parts][PART_FLOATS]
    float *scales, *offsets, *rms; // offsets, rms nullable
    double* normal;                // nullable
    int *info, *status;            // nullable
    int n_frames, n_parts, K, has_base;
    float ridge;
    int grp[22];     // entry 0 unused
    float base[66];  // read when has_base (else the image's bones)
    float prior[MAXK];
};

inline int parts_of(int n_frames) { return (n_frames + WPB - 1) / WPB; }

} // namespace dpfit

hipError_t dp_launch_fit(const dpfit::Args* args, hipStream_t stream);
