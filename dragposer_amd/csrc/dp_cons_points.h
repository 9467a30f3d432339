// dp_cons_points.h -- argument blocks and LDS layout of dp_cons_points.hip: the three table kernels (dp_terms_kernel, dp_terms_skel_kernel,
// dp_terms_seq_kernel) with POINTS, weighted combinations of the joints' positions that a PLANE or DISTANCE term may name in a joint's
// place (include/dragposer_points.h), shared with the host side (dp_host.cpp).  The structs and constants of dp_cons.h .. dp_cons_tether.h
// stay as they are: the fourteen other kernels' code does not change with this unit.
#pragma once
#include "dp_cons_seq.h"

namespace dpcons {

constexpr int MAX_POINTS = 4; // DP_MAX_POINTS
constexpr int PT_NJ = 22;     // coefficients per point: one per joint

// LDS: the table layouts of dp_cons.h (plain) and dp_cons_skel.h (per-frame skeletons, sequences) with two additions, both BEHIND what
// was there, so that no existing offset (L_TBL, L_WAVE0_T, W_P, W_G, W_ROW, W_SKEL_T) moves:
//   W_PT    [MAX_POINTS][4] at the end of each wave's block: the points' positions P_(22+k) of the iteration, formed after the forward
//           kinematics by lanes 4k + c and read by every lane where a term names index 22 + k -- the row format of W_P, so a term's
//           position is `base + 4 * index` with one of two bases
//   L_COEF  [MAX_POINTS][22] behind the last wave's block, staged once per workgroup with the term table: m_k[j] at k * 22 + j.  The
//           gradient's read is lane j reading word k * 22 + j of one row: 22 consecutive words, 22 of a 4-byte read's 32 banks, no
//           conflict.  The forward's read is lane 4k + c reading m_k[j] for the same j: lanes of one point read one word (a broadcast),
//           lanes of different points words 22 apart -- banks 0, 22, 12, 2 (+ j, mod 32), distinct.
constexpr int PT_W_FLOATS = 4 * MAX_POINTS;                           // 16 floats per wave: the block stays 16-byte aligned
constexpr int PT_COEF_FLOATS = MAX_POINTS * PT_NJ;                    // 88
constexpr int PT_W_PT = W_FLOATS_T, PT_SK_W_PT = SK_W_FLOATS_T;       // where the area starts in the wave's block
constexpr int PT_W_STRIDE = W_FLOATS_T + PT_W_FLOATS, PT_SK_W_STRIDE = SK_W_FLOATS_T + PT_W_FLOATS;
constexpr int PT_L_COEF = L_WAVE0_T + WPB * PT_W_STRIDE, PT_SK_L_COEF = L_WAVE0_T + WPB * PT_SK_W_STRIDE;
constexpr int PT_LDS_FLOATS = PT_L_COEF + PT_COEF_FLOATS, PT_SK_LDS_FLOATS = PT_SK_L_COEF + PT_COEF_FLOATS;
constexpr int PT_LDS_BYTES = 4 * PT_LDS_FLOATS, PT_SK_LDS_BYTES = 4 * PT_SK_LDS_FLOATS;
static_assert(PT_LDS_BYTES == LDS_BYTES_T + 864 && PT_SK_LDS_BYTES == SK_LDS_BYTES_T + 864, "the table and the areas: 352 + 8 * 64 bytes");
static_assert(PT_LDS_BYTES == 75152 && PT_SK_LDS_BYTES == 77328, "the LDS budget stated in DESIGN.md section 13i");
static_assert(2 * PT_SK_LDS_BYTES <= 160 * 1024, "two workgroups of any of the three kernels fit a CU's LDS");
static_assert(PT_W_STRIDE % 4 == 0 && PT_SK_W_STRIDE % 4 == 0, "every wave's block stays 16-byte aligned");

struct PointFields {
    int n_points;                 // 0..MAX_POINTS
    float coeff[PT_COEF_FLOATS];  // [n_points][22], the rest 0: travels in the launch
};

struct PointTermArgs : TermArgs {
    PointFields pt;
};
struct PointTermSkelArgs : TermSkelArgs {
    PointFields pt;
};
struct PointSeqTermArgs : SeqTermArgs {
    PointFields pt;
};

} // namespace dpcons

hipError_t dp_launch_terms_points(const dpcons::PointTermArgs* args, hipStream_t stream);
hipError_t dp_launch_terms_points_skel(const dpcons::PointTermSkelArgs* args, hipStream_t stream);
hipError_t dp_launch_terms_points_seq(const dpcons::PointSeqTermArgs* args, hipStream_t stream);
