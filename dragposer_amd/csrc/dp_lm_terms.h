// dp_lm_terms.h -- argument block and LDS budget of dp_lm_terms.hip: dp_lm.hip's frame with a table of constraint terms in its loss
// (include/dragposer_lm_terms.h), shared with the host side (dp_host.cpp).  dp_lm.h's struct and constants stay as they are: dp_lm_kernel's
// code does not change with this unit.
#pragma once
#include "dp_cons.h"
#include "dp_lm.h"

namespace dplm {

constexpr int MAX_TERMS = dpcons::MAX_TERMS; // DP_MAX_TERMS
constexpr int TW = dpcons::TW;               // words per staged term, dp_cons.h's T_* layout

// LDS: dp_lm.h's layout, unchanged, and a second array: the term table [MAX_TERMS][TW], staged once per workgroup, then one block per wave
// of the frame's rows [MAX_TERMS][4] (vector, s_f; defaults filled in), as dp_cons.h arranges them.  Lane t writes row t at the screening;
// every lane reads the rows behind a wave_sync().
constexpr int TL_TBL = 0;
constexpr int TL_ROW0 = TL_TBL + MAX_TERMS * TW;
constexpr int TW_ROW = 4 * MAX_TERMS;
constexpr int TERM_LDS_FLOATS = TL_ROW0 + WPB * TW_ROW;
constexpr int TERMS_LDS_BYTES = LDS_BYTES + 4 * TERM_LDS_FLOATS;
static_assert(TERMS_LDS_BYTES == 123920 && TERMS_LDS_BYTES <= 160 * 1024, "the LDS budget stated in DESIGN.md section 16b");
static_assert(TL_TBL % 2 == 0 && TW % 2 == 0 && dpcons::T_ROW % 2 == 0, "per-frame row pointers are read from LDS as 8-byte words");
static_assert(92 * ST * 4 >= (40 + 60 + 92 + 198 + 66 + 66 + 198) * 8, "the pass in double, with P and G of every joint, fits the tangents' place");

// What the table adds to a frame's arguments (dpcons::TermArgs' fields under the same names: dp_host.cpp's take_terms writes either)
struct TermArgs : Args {
    const float* global_pos;      // [B][3], read only when need_gp
    int up;                       // the component DP_TERM_DROP_UP zeroes
    int n_terms, need_gp;         // need_gp: an active PLANE or point-DISTANCE term exists
    float* loss_terms;            // [B][n_terms], nullable
    unsigned tbl[MAX_TERMS * TW]; // T_* layout; DISTANCE's p0 / p1 hold lo^2 / hi^2
};

} // namespace dplm

hipError_t dp_launch_lm_terms(const dplm::TermArgs* args, hipStream_t stream);
