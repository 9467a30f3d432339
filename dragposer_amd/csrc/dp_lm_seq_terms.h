// dp_lm_seq_terms.h -- argument block and LDS budget of dp_lm_seq_terms.hip: dp_lm_seq.hip's step loop around dp_lm_terms.hip's frame
// (include/dragposer_sequence_lm_terms.h), shared with the host side (dp_host.cpp).  dp_lm.h's, dp_lm_seq.h's and dp_lm_terms.h's structs and
// constants stay as they are: the code of dp_lm_kernel, dp_lm_seq_kernel and dp_lm_terms_kernel does not change with this unit.
#pragma once
#include "dp_cons_seq.h"
#include "dp_lm_seq.h"
#include "dp_lm_terms.h"

namespace dplm {

// the staged term's free word, dp_cons_seq.h's: floats between two steps' rows of the term's per_frame array, 0 = one row per sequence held
// for all steps.  The row step travels in the table, inside the argument block; dp_lm_terms_kernel never reads it.
constexpr int T_STEP = dpcons::T_STEP;

// LDS: the three arrays of the two units this one combines, each as its own header lays it out -- dp_lm.h's weights and blocks, dp_lm_seq.h's
// history rows of the predictor (an area per wave), dp_lm_terms.h's term table and rows (a block per wave).
constexpr int SEQ_TERMS_LDS_BYTES = LDS_BYTES + 4 * TERM_LDS_FLOATS + WPB * 4 * AR_W_FLOATS;
static_assert(SEQ_TERMS_LDS_BYTES == 121488 + 1408 + 4 * 256 + 4 * 4 * 96 && SEQ_TERMS_LDS_BYTES == 125456 && SEQ_TERMS_LDS_BYTES <= 160 * 1024,
              "the LDS budget stated in DESIGN.md section 16c");

// What the table adds to a sequence's arguments: TermArgs' fields under the same names (dp_host.cpp's take_terms writes either).
struct SeqTermArgs : SeqArgs {
    const float* global_pos;      // what take_terms leaves here is not read: the terms' global position is the carried one (SeqFields::global_pos)
    int up;                       // the component DP_TERM_DROP_UP zeroes
    int n_terms, need_gp;         // need_gp: an active PLANE or point-DISTANCE term exists -- the carried position is then screened every step
    float* loss_terms;            // [T][S][n_terms], nullable (dp_seq_extra.loss_terms)
    unsigned tbl[MAX_TERMS * TW]; // T_* layout with T_STEP; DISTANCE's p0 / p1 hold lo^2 / hi^2
};

} // namespace dplm

hipError_t dp_launch_lm_seq_terms(const dplm::SeqTermArgs* args, hipStream_t stream);
