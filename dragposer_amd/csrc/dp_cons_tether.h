// dp_cons_tether.h -- argument blocks and LDS budget of dp_cons_tether.hip: dp_cons_gap.hip's two kernels with tethers
// (include/dragposer_tethers.h), shared with the host side (dp_host.cpp).  The structs and constants of dp_cons.h .. dp_cons_live.h stay as they
// are: the fourteen other kernels' code does not change with this unit.
#pragma once
#include "dp_cons_gap.h"

namespace dpcons {

constexpr int MAX_TETHERS = 4; // DP_MAX_TETHERS
static_assert(MAX_TETHERS == MAX_HOLDS, "hold_of (dp_cons_hold.h) walks both maps");
constexpr int TETHER_ROW = 8;  // DP_TETHER_STATE_FLOATS: (x, y, z, live) the term's row, (wx, wy, wz, have) the joint's last world position

// LDS: dp_cons_gap.h's two layouts, unchanged, and one more array with one area per wave.  A tether's row (x, y, z, live) of the wave's
// sequence lives in the tethered term's row of the wave's block (W_ROW + 4 * term), exactly as a hold's: read from `state` before the first
// step, screened and read by the terms from there, rewritten by the step's epilogue, written back after the last step.  The joint's last
// world position (wx, wy, wz, have) of tether k lives in words 4k .. 4k + 3 of the wave's area of the new array; lane `term` is the only
// lane that reads or writes them.  Nothing of a tether is kept in a register across the iteration loop.
// (-DDP_TETHER_WPREV_GLOBAL=1 builds the variant DESIGN.md section 13h measured against: no new array, the four words stay in `state` and
// cost a global round trip per step.)
#ifndef DP_TETHER_WPREV_GLOBAL
#define DP_TETHER_WPREV_GLOBAL 0
#endif
constexpr int TETHER_W_FLOATS = DP_TETHER_WPREV_GLOBAL ? 0 : MAX_TETHERS * 4;
constexpr int TETHER_LDS_BYTES = GAP_LDS_BYTES + WPB * 4 * TETHER_W_FLOATS, TETHER_AR_LDS_BYTES = GAP_AR_LDS_BYTES + WPB * 4 * TETHER_W_FLOATS;
static_assert(DP_TETHER_WPREV_GLOBAL || (TETHER_LDS_BYTES == 76976 && TETHER_AR_LDS_BYTES == 80048), "the LDS budget stated in DESIGN.md section 13h");
static_assert(TETHER_LDS_BYTES <= TETHER_AR_LDS_BYTES && 2 * TETHER_AR_LDS_BYTES <= 160 * 1024, "two workgroups of either kernel fit a CU's LDS");

// A tethered term is a point-DISTANCE term no hold refers to, which never reads its staged axis_a words: the host puts alpha in the first.
constexpr int T_TALPHA = T_AXA;

struct TetherFields {
    float* state;   // [S][n_tethers][8] in / out
    float* trace;   // [T][S][n_tethers][8] or NULL
    int n_tethers;  // 0..MAX_TETHERS
    unsigned terms; // byte k: the term tether k refers to (no two tethers share a term)
};
static_assert(MAX_TETHERS * 8 <= 32 && MAX_TERMS <= 256, "a term index per byte of TetherFields::terms");

struct TetherSeqArgs : GapSeqArgs {
    TetherFields t;
};
struct TetherArSeqArgs : GapArSeqArgs {
    TetherFields t;
};

} // namespace dpcons

hipError_t dp_launch_terms_tether_seq(const dpcons::TetherSeqArgs* args, hipStream_t stream);
hipError_t dp_launch_terms_tether_ar_seq(const dpcons::TetherArSeqArgs* args, hipStream_t stream);
