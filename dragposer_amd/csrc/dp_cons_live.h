// dp_cons_live.h -- argument blocks of dp_cons_live.hip: dp_cons_gap.hip's two kernels for ONE step, with the step's row appended to the three
// history buffers by the kernel itself (include/dragposer_live.h), shared with the host side (dp_host.cpp).  The structs and constants of
// dp_cons.h .. dp_cons_gap.h stay as they are: the twelve other kernels' code does not change with this unit.
#pragma once
#include "dp_cons_gap.h"

namespace dpcons {

// LDS: dp_cons_gap.h's two layouts, unchanged.  The appended row stays in registers: lane c < 27 + n_heights keeps column c's value from the
// step's `stop` (lanes < 24 their z; the displacement and the heights are lane 0's, handed over by v_readfirstlane) to the end of the kernel,
// where it moves its column of the sequence's buffers up by one row, LIVE_CHUNK rows at a time, and stores the value in the last row.
constexpr int LIVE_LDS_BYTES = GAP_LDS_BYTES, LIVE_AR_LDS_BYTES = GAP_AR_LDS_BYTES;
// rows of a column in flight at once.  Each chunk is one round trip to memory, paid in series: 8 rows measured 6 us per frame for the append
// of a 60-row history, 64 rows spill; 32 rows are two round trips and fit the registers the iteration loop has let go of
constexpr int LIVE_CHUNK = 32;

struct LiveFields {
    float* latent_buf;  // [S][history][24], the state's arrays: in / out
    float* disp_buf;    // [S][history][3]
    float* heights_buf; // [S][history][n_heights]
    int history;        // >= 1
};

struct LiveSeqArgs : GapSeqArgs {
    LiveFields l;
};
struct LiveArSeqArgs : GapArSeqArgs {
    LiveFields l;
};

} // namespace dpcons

hipError_t dp_launch_live(const dpcons::LiveSeqArgs* args, hipStream_t stream);
hipError_t dp_launch_live_ar(const dpcons::LiveArSeqArgs* args, hipStream_t stream);
