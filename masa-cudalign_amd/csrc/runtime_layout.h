// Internal header of the host runtime (runtime.cpp): the ONE definition of the words that host, kernels and neighbour GPU
// share, and of the score domains.  Not part of the C ABI (include/mi355sw.h); the kernels do not see it either -- they get
// pointers through KernelArgs.
#ifndef MI355SW_RUNTIME_LAYOUT_H_
#define MI355SW_RUNTIME_LAYOUT_H_

#include <hip/hip_runtime.h>

namespace mi355sw {

// ------------------------------------------------------------------------------------------------
// Words shared between the host, the kernels and the neighbour GPU.  All three blocks are addressed in INT indices
// ((int*) block + WORD).  Words that different agents write lie 64 bytes (16 ints) apart on purpose -- one cache line
// each, so that a poll of one word never contends with the stores to another; new words keep that spacing.
// ------------------------------------------------------------------------------------------------
// device control block (mi355sw_handle::d_ctrl; the seed pass keeps one of its own in its scratch): zeroed before a launch
enum CtrlWord {
    CTRL_TICKET = 0,            // next strip to claim
    CTRL_ABORT = 16,            // set by the kernel on an overflow report or a time-out: strips claimed afterwards are skipped
    CTRL_ERROR = 32,            // error code (16: the packed kernel left its exact range), then the details of that report:
    CTRL_ERROR_CAUSES = 33,     //   OVF16_* bits (csrc/sw_kernel_pk16.inc)
    CTRL_ERROR_STRIP = 34,      //   first reporting strip + 1
    CTRL_ERROR_CHUNK = 35, CTRL_ERROR_BIAS = 36, CTRL_ERROR_MAX = 37, CTRL_ERROR_FLAGS = 38,
    CTRL_PRUNED_SLABS = 40,     // 64-bit counter of skipped 64-step slabs
    CTRL_WAIT_TICKS = 44,       // 64-bit counter: 10 ns ticks spent waiting for first-column rows
    CTRL_STRIPS_DONE = 48,      // strips [0, value) complete
    CTRL_GBEST = 52,            // running global best (the running kernel family's T domain), -INF before the launch
    CTRL_GBEST_IDLE = 53,       // its never-written twin: stays at -INF (KernelArgs::gbest_in of a block-score pass)
    CTRL_STOP = 54,             // the first wavefront that sees the host's stop sets it
    CTRL_DEBUG = 56,            // 7 debug words (MI355SW_V_DEBUG_WORDS)
    CTRL_WORDS = 64, CTRL_BYTES = CTRL_WORDS * 4
};
// pinned host words (mi355sw_handle::h_pinned): the running kernel reads and writes them with system scope
enum PinnedWord {
    PIN_STRIPS_DONE = 0,        // kernel -> host
    PIN_FIRST_COL_READY = 16,   // host -> kernel: rows of a streamed first column that have arrived
    PIN_ABORT = 32,             // host -> kernel: stop
    PIN_ERROR = 48,             // kernel -> host: mirror of CTRL_ERROR | causes << 8, written before PIN_STRIPS_DONE moves past the failing strip
    PIN_BEST_HINT = 64,         // host -> kernel: a lower bound from outside (packed kernels' T domain)
    PIN_BEST_REPORT = 80,       // kernel -> host: running best as of the last completed strip (T domain)
    PIN_WORDS = 128, PIN_BYTES = PIN_WORDS * 4
};
// header of a column port (mi355sw_handle::in_port / out_port: xGMI boundary column), followed by the m + 1 cells of the column
enum PortWord {
    PORT_ROWS_READY = 0,        // rows of the column the upstream band has written
    PORT_BEST_FROM_LEFT = 16,   // running best pushed by the band on the left (T domain)
    PORT_BEST_OF_OWNER = 32,    // running best published by the port's owner, for the band on the left to read
    PORT_HEADER_WORDS = 64, PORT_HEADER_BYTES = PORT_HEADER_WORDS * 4
};
inline int* port_word(void* port, int word) { return (int*) port + word; }
inline int2* port_cells(void* port) { return (int2*) ((int*) port + PORT_HEADER_WORDS); }   // cell 0 = the corner

// mi355sw_handle::mix_first of a launch with ONE strip height (the ordinary kernels)
enum { NO_MIXED_LAUNCH = 0x7fffffff };

// Score domains.  The API and the borders carry H.  The packed kernels keep their running best, bounds and hints as
// T = H - GAP_OPEN (T_OFF in sw_kernel_pk16.inc), the int32 family as H - GAP_FIRST (GAP_FIRST in sw_kernel.hip).
// (X/CUDAligner.hpp:77-98: a gap of k cells costs GAP_OPEN + k * GAP_EXT.)
enum { GAP_OPEN = 3, GAP_EXT = 2, GAP_FIRST = GAP_OPEN + GAP_EXT };
template <typename S> inline S t_of_h(S h) { return h - GAP_OPEN; }
template <typename S> inline S h_of_t(S t) { return t + GAP_OPEN; }
inline int t32_of_t(int t) { return h_of_t(t) - GAP_FIRST; }

}  // namespace mi355sw

#endif
