// step_stream_ms_cfg.h -- what the planner (planner.cpp, plan_stream) and step_stream_ms.hip (the experimental
// k_sweep_stream_ms) agree on.
#pragma once

#include "step_stream_cfg.h"

namespace sb {
namespace stream_ms {

#ifndef SB_STREAM_S
#define SB_STREAM_S 4
#endif
constexpr int kS = SB_STREAM_S; // sweeps per pass, at most
// LDS doubles of the seam rows (kS sweeps + the input grid's) and of the exchange area (progress words, max|delta| parts,
// publish scratch), W wavefronts, NS slots
constexpr int seam_doubles(int NS, int W) { return (kS + 1) * W * (NS + 8); }
constexpr int xchg_doubles(int W) { return 16 + kS * 16 + 64 * W; }

} // namespace stream_ms
} // namespace sb
