// step_stream_cfg.h -- what the planner (planner.cpp, plan_stream) and step_stream.hip (k_sweep_stream) agree on.
#pragma once

namespace sb {
namespace stream {

constexpr int kSets = 32;   // entries of the coefficient-set table (at LDS address 0)
#ifndef SB_STREAM_ZC
#define SB_STREAM_ZC 9
#endif
constexpr int kZC = SB_STREAM_ZC; // columns of the zone-sum scratch per zone (16 lane columns + 1: odd stride)
// k_sweep_stream_roll (experimental): the odd sweeps' max |delta| parts behind the publish scratch
constexpr int kRollXchgExtra = 16;

} // namespace stream
} // namespace sb
