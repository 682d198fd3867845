// step_roll_cfg.h -- what the planner (planner.cpp, plan_roll) and step_roll.hip (k_sweep_roll) agree on.
#pragma once

namespace sb {
namespace roll {

constexpr int kSlotCounts[] = {64, 72, 80, 88, 96}; // the instantiations
// Slots of A = ap*Tprev + g kept in LDS (the rest: registers).  72 of 96: a building needs 38.2 KB of
// LDS, so four buildings -- one per SIMD -- and the shared tables (7 KB) fill a CU's 160 KB.  Rows of
// 70 slots (the stride is 2 mod 4 doubles: rows are 16-byte aligned and 16 lanes' ds_read_b128 cover
// all banks) and a second array [64][2] with slots 70, 71 (a stride of 72 would be four-way conflicted,
// 74 does not fit).  NR = 72, 80, 88: the same 70 + 2 slots in LDS (NR - 72 in registers); NR = 64: all of them,
// rows of 66.
constexpr int lds_slots(int NR) { return NR >= 72 ? 72 : ((NR / 2) % 2 ? NR : NR + 2); }
constexpr int a_stride(int NR) { return NR >= 72 ? 70 : ((NR / 2) % 2 ? NR : NR + 2); }
constexpr int kWaves = 4;     // wavefronts = buildings per workgroup
constexpr int tail_row(int NR) { return NR + 4; } // tail rows in LDS: column c at [2 + c], zero guards around
// LDS doubles of the tail scan's static multipliers, shared by the workgroup (sweep_common.h, tail_pass_static)
constexpr int tail_mul_doubles(int NR, int T) { return T > 0 ? (4 * T + 2) * (NR / 2) : 0; }

} // namespace roll
} // namespace sb
