// step_reg_cfg.h -- what the planner (planner.cpp, plan_reg) and step_reg.hip (k_sweep_reg) agree on.
#pragma once

namespace sb {
namespace reg {

constexpr int kPair = 2; // template parameter P: 1 = one wavefront per building, kPair = two
// The instantiations (NR, P): step_reg.hip builds its dispatch table from this list
// (tail rows, overlapped sweeps: k_sweep_roll, step_roll.hip)
#define SB_REG_VARIANTS(X) X(32, 1) X(66, 1) X(66, 2) X(96, 1) X(96, 2)
constexpr bool supported(int NR, int P) {
#define SB_REG_IS(nr, p) || (NR == nr && P == p)
  return false SB_REG_VARIANTS(SB_REG_IS);
#undef SB_REG_IS
}

// Slots of A = ap*Tprev + g kept in LDS; the remaining NR - lds_slots live in registers
// (AGPRs).  96-slot plans on one wavefront: 71 of 96 slots in LDS make a building fit a
// quarter of a CU's LDS, so all four SIMDs own a building instead of three.
// The 96-slot two-wavefront variant (up to 128 x 96 cells) keeps 89 slots in LDS: two buildings
// per CU (it runs one wavefront per SIMD: 192 registers of grid + the rest do not fit twice).
constexpr int lds_slots(int NR, int P) {
  return (NR == 96 && P != kPair) ? 71 : ((NR == 96 && P == kPair) ? 89 : NR);
}
constexpr int waves_per_simd(int NR, int P) { return (P == kPair && NR <= 66) ? 2 : 1; }
// Coefficient-table stride: classes + the pad class <= stride.  The class maps hold
// class * (256 / stride) in a byte; times stride / 32 that is the class's byte offset into a
// table column (stride 32: the byte IS the offset, one SDWA add per step).
constexpr int table_stride(int NR, int P) { return (NR == 96 && P == 2) ? 64 : 32; }
constexpr int kSeamPad = 8;

} // namespace reg
} // namespace sb
