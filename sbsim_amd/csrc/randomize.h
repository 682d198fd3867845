// randomize.h -- the draw of sb_randomization_attach (include/sbsim_amd.h states the formula), shared by k_randomize
// (randomize.hip) and by host programs: one Philox block per (building, episode, field).
#ifndef SBSIM_AMD_RANDOMIZE_H_
#define SBSIM_AMD_RANDOMIZE_H_
#include <cstdint>

#include "philox.h"
#include "sbsim_amd.h"

namespace sb {

// One randomised field as the kernel reads it; the choice tables follow the descriptors in the same device buffer.
struct RandField {
  int32_t id;         // sb_rand_field::id: the draw's counter word is SB_RANDOMIZATION_TAG | id
  int32_t row;        // the field's row of its table: k of [SB_NUM_BUILDING_PARAMS][B], f of [3 M + 1][B]
  int32_t material;   // != 0: the materials' table
  int32_t kind;       // sb_rand_kind
  int32_t scale;      // != 0: value = base * d
  int32_t choice_off; // SB_RAND_CHOICE: first entry in the choice tables
  int32_t choice_len; // ... and K
  int32_t pad;
  double lo, hi;      // SB_RAND_UNIFORM
};

// d of field `f` from the four words of its Philox block (SB_RAND_UNIFORM / SB_RAND_CHOICE; episode_starts.h draws with
// the same formulas under its own tag).  choices: the concatenated choice tables.
__host__ __device__ inline double rand_of_block(const RandField &f, const double *choices, const uint32_t c[4]) {
  if (f.kind == SB_RAND_CHOICE) return choices[f.choice_off + (int)(((uint64_t)c[0] * (uint64_t)f.choice_len) >> 32)];
  const uint64_t r = ((uint64_t)c[1] << 32) | c[0];
  return f.lo + (f.hi - f.lo) * ((double)(r >> 11) * 0x1p-53);
}

// d of field `f` for global building gb in its episode e.
__host__ __device__ inline double rand_draw(const RandField &f, const double *choices, uint64_t seed, uint64_t gb, uint32_t e) {
  uint32_t c[4] = {(uint32_t)gb, (uint32_t)(gb >> 32), e, SB_RANDOMIZATION_TAG | (uint32_t)f.id};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return rand_of_block(f, choices, c);
}

// The field's value from its draw and the building's base row.
__host__ __device__ inline double rand_value(const RandField &f, double d, double base) { return f.scale ? base * d : d; }

} // namespace sb

#endif // SBSIM_AMD_RANDOMIZE_H_
