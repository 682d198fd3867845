// episode_starts.h -- the draw of sb_episode_starts_attach (include/sbsim_amd.h states the formula), shared by
// k_episode_starts (episode_starts.hip) and by host programs: one Philox block per (building, episode, field).
#ifndef SBSIM_AMD_EPISODE_STARTS_H_
#define SBSIM_AMD_EPISODE_STARTS_H_
#include <cstdint>

#include "randomize.h"

namespace sb {

// One field of a start as the kernel reads it (by value, in its arguments).  d.id is the sb_start_field_id, d.kind a
// sb_rand_kind; SB_RAND_UNIFORM_INT keeps its integers here.
struct StartField {
  RandField d;     // SB_RAND_UNIFORM / SB_RAND_CHOICE: rand_of_block's descriptor (choice_off into the starts' own table)
  int32_t present; // 1: the field is drawn; 2: every reset writes its base value (episode_starts.hip); 0: untouched
  int32_t ilo;     // SB_RAND_UNIFORM_INT: lo ...
  int32_t step;    // ... step ...
  int32_t k;       // ... and K = (hi - lo) / step + 1 <= 2^22
};

// The field's Philox block for global building gb in its episode e.
__host__ __device__ inline void start_block(uint32_t (&c)[4], int id, uint64_t seed, uint64_t gb, uint32_t e) {
  c[0] = (uint32_t)gb; c[1] = (uint32_t)(gb >> 32); c[2] = e; c[3] = SB_EPISODE_STARTS_TAG | (uint32_t)id;
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// A weather field's draw (SB_RAND_UNIFORM / SB_RAND_CHOICE).
__host__ __device__ inline double start_draw(const StartField &f, const double *choices, uint64_t seed, uint64_t gb, uint32_t e) {
  uint32_t c[4];
  start_block(c, f.d.id, seed, gb, e);
  return rand_of_block(f.d, choices, c);
}

// The offset's draw, in rows: SB_RAND_UNIFORM_INT in integers only; SB_RAND_CHOICE one of the table's whole numbers.
__host__ __device__ inline int start_offset_draw(const StartField &f, const double *choices, uint64_t seed, uint64_t gb, uint32_t e) {
  uint32_t c[4];
  start_block(c, f.d.id, seed, gb, e);
  if (f.d.kind == SB_RAND_UNIFORM_INT) return f.ilo + f.step * (int)(((uint64_t)c[0] * (uint64_t)f.k) >> 32);
  return (int)rand_of_block(f.d, choices, c);
}

} // namespace sb

#endif // SBSIM_AMD_EPISODE_STARTS_H_
