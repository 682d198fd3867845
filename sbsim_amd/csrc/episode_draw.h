// episode_draw.h -- the draws at the start of a building's episode (include/sbsim_amd.h states the formulas), shared by the
// kernels that draw (runtime.hip: the start temperatures' jitter; randomize.hip: k_randomize; episode_starts.hip:
// k_episode_starts) and by host programs: one Philox block per (building, episode, tag | field), and a building's
// episode counter.
#ifndef SBSIM_AMD_EPISODE_DRAW_H_
#define SBSIM_AMD_EPISODE_DRAW_H_
#include <cstdint>

#include "philox.h"
#include "sbsim_amd.h"

namespace sb {

// ---- a building's episode counter: the number of its NEXT episode, 0 at attach ----
// The counter after a reset that drew episode e.
__host__ __device__ inline int next_episode(int e) { return (int)((unsigned)e + 1u); }
// The episode in force for counter t: the one the building's last reset drew, t - 1 ...
__host__ __device__ inline int episode_in_force(int t) { return t - 1; }
// ... and whether there is none yet (t < 1: no reset since the attach): the base values are in force.
__host__ __device__ inline bool before_first_episode(int t) { return t < 1; }

// ---- one block, and a value from its words ----
// The block of global building gb in its episode e under `tag_word` (an attachment's tag | the field's id).
__host__ __device__ inline void episode_block(uint32_t (&c)[4], uint32_t tag_word, uint64_t seed, uint64_t gb, uint32_t e) {
  c[0] = (uint32_t)gb; c[1] = (uint32_t)(gb >> 32); c[2] = e; c[3] = tag_word;
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// lo + (hi - lo) * u, u the 53-bit uniform of the block's first two words.
__host__ __device__ inline double uniform_of_block(double lo, double hi, const uint32_t c[4]) {
  const uint64_t r = ((uint64_t)c[1] << 32) | c[0];
  return lo + (hi - lo) * ((double)(r >> 11) * 0x1p-53);
}

// One of k equally likely indices from the block's first word, in integers only.
__host__ __device__ inline int index_of_block(int k, const uint32_t c[4]) { return (int)(((uint64_t)c[0] * (uint64_t)k) >> 32); }

__host__ __device__ inline double choice_of_block(const double *choices, int off, int k, const uint32_t c[4]) {
  return choices[off + index_of_block(k, c)];
}

__host__ __device__ inline int uniform_int_of_block(int ilo, int step, int k, const uint32_t c[4]) {
  return ilo + step * index_of_block(k, c);
}

// ---- sb_initial_conditions_attach: the jitter u(b, e) ----
__host__ __device__ inline double initial_conditions_draw(double lo, double hi, uint64_t seed, uint64_t gb, uint32_t e) {
  uint32_t c[4];
  episode_block(c, SB_INITIAL_CONDITIONS_TAG, seed, gb, e);
  return uniform_of_block(lo, hi, c);
}

// ---- sb_randomization_attach ----
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

// d of field `f` from the four words of its block (SB_RAND_UNIFORM / SB_RAND_CHOICE).  choices: the concatenated choice
// tables.
__host__ __device__ inline double rand_of_block(const RandField &f, const double *choices, const uint32_t c[4]) {
  if (f.kind == SB_RAND_CHOICE) return choice_of_block(choices, f.choice_off, f.choice_len, c);
  return uniform_of_block(f.lo, f.hi, c);
}

// d of field `f` for global building gb in its episode e.
__host__ __device__ inline double rand_draw(const RandField &f, const double *choices, uint64_t seed, uint64_t gb, uint32_t e) {
  uint32_t c[4];
  episode_block(c, SB_RANDOMIZATION_TAG | (uint32_t)f.id, seed, gb, e);
  return rand_of_block(f, choices, c);
}

// The field's value from its draw and the building's base row.
__host__ __device__ inline double rand_value(const RandField &f, double d, double base) { return f.scale ? base * d : d; }

// ---- sb_episode_starts_attach ----
// One field of a start as the kernel reads it (by value, in its arguments).  d.id is the sb_start_field_id, d.kind a
// sb_rand_kind; SB_RAND_UNIFORM_INT keeps its integers here.
struct StartField {
  RandField d;     // SB_RAND_UNIFORM / SB_RAND_CHOICE: rand_of_block's descriptor (choice_off into the starts' own table)
  int32_t present; // 1: the field is drawn; 2: every reset writes its base value (episode_starts.hip); 0: untouched
  int32_t ilo;     // SB_RAND_UNIFORM_INT: lo ...
  int32_t step;    // ... step ...
  int32_t k;       // ... and K = (hi - lo) / step + 1 <= 2^22
};

// A weather field's draw (SB_RAND_UNIFORM / SB_RAND_CHOICE).
__host__ __device__ inline double start_draw(const StartField &f, const double *choices, uint64_t seed, uint64_t gb, uint32_t e) {
  uint32_t c[4];
  episode_block(c, SB_EPISODE_STARTS_TAG | (uint32_t)f.d.id, seed, gb, e);
  return rand_of_block(f.d, choices, c);
}

// The offset's draw, in rows: SB_RAND_UNIFORM_INT in integers only; SB_RAND_CHOICE one of the table's whole numbers.
__host__ __device__ inline int start_offset_draw(const StartField &f, const double *choices, uint64_t seed, uint64_t gb, uint32_t e) {
  uint32_t c[4];
  episode_block(c, SB_EPISODE_STARTS_TAG | (uint32_t)f.d.id, seed, gb, e);
  if (f.d.kind == SB_RAND_UNIFORM_INT) return uniform_int_of_block(f.ilo, f.step, f.k, c);
  return (int)rand_of_block(f.d, choices, c);
}

} // namespace sb

#endif // SBSIM_AMD_EPISODE_DRAW_H_
