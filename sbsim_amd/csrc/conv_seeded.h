// conv_seeded.h -- the reference's SEEDED convection shuffle, draw for draw: Python's random.Random(seed) consumed the way
// StochasticConvectionSimulator consumes it (stochastic_convection_simulator.py:78-145).  Shared by the host (seeding,
// the stand-alone known-answer program of tests/test_convection_seeded_cpu.py) and the device (conv_seeded.hip): no HIP
// runtime call, a plain host compiler takes it too.
//
// The generator is MT19937 (Matsumoto & Nishimura 1998) as CPython's _randommodule.c drives it; the consumers are
// CPython 3.10's random.py: random(), _randbelow_with_getrandbits(), shuffle().  They are templates over a WORD SOURCE
// `Src` with `uint32_t next()` (the next tempered 32-bit word): MtHost below, or the kernel's LDS-resident block.
#ifndef SBSIM_AMD_CONV_SEEDED_H_
#define SBSIM_AMD_CONV_SEEDED_H_
#include <stdint.h>

#if defined(__HIPCC__)
#define SBC_HD __host__ __device__
#else
#define SBC_HD
#endif

namespace sbconv {

constexpr int kMtN = 624, kMtM = 397;
constexpr int kRngWords = kMtN + 1; // a building's row of the generator table: the block, then the index of the next word
constexpr uint32_t kMtMatrix = 0x9908b0dfu, kMtUpper = 0x80000000u, kMtLower = 0x7fffffffu;

// One word of the block regeneration: the new mt[k] from mt[k], mt[k + 1] and mt[k + 397] (indices modulo 624).  Words
// 0..226 read only old values; 227..623 read the NEW mt[k - 227], and 623 the new mt[0]: in increasing k the update is
// in place, and any run of at most 227 consecutive k can be formed from reads made before the run's first write.
SBC_HD inline uint32_t mt_twist(uint32_t cur, uint32_t nxt, uint32_t far) {
  const uint32_t y = (cur & kMtUpper) | (nxt & kMtLower);
  return far ^ (y >> 1) ^ ((y & 1u) ? kMtMatrix : 0u);
}
SBC_HD inline uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// ---- seeding (host only): random.seed(int) = init_by_array over the 32-bit little-endian words of |seed|, at least one
// (_randommodule.c random_seed, init_by_array); afterwards the index is 624: the first draw regenerates the block
inline void mt_init_genrand(uint32_t *mt, uint32_t s) {
  mt[0] = s;
  for (int i = 1; i < kMtN; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}
inline void mt_seed_python(uint32_t *row /* [kRngWords] */, uint64_t seed) {
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const int key_len = key[1] ? 2 : 1;
  uint32_t *mt = row;
  mt_init_genrand(mt, 19650218u);
  int i = 1, j = 0;
  for (int k = kMtN > key_len ? kMtN : key_len; k; --k) {
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
    ++i; ++j;
    if (i >= kMtN) { mt[0] = mt[kMtN - 1]; i = 1; }
    if (j >= key_len) j = 0;
  }
  for (int k = kMtN - 1; k; --k) {
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
    ++i;
    if (i >= kMtN) { mt[0] = mt[kMtN - 1]; i = 1; }
  }
  mt[0] = 0x80000000u;
  row[kMtN] = (uint32_t)kMtN;
}

// A generator row on the host: the word source of the known-answer program.
struct MtHost {
  uint32_t row[kRngWords];
  explicit MtHost(uint64_t seed) { mt_seed_python(row, seed); }
  uint32_t next() {
    if (row[kMtN] >= (uint32_t)kMtN) { // (a stored index above 624 counts as 624)
      for (int k = 0; k < kMtN; ++k) row[k] = mt_twist(row[k], row[(k + 1) % kMtN], row[(k + kMtM) % kMtN]);
      row[kMtN] = 0;
    }
    return mt_temper(row[row[kMtN]++]);
  }
};

// ---- the consumers
// random.random(): two words, 27 + 26 bits (_randommodule.c random_random); uniform(0, 1) = 0 + (1 - 0) * random()
template <class Src>
SBC_HD inline double uniform01(Src &s) {
  const uint32_t a = s.next() >> 5;
  const uint32_t b = s.next() >> 6;
  return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}
// Random._randbelow_with_getrandbits(n), n >= 1: k = n.bit_length(); getrandbits(k) until the value is below n.  n == 1
// draws too (k = 1), until it gets a 0.
template <class Src>
SBC_HD inline uint32_t randbelow(Src &s, uint32_t n) {
  const int shift = __builtin_clz(n); // 32 - bit_length(n)
  uint32_t r;
  do r = s.next() >> shift; while (r >= n);
  return r;
}
// Random.shuffle(x): for i = len - 1 .. 1: j = randbelow(i + 1); x[i], x[j] = x[j], x[i].  0 or 1 entries: no draw.
template <class Src, class Arr>
SBC_HD inline void shuffle(Src &s, Arr x, int len) {
  for (int i = len - 1; i >= 1; --i) {
    const uint32_t j = randbelow(s, (uint32_t)i + 1u);
    const auto t = x[i];
    x[i] = x[j];
    x[j] = t;
  }
}

// ---- one room pass, windowed (_shuffle_max_dist, :101-145).  The room's n cells in the caller's raster order; cnt[r]:
// how many in-room candidates cell r has inside the window (>= 1: the cell itself).  Per cell one uniform -- the cell
// moves unless it is > p -- and for a moving cell one randbelow(cnt[r]): the pick among its candidates in window raster
// order.  rec[k] <- cell << 16 | pick for the k-th moving cell; returns their number.  The caller resolves the picks to
// cells, shuffles the list (shuffle above) and applies the swaps in that order.
// A one-cell room consumes its draws like any other.
template <class Src, class Cnt, class Rec>
SBC_HD inline int room_draws(Src &s, int n, double p, Cnt cnt, Rec rec) {
  int m = 0;
  for (int r = 0; r < n; ++r) {
    if (uniform01(s) > p) continue;
    const uint32_t pick = randbelow(s, (uint32_t)cnt[r]);
    rec[m++] = ((uint32_t)r << 16) | pick;
  }
  return m;
}
// ... the swaps, one after the other: rec[k] = cell << 16 | other cell
template <class Rec, class Val>
SBC_HD inline void room_swaps(Rec rec, int m, Val val) {
  for (int k = 0; k < m; ++k) {
    const uint32_t w = rec[k], a = w >> 16, b = w & 0xffffu;
    const auto t = val[a];
    val[a] = val[b];
    val[b] = t;
  }
}
// The whole-room case (p == 1, distance == -1, :83-99) is shuffle() of order = 0 .. n - 1: the value of cell i goes to
// cell order[i].

} // namespace sbconv
#endif // SBSIM_AMD_CONV_SEEDED_H_
