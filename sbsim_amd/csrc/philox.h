// philox.h -- the counter-based generator the device generators share (generators.hip: occupancy, convection;
// episode_draw.h: the per-episode draws -- start temperatures, per-building parameters and materials, episode starts).
#ifndef SBSIM_AMD_PHILOX_H_
#define SBSIM_AMD_PHILOX_H_
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#elif !defined(__host__) // a host-only program built by a plain C++ compiler (episode_draw.h's users): the qualifiers mean nothing
#define __host__
#define __device__
#endif

#include <cstdint>

namespace sb {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten
// rounds of two 32x32 -> 64 multiplies on a 128-bit counter under a 64-bit key.
__host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

} // namespace sb

#endif // SBSIM_AMD_PHILOX_H_
