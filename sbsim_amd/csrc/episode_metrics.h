// episode_metrics.h -- a building's episode totals (include/sbsim_amd.h states the table: sb_episode_metrics_attach),
// shared by the kernels that keep them (episode_metrics.hip: k_episode_metrics after k_post, k_episode_metrics_close in
// front of a reset) and by host programs: one step added to a running row, and the latch that closes an episode.
// A row is SB_EM_FIELDS doubles of one building, contiguous here (the kernels hold it in registers; the device tables
// are field-major).  Every sum is a double += of an fp32 value widened, one rounding per operation (-ffp-contract=off).
#ifndef SBSIM_AMD_EPISODE_METRICS_H_
#define SBSIM_AMD_EPISODE_METRICS_H_
#include <cmath>

#include "sbsim_amd.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#elif !defined(__host__) // a host-only program built by a plain C++ compiler: the qualifiers mean nothing
#define __host__
#define __device__
#endif

namespace sb {

// W s -> kWh (the reference's conversion_utils.py:173-213 divides by 3600 and by 1000)
constexpr double kMetricsKwh = 1.0 / 3600.0 / 1000.0;

// The row of a building that starts episode `episode`: zeros, the extremes at +inf / -inf.
__host__ __device__ inline void metrics_init(double (&row)[SB_EM_FIELDS], double episode) {
#pragma unroll
  for (int k = 0; k < SB_EM_FIELDS; ++k) row[k] = 0.0;
  row[SB_EM_EPISODE] = episode;
  row[SB_EM_ZONE_TEMP_MIN] = INFINITY;
  row[SB_EM_ZONE_TEMP_MAX] = -INFINITY;
}

// One step: `reward` as sb_step returned it (fp32; -inf: the request was rejected), `info` the building's
// [SB_INFO_STRIDE] row as k_post wrote it, `zmean` its Z post-update zone means, dt = sb_params.dt.
__host__ __device__ inline void metrics_step(double (&row)[SB_EM_FIELDS], float reward, const float *info, const double *zmean,
                                             int Z, double dt) {
  const bool rejected = reward == -INFINITY;
  row[SB_EM_STEPS] += 1.0;
  if (rejected) row[SB_EM_REJECTED_STEPS] += 1.0;
  row[SB_EM_RETURN] += (double)reward;
  if (!rejected) row[SB_EM_ACCEPTED_RETURN] += (double)reward;
  row[SB_EM_ELECTRICAL_ENERGY] += ((double)info[0] * dt * kMetricsKwh + (double)info[1] * dt * kMetricsKwh) + (double)info[3] * dt * kMetricsKwh;
  row[SB_EM_NATURAL_GAS_ENERGY] += (double)info[2] * dt * kMetricsKwh;
  row[SB_EM_ELECTRICITY_ENERGY_COST] += (double)info[9];
  row[SB_EM_NATURAL_GAS_ENERGY_COST] += (double)info[10];
  row[SB_EM_CARBON_EMITTED] += (double)info[11];
  row[SB_EM_TOTAL_OCCUPANCY] += (double)info[17];
  row[SB_EM_PRODUCTIVITY_REGRET] += (double)info[20];
  row[SB_EM_NORMALIZED_PRODUCTIVITY_REGRET] += (double)info[21];
  row[SB_EM_NORMALIZED_ENERGY_COST] += (double)info[22];
  row[SB_EM_NORMALIZED_CARBON_EMISSION] += (double)info[23];
  row[SB_EM_PRODUCTIVITY_REWARD] += (double)info[8];
  row[SB_EM_SWEEPS] += (double)info[4];
  if (info[5] == 0.0f) row[SB_EM_UNCONVERGED_STEPS] += 1.0;
  double lo = row[SB_EM_ZONE_TEMP_MIN], hi = row[SB_EM_ZONE_TEMP_MAX];
  for (int z = 0; z < Z; ++z) {
    const double t = zmean[z];
    lo = t < lo ? t : lo;
    hi = t > hi ? t : hi;
  }
  row[SB_EM_ZONE_TEMP_MIN] = lo;
  row[SB_EM_ZONE_TEMP_MAX] = hi;
}

// The latch in front of a reset.  A running row with at least one step is copied to `completed`, and `running` becomes
// the row of the next episode; returns whether it closed.  Without a step (the first reset, a second reset in a row)
// nothing closes and neither row changes.
__host__ __device__ inline bool metrics_close(double (&running)[SB_EM_FIELDS], double (&completed)[SB_EM_FIELDS]) {
  if (!(running[SB_EM_STEPS] > 0.0)) return false;
#pragma unroll
  for (int k = 0; k < SB_EM_FIELDS; ++k) completed[k] = running[k];
  metrics_init(running, running[SB_EM_EPISODE] + 1.0);
  return true;
}

} // namespace sb

#endif // SBSIM_AMD_EPISODE_METRICS_H_
