// telemetry.h -- a building scored against recorded zone temperatures (include/sbsim_amd.h states the table:
// sb_telemetry_attach), shared by the kernels that keep the scores (telemetry.hip: k_telemetry after k_post,
// k_telemetry_close in front of a reset) and by host programs: one sample, one step added to a running row, and the latch
// that closes an episode.  A scalar row is SB_TL_FIELDS doubles of one building, contiguous here (the kernels hold it
// in registers; the device tables are field-major).  The optional per-zone rows are reached through two strides, so that
// the same code walks a host program's [Z][4] block (zs = 4, ks = 1) and the device's [4][Z][B] table (zs = B,
// ks = Z * B, the pointer moved to the building).  Every operation is one IEEE double operation, one rounding each
// (-ffp-contract=off), in the order written here.
#ifndef SBSIM_AMD_TELEMETRY_H_
#define SBSIM_AMD_TELEMETRY_H_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "sbsim_amd.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#elif !defined(__host__) // a host-only program built by a plain C++ compiler: the qualifiers mean nothing
#define __host__
#define __device__
#endif

namespace sb {

constexpr int kTelemetryZoneFields = 4; // a zone's row: samples, sum_err, sum_abs_err, sum_sq_err

// NaN and finiteness from the bits: the library is built with -fno-honor-nans, under which a compiler may fold x != x.
__host__ __device__ inline uint64_t telemetry_bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u & 0x7fffffffffffffffull;
}
__host__ __device__ inline bool telemetry_is_nan(double x) { return telemetry_bits(x) > 0x7ff0000000000000ull; }
__host__ __device__ inline bool telemetry_is_inf(double x) { return telemetry_bits(x) == 0x7ff0000000000000ull; }

// The row of a building that starts episode `episode`: zeros; the maximum, its row and its zone at -1 (no sample yet:
// the first sample's |e| >= 0 is strictly larger, so it always becomes the maximum).
__host__ __device__ inline void telemetry_init(double (&row)[SB_TL_FIELDS], double episode) {
#pragma unroll
  for (int k = 0; k < SB_TL_FIELDS; ++k) row[k] = 0.0;
  row[SB_TL_EPISODE] = episode;
  row[SB_TL_MAX_ABS_ERR] = -1.0;
  row[SB_TL_MAX_ABS_ROW] = -1.0;
  row[SB_TL_MAX_ABS_ZONE] = -1.0;
}

// One zone of one step: `sim` the simulated post-update zone mean, `obs` the recorded one (NaN: no sample), `w` the
// zone's weight, `r` the trace row, `zrow` the zone's per-zone row (NULL: none kept) with its fields `ks` apart.
// A simulated mean that is not finite is a sample: it goes into the sums (a NaN |e| never becomes the maximum).
__host__ __device__ inline void telemetry_sample(double (&row)[SB_TL_FIELDS], double *zrow, size_t ks, int z, double sim, double obs,
                                                 double w, double r) {
  if (telemetry_is_nan(obs)) {
    row[SB_TL_MISSING] += 1.0;
    return;
  }
  const double e = sim - obs;
  const double a = fabs(e);
  const double q = e * e;
  row[SB_TL_SAMPLES] += 1.0;
  row[SB_TL_SUM_ERR] += e;
  row[SB_TL_SUM_ABS_ERR] += a;
  row[SB_TL_SUM_SQ_ERR] += q;
  if (a > row[SB_TL_MAX_ABS_ERR]) {
    row[SB_TL_MAX_ABS_ERR] = a;
    row[SB_TL_MAX_ABS_ROW] = r;
    row[SB_TL_MAX_ABS_ZONE] = (double)z;
  }
  row[SB_TL_WEIGHTED_ABS_ERR] += w * a;
  row[SB_TL_WEIGHTED_SQ_ERR] += w * q;
  row[SB_TL_WEIGHT_SUM] += w;
  if (zrow) {
    zrow[0] += 1.0;
    zrow[ks] += e;
    zrow[2 * ks] += a;
    zrow[3 * ks] += q;
  }
}

// The step's head: one more step; a row past the end of the trace (trace_row NULL) counts Z missing samples and reads
// nothing.  Returns whether there is a row to walk.
__host__ __device__ inline bool telemetry_begin(double (&row)[SB_TL_FIELDS], const double *trace_row, int Z) {
  row[SB_TL_STEPS] += 1.0;
  if (!trace_row) row[SB_TL_MISSING] += (double)Z;
  return trace_row != nullptr;
}

// One step: `zmean` the building's Z post-update zone means, `trace_row` the Z recorded values of trace row `r` (NULL:
// the row lies at or beyond n_rows), `weights` the Z zone weights; `zone` the building's per-zone rows or NULL, zone z's
// field k at zone[z * zs + k * ks].  Zones in the order 0 .. Z-1.
__host__ __device__ inline void telemetry_step(double (&row)[SB_TL_FIELDS], double *zone, size_t zs, size_t ks, const double *zmean,
                                               const double *trace_row, double r, const double *weights, int Z) {
  if (!telemetry_begin(row, trace_row, Z)) return;
  for (int z = 0; z < Z; ++z) telemetry_sample(row, zone ? zone + (size_t)z * zs : nullptr, ks, z, zmean[z], trace_row[z], weights[z], r);
}

// The trace row a building with `steps` steps since its reset is scored on next, and the one sb_telemetry_actions hands
// out: past the end of the recording, the LAST row's setpoints (the scores count those steps as missing).
// (A step count put there by sb_telemetry_set may be anything: a row that is negative or NaN is outside the trace too,
// and its setpoints are row 0's / the last row's.)
__host__ __device__ inline double telemetry_row(int first_row, double steps) { return (double)first_row + steps; }
__host__ __device__ inline bool telemetry_in_trace(double r, int n_rows) { return r >= 0.0 && r < (double)n_rows; }
__host__ __device__ inline int telemetry_action_row(int first_row, double steps, int n_rows) {
  const double r = telemetry_row(first_row, steps);
  return r < (double)n_rows ? (r >= 0.0 ? (int)r : 0) : n_rows - 1;
}

// The latch in front of a reset, metrics_close's semantics.  A running row with at least one step is copied to
// `completed`, and `running` becomes the row of the next episode; returns whether it closed.  Without a step (the first
// reset, a second reset in a row) nothing closes and neither row changes.  The per-zone rows follow the same latch:
// where this returns true, telemetry_zone_close moves them.
__host__ __device__ inline bool telemetry_close(double (&running)[SB_TL_FIELDS], double (&completed)[SB_TL_FIELDS]) {
  if (!(running[SB_TL_STEPS] > 0.0)) return false;
#pragma unroll
  for (int k = 0; k < SB_TL_FIELDS; ++k) completed[k] = running[k];
  telemetry_init(running, running[SB_TL_EPISODE] + 1.0);
  return true;
}

__host__ __device__ inline void telemetry_zone_close(double *running, double *completed, size_t zs, size_t ks, int Z) {
  for (int z = 0; z < Z; ++z)
#pragma unroll
    for (int k = 0; k < kTelemetryZoneFields; ++k) {
      const size_t i = (size_t)z * zs + (size_t)k * ks;
      completed[i] = running[i];
      running[i] = 0.0;
    }
}

} // namespace sb

#endif // SBSIM_AMD_TELEMETRY_H_
