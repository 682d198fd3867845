// telemetry.hip -- sb_telemetry_attach: every building scored against recorded zone temperatures on the device
// (include/sbsim_amd.h states the table and the semantics; telemetry.h the arithmetic).  sb_step's POST phase launches
// k_telemetry behind k_post (behind k_episode_metrics where both are attached), a reset launches k_telemetry_close in
// front of its redraws and its reset kernel; both are stream-ordered launches on tables allocated at attach, so a
// captured step replays.
//
// Layout: the scalar tables are field-major, [SB_TL_FIELDS][B] doubles, the per-zone tables [SB_TL_ZONE_FIELDS][Z][B] --
// one thread owns one building, so the 64 lanes of a wavefront read and write 512 contiguous bytes of every field and of
// every zone's field.  The scalar row lives in registers between its loads and its stores; the zone loop walks the
// building's zone means, its trace row and the weights value by value (in 16-byte pairs where Z is even, which makes
// every row 16-byte aligned) and keeps no array indexed by the zone: no LDS, no scratch
// (profiles/telemetry_resource_usage.txt).  Buildings of a wavefront on the same trace and row read the same addresses;
// staggered buildings read rows of 8 Z bytes scattered over a recording that stays in L2.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (one rounding per operation: the sums are restated in NumPy).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "sb_host.h"
#include "telemetry.h"

using namespace sb;

namespace {

static_assert(SB_TL_ZONE_FIELDS == kTelemetryZoneFields, "the per-zone row of telemetry.h");

// One thread per building, the building the fast index of the tables.  The episode's index (field 0) does not change in
// a step: neither read nor written.  VEC: Z is even, so the three [.][Z] rows are 16-byte aligned; ZONE: per-zone tables.
template <bool VEC, bool ZONE>
__global__ void __launch_bounds__(kDrawThreads) k_telemetry(double *running, double *zone, const double *zmean, const double *traces,
                                                            const double *weights, const int *trace_of, const int *first_row, int B,
                                                            int Z, int n_rows) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    double row[SB_TL_FIELDS];
    row[SB_TL_EPISODE] = 0.0;
#pragma unroll
    for (int k = 1; k < SB_TL_FIELDS; ++k) row[k] = running[(size_t)k * B + b];
    const double r = telemetry_row(first_row[b], row[SB_TL_STEPS]);
    const double *tr = telemetry_in_trace(r, n_rows) ? traces + ((size_t)trace_of[b] * n_rows + (size_t)r) * Z : nullptr;
    const double *zm = zmean + (size_t)b * Z;
    double *zr = ZONE ? zone + b : nullptr;
    const size_t zs = (size_t)B, ks = (size_t)Z * B;
    if (telemetry_begin(row, tr, Z)) {
      if constexpr (VEC) {
        for (int z = 0; z < Z; z += 2) {
          const double2 s = *reinterpret_cast<const double2 *>(zm + z), o = *reinterpret_cast<const double2 *>(tr + z),
                        w = *reinterpret_cast<const double2 *>(weights + z);
          telemetry_sample(row, ZONE ? zr + (size_t)z * zs : nullptr, ks, z, s.x, o.x, w.x, r);
          telemetry_sample(row, ZONE ? zr + (size_t)(z + 1) * zs : nullptr, ks, z + 1, s.y, o.y, w.y, r);
        }
      } else {
        for (int z = 0; z < Z; ++z) telemetry_sample(row, ZONE ? zr + (size_t)z * zs : nullptr, ks, z, zm[z], tr[z], weights[z], r);
      }
    }
#pragma unroll
    for (int k = 1; k < SB_TL_FIELDS; ++k) running[(size_t)k * B + b] = row[k];
  }
}

// The latch: mask NULL -- every building.  A building outside the mask, or without a step, is not written.
__global__ void __launch_bounds__(kDrawThreads) k_telemetry_close(double *running, double *completed, double *zone_running,
                                                                  double *zone_completed, const uint8_t *mask, int B, int Z) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    if (mask && !mask[b]) continue;
    if (!(running[(size_t)SB_TL_STEPS * B + b] > 0.0)) continue;
    double row[SB_TL_FIELDS], done[SB_TL_FIELDS];
#pragma unroll
    for (int k = 0; k < SB_TL_FIELDS; ++k) row[k] = running[(size_t)k * B + b];
    telemetry_close(row, done);
#pragma unroll
    for (int k = 0; k < SB_TL_FIELDS; ++k) {
      completed[(size_t)k * B + b] = done[k];
      running[(size_t)k * B + b] = row[k];
    }
    if (zone_running) telemetry_zone_close(zone_running + b, zone_completed + b, (size_t)B, (size_t)Z * B, Z);
  }
}

// sb_telemetry_attach: running rows of episode 0; completed rows of episode -1 (none closed yet).
__global__ void __launch_bounds__(kDrawThreads) k_telemetry_init(double *running, double *completed, int B) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    double row[SB_TL_FIELDS], none[SB_TL_FIELDS];
    telemetry_init(row, 0.0);
    telemetry_init(none, -1.0);
#pragma unroll
    for (int k = 0; k < SB_TL_FIELDS; ++k) {
      running[(size_t)k * B + b] = row[k];
      completed[(size_t)k * B + b] = none[k];
    }
  }
}

// sb_telemetry_get / _set and _zone_get / _zone_set: the caller's building-major [B][M][K] from / into a table
// [K][M][B] (the scalar tables: M = 1, K = SB_TL_FIELDS; the per-zone tables: M = Z, K = SB_TL_ZONE_FIELDS).  One thread
// per value, the caller's array the fast index.
template <bool OUT>
__global__ void __launch_bounds__(kDrawThreads) k_telemetry_copy(double *table, double *rows, int B, int M, int K) {
  const size_t per = (size_t)M * K, n = (size_t)B * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / per, m = (i % per) / K, k = i % K;
    const size_t at = (k * M + m) * B + b;
    if constexpr (OUT) rows[i] = table[at];
    else table[at] = rows[i];
  }
}

// sb_telemetry_actions: one thread per value of the caller's [B][A]; `steps` is the running table's steps field.
__global__ void __launch_bounds__(kDrawThreads) k_telemetry_actions(float *out, const float *actions, const double *steps,
                                                                    const int *trace_of, const int *first_row, int B, int A, int n_rows) {
  const size_t n = (size_t)B * A;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / A, a = i % A;
    const int row = telemetry_action_row(first_row[b], steps[b], n_rows);
    out[i] = actions[((size_t)trace_of[b] * n_rows + row) * A + a];
  }
}

bool finite32(float x) { // (from the bits: -fno-honor-nans)
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}

const char *const kNoTelemetry = "the handle has no telemetry (sb_telemetry_attach)";

int telemetry_copy(sb_handle *h, const char *who, double *running_dev, double *completed_dev, bool zone, bool out, hipStream_t stream) {
  SB_CHECK(draws_attached(h, &sb_handle::tl_draws, who, kNoTelemetry, running_dev || completed_dev));
  if (zone && !h->tl_zone_running.p) return fail(SB_ERR_UNSUPPORTED, std::string(who) + ": the telemetry was attached without per_zone");
  SB_ON_DEVICE(h->device);
  const int B = h->d.B, M = zone ? h->d.Z : 1, K = zone ? SB_TL_ZONE_FIELDS : SB_TL_FIELDS;
  const dim3 grid(draw_blocks(h, (size_t)B * M * K)), block(kDrawThreads);
  double *const tabs[2] = {zone ? h->tl_zone_running.p : h->tl_running.p, zone ? h->tl_zone_completed.p : h->tl_completed.p};
  double *const rows[2] = {running_dev, completed_dev};
  for (int t = 0; t < 2; ++t) {
    if (!rows[t]) continue;
    if (out) hipLaunchKernelGGL(k_telemetry_copy<true>, grid, block, 0, stream, tabs[t], rows[t], B, M, K);
    else hipLaunchKernelGGL(k_telemetry_copy<false>, grid, block, 0, stream, tabs[t], rows[t], B, M, K);
  }
  SB_HIP(hipGetLastError());
  return SB_OK;
}

template <typename Tp>
void take(DevBuf<Tp> &into, DevBuf<Tp> &from) { // (the device is idle)
  drop(into);
  std::swap(into.p, from.p);
}

void drop_all(sb_handle *h) {
  drop(h->tl_running); drop(h->tl_completed); drop(h->tl_zone_running); drop(h->tl_zone_completed);
  drop(h->tl_traces); drop(h->tl_weights); drop(h->tl_actions); drop(h->tl_trace_of); drop(h->tl_first_row);
}

} // namespace

int sb_telemetry_step(sb_handle *h, hipStream_t stream) {
  const Dev &d = h->d;
  const dim3 grid(draw_blocks(h, (size_t)d.B)), block(kDrawThreads);
  const bool vec = d.Z % 2 == 0, zone = h->tl_zone_running.p != nullptr;
#define SB_TL_LAUNCH(V, Zn)                                                                                                   \
  hipLaunchKernelGGL((k_telemetry<V, Zn>), grid, block, 0, stream, h->tl_running.p, h->tl_zone_running.p, d.zmean, h->tl_traces.p, \
                     h->tl_weights.p, h->tl_trace_of.p, h->tl_first_row.p, d.B, d.Z, h->tl_n_rows)
  if (vec && zone) SB_TL_LAUNCH(true, true);
  else if (vec) SB_TL_LAUNCH(true, false);
  else if (zone) SB_TL_LAUNCH(false, true);
  else SB_TL_LAUNCH(false, false);
#undef SB_TL_LAUNCH
  SB_HIP(hipGetLastError());
  return SB_OK;
}

int sb_telemetry_close(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream) {
  hipLaunchKernelGGL(k_telemetry_close, dim3(draw_blocks(h, (size_t)h->d.B)), dim3(kDrawThreads), 0, stream, h->tl_running.p,
                     h->tl_completed.p, h->tl_zone_running.p, h->tl_zone_completed.p, mask_dev, h->d.B, h->d.Z);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

extern "C" {

int sb_telemetry_attach(sb_handle *h, const sb_telemetry *t) {
  const std::string who = "sb_telemetry_attach: ";
  if (!h || !t || !t->traces) return fail(SB_ERR_INVALID, who + "null argument");
  const size_t B = (size_t)h->d.B, Z = (size_t)h->d.Z;
  const int A = h->d.p.n_actions;
  if (t->n_traces < 1 || t->n_rows < 1) return fail(SB_ERR_INVALID, who + "n_traces and n_rows must be at least 1");
  const size_t rows = (size_t)t->n_traces * (size_t)t->n_rows;
  for (size_t i = 0; i < rows * Z; ++i)
    if (telemetry_is_inf(t->traces[i]))
      return fail(SB_ERR_INVALID, who + "trace " + std::to_string(i / Z / t->n_rows) + " row " + std::to_string(i / Z % t->n_rows) +
                                      " zone " + std::to_string(i % Z) + " is infinite (NaN is \"no sample\")");
  std::vector<int> trace_of(B, 0), first_row(B, 0);
  for (size_t b = 0; b < B; ++b) {
    if (t->trace_of) trace_of[b] = t->trace_of[b];
    if (t->first_row) first_row[b] = t->first_row[b];
    if (trace_of[b] < 0 || trace_of[b] >= t->n_traces)
      return fail(SB_ERR_INVALID, who + "building " + std::to_string(b) + ": trace_of " + std::to_string(trace_of[b]) + " is outside [0, " +
                                      std::to_string(t->n_traces) + ")");
    if (first_row[b] < 0 || first_row[b] >= t->n_rows)
      return fail(SB_ERR_INVALID, who + "building " + std::to_string(b) + ": first_row " + std::to_string(first_row[b]) + " is outside [0, " +
                                      std::to_string(t->n_rows) + ")");
  }
  std::vector<double> weights(Z, 1.0);
  for (size_t z = 0; z < Z && t->zone_weights; ++z) {
    weights[z] = t->zone_weights[z];
    if (telemetry_is_nan(weights[z]) || telemetry_is_inf(weights[z]) || weights[z] < 0.0)
      return fail(SB_ERR_INVALID, who + "zone_weights[" + std::to_string(z) + "] must be finite and >= 0");
  }
  if (t->actions) {
    if (t->n_actions != A)
      return fail(SB_ERR_INVALID, who + "n_actions is " + std::to_string(t->n_actions) + ", the handle's is " + std::to_string(A));
    for (size_t i = 0; i < rows * A; ++i)
      if (!finite32(t->actions[i]))
        return fail(SB_ERR_INVALID, who + "actions of trace " + std::to_string(i / A / t->n_rows) + " row " +
                                        std::to_string(i / A % t->n_rows) + " are not finite");
  }
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device(who));
  // everything new is built aside: a failure here leaves the attachment in force as it was
  DevBuf<double> running, completed, zone_running, zone_completed, traces, w;
  DevBuf<float> actions;
  DevBuf<int> tof, frow;
  SB_CHECK(alloc_zero(running, B * SB_TL_FIELDS));
  SB_CHECK(alloc_zero(completed, B * SB_TL_FIELDS));
  if (t->per_zone) {
    SB_CHECK(alloc_zero(zone_running, B * Z * SB_TL_ZONE_FIELDS));
    SB_CHECK(alloc_zero(zone_completed, B * Z * SB_TL_ZONE_FIELDS));
  }
  SB_CHECK(upload(traces, t->traces, rows * Z));
  SB_CHECK(upload(w, weights.data(), Z));
  if (t->actions) SB_CHECK(upload(actions, t->actions, rows * A));
  SB_CHECK(upload(tof, trace_of.data(), B));
  SB_CHECK(upload(frow, first_row.data(), B));
  hipLaunchKernelGGL(k_telemetry_init, dim3(draw_blocks(h, B)), dim3(kDrawThreads), 0, nullptr, running.p, completed.p, h->d.B);
  SB_HIP(hipGetLastError());
  SB_HIP(hipDeviceSynchronize());
  take(h->tl_running, running); take(h->tl_completed, completed);
  take(h->tl_zone_running, zone_running); take(h->tl_zone_completed, zone_completed);
  take(h->tl_traces, traces); take(h->tl_weights, w); take(h->tl_actions, actions);
  take(h->tl_trace_of, tof); take(h->tl_first_row, frow);
  h->tl_n_traces = t->n_traces;
  h->tl_n_rows = t->n_rows;
  h->tl_draws.attached = true;
  return SB_OK;
}

int sb_telemetry_detach(sb_handle *h) {
  const std::string who = "sb_telemetry_detach: ";
  if (!h) return fail(SB_ERR_INVALID, who + "null handle");
  if (!h->tl_draws.attached) return SB_OK;
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device(who));
  h->tl_draws.attached = false;
  drop_all(h);
  h->tl_n_traces = h->tl_n_rows = 0;
  return SB_OK;
}

int sb_telemetry_get(sb_handle *h, double *running_dev, double *completed_dev, void *stream) {
  return telemetry_copy(h, "sb_telemetry_get", running_dev, completed_dev, false, true, (hipStream_t)stream);
}

int sb_telemetry_set(sb_handle *h, const double *running_dev, const double *completed_dev, void *stream) {
  return telemetry_copy(h, "sb_telemetry_set", const_cast<double *>(running_dev), const_cast<double *>(completed_dev), false, false,
                        (hipStream_t)stream);
}

int sb_telemetry_zone_get(sb_handle *h, double *running_dev, double *completed_dev, void *stream) {
  return telemetry_copy(h, "sb_telemetry_zone_get", running_dev, completed_dev, true, true, (hipStream_t)stream);
}

int sb_telemetry_zone_set(sb_handle *h, const double *running_dev, const double *completed_dev, void *stream) {
  return telemetry_copy(h, "sb_telemetry_zone_set", const_cast<double *>(running_dev), const_cast<double *>(completed_dev), true, false,
                        (hipStream_t)stream);
}

int sb_telemetry_actions(sb_handle *h, float *actions_dev, void *stream) {
  const char *who = "sb_telemetry_actions";
  SB_CHECK(draws_attached(h, &sb_handle::tl_draws, who, kNoTelemetry, actions_dev != nullptr));
  if (!h->tl_actions.p) return fail(SB_ERR_UNSUPPORTED, std::string(who) + ": the telemetry was attached without an action table");
  SB_ON_DEVICE(h->device);
  const int B = h->d.B, A = h->d.p.n_actions;
  hipLaunchKernelGGL(k_telemetry_actions, dim3(draw_blocks(h, (size_t)B * A)), dim3(kDrawThreads), 0, (hipStream_t)stream, actions_dev,
                     h->tl_actions.p, h->tl_running.p + (size_t)SB_TL_STEPS * B, h->tl_trace_of.p, h->tl_first_row.p, B, A, h->tl_n_rows);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

} // extern "C"
