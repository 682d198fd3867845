// episode_metrics.hip -- sb_episode_metrics_attach: every building's episode totals on the device (include/sbsim_amd.h
// states the table and the semantics; episode_metrics.h the arithmetic).  sb_step's POST phase launches
// k_episode_metrics behind k_post, a reset launches k_episode_metrics_close in front of its redraws and its reset kernel;
// both are stream-ordered launches on tables allocated at attach, so a captured step replays.
//
// Layout: both tables are field-major, [SB_EM_FIELDS][B] doubles -- one thread owns one building, so the 64 lanes of a
// wavefront read and write 512 contiguous bytes of every field.  The building's 96-byte info row is read in 16-byte
// pieces (the piece of columns 12..15 holds nothing the table sums and is not read); the row lives in registers between
// its loads and its stores: no LDS, no scratch (profiles/episode_metrics_resource_usage.txt).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (one rounding per operation: the sums are restated in NumPy).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "episode_metrics.h"
#include "sb_host.h"

using namespace sb;

namespace {

static_assert(SB_INFO_STRIDE == 24, "k_episode_metrics reads the info row as six 16-byte pieces");

// The building's info row in registers.  VEC: the caller's buffer is 16-byte aligned (rows are 96 bytes apart).
template <bool VEC>
__device__ inline void load_info(float (&I)[SB_INFO_STRIDE], const float *info, size_t b) {
  const float *row = info + b * SB_INFO_STRIDE;
  if constexpr (VEC) {
    const float4 *q = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int k = 0; k < SB_INFO_STRIDE / 4; ++k) {
      if (k == 3) continue; // columns 12..15: carbon_cost and the three weights
      const float4 v = q[k];
      I[4 * k] = v.x; I[4 * k + 1] = v.y; I[4 * k + 2] = v.z; I[4 * k + 3] = v.w;
    }
    I[12] = I[13] = I[14] = I[15] = 0.0f;
  } else {
#pragma unroll
    for (int k = 0; k < SB_INFO_STRIDE; ++k) I[k] = row[k];
  }
}

// One thread per building, the building the fast index of the table.  The episode's index (field 0) does not change in
// a step: neither read nor written.
template <bool VEC>
__global__ void __launch_bounds__(kDrawThreads) k_episode_metrics(double *running, const float *reward, const float *info,
                                                                  const double *zmean, int B, int Z, double dt) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    double row[SB_EM_FIELDS];
    float I[SB_INFO_STRIDE];
    row[SB_EM_EPISODE] = 0.0;
#pragma unroll
    for (int k = 1; k < SB_EM_FIELDS; ++k) row[k] = running[(size_t)k * B + b];
    load_info<VEC>(I, info, (size_t)b);
    metrics_step(row, reward[b], I, zmean + (size_t)b * Z, Z, dt);
#pragma unroll
    for (int k = 1; k < SB_EM_FIELDS; ++k) running[(size_t)k * B + b] = row[k];
  }
}

// The latch: mask NULL -- every building.  A building outside the mask, or without a step, is not written.
__global__ void __launch_bounds__(kDrawThreads) k_episode_metrics_close(double *running, double *completed, const uint8_t *mask, int B) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    if (mask && !mask[b]) continue;
    if (!(running[(size_t)SB_EM_STEPS * B + b] > 0.0)) continue;
    double row[SB_EM_FIELDS], done[SB_EM_FIELDS];
#pragma unroll
    for (int k = 0; k < SB_EM_FIELDS; ++k) row[k] = running[(size_t)k * B + b];
    metrics_close(row, done);
#pragma unroll
    for (int k = 0; k < SB_EM_FIELDS; ++k) {
      completed[(size_t)k * B + b] = done[k];
      running[(size_t)k * B + b] = row[k];
    }
  }
}

// sb_episode_metrics_attach: running rows of episode 0; completed rows of episode -1 (none closed yet).
__global__ void __launch_bounds__(kDrawThreads) k_episode_metrics_init(double *running, double *completed, int B) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    double row[SB_EM_FIELDS], none[SB_EM_FIELDS];
    metrics_init(row, 0.0);
    metrics_init(none, -1.0);
#pragma unroll
    for (int k = 0; k < SB_EM_FIELDS; ++k) {
      running[(size_t)k * B + b] = row[k];
      completed[(size_t)k * B + b] = none[k];
    }
  }
}

// sb_episode_metrics_get / _set: the caller's building-major [B][SB_EM_FIELDS] from / into a field-major table.  One
// thread per value, the caller's array the fast index.
template <bool OUT>
__global__ void __launch_bounds__(kDrawThreads) k_episode_metrics_copy(double *table, double *rows, int B) {
  const size_t n = (size_t)B * SB_EM_FIELDS;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / SB_EM_FIELDS, k = i % SB_EM_FIELDS;
    if constexpr (OUT) rows[i] = table[k * B + b];
    else table[k * B + b] = rows[i];
  }
}

const char *const kNoMetrics = "the handle has no episode metrics (sb_episode_metrics_attach)";

int metrics_copy(sb_handle *h, const char *who, double *running_dev, double *completed_dev, bool out, hipStream_t stream) {
  SB_CHECK(draws_attached(h, &sb_handle::em_draws, who, kNoMetrics, running_dev || completed_dev));
  SB_ON_DEVICE(h->device);
  const int B = h->d.B;
  const dim3 grid(draw_blocks(h, (size_t)B * SB_EM_FIELDS)), block(kDrawThreads);
  double *const tabs[2] = {h->em_running.p, h->em_completed.p}, *const rows[2] = {running_dev, completed_dev};
  for (int t = 0; t < 2; ++t) {
    if (!rows[t]) continue;
    if (out) hipLaunchKernelGGL(k_episode_metrics_copy<true>, grid, block, 0, stream, tabs[t], rows[t], B);
    else hipLaunchKernelGGL(k_episode_metrics_copy<false>, grid, block, 0, stream, tabs[t], rows[t], B);
  }
  SB_HIP(hipGetLastError());
  return SB_OK;
}

} // namespace

int sb_episode_metrics_step(sb_handle *h, const float *reward_dev, const float *info_dev, hipStream_t stream) {
  const Dev &d = h->d;
  const dim3 grid(draw_blocks(h, (size_t)d.B)), block(kDrawThreads);
  if (((uintptr_t)info_dev & 15u) == 0)
    hipLaunchKernelGGL(k_episode_metrics<true>, grid, block, 0, stream, h->em_running.p, reward_dev, info_dev, d.zmean, d.B, d.Z, d.p.dt);
  else
    hipLaunchKernelGGL(k_episode_metrics<false>, grid, block, 0, stream, h->em_running.p, reward_dev, info_dev, d.zmean, d.B, d.Z, d.p.dt);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

int sb_episode_metrics_close(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream) {
  hipLaunchKernelGGL(k_episode_metrics_close, dim3(draw_blocks(h, (size_t)h->d.B)), dim3(kDrawThreads), 0, stream,
                     h->em_running.p, h->em_completed.p, mask_dev, h->d.B);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

extern "C" {

int sb_episode_metrics_attach(sb_handle *h) {
  const std::string who = "sb_episode_metrics_attach: ";
  if (!h) return fail(SB_ERR_INVALID, who + "null handle");
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device(who));
  const size_t B = (size_t)h->d.B;
  if (!h->em_draws.attached) {
    drop(h->em_running); drop(h->em_completed); drop(h->em_info);
    SB_CHECK(alloc_zero(h->em_running, B * SB_EM_FIELDS));
    SB_CHECK(alloc_zero(h->em_completed, B * SB_EM_FIELDS));
    SB_CHECK(alloc_zero(h->em_info, B * SB_INFO_STRIDE)); // k_post's info rows when the caller passes none
  }
  hipLaunchKernelGGL(k_episode_metrics_init, dim3(draw_blocks(h, B)), dim3(kDrawThreads), 0, nullptr, h->em_running.p,
                     h->em_completed.p, h->d.B);
  SB_HIP(hipGetLastError());
  SB_HIP(hipDeviceSynchronize());
  h->em_draws.attached = true;
  return SB_OK;
}

int sb_episode_metrics_detach(sb_handle *h) {
  const std::string who = "sb_episode_metrics_detach: ";
  if (!h) return fail(SB_ERR_INVALID, who + "null handle");
  if (!h->em_draws.attached) return SB_OK;
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device(who));
  h->em_draws.attached = false;
  drop(h->em_running); drop(h->em_completed); drop(h->em_info);
  return SB_OK;
}

int sb_episode_metrics_get(sb_handle *h, double *running_dev, double *completed_dev, void *stream) {
  return metrics_copy(h, "sb_episode_metrics_get", running_dev, completed_dev, true, (hipStream_t)stream);
}

int sb_episode_metrics_set(sb_handle *h, const double *running_dev, const double *completed_dev, void *stream) {
  return metrics_copy(h, "sb_episode_metrics_set", const_cast<double *>(running_dev), const_cast<double *>(completed_dev), false,
                      (hipStream_t)stream);
}

} // extern "C"
