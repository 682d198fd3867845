// spatial.hip -- sb_spatial_attach / sb_spatial: zone {min, max, mean} and a pooled temperature map straight from the
// device state (include/sbsim_amd.h has the semantics and the SUMMATION ORDER this file implements).
//
// k_spatial<E, STAGE>: one workgroup of 256 threads per output row at a time, grid-stride over the rows.  E is the
// state's element (double; float on a Jacobi handle).  A building's state is one contiguous run of state_len elements,
// whatever its layout means; the index tables (spatial.h, built by spatial_plan.cpp at attach) say which element -- or
// which cell of the register layouts' exterior ring -- every control volume of the CALLER's grid is.
//   STAGE: the run is copied to LDS once with 16-byte loads (R9: 50.7 KB, three workgroups per CU), then every lane
//          reduces its tiles and every wavefront its zones from LDS.
//   else:  plans beyond 64 KiB gather from global memory through the same tables (the run is contiguous: it is still
//          fetched from HBM once, the zones' second read hits the caches).
// Bandwidth-bound: state_len * sizeof(E) bytes read per building, a few kilobytes written; the tables (4 bytes per
// tile cell and per zone cell) are shared by all buildings and stay in L2.  No scratch memory, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sb_host.h"
#include "spatial.h"

using namespace sb;

namespace {

constexpr int kSpThreads = 256, kSpWaves = kSpThreads / 64, kSpUnroll = 4;
constexpr int kSpBatch = 8;            // table entries a lane fetches before it reads the values they name
constexpr int kSpStageCap = 64 * 1024; // stage up to this many bytes: at least two workgroups stay resident per CU

struct SpArgs {
  const void *state;      // [B][stride] elements
  size_t stride;          // elements between two buildings' states
  int state_len;          // elements staged / addressed per building
  const double *scal;     // [B][kNScal]: [16], [17] the ring's extremes
  const double *ring;     // [B][n_ring] (NULL: no ring)
  int n_ring, B, Z;
  int n_tiles, tile_len, tile_wave; // n_tiles == 0: no map attached
  const int *tile_src, *tile_off, *tile_cnt, *zone_off, *zone_src;
};

// wave order (sbsim_amd.h): every lane ends with the same bits
__device__ __forceinline__ double wave_order_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  return s;
}

// A lane's part of a list in wave order: +0.0, then the cells src[i], src[i + 64], ... below `end` in sequence.  The
// table entries are fetched kSpBatch at a time before the values they name: the additions keep the list's order, the
// latency of the table reads (L2) is paid once per batch instead of once per cell.
template <typename Val>
__device__ __forceinline__ double lane_list_sum(const int *src, int i0, int end, const Val &val) {
  double s = 0.0;
  for (; i0 < end; i0 += 64 * kSpBatch) {
    int i[kSpBatch];
#pragma unroll
    for (int u = 0; u < kSpBatch; ++u) i[u] = i0 + 64 * u < end ? src[i0 + 64 * u] : -1;
#pragma unroll
    for (int u = 0; u < kSpBatch; ++u)
      if (i[u] >= 0) s += val(i[u]);
  }
  return s;
}

template <typename E, bool STAGE>
__global__ void __launch_bounds__(kSpThreads) k_spatial(SpArgs a, const int *pick, int rows, double *stats, float *map) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sp_lds[];
  E *buf = (E *)sp_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kVec = 16 / (int)sizeof(E); // elements per 16-byte load
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int b = pick ? pick[r] : r;
    if (b < 0 || b >= a.B) continue; // (workgroup-uniform) a pick outside the batch leaves its row untouched
    const E *T = (const E *)a.state + (size_t)b * a.stride;
    const double *S = a.scal + (size_t)b * kNScal;
    const double ring_lo = S[16];
    const bool ring_uniform = ring_lo == S[17];
    const double *ring = a.ring ? a.ring + (size_t)b * a.n_ring : nullptr;
    if (STAGE) {
      // elements in front of the first 16-byte boundary, the aligned body kSpUnroll loads per lane in flight, the rest
      const int head = (int)(((16 - ((uintptr_t)T & 15)) & 15) / sizeof(E));
      const int h0 = head < a.state_len ? head : a.state_len;
      const int nvec = (a.state_len - h0) / kVec;
      if (tid < h0) buf[tid] = T[tid];
      const uint4 *src = (const uint4 *)(T + h0);
      for (int v0 = tid; v0 < nvec; v0 += kSpThreads * kSpUnroll) {
        uint4 x[kSpUnroll];
#pragma unroll
        for (int u = 0; u < kSpUnroll; ++u) {
          const int v = v0 + kSpThreads * u;
          if (v < nvec) x[u] = src[v];
        }
#pragma unroll
        for (int u = 0; u < kSpUnroll; ++u) {
          const int v = v0 + kSpThreads * u;
          if (v < nvec) {
            const E *e = (const E *)&x[u];
#pragma unroll
            for (int k = 0; k < kVec; ++k) buf[h0 + v * kVec + k] = e[k]; // (LDS side: h0 may be odd, element stores)
          }
        }
      }
      const int t0 = h0 + nvec * kVec;
      if (tid < a.state_len - t0) buf[t0 + tid] = T[t0 + tid];
      __syncthreads();
    }
    auto val = [&](int s) -> double {
      if (s < a.state_len) return STAGE ? (double)buf[s] : (double)T[s];
      return ring_uniform ? ring_lo : ring[s - a.state_len];
    };
    if (map && a.n_tiles) {
      float *M = map + (size_t)r * a.n_tiles;
      if (!a.tile_wave) { // lanes = tiles, a tile's cells row-major in sequence
        for (int t = tid; t < a.n_tiles; t += kSpThreads) {
          double s = 0.0;
          for (int k0 = 0; k0 < a.tile_len; k0 += kSpBatch) { // kSpBatch table entries in flight, added in the table's order
            int i[kSpBatch];
#pragma unroll
            for (int u = 0; u < kSpBatch; ++u) i[u] = k0 + u < a.tile_len ? a.tile_src[(size_t)(k0 + u) * a.n_tiles + t] : -1;
#pragma unroll
            for (int u = 0; u < kSpBatch; ++u)
              if (i[u] >= 0) s += val(i[u]);
          }
          M[t] = (float)(s / (double)a.tile_cnt[t]);
        }
      } else { // a wavefront per tile, wave order
        for (int t = wave; t < a.n_tiles; t += kSpWaves) {
          const int c0 = a.tile_off[t], c1 = a.tile_off[t + 1];
          const double s = wave_order_sum(lane_list_sum(a.tile_src, c0 + lane, c1, val));
          if (lane == 0) M[t] = (float)(s / (double)(c1 - c0));
        }
      }
    }
    if (stats) {
      double *Q = stats + (size_t)r * a.Z * 3;
      for (int z = wave; z < a.Z; z += kSpWaves) {
        const int c0 = a.zone_off[z], c1 = a.zone_off[z + 1];
        double s = 0.0, lo = INFINITY, hi = -INFINITY;
        for (int i0 = c0 + lane; i0 < c1; i0 += 64 * kSpBatch) { // as lane_list_sum, with the extremes
          int i[kSpBatch];
#pragma unroll
          for (int u = 0; u < kSpBatch; ++u) i[u] = i0 + 64 * u < c1 ? a.zone_src[i0 + 64 * u] : -1;
#pragma unroll
          for (int u = 0; u < kSpBatch; ++u)
            if (i[u] >= 0) {
              const double x = val(i[u]);
              s += x;
              lo = fmin(lo, x);
              hi = fmax(hi, x);
            }
        }
        s = wave_order_sum(s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          lo = fmin(lo, __shfl_xor(lo, o, 64));
          hi = fmax(hi, __shfl_xor(hi, o, 64));
        }
        if (lane == 0) { Q[3 * z] = lo; Q[3 * z + 1] = hi; Q[3 * z + 2] = s / (double)(c1 - c0); }
      }
    }
    if (STAGE) __syncthreads(); // buf is the next row's
  }
}

template <typename Tp>
int replace(DevBuf<Tp> &buf, const std::vector<Tp> &v) {
  if (buf.p) { SB_HIP(hipFree(buf.p)); buf.p = nullptr; }
  return upload(buf, v.data(), v.size());
}

} // namespace

extern "C" {

int sb_spatial_attach(sb_handle *h, int32_t pool_h, int32_t pool_w, int32_t transposed) {
  if (!h) return fail(SB_ERR_INVALID, "sb_spatial_attach: null handle");
  const Dev &d = h->d;
  const bool jac = h->kernel == SB_KERNEL_JACOBI;
  const int state_len = jac ? d.N : d.reg ? d.state_doubles : d.Np;
  const int n_ring = !jac && d.reg ? d.n_ring : 0;
  SpatialTables t;
  SB_CHECK(build_spatial_tables(d.H, d.W, transposed != 0, d.Z, h->h_zone_off.data(), h->h_zone_cells.data(), h->h_state_index,
                                state_len, n_ring, pool_h, pool_w, t));
  SB_ON_DEVICE(h->device);
  SB_HIP(hipDeviceSynchronize()); // a launch still queued may read the tables this call replaces
  h->sp_attached = false;
  SB_CHECK(replace(h->sp_tile_src, t.tile_src));
  SB_CHECK(replace(h->sp_tile_off, t.tile_off));
  SB_CHECK(replace(h->sp_tile_cnt, t.tile_cnt));
  SB_CHECK(replace(h->sp_zone_off, t.zone_off));
  SB_CHECK(replace(h->sp_zone_src, t.zone_src));
  h->sp_map_h = t.map_h; h->sp_map_w = t.map_w; h->sp_tile_len = t.tile_len; h->sp_tile_wave = t.tile_wave;
  h->sp_state_len = state_len;
  const size_t bytes = (size_t)state_len * (jac ? sizeof(float) : sizeof(double));
  h->sp_stage_bytes = bytes <= (size_t)kSpStageCap ? (int)bytes : 0;
  h->sp_attached = true;
  return SB_OK;
}

int sb_spatial(sb_handle *h, const int32_t *pick_dev, int32_t n, double *zone_stats_dev, float *map_dev, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_spatial: null handle");
  if (!h->sp_attached) return fail(SB_ERR_INVALID, "sb_spatial: sb_spatial_attach first");
  if (!h->was_reset) return fail(SB_ERR_INVALID, "sb_spatial: sb_reset first");
  if (n <= 0) return fail(SB_ERR_INVALID, "sb_spatial: need n > 0 rows");
  if (!pick_dev && n != h->d.B) return fail(SB_ERR_INVALID, "sb_spatial: without pick_dev, n must be the batch size");
  if (!zone_stats_dev && !map_dev) return fail(SB_ERR_INVALID, "sb_spatial: both outputs are NULL");
  if (map_dev && h->sp_map_h == 0)
    return fail(SB_ERR_INVALID, "sb_spatial: a map needs a pool size (sb_spatial_attach was given pool_h = pool_w = 0)");
  SB_ON_DEVICE(h->device);
  const Dev &d = h->d;
  const bool jac = h->kernel == SB_KERNEL_JACOBI;
  SpArgs a{};
  a.state = jac ? (const void *)h->jgrid.p : (const void *)d.temp;
  a.stride = jac ? (size_t)d.N : d.reg ? (size_t)d.state_doubles : (size_t)d.Np;
  a.state_len = h->sp_state_len;
  a.scal = d.scal;
  a.ring = !jac && d.reg && d.n_ring > 0 ? d.ring : nullptr;
  a.n_ring = a.ring ? d.n_ring : 0;
  a.B = d.B; a.Z = d.Z;
  a.n_tiles = h->sp_map_h * h->sp_map_w; a.tile_len = h->sp_tile_len; a.tile_wave = h->sp_tile_wave;
  a.tile_src = h->sp_tile_src.p; a.tile_off = h->sp_tile_off.p; a.tile_cnt = h->sp_tile_cnt.p;
  a.zone_off = h->sp_zone_off.p; a.zone_src = h->sp_zone_src.p;
  const dim3 grid(std::max(1, std::min((int)n, h->cus * 8))), block(kSpThreads);
  const size_t lds = (size_t)h->sp_stage_bytes;
  hipStream_t st = (hipStream_t)stream;
  if (jac) {
    if (lds) hipLaunchKernelGGL((k_spatial<float, true>), grid, block, lds, st, a, pick_dev, n, zone_stats_dev, map_dev);
    else hipLaunchKernelGGL((k_spatial<float, false>), grid, block, 0, st, a, pick_dev, n, zone_stats_dev, map_dev);
  } else {
    if (lds) hipLaunchKernelGGL((k_spatial<double, true>), grid, block, lds, st, a, pick_dev, n, zone_stats_dev, map_dev);
    else hipLaunchKernelGGL((k_spatial<double, false>), grid, block, 0, st, a, pick_dev, n, zone_stats_dev, map_dev);
  }
  SB_HIP(hipGetLastError());
  return SB_OK;
}

} // extern "C"
