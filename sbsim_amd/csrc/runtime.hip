// runtime.hip -- the step runtime behind the C ABI (include/sbsim_amd.h): the state kernels (reset, observe, copies,
// k_pre / k_post around the sweep), the dispatch to the sweep kernel sb_create chose, and every entry point but
// sb_plan_info / sb_create (sbsim_hip.hip; the planner behind them: planner.cpp).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (fma only where written).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "episode_draw.h"
#include "sb_host.h"

using namespace sb;

namespace {

// ---------------------------------------------------------------- kernels
// Episodes per building (sb_reset_buildings): which buildings a reset kernel resets, and what it keeps per building.
struct EpisodeArgs {
  const uint8_t *mask; // [B] the buildings to reset (mask[b] != 0); NULL: every building (sb_reset)
  int *ep_start;       // [B] the handle's steps_since_reset at the building's own last reset; NULL: never allocated, all 0
  int *eff;            // [B] a masked reset writes the building's effective clock offset; NULL: no clock
  const int *offs0;    // [B] the attached offsets
  int restart_pos;     // the batch position of the masked buildings' next step
};
__device__ __forceinline__ bool skips(const uint8_t *mask, int b) { return mask && !mask[b]; }

// The end of a building's reset (lane 0 of its wavefront), shared by k_reset and k_reset_jacobi: Thermostat._previous_timestamp
// and SmartDevice._action_timestamp are construction state, Simulator.reset() leaves them alone (thermostat.py:66-69,
// smart_device.py:71-72) ... but the clock rewinds under them: the boiler's age of its last action goes negative, by the
// building's own steps since its own last reset (ep_start all 0: by steps_since_reset, the batch's).
__device__ __forceinline__ void reset_episode(double *S, const EpisodeArgs &ep, int b, int first, int steps_since_reset) {
  if (first) { S[18] = -1.0; S[19] = kAgeNone; }
  else if (!age_is_none(S[19])) S[19] -= (double)(steps_since_reset - (ep.ep_start ? ep.ep_start[b] : 0));
  if (ep.ep_start) ep.ep_start[b] = ep.mask ? steps_since_reset : 0;
  if (ep.mask && ep.eff) ep.eff[b] = ep.offs0[b] - ep.restart_pos;
}

// sb_initial_conditions_attach: the third source of a reset's cell values, after `temps` and before the call's scalar
// (include/sbsim_amd.h states the formula).  The arrays are the handle's; a NULL one is an absent field.
struct StartView {
  const double *grids; // [K][N] in the handle's orientation
  const int *grid_of;  // [B]; NULL: grid 0
  const double *base;  // [B] initial_temp
  const double *offset; // [B]
  int *episode;        // [B] the number of the building's next episode
  double lo, hi;       // the jitter's interval
  uint64_t seed;
  long long first;     // global index of building 0
  int jitter;
};

// One building's start: where a cell's value comes from and what is added to it.  Everything here is the wavefront's
// (uniform); `e` is lane 0's alone.
struct Start {
  const double *grid; // the building's grid; NULL: `base` in every cell
  double base, offset, u;
  bool has_offset, has_jitter;
  int e;
  __device__ __forceinline__ double at(int g) const {
    double v = grid ? grid[g] : base;
    if (has_offset) v = v + offset; // (nothing is added for an absent field: -0.0 stays -0.0)
    if (has_jitter) v = v + u;
    return v;
  }
};

__device__ __forceinline__ double wave_first(double x) { // lane 0's value in every lane (a scalar register pair)
  const long long bits = __double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)bits), hi = __builtin_amdgcn_readfirstlane((unsigned)(bits >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The top of a building's reset with conditions attached.  The draw (episode_draw.h: initial_conditions_draw) is one
// Philox block per building, in lane 0, and broadcast.
__device__ __forceinline__ Start start_of(const StartView &ic, int b, int lane, int N, double initial_temp) {
  Start st;
  st.grid = ic.grids ? ic.grids + (size_t)(ic.grid_of ? ic.grid_of[b] : 0) * N : nullptr;
  st.base = ic.base ? ic.base[b] : initial_temp;
  st.has_offset = ic.offset != nullptr;
  st.offset = st.has_offset ? ic.offset[b] : 0.0;
  st.has_jitter = ic.jitter != 0;
  st.e = lane == 0 ? ic.episode[b] : 0;
  st.u = 0.0;
  if (st.has_jitter) {
    double u = 0.0;
    if (lane == 0) u = initial_conditions_draw(ic.lo, ic.hi, ic.seed, (uint64_t)(ic.first + b), (uint32_t)st.e);
    st.u = wave_first(u);
  }
  return st;
}

// Simulator.reset(): grid (either state layout), zone means, device scalars.
// temps_only (sb_set_temps): the grid inside the building and the zone means follow `temps`; every device state stays.
// IC (k_reset_ic): a cell without `temps` takes its value from the attached conditions, and the building's episode
// counter advances whichever source its values had.  The sums add the same values in the same lane order either way.
template <bool IC>
__device__ __forceinline__ void reset_grid(Dev a, EpisodeArgs ep, StartView ic, double initial_temp,
                                           const double *temps, int first, int steps_since_reset, int temps_only) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * (blockDim.x >> 6);
  for (int b = wave; b < a.B; b += nwaves) {
    if (skips(ep.mask, b)) continue; // (b is the wavefront's: uniform)
    Start st{};
    if (IC) st = start_of(ic, b, lane, a.N, initial_temp);
    auto start = [&](int g) { return temps ? temps[(size_t)b * a.N + g] : IC ? st.at(g) : initial_temp; };
    double s = 0.0, rlo = INFINITY, rhi = -INFINITY;
    if (a.reg) {
      double *T = a.temp + (size_t)b * a.state_doubles;
      const double *S0 = a.scal + (size_t)b * kNScal;
      const bool ring_uniform = S0[16] == S0[17]; // (temps_only) the ring holds one value: the ambient temperature of the last step
      for (int g = lane; g < a.N; g += 64) {
        double v = start(g);
        const int cs = a.cell_state[g];
        if (cs >= 0) {
          T[cs] = v;
        } else if (!temps_only) {
          a.ring[(size_t)b * a.n_ring + (-cs - 1)] = v;
          rlo = fmin(rlo, v);
          rhi = fmax(rhi, v);
        } else { // sb_set_temps leaves exterior space alone: the grid mean counts what the ring holds, not what `temps` says
          v = ring_uniform ? S0[16] : a.ring[(size_t)b * a.n_ring + (-cs - 1)];
        }
        s += v;
      }
      rlo = wave_min(rlo);
      rhi = wave_max(rhi);
    } else {
      double *T = a.temp + (size_t)b * a.Np;
      for (int i = lane; i < a.Np; i += 64) {
        const int g = i - kPad;
        double v = (g >= 0 && g < a.N) ? start(g) : 0.0;
        T[i] = v;
        s += v;
      }
    }
    s = wave_sum(s);
    for (int z = 0; z < a.Z; ++z) {
      double zs = 0.0;
      const int b0 = a.zone_off[z], b1 = a.zone_off[z + 1];
      for (int i = b0 + lane; i < b1; i += 64) {
        int li = a.zone_cells_l[i];
        int g = a.pitch == a.W ? li : (li / a.pitch) * a.W + (li % a.pitch);
        zs += start(g);
      }
      zs = wave_sum(zs);
      if (lane == 0) {
        size_t o = (size_t)b * a.Z + z;
        a.zmean[o] = zs / (double)(b1 - b0);
        if (temps_only) continue;
        a.zair[o] = 0.0;   // vav.py:93-99
        a.damper[o] = 0.1;
        a.mode[o] &= kModeMask; // ... the reheat valve closes; the thermostat keeps its mode
        a.qz[o] = 0.0;     // building.py:791 input_q <- 0
      }
    }
    // sb_set_temps: the recirculation temperature of the next step is the mean of the NEW grid (simulator.py:423-426 takes
    // building.temp.mean() every step; S[11] caches it between steps)
    if (lane == 0 && temps_only) a.scal[(size_t)b * kNScal + 11] = s / (double)a.N;
    if (lane == 0 && !temps_only) {
      double *S = a.scal + (size_t)b * kNScal;
      const double blr_sp = bparam(a, SB_BP_BLR_SETPOINT, b); // the building's own row (sb_set_building_params)
      S[0] = bparam(a, SB_BP_AHU_HEAT_SP, b); S[1] = bparam(a, SB_BP_AHU_COOL_SP, b); S[2] = 0.0; S[3] = 0.0; // air_handler.py:131-139
      S[4] = blr_sp; S[5] = 0.0; S[6] = 0.0; S[7] = 0.0;                      // boiler.py:110-121
      S[8] = blr_sp; S[9] = 0.0; S[10] = 0.0;
      S[11] = s / (double)a.N;
      S[12] = S[13] = S[14] = S[15] = 0.0;
      S[16] = a.reg && a.n_ring > 0 ? rlo : 0.0; // extremes of the exterior-space ring (register path)
      S[17] = a.reg && a.n_ring > 0 ? rhi : 0.0;
      reset_episode(S, ep, b, first, steps_since_reset);
      if (IC) ic.episode[b] = next_episode(st.e);
    }
  }
}

__global__ void k_reset(Dev a, EpisodeArgs ep, double initial_temp, const double *temps, int first, int steps_since_reset, int temps_only) {
  reset_grid<false>(a, ep, StartView{}, initial_temp, temps, first, steps_since_reset, temps_only);
}

__global__ void k_reset_ic(Dev a, EpisodeArgs ep, StartView ic, double initial_temp, const double *temps, int first, int steps_since_reset) {
  reset_grid<true>(a, ep, ic, initial_temp, temps, first, steps_since_reset, 0);
}

// in: the observation's inputs as a step's "now" half (aux, num_occupants_dev, occupancy_norm, the weather at t);
// t_amb_b: sb_observe's [B] ambient temperatures (override); clk: the building's own row at the position sought;
// mask (sb_observe_buildings): the buildings to observe, NULL: every building
template <bool CLK> // a calendar per building (sb_clock_attach): a kernel per value, see sb_device.h clocked()
__global__ void k_observe(Dev a, ClockView clk, sb_step_in in, const double *t_amb_b, float *obs, const uint8_t *mask) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < a.B; b += gridDim.x * blockDim.x) {
    if (skips(mask, b)) continue;
    double *S = a.scal + (size_t)b * kNScal;
    observe_boiler(a, S, b);
    const int crow = clock_row<CLK>(clk, b);
    write_obs<CLK>(a, b, obs, in.aux, t_amb_b ? t_amb_b[b] : ambient_temp<CLK>(in, clk, crow, b, false), S, in.num_occupants_dev,
              in.occupancy_norm, clk, crow);
  }
}

// Thermostat modes without the valve bit.
__global__ void k_copy_modes(Dev a, int32_t *out) {
  const size_t n = (size_t)a.B * a.Z;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = a.mode[i] & kModeMask;
}

// building.temp in the caller's row-major layout, whichever state layout the handle uses.
__global__ void k_copy_temps(Dev a, double *out) {
  size_t n = (size_t)a.B * a.N;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / a.N;
    const int g = (int)(i - b * a.N);
    if (a.reg) {
      const int cs = a.cell_state[g];
      if (cs >= 0) {
        out[i] = a.temp[b * a.state_doubles + cs];
      } else { // exterior space: T_ambient of the last step, or what sb_reset stored
        const double *S = a.scal + b * kNScal;
        out[i] = S[16] == S[17] ? S[16] : a.ring[b * a.n_ring + (-cs - 1)];
      }
    } else {
      out[i] = a.temp[b * a.Np + kPad + g];
    }
  }
}

__global__ void k_copy_scalars(Dev a, double *out) {
  size_t n = (size_t)a.B * kNScalOut;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    out[i] = a.scal[(i / kNScalOut) * kNScal + (i % kNScalOut)];
}

// sb_state_save / sb_state_load: one workgroup per snapshot row (save) / building (load), grid-stride.  The grid is
// converted between the handle's layout and the caller's row-major [H*W] the way k_copy_temps / k_reset do; on the
// snapshot side every lane moves 16 bytes at a time (a row that starts at an odd double has a lone cell in front).
// Load recomputes scal[16..17], which describe the register layout's exterior ring, from the grid's ring cells (k_reset).
// Padding slots of the register state are written by neither direction.
constexpr int kStateThreads = 256, kStateUnroll = 4;
template <bool SAVE>
__global__ void __launch_bounds__(kStateThreads) k_state(Dev a, sb_state_view v, uint32_t *occ, const int *pick,
                                                         int rows, int transposed) {
  __shared__ double red[2][kStateThreads / 64];
  const int tid = threadIdx.x;
  const int count = SAVE ? rows : a.B;
  for (int i = blockIdx.x; i < count; i += gridDim.x) {
    const int p = pick ? pick[i] : i;
    const int b = SAVE ? p : i, r = SAVE ? i : p;
    if (b < 0 || b >= a.B || r < 0 || r >= v.n) continue; // (load: pick < 0 keeps the building; the host checks the rest)
    double *G = v.grid + (size_t)r * a.N;
    const int head = (int)(((size_t)r * a.N) & 1);
    double *T = a.temp + (size_t)b * (a.reg ? (size_t)a.state_doubles : (size_t)a.Np);
    double *ring = a.ring + (size_t)b * a.n_ring;
    const double *S = a.scal + (size_t)b * kNScal;
    const bool ring_uniform = S[16] == S[17]; // (save) after a step the ring holds the ambient temperature of the step
    const bool plain = !a.reg && !transposed && ((kPad + head) & 1) == 0; // both sides contiguous and 16-byte aligned
    auto hcell = [&](int g0) { return transposed ? (g0 % a.H) * a.W + g0 / a.H : g0; };
    auto get = [&](int g0) -> double {
      const int g = hcell(g0);
      if (!a.reg) return T[kPad + g];
      const int cs = a.cell_state[g];
      return cs >= 0 ? T[cs] : ring_uniform ? S[16] : ring[-cs - 1];
    };
    double lo = INFINITY, hi = -INFINITY;
    auto put = [&](int g0, double x) {
      const int g = hcell(g0);
      if (!a.reg) { T[kPad + g] = x; return; }
      const int cs = a.cell_state[g];
      if (cs >= 0) { T[cs] = x; return; }
      ring[-cs - 1] = x;
      lo = fmin(lo, x);
      hi = fmax(hi, x);
    };
    // cells head + 2k, head + 2k + 1: kStateUnroll pairs per lane in flight
    for (int j0 = head + 2 * tid; j0 + 1 < a.N; j0 += 2 * kStateThreads * kStateUnroll) {
      double2 x[kStateUnroll];
#pragma unroll
      for (int u = 0; u < kStateUnroll; ++u) {
        const int j = j0 + 2 * kStateThreads * u;
        if (j + 1 >= a.N) break;
        if (!SAVE) x[u] = *(const double2 *)(G + j);
        else if (plain) x[u] = *(const double2 *)(T + kPad + j);
        else x[u] = make_double2(get(j), get(j + 1));
      }
#pragma unroll
      for (int u = 0; u < kStateUnroll; ++u) {
        const int j = j0 + 2 * kStateThreads * u;
        if (j + 1 >= a.N) break;
        if (SAVE) *(double2 *)(G + j) = x[u];
        else if (plain) *(double2 *)(T + kPad + j) = x[u];
        else { put(j, x[u].x); put(j + 1, x[u].y); }
      }
    }
    const int lone = tid == 0 && head ? 0 : tid == 1 && ((a.N - head) & 1) ? a.N - 1 : -1;
    if (lone >= 0) {
      if (SAVE) G[lone] = get(lone);
      else put(lone, G[lone]);
    }
    // the per-building rows: zone arrays, modes, scalars, sweep count, occupants
    const size_t zb = (size_t)b * a.Z;
    double *zs = v.zone + (size_t)r * 4 * a.Z;
    double *zh[4] = {a.zmean + zb, a.zair + zb, a.damper + zb, a.qz + zb};
    for (int k = tid; k < 4 * a.Z; k += kStateThreads) {
      double *h = zh[k / a.Z] + k % a.Z;
      if (SAVE) zs[k] = *h;
      else *h = zs[k];
    }
    for (int z = tid; z < a.Z; z += kStateThreads) {
      int *m = a.mode + zb + z, *ms = v.mode + (size_t)r * a.Z + z;
      if (SAVE) *ms = *m;
      else *m = *ms;
      if (occ) {
        uint32_t *o = occ + zb + z, *os = v.occ + (size_t)r * a.Z + z;
        if (SAVE) *os = *o;
        else *o = *os;
      }
    }
    double *Ss = v.scal + (size_t)r * kNScal, *Sh = a.scal + (size_t)b * kNScal;
    if (SAVE) {
      if (tid < kNScal) Ss[tid] = Sh[tid];
      if (tid == 0) v.nsw[r] = a.nsw[b];
      continue;
    }
    if (tid < kNScal && tid != 16 && tid != 17) Sh[tid] = Ss[tid];
    if (tid == 0) a.nsw[b] = v.nsw[r];
    if (a.reg && a.n_ring > 0) { // the ring's extremes, as k_reset computes them (every lane of the workgroup holds cells)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, 64));
        hi = fmax(hi, __shfl_xor(hi, o, 64));
      }
      if ((tid & 63) == 0) { red[0][tid >> 6] = lo; red[1][tid >> 6] = hi; }
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < kStateThreads / 64; ++w) { lo = fmin(lo, red[0][w]); hi = fmax(hi, red[1][w]); }
        Sh[16] = lo; Sh[17] = hi;
      }
      __syncthreads(); // red is reused by the workgroup's next building
    } else if (tid == 0) {
      Sh[16] = Sh[17] = 0.0;
    }
  }
}

// SB_KERNEL_JACOBI: Simulator.reset() on the float32 grid.  The grid is stored rounded to float32 (as the reference's first
// FD update reads it); the zone means and the grid mean the first step reads are the float64 values, as the reference's
// are.  The scalars as k_reset sets them.  One wavefront per building.
// IC (k_reset_jacobi_ic): as reset_grid's -- the stored cell is (float)v of the float64 v, rounded once.
template <bool IC>
__device__ __forceinline__ void reset_jacobi(Dev a, EpisodeArgs ep, StartView ic, float *grid,
                                             double initial_temp, const double *temps, int first, int steps_since_reset) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * (blockDim.x >> 6);
  for (int b = wave; b < a.B; b += nwaves) {
    if (skips(ep.mask, b)) continue;
    Start st{};
    if (IC) st = start_of(ic, b, lane, a.N, initial_temp);
    auto start = [&](int g) { return temps ? temps[(size_t)b * a.N + g] : IC ? st.at(g) : initial_temp; };
    double s = 0.0;
    for (int g = lane; g < a.N; g += 64) {
      const double v = start(g);
      grid[(size_t)b * a.N + g] = (float)v;
      s += v;
    }
    s = wave_sum(s);
    for (int z = 0; z < a.Z; ++z) {
      double zs = 0.0;
      const int b0 = a.zone_off[z], b1 = a.zone_off[z + 1];
      for (int i = b0 + lane; i < b1; i += 64) zs += start(a.zone_cells_l[i]);
      zs = wave_sum(zs);
      if (lane == 0) {
        const size_t o = (size_t)b * a.Z + z;
        a.zmean[o] = zs / (double)(b1 - b0);
        a.zair[o] = 0.0;   // vav.py:93-99
        a.damper[o] = 0.1;
        a.mode[o] &= kModeMask;
        a.qz[o] = 0.0;     // building.py:791 input_q <- 0
      }
    }
    if (lane == 0) {
      double *S = a.scal + (size_t)b * kNScal;
      const double blr_sp = bparam(a, SB_BP_BLR_SETPOINT, b); // the building's own row (sb_set_building_params)
      S[0] = bparam(a, SB_BP_AHU_HEAT_SP, b); S[1] = bparam(a, SB_BP_AHU_COOL_SP, b); S[2] = 0.0; S[3] = 0.0; // air_handler.py:131-139
      S[4] = blr_sp; S[5] = 0.0; S[6] = 0.0; S[7] = 0.0;                      // boiler.py:110-121
      S[8] = blr_sp; S[9] = 0.0; S[10] = 0.0;
      S[11] = s / (double)a.N;
      S[12] = S[13] = S[14] = S[15] = 0.0;
      S[16] = S[17] = 0.0; // (the register path's ring extremes: no ring here)
      reset_episode(S, ep, b, first, steps_since_reset);
      if (IC) ic.episode[b] = next_episode(st.e);
    }
  }
}

__global__ void k_reset_jacobi(Dev a, EpisodeArgs ep, float *grid, double initial_temp, const double *temps, int first, int steps_since_reset) {
  reset_jacobi<false>(a, ep, StartView{}, grid, initial_temp, temps, first, steps_since_reset);
}

__global__ void k_reset_jacobi_ic(Dev a, EpisodeArgs ep, StartView ic, float *grid, double initial_temp, const double *temps, int first,
                                  int steps_since_reset) {
  reset_jacobi<true>(a, ep, ic, grid, initial_temp, temps, first, steps_since_reset);
}

__global__ void k_copy_temps_jacobi(const float *grid, size_t n, double *out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (double)grid[i];
}

// Per-building algebra before / after the sweep kernel (sb_device.h).  k_pre: one 16-lane row of a wavefront per building,
// lanes = zones -- four buildings per wavefront, sixteen per workgroup; the building's demand sums in the reference's zone
// order through DPP row broadcasts.  k_post: one thread per building (the row shape was measured slower: sb_device.h).
// only >= 0: that building alone (the known-answer taps).
constexpr int kRowsPerBlock = 16; // buildings per workgroup of 256 threads
template <bool MAT, bool CLK> // the building's own coefficient rows (sb_create_materials), its own calendar (sb_clock_attach): a kernel per value, see pre_building
__global__ void __launch_bounds__(16 * kRowsPerBlock) k_pre(Dev a, StepArgs s, int only) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { // the sweep kernel's draw counter; k_sweep_roll: the redo list's counters
    *a.next_b = 0;
    if (a.redo_ctr) a.redo_ctr[0] = a.redo_ctr[1] = 0;
  }
  const int i = threadIdx.x & 15, r = threadIdx.x >> 4;
  if (only >= 0) {
    if (blockIdx.x == 0 && r == 0) pre_building<MAT, CLK>(a, s, only, i);
    return;
  }
  for (int b = blockIdx.x * kRowsPerBlock + r; b < a.B; b += gridDim.x * kRowsPerBlock) pre_building<MAT, CLK>(a, s, b, i);
}

// k_pre of the handle (sb_create_materials: the variant that reads the building's own gc and sc); only >= 0: that building alone
void launch_pre(const sb_handle *h, const StepArgs &s, dim3 grid, hipStream_t stream, int only) {
  const dim3 block(16 * kRowsPerBlock);
  if (s.clk.rows) {
    if (h->d.ctab_b) hipLaunchKernelGGL((k_pre<true, true>), grid, block, 0, stream, h->d, s, only);
    else hipLaunchKernelGGL((k_pre<false, true>), grid, block, 0, stream, h->d, s, only);
  } else if (h->d.ctab_b) hipLaunchKernelGGL((k_pre<true, false>), grid, block, 0, stream, h->d, s, only);
  else hipLaunchKernelGGL((k_pre<false, false>), grid, block, 0, stream, h->d, s, only);
}

template <int KIND, bool CLK> // the reward function (sb_reward_kind), a calendar per building: a kernel per value, see post_building
__global__ void __launch_bounds__(64) k_post(Dev a, StepArgs s, sb_reward_config rc, int only) { // one thread per building: see sb_device.h
  if (only >= 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) post_building<KIND, CLK>(a, s, rc, only);
    return;
  }
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < a.B; b += gridDim.x * blockDim.x) post_building<KIND, CLK>(a, s, rc, b);
}

// sb_create_materials: every building's coefficient rows from its own materials and convection coefficient.  One thread
// per (building, class); FloorPlan.compile's arithmetic (sbsim_amd/floorplan.py, structural_class_coef) operation for
// operation -- this file is built with -ffp-contract=off, and float64 division is correctly rounded -- so a row equals the
// host's bit for bit.  desc: {material slot, neighbour count, present mask, half-factor mask}; tab: [3 M + 1][B], field
// kind * M + slot (conductivity, heat capacity, density), h_conv last; out: [B][ncls + 1][8], row ncls the pad class.
// MASKED (sb_randomization_attach's redraw): only the buildings with mask[b] != 0; the arithmetic is the one body.
template <bool MASKED>
__device__ __forceinline__ void class_coef(const int4 *desc, const double *diff, const double *tab, int B, int ncls, int M,
                                           double dt, double dx, double dx2, double zh, double *out, const uint8_t *mask) {
  const size_t n = (size_t)B * (ncls + 1);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / (ncls + 1)), c = (int)(i - (size_t)b * (ncls + 1));
    if (MASKED && !mask[b]) continue;
    double bn[4] = {0.0, 0.0, 0.0, 0.0}, ap = 0.0, gc = 0.0, sc = 0.0;
    if (c == ncls) {
      ap = 1.0; // the pad class: T' = Tprev
    } else {
      const int4 e = desc[c];
      const double kk = tab[(size_t)e.x * B + b], cc = tab[(size_t)(M + e.x) * B + b], rr = tab[(size_t)(2 * M + e.x) * B + b];
      const double h_conv = tab[(size_t)3 * M * B + b];
      const int n_nb = e.y, present = e.z, half = e.w;
      if (n_nb <= 1) { // simulator.py:256-258 exterior CVs return ambient
        gc = 1.0;
      } else if (n_nb == 2) { // corner :130-142
        const double t0 = rr * dx2 * cc / dt / 2.0;
        const double den = 2.0 * kk + 2.0 * h_conv * dx + t0;
        for (int j = 0; j < 4; ++j)
          if (present >> j & 1) bn[j] = kk / den;
        ap = t0 / den; gc = 2.0 * h_conv * dx / den;
      } else if (n_nb == 3) { // edge :176-195
        const double t0 = rr * dx2 / 2.0 * cc / dt;
        const double den = 2.0 * kk + h_conv * dx + t0;
        for (int j = 0; j < 4; ++j)
          if (present >> j & 1) bn[j] = kk * ((half >> j & 1) ? 0.5 : 1.0) / den;
        ap = t0 / den; gc = h_conv * dx / den;
      } else { // interior :225-237
        const double alpha = kk / rr / cc;
        const double t0 = dx2 / dt / alpha;
        const double den = 4.0 + t0;
        bn[0] = bn[1] = bn[2] = bn[3] = 1.0 / den;
        ap = t0 / den;
        const double dw = diff[c];
        if (dw > 0.0) sc = dw / kk / zh / den; // building.py:873-889
      }
    }
    double2 *o = (double2 *)(out + i * 8);
    o[0] = make_double2(bn[0], bn[1]); o[1] = make_double2(bn[2], bn[3]);
    o[2] = make_double2(ap, gc); o[3] = make_double2(sc, 0.0);
  }
}

__global__ void __launch_bounds__(256) k_class_coef(const int4 *desc, const double *diff, const double *tab, int B, int ncls,
                                                    int M, double dt, double dx, double dx2, double zh, double *out) {
  class_coef<false>(desc, diff, tab, B, ncls, M, dt, dx, dx2, zh, out, nullptr);
}

__global__ void __launch_bounds__(256) k_class_coef_masked(const int4 *desc, const double *diff, const double *tab, int B, int ncls,
                                                           int M, double dt, double dx, double dx2, double zh, double *out,
                                                           const uint8_t *mask) {
  class_coef<true>(desc, diff, tab, B, ncls, M, dt, dx, dx2, zh, out, mask);
}

// k_post of the handle's reward function (sb_set_reward_function); only >= 0: that building alone
void launch_post(const sb_handle *h, const StepArgs &s, dim3 grid, hipStream_t stream, int only) {
  const bool dollars = h->reward.kind == SB_REWARD_SETPOINT_ENERGY_CARBON;
  if (s.clk.rows) {
    if (dollars) hipLaunchKernelGGL((k_post<SB_REWARD_SETPOINT_ENERGY_CARBON, true>), grid, dim3(64), 0, stream, h->d, s, h->reward, only);
    else hipLaunchKernelGGL((k_post<SB_REWARD_REGRET, true>), grid, dim3(64), 0, stream, h->d, s, h->reward, only);
  } else if (dollars) hipLaunchKernelGGL((k_post<SB_REWARD_SETPOINT_ENERGY_CARBON, false>), grid, dim3(64), 0, stream, h->d, s, h->reward, only);
  else hipLaunchKernelGGL((k_post<SB_REWARD_REGRET, false>), grid, dim3(64), 0, stream, h->d, s, h->reward, only);
}

} // namespace

int prepare_sweep(const sb_handle *h) {
  const Dev &d = h->d;
  const int waves = h->info.waves_per_workgroup;
  switch (h->kernel) {
    case SB_KERNEL_LDS: return prepare_sweep_lds(d, (size_t)h->info.lds_bytes_per_workgroup);
    case SB_KERNEL_REG: case SB_KERNEL_REG_PAIR: return prepare_sweep_reg(d);
    case SB_KERNEL_ROLL: return prepare_sweep_roll(d);
    case SB_KERNEL_TWO_ROWS: return prepare_sweep_two(d);
    case SB_KERNEL_BAND: return prepare_sweep_band(d);
    case SB_KERNEL_STREAM:
      if (h->stream_variant == kStreamMs) return prepare_sweep_stream_ms(d, waves);
      if (h->stream_variant == kStreamRoll) return prepare_sweep_stream_roll(d, waves);
      return prepare_sweep_stream(d, waves);
    case SB_KERNEL_JACOBI: return prepare_sweep_jacobi(d.H, d.W, d.ncls, h->jac.path);
  }
  return (int)hipErrorInvalidValue;
}

int launch_sweep(const sb_handle *h, hipStream_t stream) {
  const Dev &d = h->d;
  const int waves = h->info.waves_per_workgroup;
  switch (h->kernel) {
    case SB_KERNEL_LDS: return launch_sweep_lds(d, h->info.workgroups, waves, (size_t)h->info.lds_bytes_per_workgroup, stream);
    case SB_KERNEL_REG: case SB_KERNEL_REG_PAIR: return launch_sweep_reg(d, h->cus, stream);
    case SB_KERNEL_ROLL: return launch_sweep_roll(d, stream);
    case SB_KERNEL_TWO_ROWS: return launch_sweep_two(d, stream);
    case SB_KERNEL_BAND: return launch_sweep_band(d, stream);
    case SB_KERNEL_STREAM:
      if (h->stream_variant == kStreamMs) return launch_sweep_stream_ms(d, h->abuf.p, h->ebuf.p, waves, stream);
      if (h->stream_variant == kStreamRoll) return launch_sweep_stream_roll(d, h->abuf.p, h->ebuf.p, waves, stream);
      return launch_sweep_stream(d, h->abuf.p, waves, stream);
    case SB_KERNEL_JACOBI: return launch_sweep_jacobi(d, h->jac, h->info.workgroups, stream);
  }
  return (int)hipErrorInvalidValue;
}

int launch_class_coef(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream) {
  const Dev &d = h->d;
  const size_t n = (size_t)d.B * (d.ncls + 1);
  const int blocks = (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)h->cus * 32));
  if (mask_dev)
    hipLaunchKernelGGL(k_class_coef_masked, dim3(blocks), dim3(256), 0, stream, h->mat_desc.p, h->mat_diff.p, h->mat_tab.p, d.B,
                       d.ncls, h->mat_slots, d.p.dt, h->mat_dx, h->mat_dx2, h->mat_zh, h->ctab_b.p, mask_dev);
  else
    hipLaunchKernelGGL(k_class_coef, dim3(blocks), dim3(256), 0, stream, h->mat_desc.p, h->mat_diff.p, h->mat_tab.p, d.B, d.ncls,
                       h->mat_slots, d.p.dt, h->mat_dx, h->mat_dx2, h->mat_zh, h->ctab_b.p);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

// sb_create_materials / sb_set_building_materials: the value table and k_class_coef on `stream`, and waits for them (the
// copy reads host memory that goes away with this call)
int apply_building_materials(sb_handle *h, const std::vector<double> &tab, hipStream_t stream) {
  const Dev &d = h->d;
  const int M = h->mat_slots, F = 3 * M + 1, B = d.B;
  std::vector<double> own;
  if (tab.empty()) { // the plan's own values in every row
    own.resize((size_t)F * B);
    for (int f = 0; f < F; ++f) std::fill_n(own.begin() + (size_t)f * B, B, h->mat_default[f]);
  }
  const std::vector<double> &src = tab.empty() ? own : tab;
  SB_HIP(hipMemcpyAsync(h->mat_tab.p, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  SB_CHECK(launch_class_coef(h, nullptr, stream));
  SB_HIP(hipStreamSynchronize(stream));
  return SB_OK;
}

// The bounds sb_clock_seek checks, from the host shadow of the restart positions (episode_starts.hip calls it too).
void episode_bounds(sb_handle *h) {
  int max_eff = INT32_MIN, max_restart = 0;
  for (size_t b = 0; b < h->h_clock_offs.size(); ++b) {
    const int r = h->restart_pos.empty() ? 0 : h->restart_pos[b];
    max_eff = std::max(max_eff, h->h_clock_offs[b] - r);
    max_restart = std::max(max_restart, r);
  }
  h->clock_max_off = h->h_clock_offs.empty() ? 0 : max_eff;
  h->max_restart = max_restart;
}

extern "C" {

int sb_abi_version(void) { return SB_ABI_VERSION; }
int sb_has_experimental_kernels(void) { return kExperimental ? 1 : 0; }
const char *sb_last_error(void) { return sb::host::g_err.c_str(); }

void sb_destroy(sb_handle *h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  delete h;
}

int sb_get_launch_info(const sb_handle *h, sb_launch_info *out) {
  if (!h || !out) return fail(SB_ERR_INVALID, "sb_get_launch_info: null argument");
  *out = h->info;
  return SB_OK;
}

// The reset kernel of the handle's state layout on the buildings of `ep` (sb_reset: every building; sb_reset_buildings: its mask).
static void launch_reset(sb_handle *h, const EpisodeArgs &ep, double initial_temp, const double *temps_dev, hipStream_t stream) {
  const int wpb = 4;
  const int blocks = std::min((h->d.B + wpb - 1) / wpb, 4096);
  if (h->ic_draws.attached) { // the conditions' kernels: the values without temps_dev, the episode counters either way
    const StartView ic{h->ic_grids.p, h->ic_grid_of.p, h->ic_base.p, h->ic_offset.p, h->ic_draws.episode.p,
                       h->ic_lo, h->ic_hi, h->ic_draws.seed, h->ic_draws.first, h->ic_jitter ? 1 : 0};
    if (h->kernel == SB_KERNEL_JACOBI)
      hipLaunchKernelGGL(k_reset_jacobi_ic, dim3(blocks), dim3(64 * wpb), 0, stream, h->d, ep, ic, h->jgrid.p,
                         initial_temp, temps_dev, h->was_reset ? 0 : 1, h->steps_since_reset);
    else
      hipLaunchKernelGGL(k_reset_ic, dim3(blocks), dim3(64 * wpb), 0, stream, h->d, ep, ic, initial_temp,
                         temps_dev, h->was_reset ? 0 : 1, h->steps_since_reset);
  } else if (h->kernel == SB_KERNEL_JACOBI)
    hipLaunchKernelGGL(k_reset_jacobi, dim3(blocks), dim3(64 * wpb), 0, stream, h->d, ep, h->jgrid.p,
                       initial_temp, temps_dev, h->was_reset ? 0 : 1, h->steps_since_reset);
  else
    hipLaunchKernelGGL(k_reset, dim3(blocks), dim3(64 * wpb), 0, stream, h->d, ep, initial_temp,
                       temps_dev, h->was_reset ? 0 : 1, h->steps_since_reset, 0);
}

int sb_reset(sb_handle *h, double initial_temp, const double *temps_dev, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_reset: null handle");
  SB_ON_DEVICE(h->device);
  if (h->em_draws.attached) SB_CHECK(sb_episode_metrics_close(h, nullptr, (hipStream_t)stream)); // the episodes that end here: their totals latched
  if (h->tl_draws.attached) SB_CHECK(sb_telemetry_close(h, nullptr, (hipStream_t)stream)); // ... and their scores against the recording
  if (h->rz_draws.attached) SB_CHECK(sb_randomization_redraw(h, nullptr, (hipStream_t)stream)); // the new episode's rows, before the reset reads them
  if (h->es_draws.attached) SB_CHECK(sb_episode_starts_redraw(h, nullptr, (hipStream_t)stream)); // ... its start and weather
  launch_reset(h, EpisodeArgs{nullptr, h->ep_start.p, nullptr, nullptr, 0}, initial_temp, temps_dev, (hipStream_t)stream);
  h->was_reset = true;
  h->steps_since_reset = 0;
  h->counters_zeroed_on = (void *)(uintptr_t)1; // (whatever came before a reset is no promise about the draw counters)
  SB_HIP(hipGetLastError());
  h->ep_dirty = false; // (the kernel above zeroes ep_start)
  const bool new_offs = !h->h_clock_next.empty(); // sb_clock_set_offsets: every building takes its new offset now
  if (new_offs) {
    h->h_clock_offs = std::move(h->h_clock_next);
    h->h_clock_next.clear();
  }
  if (h->es_draws.attached) sb_episode_starts_after_reset(h, nullptr);
  if (!h->restart_pos.empty() || h->own_prev || new_offs) { // episodes per building: every building back on the attached calendar
    if (h->clock_eff.p)
      SB_HIP(hipMemcpyAsync(h->clock_eff.p, h->clock_offs.p, (size_t)h->d.B * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    h->restart_pos.clear();
    h->own_prev = false;
    episode_bounds(h);
  }
  return SB_OK;
}

// sb_reset_buildings / sb_observe_buildings: the mask on the device, after the work queued on `stream` (the copy reads
// host memory that may go away with the call: the stream is drained before it returns).
static int upload_mask(sb_handle *h, const uint8_t *mask_host, const char *who, hipStream_t stream) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  SB_HIP(hipStreamIsCapturing(stream, &cap));
  if (cap != hipStreamCaptureStatusNone)
    return fail(SB_ERR_INVALID, std::string(who) + ": not while the stream is being captured into a graph");
  const size_t B = (size_t)h->d.B;
  if (!h->ep_mask.p) SB_HIP(hipMalloc((void **)&h->ep_mask.p, B));
  SB_HIP(hipMemcpyAsync(h->ep_mask.p, mask_host, B, hipMemcpyHostToDevice, stream));
  SB_HIP(hipStreamSynchronize(stream));
  return SB_OK;
}

int sb_reset_buildings(sb_handle *h, const uint8_t *mask_host, int32_t restart_pos, double initial_temp,
                       const double *temps_dev, void *stream) {
  if (!h || !mask_host) return fail(SB_ERR_INVALID, "sb_reset_buildings: null argument");
  if (!h->was_reset) return fail(SB_ERR_INVALID, "sb_reset_buildings: sb_reset first");
  const int B = h->d.B;
  const bool clk = h->clock_rows.p != nullptr;
  if (!clk) restart_pos = 0; // (ignored without a clock)
  if (restart_pos < 0) return fail(SB_ERR_INVALID, "sb_reset_buildings: restart_pos must be >= 0");
  bool any = false;
  for (int b = 0; b < B; ++b) {
    if (!mask_host[b]) continue;
    any = true;
    // the rows of the building's next launch: at the position sought now, or at restart_pos once the caller has sought
    // there (sb_clock_seek refuses a position below it)
    if (!clk) continue;
    const int off = h->h_clock_next.empty() ? h->h_clock_offs[b] : h->h_clock_next[b]; // (sb_clock_set_offsets: its next offset)
    const long long now = (long long)off + std::max(0LL, (long long)h->clock_pos - restart_pos);
    if (now > (long long)h->clock_n_rows - 2)
      return fail(SB_ERR_INVALID, "sb_reset_buildings: building " + std::to_string(b) + ": restarting at position " +
                                      std::to_string(restart_pos) + " with the clock at " + std::to_string(h->clock_pos) +
                                      " leaves no two rows of the table's " + std::to_string(h->clock_n_rows));
  }
  if (!any) return SB_OK;
  SB_ON_DEVICE(h->device);
  SB_CHECK(upload_mask(h, mask_host, "sb_reset_buildings", (hipStream_t)stream));
  if (!h->ep_start.p) SB_CHECK(alloc_zero(h->ep_start, (size_t)B));
  if (h->em_draws.attached) SB_CHECK(sb_episode_metrics_close(h, h->ep_mask.p, (hipStream_t)stream)); // the masked buildings' totals latched
  if (h->tl_draws.attached) SB_CHECK(sb_telemetry_close(h, h->ep_mask.p, (hipStream_t)stream)); // ... and their scores against the recording
  if (h->rz_draws.attached) SB_CHECK(sb_randomization_redraw(h, h->ep_mask.p, (hipStream_t)stream)); // the masked buildings' new rows
  if (h->es_draws.attached) SB_CHECK(sb_episode_starts_redraw(h, h->ep_mask.p, (hipStream_t)stream)); // ... their starts and weather
  launch_reset(h, EpisodeArgs{h->ep_mask.p, h->ep_start.p, clk ? h->clock_eff.p : nullptr, h->clock_offs.p, restart_pos},
               initial_temp, temps_dev, (hipStream_t)stream);
  SB_HIP(hipGetLastError());
  h->own_prev = h->ep_dirty = true;
  if (clk) {
    if (h->restart_pos.empty()) h->restart_pos.assign((size_t)B, 0);
    for (int b = 0; b < B; ++b)
      if (mask_host[b]) {
        h->restart_pos[b] = restart_pos;
        if (!h->h_clock_next.empty()) h->h_clock_offs[b] = h->h_clock_next[b];
      }
    if (h->es_draws.attached) sb_episode_starts_after_reset(h, mask_host);
    episode_bounds(h);
  } else if (h->es_draws.attached) {
    sb_episode_starts_after_reset(h, mask_host);
  }
  return SB_OK;
}

int sb_set_temps(sb_handle *h, const double *temps_dev, void *stream) {
  if (!h || !temps_dev) return fail(SB_ERR_INVALID, "sb_set_temps: null argument");
  if (!h->was_reset) return fail(SB_ERR_INVALID, "sb_set_temps: sb_reset first");
  if (h->kernel == SB_KERNEL_JACOBI) return fail(SB_ERR_UNSUPPORTED, "sb_set_temps: not implemented for the Jacobi solver");
  SB_ON_DEVICE(h->device);
  const int wpb = 4;
  const int blocks = std::min((h->d.B + wpb - 1) / wpb, 4096);
  hipLaunchKernelGGL(k_reset, dim3(blocks), dim3(64 * wpb), 0, (hipStream_t)stream, h->d, EpisodeArgs{}, 0.0, temps_dev, 0, 0, 1);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

// The handle's clock as the kernels take it (sb_clock_attach / sb_clock_seek); rows == NULL without one.
static int launch_observe(sb_handle *h, const sb_step_in &in, const double *t_amb_b, float *obs_dev, void *stream,
                          const uint8_t *mask_host = nullptr) {
  ClockView clk;
  SB_CHECK(handle_clock_view(h, mask_host ? "sb_observe_buildings" : "sb_observe", &clk));
  SB_ON_DEVICE(h->device);
  const uint8_t *mask = nullptr;
  if (mask_host) {
    if (!std::any_of(mask_host, mask_host + h->d.B, [](uint8_t m) { return m != 0; })) return SB_OK;
    SB_CHECK(upload_mask(h, mask_host, "sb_observe_buildings", (hipStream_t)stream));
    mask = h->ep_mask.p;
  }
  const int blocks = std::max(1, std::min((h->d.B + 63) / 64, 4096));
  if (clk.rows) hipLaunchKernelGGL(k_observe<true>, dim3(blocks), dim3(64), 0, (hipStream_t)stream, h->d, clk, in, t_amb_b, obs_dev, mask);
  else hipLaunchKernelGGL(k_observe<false>, dim3(blocks), dim3(64), 0, (hipStream_t)stream, h->d, clk, in, t_amb_b, obs_dev, mask);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

int sb_observe_buildings(sb_handle *h, const uint8_t *mask_host, const sb_step_in *in, float *obs_dev, void *stream) {
  if (!h || !mask_host || !in || !obs_dev) return fail(SB_ERR_INVALID, "sb_observe_buildings: null argument");
  return launch_observe(h, *in, nullptr, obs_dev, stream, mask_host);
}

int sb_observe_occupancy(sb_handle *h, const float aux[SB_NUM_AUX], double t_amb, const double *t_amb_dev,
                         const float *num_occupants_dev, double occupancy_norm, float *obs_dev, void *stream) {
  if (!h || !aux || !obs_dev) return fail(SB_ERR_INVALID, "sb_observe: null argument");
  sb_step_in in{};
  in.t_amb_now = t_amb;
  in.num_occupants_dev = num_occupants_dev;
  in.occupancy_norm = occupancy_norm;
  std::copy_n(aux, SB_NUM_AUX, in.aux);
  return launch_observe(h, in, t_amb_dev, obs_dev, stream);
}

int sb_observe_step_in(sb_handle *h, const sb_step_in *in, float *obs_dev, void *stream) {
  if (!h || !in || !obs_dev) return fail(SB_ERR_INVALID, "sb_observe_step_in: null argument");
  return launch_observe(h, *in, nullptr, obs_dev, stream);
}

int sb_observe(sb_handle *h, const float aux[SB_NUM_AUX], double t_amb, const double *t_amb_dev,
               float *obs_dev, void *stream) {
  return sb_observe_occupancy(h, aux, t_amb, t_amb_dev, nullptr, 0.0, obs_dev, stream);
}

int sb_step_phases(sb_handle *h, const float *actions_dev, const sb_step_in *in, float *obs_dev,
                   float *reward_dev, float *info_dev, void *stream, int32_t phases) {
  if (!h || !in || !reward_dev) return fail(SB_ERR_INVALID, "sb_step: null argument");
  if (in->has_action && !actions_dev) return fail(SB_ERR_INVALID, "sb_step: has_action set but actions_dev is NULL");
  StepArgs s;
  s.actions = actions_dev; s.obs = obs_dev; s.reward = reward_dev; s.info = info_dev; s.in = *in;
  if (!info_dev && h->em_draws.attached) s.info = h->em_info.p; // the episode metrics sum info columns: k_post writes the library's own rows
  SB_CHECK(handle_clock_view(h, "sb_step", &s.clk));
  SB_ON_DEVICE(h->device);
  const Dev &d = h->d;
  const int blocks = std::max(1, std::min((d.B + kRowsPerBlock - 1) / kRowsPerBlock, h->cus * 32)); // a 16-lane row per building
  if (phases & SB_PHASE_PRE) {
    launch_pre(h, s, dim3(blocks), (hipStream_t)stream, -1);
    SB_HIP(hipGetLastError());
    h->counters_zeroed_on = stream; // k_pre zeroes the sweep kernel's draw counters
  }
  if (phases & SB_PHASE_SWEEP) {
    // without a k_pre in front of it ON THIS STREAM since the last sweep launch (phase by phase: bench.py brackets the
    // sweep with events, so k_pre came with the previous call), the counters are zeroed here -- two more dispatches
    if (h->counters_zeroed_on != stream) {
      SB_HIP(hipMemsetAsync(d.next_b, 0, sizeof(int), (hipStream_t)stream));
      if (d.redo_ctr) SB_HIP(hipMemsetAsync(d.redo_ctr, 0, 2 * sizeof(int), (hipStream_t)stream));
    }
    h->counters_zeroed_on = (void *)(uintptr_t)1; // (no stream)
    const int e = launch_sweep(h, (hipStream_t)stream);
    if (e != (int)hipSuccess)
      return fail(SB_ERR_HIP, std::string("sweep kernel launch: ") + hipGetErrorString((hipError_t)e));
  }
  if (phases & SB_PHASE_POST) {
    if (h->conv_attached) { // simulator_flexible_floor_plan.py:156: after the FD update; the zone sums of
      const int rc = sb_launch_convection(h, (hipStream_t)stream); // k_post do not change (values move inside rooms)
      if (rc != SB_OK) return rc;
    } else if (seeded_in_force(h)) { // sb_convection_attach_seeded: the same place, the reference's own draws per building
      const int rc = sb_launch_convection_seeded(h, (hipStream_t)stream);
      if (rc != SB_OK) return rc;
    }
    launch_post(h, s, dim3(std::max(1, std::min((d.B + 63) / 64, h->cus * 16))), (hipStream_t)stream, -1);
    ++h->steps_since_reset;
    SB_HIP(hipGetLastError());
    if (h->em_draws.attached) SB_CHECK(sb_episode_metrics_step(h, reward_dev, s.info, (hipStream_t)stream)); // a launch of its own: k_post is untouched
    if (h->tl_draws.attached) SB_CHECK(sb_telemetry_step(h, (hipStream_t)stream)); // the zone means k_post left, against the recording
  }
  return SB_OK;
}

int sb_step(sb_handle *h, const float *actions_dev, const sb_step_in *in, float *obs_dev,
            float *reward_dev, float *info_dev, void *stream) {
  return sb_step_phases(h, actions_dev, in, obs_dev, reward_dev, info_dev, stream,
                        SB_PHASE_PRE | SB_PHASE_SWEEP | SB_PHASE_POST);
}

int sb_get_temps(sb_handle *h, double *out_dev, void *stream) {
  if (!h || !out_dev) return fail(SB_ERR_INVALID, "sb_get_temps: null argument");
  SB_ON_DEVICE(h->device);
  if (h->kernel == SB_KERNEL_JACOBI)
    hipLaunchKernelGGL(k_copy_temps_jacobi, dim3(2048), dim3(256), 0, (hipStream_t)stream, h->jgrid.p,
                       (size_t)h->d.B * h->d.N, out_dev);
  else
    hipLaunchKernelGGL(k_copy_temps, dim3(2048), dim3(256), 0, (hipStream_t)stream, h->d, out_dev);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

int sb_get_scalars(sb_handle *h, double *out_dev, void *stream) {
  if (!h || !out_dev) return fail(SB_ERR_INVALID, "sb_get_scalars: null argument");
  SB_ON_DEVICE(h->device);
  hipLaunchKernelGGL(k_copy_scalars, dim3(256), dim3(256), 0, (hipStream_t)stream, h->d, out_dev);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

#define SB_COPY_OUT(name, src, count, type)                                                       \
  int name(sb_handle *h, type *out_dev, void *stream) {                                           \
    if (!h || !out_dev) return fail(SB_ERR_INVALID, #name ": null argument");                     \
    SB_ON_DEVICE(h->device);                                                              \
    SB_HIP(hipMemcpyAsync(out_dev, src, (size_t)(count) * sizeof(type), hipMemcpyDeviceToDevice,  \
                          (hipStream_t)stream));                                                  \
    return SB_OK;                                                                                 \
  }
SB_COPY_OUT(sb_get_zone_temps, h->d.zmean, (size_t)h->d.B *h->d.Z, double)
int sb_get_modes(sb_handle *h, int32_t *out_dev, void *stream) {
  if (!h || !out_dev) return fail(SB_ERR_INVALID, "sb_get_modes: null argument");
  SB_ON_DEVICE(h->device);
  hipLaunchKernelGGL(k_copy_modes, dim3(256), dim3(256), 0, (hipStream_t)stream, h->d, out_dev);
  SB_HIP(hipGetLastError());
  return SB_OK;
}
SB_COPY_OUT(sb_get_zone_power, h->d.qz, (size_t)h->d.B *h->d.Z, double)

/* ---- state snapshots ---- */
static int check_state_view(const sb_handle *h, const sb_state_view *v, const char *who) {
  const std::string w(who);
  if (!v) return fail(SB_ERR_INVALID, w + ": null view");
  if (v->n <= 0) return fail(SB_ERR_INVALID, w + ": the view needs n > 0 rows");
  if (!v->grid || !v->zone || !v->mode || !v->scal || !v->nsw) return fail(SB_ERR_INVALID, w + ": null view field");
  if ((uintptr_t)v->grid % 16) return fail(SB_ERR_INVALID, w + ": grid must be 16-byte aligned");
  if ((v->occ != nullptr) != h->occ_attached)
    return fail(SB_ERR_INVALID, w + (h->occ_attached ? ": the handle has device occupancy: occ is needed"
                                                     : ": occ given, but the handle has no device occupancy"));
  return SB_OK;
}

static void launch_state(const sb_handle *h, bool save, const int32_t *pick, int rows, const sb_state_view *v,
                         int transposed, hipStream_t stream) {
  const int count = save ? rows : h->d.B;
  const dim3 grid(std::max(1, std::min(count, h->cus * 8))), block(kStateThreads);
  uint32_t *occ = v->occ ? h->occ_state.p : nullptr;
  if (save) hipLaunchKernelGGL(k_state<true>, grid, block, 0, stream, h->d, *v, occ, pick, rows, transposed);
  else hipLaunchKernelGGL(k_state<false>, grid, block, 0, stream, h->d, *v, occ, pick, rows, transposed);
}

int sb_state_save(sb_handle *h, const int32_t *pick_dev, int32_t n, const sb_state_view *view,
                  sb_state_clock *clock_out, int32_t transposed, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_state_save: null handle");
  if (h->kernel == SB_KERNEL_JACOBI) return fail(SB_ERR_UNSUPPORTED, "sb_state_save: not implemented for the Jacobi solver");
  SB_CHECK(check_state_view(h, view, "sb_state_save"));
  if (n <= 0 || n > view->n) return fail(SB_ERR_INVALID, "sb_state_save: need 0 < n <= view->n");
  if (!pick_dev && n != h->d.B) return fail(SB_ERR_INVALID, "sb_state_save: without pick_dev, n must be the batch size");
  SB_ON_DEVICE(h->device);
  launch_state(h, true, pick_dev, n, view, transposed, (hipStream_t)stream);
  SB_HIP(hipGetLastError());
  if (clock_out) *clock_out = sb_state_clock{h->occ_queries, h->conv_calls, h->steps_since_reset, h->was_reset ? 1 : 0};
  return SB_OK;
}

int sb_state_load(sb_handle *h, const int32_t *pick_dev, const sb_state_view *view, const sb_state_clock *clock_in,
                  int32_t transposed, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_state_load: null handle");
  if (h->kernel == SB_KERNEL_JACOBI) return fail(SB_ERR_UNSUPPORTED, "sb_state_load: not implemented for the Jacobi solver");
  SB_CHECK(check_state_view(h, view, "sb_state_load"));
  if (!pick_dev && view->n != h->d.B) return fail(SB_ERR_INVALID, "sb_state_load: without pick_dev, view->n must be the batch size");
  if (clock_in && clock_in->steps_since_reset < 0) return fail(SB_ERR_INVALID, "sb_state_load: negative steps_since_reset");
  if (h->ep_dirty || h->own_prev) // the snapshot carries neither the buildings' restart positions nor their own step counts
    return fail(SB_ERR_INVALID, "sb_state_load: buildings were reset by themselves (sb_reset_buildings) since the last sb_reset: "
                                "their episode positions are not in a snapshot; sb_reset first");
  SB_ON_DEVICE(h->device);
  launch_state(h, false, pick_dev, 0, view, transposed, (hipStream_t)stream);
  SB_HIP(hipGetLastError());
  if (clock_in) {
    h->occ_queries = clock_in->occ_queries;
    h->conv_calls = clock_in->conv_calls;
    h->steps_since_reset = clock_in->steps_since_reset;
    h->was_reset = clock_in->was_reset != 0;
  }
  return SB_OK;
}

/* ---- per-building parameters ---- */
static_assert(offsetof(sb_params, w_carbon) - offsetof(sb_params, vav_max_air_flow) ==
                  (SB_NUM_BUILDING_PARAMS - 1) * sizeof(double),
              "sb_building_param numbers the contiguous double fields vav_max_air_flow .. w_carbon of sb_params");

static const char *const kBuildingParamNames[SB_NUM_BUILDING_PARAMS] = {
    "vav_max_air_flow", "vav_max_water_flow", "ahu_recirc", "ahu_heat_sp", "ahu_cool_sp", "ahu_dp", "ahu_eff",
    "ahu_max_flow", "blr_setpoint", "blr_head", "blr_pump_eff", "blr_heating_rate", "blr_cooling_rate", "blr_conv",
    "blr_len", "blr_radius", "blr_capacity", "blr_ins_k", "blr_ins_thick", "comfort_lo", "comfort_hi", "eco_lo",
    "eco_hi", "max_prod", "min_prod", "max_elec", "max_gas", "prod_delta", "prod_stiff", "w_prod", "w_cost",
    "w_carbon"};
} // extern "C"
const char *building_param_name(int k) { return kBuildingParamNames[k]; }
extern "C" {

// Building b's effective row (tab: [SB_NUM_BUILDING_PARAMS][B]) against the reference's constructor checks.
static int check_building_row(const std::vector<double> &tab, int B, int b) {
  auto v = [&](int k) { return tab[(size_t)k * B + b]; };
  const std::string at = "sb_set_building_params: building " + std::to_string(b) + ": ";
  for (int k = 0; k < SB_NUM_BUILDING_PARAMS; ++k)
    if (!std::isfinite(v(k))) return fail(SB_ERR_INVALID, at + kBuildingParamNames[k] + " is not finite");
  // fields the device algebra divides by (sb_device.h: the VAV's supply temperature, the fan power and speed, the pump,
  // the tank's heat loss) and the rest of the boiler's geometry
  static const int positive[] = {SB_BP_VAV_MAX_AIR_FLOW, SB_BP_AHU_EFF, SB_BP_AHU_MAX_FLOW, SB_BP_BLR_PUMP_EFF,
                                 SB_BP_BLR_CONV, SB_BP_BLR_LEN, SB_BP_BLR_RADIUS, SB_BP_BLR_INS_K, SB_BP_BLR_INS_THICK};
  for (const int k : positive)
    if (!(v(k) > 0.0)) return fail(SB_ERR_INVALID, at + kBuildingParamNames[k] + " must be positive");
  if (!(v(SB_BP_W_PROD) + v(SB_BP_W_COST) + v(SB_BP_W_CARBON) > 0.0))
    return fail(SB_ERR_INVALID, at + "w_prod + w_cost + w_carbon must be positive");
  if (v(SB_BP_AHU_COOL_SP) <= v(SB_BP_AHU_HEAT_SP)) // air_handler.py:60-64
    return fail(SB_ERR_INVALID, at + "ahu_cool_sp: cooling_air_temp_setpoint must greater than heating_air_temp_setpoint");
  if (v(SB_BP_COMFORT_LO) > v(SB_BP_COMFORT_HI)) // setpoint_schedule.py:66-75
    return fail(SB_ERR_INVALID, at + "comfort_lo: comfort_temp_window[0] must be less than comfort_temp_window[1]");
  if (v(SB_BP_ECO_LO) > v(SB_BP_ECO_HI))
    return fail(SB_ERR_INVALID, at + "eco_lo: eco_temp_window[0] must be less than eco_temp_window[1]");
  return SB_OK;
}

int sb_set_building_params(sb_handle *h, int32_t n_fields, const int32_t *fields, const double *values, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_set_building_params: null handle");
  if (n_fields < 0 || n_fields > SB_NUM_BUILDING_PARAMS)
    return fail(SB_ERR_INVALID, "sb_set_building_params: n_fields must be in 0 .. SB_NUM_BUILDING_PARAMS");
  if (n_fields > 0 && (!fields || !values)) return fail(SB_ERR_INVALID, "sb_set_building_params: null argument");
  if (h->rz_draws.attached)
    return fail(SB_ERR_INVALID, "sb_set_building_params: a randomisation is attached, which owns the rows (sb_randomization_detach first)");
  const int B = h->d.B;
  std::vector<double> tab;
  if (n_fields > 0) {
    bool named[SB_NUM_BUILDING_PARAMS] = {};
    for (int i = 0; i < n_fields; ++i) {
      const int k = fields[i];
      if (k < 0 || k >= SB_NUM_BUILDING_PARAMS)
        return fail(SB_ERR_INVALID, "sb_set_building_params: unknown field " + std::to_string(k));
      if (named[k]) return fail(SB_ERR_INVALID, std::string("sb_set_building_params: field ") + kBuildingParamNames[k] + " named twice");
      named[k] = true;
    }
    tab.resize((size_t)SB_NUM_BUILDING_PARAMS * B); // every field sb_params' value, then the named rows over it
    for (int k = 0; k < SB_NUM_BUILDING_PARAMS; ++k) std::fill_n(tab.begin() + (size_t)k * B, B, param_field(h->d.p, k));
    for (int i = 0; i < n_fields; ++i) std::copy_n(values + (size_t)i * B, B, tab.begin() + (size_t)fields[i] * B);
    for (int b = 0; b < B; ++b) SB_CHECK(check_building_row(tab, B, b));
  }
  SB_ON_DEVICE(h->device);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  SB_HIP(hipStreamIsCapturing((hipStream_t)stream, &cap));
  if (cap != hipStreamCaptureStatusNone)
    return fail(SB_ERR_INVALID, "sb_set_building_params: not while the stream is being captured into a graph");
  // the kernels already queued on `stream` read the old table: the new one is copied after them, and the stream is
  // drained before the old buffer goes (a dropped table) or the call returns (the host rows may be freed)
  if (n_fields == 0) {
    SB_HIP(hipStreamSynchronize((hipStream_t)stream));
    h->d.bp = nullptr;
    if (h->bp.p) {
      SB_HIP(hipFree(h->bp.p));
      h->bp.p = nullptr;
    }
    return SB_OK;
  }
  if (!h->bp.p) SB_HIP(hipMalloc((void **)&h->bp.p, tab.size() * sizeof(double)));
  SB_HIP(hipMemcpyAsync(h->bp.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
  SB_HIP(hipStreamSynchronize((hipStream_t)stream));
  h->d.bp = h->bp.p;
  return SB_OK;
}

/* ---- per-building materials ---- */
} // extern "C"
std::string material_field_name(int f, int M) {
  static const char *const kinds[3] = {"conductivity", "heat_capacity", "density"};
  if (f == 3 * M) return "h_conv";
  return std::string(kinds[f / M]) + "[" + std::to_string(f % M) + "]";
}
extern "C" {

int sb_set_building_materials(sb_handle *h, int32_t n_fields, const int32_t *fields, const double *values, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_set_building_materials: null handle");
  if (!h->materials)
    return fail(SB_ERR_UNSUPPORTED, "sb_set_building_materials: the handle has one coefficient table for every building "
                                    "(sb_create / sb_create_jacobi); create it with sb_create_materials");
  if (h->rz_draws.attached)
    return fail(SB_ERR_INVALID, "sb_set_building_materials: a randomisation is attached, which owns the rows (sb_randomization_detach first)");
  const int M = h->mat_slots, F = 3 * M + 1, B = h->d.B;
  if (n_fields < 0 || n_fields > F)
    return fail(SB_ERR_INVALID, "sb_set_building_materials: n_fields must be in 0 .. 3 * n_slots + 1");
  if (n_fields > 0 && (!fields || !values)) return fail(SB_ERR_INVALID, "sb_set_building_materials: null argument");
  std::vector<double> tab;
  if (n_fields > 0) {
    std::vector<char> named((size_t)F, 0);
    for (int i = 0; i < n_fields; ++i) {
      const int f = fields[i];
      if (f < 0 || f >= F) return fail(SB_ERR_INVALID, "sb_set_building_materials: unknown field " + std::to_string(f));
      if (named[f]) return fail(SB_ERR_INVALID, "sb_set_building_materials: field " + material_field_name(f, M) + " named twice");
      named[f] = 1;
    }
    tab.resize((size_t)F * B); // every field the plan's own value, then the named rows over it
    for (int f = 0; f < F; ++f) std::fill_n(tab.begin() + (size_t)f * B, B, h->mat_default[f]);
    for (int i = 0; i < n_fields; ++i) std::copy_n(values + (size_t)i * B, B, tab.begin() + (size_t)fields[i] * B);
    for (int b = 0; b < B; ++b)
      for (int f = 0; f < F; ++f) {
        const double v = tab[(size_t)f * B + b];
        const char *what = !std::isfinite(v) ? " is not finite" : f < 3 * M && !(v > 0.0) ? " must be positive"
                           : f == 3 * M && v < 0.0 ? " must not be negative" : nullptr;
        if (what)
          return fail(SB_ERR_INVALID, "sb_set_building_materials: building " + std::to_string(b) + ": " +
                                          material_field_name(f, M) + what);
      }
  }
  SB_ON_DEVICE(h->device);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  SB_HIP(hipStreamIsCapturing((hipStream_t)stream, &cap));
  if (cap != hipStreamCaptureStatusNone)
    return fail(SB_ERR_INVALID, "sb_set_building_materials: not while the stream is being captured into a graph");
  // ordered on `stream`: the steps already queued there read the old rows, k_class_coef writes the new ones after them
  SB_CHECK(apply_building_materials(h, tab, (hipStream_t)stream));
  return SB_OK;
}

int sb_get_building_coef(sb_handle *h, double *out_dev, void *stream) {
  if (!h || !out_dev) return fail(SB_ERR_INVALID, "sb_get_building_coef: null argument");
  if (!h->materials)
    return fail(SB_ERR_UNSUPPORTED, "sb_get_building_coef: the handle has no coefficient rows per building (sb_create_materials)");
  SB_ON_DEVICE(h->device);
  const size_t row = (size_t)h->d.ncls * 8 * sizeof(double); // the pad row stays behind
  SB_HIP(hipMemcpy2DAsync(out_dev, row, h->ctab_b.p, row + 8 * sizeof(double), row, (size_t)h->d.B, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
  return SB_OK;
}

/* ---- a calendar per building ---- */
static const char *const kClockFieldNames[SB_CLOCK_FIELDS] = {
    "t_amb", "weather_f", "weather_t", "comfort", "aux[0]", "aux[1]", "aux[2]", "aux[3]", "aux[4]", "aux[5]", "aux[6]",
    "occupancy", "e_price", "e_carbon", "g_price", "g_carbon", "occ_hour", "occ_workday", "occ_hour5", "occ_workday5"};

static int drop_clock(sb_handle *h) { // the kernels in flight read the table: it goes once the device is idle
  if (!h->clock_rows.p && !h->clock_offs.p && !h->clock_eff.p) return SB_OK;
  SB_HIP(hipDeviceSynchronize());
  if (h->clock_rows.p) SB_HIP(hipFree(h->clock_rows.p));
  h->clock_rows.p = nullptr;
  if (h->clock_offs.p) SB_HIP(hipFree(h->clock_offs.p));
  h->clock_offs.p = nullptr;
  if (h->clock_eff.p) SB_HIP(hipFree(h->clock_eff.p));
  h->clock_eff.p = nullptr;
  h->h_clock_offs.clear();
  h->h_clock_next.clear();
  sb_episode_starts_forget(h);
  h->restart_pos.clear(); // a clock attached later starts from its own offsets and reads its own previous row
  h->own_prev = false;
  h->max_restart = 0;
  h->clock_n_rows = h->clock_max_off = 0;
  h->clock_pos = h->clock_prev = -1;
  return SB_OK;
}

int sb_clock_attach(sb_handle *h, const double *rows_host, int32_t n_rows, int32_t n_fields, const int32_t *offsets_host) {
  if (!h || !rows_host || !offsets_host) return fail(SB_ERR_INVALID, "sb_clock_attach: null argument");
  if (n_fields != SB_CLOCK_FIELDS)
    return fail(SB_ERR_INVALID, "sb_clock_attach: n_fields is " + std::to_string(n_fields) + ", this library's rows have " +
                                    std::to_string((int)SB_CLOCK_FIELDS) + " fields (sb_clock_field)");
  if (n_rows > SB_CLOCK_MAX_ROWS) return fail(SB_ERR_TOO_LARGE, "sb_clock_attach: more than 2^22 rows");
  if (n_rows < 2) return fail(SB_ERR_INVALID, "sb_clock_attach: a step reads two rows: n_rows must be at least 2");
  const int B = h->d.B;
  int max_off = 0;
  for (int b = 0; b < B; ++b) {
    if (offsets_host[b] < 0)
      return fail(SB_ERR_INVALID, "sb_clock_attach: building " + std::to_string(b) + ": negative offset " + std::to_string(offsets_host[b]));
    if (offsets_host[b] > n_rows - 2)
      return fail(SB_ERR_INVALID, "sb_clock_attach: building " + std::to_string(b) + ": offset " + std::to_string(offsets_host[b]) +
                                      " leaves no two rows of the table's " + std::to_string(n_rows));
    max_off = std::max(max_off, (int)offsets_host[b]);
  }
  for (size_t i = 0; i < (size_t)n_rows * SB_CLOCK_FIELDS; ++i)
    if (!std::isfinite(rows_host[i]))
      return fail(SB_ERR_INVALID, "sb_clock_attach: row " + std::to_string(i / SB_CLOCK_FIELDS) + ": " +
                                      kClockFieldNames[i % SB_CLOCK_FIELDS] + " is not finite");
  SB_ON_DEVICE(h->device);
  SB_CHECK(drop_clock(h));
  SB_CHECK(upload(h->clock_rows, rows_host, (size_t)n_rows * SB_CLOCK_FIELDS));
  SB_CHECK(upload(h->clock_offs, offsets_host, (size_t)B));
  SB_CHECK(upload(h->clock_eff, offsets_host, (size_t)B)); // every building on its attached offset until sb_reset_buildings
  h->h_clock_offs.assign(offsets_host, offsets_host + B);
  h->clock_n_rows = n_rows;
  h->clock_max_off = max_off;
  return SB_OK;
}

int sb_clock_seek(sb_handle *h, int32_t pos, int32_t prev_pos) {
  if (!h) return fail(SB_ERR_INVALID, "sb_clock_seek: null handle");
  if (!h->clock_rows.p) return fail(SB_ERR_INVALID, "sb_clock_seek: sb_clock_attach first");
  if (pos < 0 || prev_pos < -1) return fail(SB_ERR_INVALID, "sb_clock_seek: pos must be >= 0 and prev_pos >= -1");
  // (64-bit sums: the rows a kernel reads stay inside the table whatever the arguments)
  if ((long long)h->clock_max_off + pos > (long long)h->clock_n_rows - 2 ||
      (long long)h->clock_max_off + prev_pos > (long long)h->clock_n_rows - 1)
    return fail(SB_ERR_INVALID, "sb_clock_seek: position " + std::to_string(pos) + " (previous " + std::to_string(prev_pos) +
                                    ") plus the largest offset " + std::to_string(h->clock_max_off) + " runs past the table's " +
                                    std::to_string(h->clock_n_rows) + " rows");
  if (pos < h->max_restart) // (sb_reset_buildings) a building's rows start at its restart position: below it, row < its offset -- or < 0
    return fail(SB_ERR_INVALID, "sb_clock_seek: position " + std::to_string(pos) + " is below a building's restart position " +
                                    std::to_string(h->max_restart) + " (sb_reset_buildings)");
  h->clock_pos = pos;
  h->clock_prev = prev_pos;
  return SB_OK;
}

int sb_clock_detach(sb_handle *h) {
  if (!h) return fail(SB_ERR_INVALID, "sb_clock_detach: null handle");
  SB_ON_DEVICE(h->device);
  return drop_clock(h);
}

/* ---- start temperatures per building ---- */
static int drop_initial_conditions(sb_handle *h) { // the kernels in flight read the arrays: they go once the device is idle
  if (!h->ic_draws.attached) return SB_OK;
  SB_HIP(hipDeviceSynchronize());
  h->ic_draws.attached = false; // (launch_reset: the kernels of the handle without, from here on)
  drop(h->ic_grids); drop(h->ic_grid_of); drop(h->ic_base); drop(h->ic_offset); drop(h->ic_draws.episode);
  h->ic_n_grids = 0;
  h->ic_jitter = false;
  return SB_OK;
}

int sb_initial_conditions_attach(sb_handle *h, const sb_initial_conditions *ic) {
  const std::string who = "sb_initial_conditions_attach: ";
  if (!h || !ic) return fail(SB_ERR_INVALID, who + "null argument");
  const int B = h->d.B;
  const size_t N = (size_t)h->d.N;
  if (ic->n_grids < 0 || (ic->grids != nullptr) != (ic->n_grids > 0))
    return fail(SB_ERR_INVALID, who + "reset_temp_values: grids and n_grids >= 1 go together");
  if (ic->n_grids > 1 && !ic->grid_of) return fail(SB_ERR_INVALID, who + "grid_of: needed with more than one grid");
  if (ic->grid_of && !ic->grids) return fail(SB_ERR_INVALID, who + "grid_of: given without grids");
  if (ic->grids && ic->initial_temp)
    return fail(SB_ERR_INVALID, who + "initial_temp: not together with grids (two bases)");
  if (!ic->grids && !ic->initial_temp && !ic->offset && !ic->has_jitter)
    return fail(SB_ERR_INVALID, who + "no field given (sb_initial_conditions_detach returns to the handle without)");
  if (ic->first_building < 0) return fail(SB_ERR_INVALID, who + "first_building must be >= 0");
  for (size_t i = 0; i < (size_t)ic->n_grids * N; ++i)
    if (!std::isfinite(ic->grids[i]))
      return fail(SB_ERR_INVALID, who + "reset_temp_values: grid " + std::to_string(i / N) + " cell " + std::to_string(i % N) + " is not finite");
  const struct { const char *name; const double *v; } rows[] = {{"initial_temp", ic->initial_temp}, {"offset", ic->offset}};
  for (int b = 0; b < B; ++b) {
    if (ic->grid_of && (ic->grid_of[b] < 0 || ic->grid_of[b] >= ic->n_grids))
      return fail(SB_ERR_INVALID, who + "building " + std::to_string(b) + ": grid_of " + std::to_string(ic->grid_of[b]) +
                                      " is outside the " + std::to_string(ic->n_grids) + " grids");
    for (const auto &r : rows)
      if (r.v && !std::isfinite(r.v[b]))
        return fail(SB_ERR_INVALID, who + "building " + std::to_string(b) + ": " + r.name + " is not finite");
  }
  if (ic->has_jitter && !(std::isfinite(ic->jitter_lo) && std::isfinite(ic->jitter_hi) && ic->jitter_lo <= ic->jitter_hi))
    return fail(SB_ERR_INVALID, who + "jitter: needs finite lo <= hi");
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device(who));
  SB_CHECK(drop_initial_conditions(h));
  if (ic->grids) SB_CHECK(upload(h->ic_grids, ic->grids, (size_t)ic->n_grids * N));
  if (ic->grid_of) SB_CHECK(upload(h->ic_grid_of, ic->grid_of, (size_t)B));
  if (ic->initial_temp) SB_CHECK(upload(h->ic_base, ic->initial_temp, (size_t)B));
  if (ic->offset) SB_CHECK(upload(h->ic_offset, ic->offset, (size_t)B));
  SB_CHECK(alloc_zero(h->ic_draws.episode, (size_t)B));
  h->ic_n_grids = ic->n_grids;
  h->ic_jitter = ic->has_jitter != 0;
  h->ic_lo = ic->jitter_lo; h->ic_hi = ic->jitter_hi;
  h->ic_draws.seed = ic->seed;
  h->ic_draws.first = ic->first_building;
  h->ic_draws.attached = true;
  return SB_OK;
}

int sb_initial_conditions_detach(sb_handle *h) {
  if (!h) return fail(SB_ERR_INVALID, "sb_initial_conditions_detach: null handle");
  SB_ON_DEVICE(h->device);
  return drop_initial_conditions(h);
}

static const char *const kNoInitialConditions = "the handle has no initial conditions (sb_initial_conditions_attach)";

int sb_initial_conditions_episodes_get(sb_handle *h, int32_t *out_dev, void *stream) {
  return episodes_get(h, &sb_handle::ic_draws, "sb_initial_conditions_episodes_get", kNoInitialConditions, out_dev, (hipStream_t)stream);
}

int sb_initial_conditions_episodes_set(sb_handle *h, const int32_t *in_dev, void *stream) {
  return episodes_set(h, &sb_handle::ic_draws, "sb_initial_conditions_episodes_set", kNoInitialConditions, in_dev, (hipStream_t)stream);
}

/* ---- the reward function ---- */
int sb_set_reward_function(sb_handle *h, const sb_reward_config *cfg) {
  if (!h) return fail(SB_ERR_INVALID, "sb_set_reward_function: null handle");
  if (!cfg || cfg->kind == SB_REWARD_REGRET) { // the default: sb_params' (or the buildings' rows of) regret arguments
    h->reward = sb_reward_config{};
    return SB_OK;
  }
  if (cfg->kind != SB_REWARD_SETPOINT_ENERGY_CARBON)
    return fail(SB_ERR_INVALID, "sb_set_reward_function: unknown kind " + std::to_string(cfg->kind));
  const struct { const char *name; double v; } fields[] = {
      {"energy_cost_weight", cfg->energy_cost_weight}, {"carbon_cost_weight", cfg->carbon_cost_weight},
      {"carbon_cost_factor", cfg->carbon_cost_factor}, {"normalizer_shift", cfg->normalizer_shift},
      {"normalizer_scale", cfg->normalizer_scale}};
  for (const auto &f : fields)
    if (!std::isfinite(f.v)) return fail(SB_ERR_INVALID, std::string("sb_set_reward_function: ") + f.name + " is not finite");
  if (cfg->normalizer_scale == 0.0)
    return fail(SB_ERR_INVALID, "sb_set_reward_function: normalizer_scale must not be 0 (the reward divides by it)");
  h->reward = *cfg;
  return SB_OK;
}

/* ---- known-answer taps: k_pre / k_post on prescribed state of one building ---- */
int sb_tap_pre(sb_handle *h, int32_t building, const double *zone_temps, const int32_t *modes,
               const double *scalars, const float *actions, const sb_step_in *in, sb_tap_bld *bld,
               double *q_zone, double *damper, int32_t *modes_out) {
  if (!h || !zone_temps || !in) return fail(SB_ERR_INVALID, "sb_tap_pre: null argument");
  const Dev &d = h->d;
  if (building < 0 || building >= d.B) return fail(SB_ERR_INVALID, "sb_tap_pre: building out of range");
  SB_ON_DEVICE(h->device);
  h->counters_zeroed_on = (void *)(uintptr_t)1; // the tap's k_pre runs on one building: the next sweep launch zeroes its counters itself
  SB_HIP(hipDeviceSynchronize());
  const size_t zb = (size_t)building * d.Z;
  SB_HIP(hipMemcpy(d.zmean + zb, zone_temps, sizeof(double) * d.Z, hipMemcpyHostToDevice));
  if (modes) SB_HIP(hipMemcpy(d.mode + zb, modes, sizeof(int32_t) * d.Z, hipMemcpyHostToDevice));
  if (scalars) SB_HIP(hipMemcpy(d.scal + (size_t)building * kNScal, scalars, sizeof(double) * kNScalOut, hipMemcpyHostToDevice));
  DevBuf<float> act;
  if (actions) {
    std::vector<float> all((size_t)d.B * d.p.n_actions, 0.0f);
    for (int i = 0; i < d.p.n_actions; ++i) all[(size_t)building * d.p.n_actions + i] = actions[i];
    int rc = upload(act, all.data(), all.size());
    if (rc != SB_OK) return rc;
  } else if (in->has_action) {
    return fail(SB_ERR_INVALID, "sb_tap_pre: has_action without actions");
  }
  StepArgs s{};
  s.actions = act.p; s.in = *in;
  launch_pre(h, s, dim3(1), nullptr, building); // this building alone
  SB_HIP(hipGetLastError());
  SB_HIP(hipDeviceSynchronize());
  if (bld) {
    Bld v;
    SB_HIP(hipMemcpy(&v, d.bld + building, sizeof(Bld), hipMemcpyDeviceToHost));
    *bld = sb_tap_bld{v.t_now, v.t_next, v.heat_sp, v.cool_sp, v.blr_sp, v.t_sa, v.ahu_flow, v.blr_flow, v.blr_return,
                      v.ahu_count, v.blr_count, v.tank, v.tank_change, v.duration, v.rejected};
  }
  if (q_zone) SB_HIP(hipMemcpy(q_zone, d.qz + zb, sizeof(double) * d.Z, hipMemcpyDeviceToHost));
  if (damper) SB_HIP(hipMemcpy(damper, d.damper + zb, sizeof(double) * d.Z, hipMemcpyDeviceToHost));
  if (modes_out) {
    SB_HIP(hipMemcpy(modes_out, d.mode + zb, sizeof(int32_t) * d.Z, hipMemcpyDeviceToHost));
    for (int z = 0; z < d.Z; ++z) modes_out[z] &= kModeMask;
  }
  return SB_OK;
}

int sb_tap_post(sb_handle *h, int32_t building, const sb_tap_bld *bld, const double *zone_temps,
                double grid_mean, int32_t n_sweeps, const sb_step_in *in, float *reward, float *info) {
  if (!h || !bld || !zone_temps || !in || !reward) return fail(SB_ERR_INVALID, "sb_tap_post: null argument");
  const Dev &d = h->d;
  if (building < 0 || building >= d.B) return fail(SB_ERR_INVALID, "sb_tap_post: building out of range");
  SB_ON_DEVICE(h->device);
  SB_HIP(hipDeviceSynchronize());
  Bld v;
  SB_HIP(hipMemcpy(&v, d.bld + building, sizeof(Bld), hipMemcpyDeviceToHost)); // keeps the fields the tap does not expose
  v.t_now = bld->t_now; v.t_next = bld->t_next; v.heat_sp = bld->heat_sp; v.cool_sp = bld->cool_sp;
  v.blr_sp = bld->blr_sp; v.t_sa = bld->t_sa; v.ahu_flow = bld->ahu_flow; v.blr_flow = bld->blr_flow;
  v.blr_return = bld->blr_return; v.ahu_count = bld->ahu_count; v.blr_count = bld->blr_count;
  v.tank = bld->tank; v.tank_change = bld->tank_change; v.duration = bld->duration; v.rejected = bld->rejected;
  SB_HIP(hipMemcpy(d.bld + building, &v, sizeof(Bld), hipMemcpyHostToDevice));
  std::vector<double> zs(d.Z);
  for (int z = 0; z < d.Z; ++z) zs[z] = zone_temps[z] * (double)(h->h_zone_off[z + 1] - h->h_zone_off[z]);
  SB_HIP(hipMemcpy(d.zsum + (size_t)building * d.Z, zs.data(), sizeof(double) * d.Z, hipMemcpyHostToDevice));
  const double gs = grid_mean * (double)d.N;
  const int nsw = n_sweeps | (1 << 16);
  SB_HIP(hipMemcpy(d.gsum + building, &gs, sizeof(double), hipMemcpyHostToDevice));
  SB_HIP(hipMemcpy(d.nsw + building, &nsw, sizeof(int), hipMemcpyHostToDevice));
  DevBuf<float> rew, inf;
  int rc = alloc_zero(rew, (size_t)d.B);
  if (rc == SB_OK) rc = alloc_zero(inf, (size_t)d.B * SB_INFO_STRIDE);
  if (rc != SB_OK) return rc;
  StepArgs s{};
  s.reward = rew.p; s.info = inf.p; s.in = *in;
  launch_post(h, s, dim3(1), nullptr, building); // this building alone, under the handle's reward function
  SB_HIP(hipGetLastError());
  SB_HIP(hipDeviceSynchronize());
  SB_HIP(hipMemcpy(reward, rew.p + building, sizeof(float), hipMemcpyDeviceToHost));
  if (info) SB_HIP(hipMemcpy(info, inf.p + (size_t)building * SB_INFO_STRIDE, sizeof(float) * SB_INFO_STRIDE, hipMemcpyDeviceToHost));
  return SB_OK;
}

int sb_tap_jacobi(sb_handle *h, int32_t n, const float *tprev, const float *q, const double *tinf, float *grid_out,
                  int32_t *iterations, int32_t *converged) {
  if (!h || !tprev || !q || !tinf) return fail(SB_ERR_INVALID, "sb_tap_jacobi: null argument");
  if (h->kernel != SB_KERNEL_JACOBI) return fail(SB_ERR_INVALID, "sb_tap_jacobi: not a Jacobi handle (sb_create_jacobi)");
  const Dev &d = h->d;
  if (n < 1 || n > d.B) return fail(SB_ERR_INVALID, "sb_tap_jacobi: need 1 <= n <= n_buildings");
  SB_ON_DEVICE(h->device);
  h->counters_zeroed_on = (void *)(uintptr_t)1; // the next sweep launch zeroes the draw counter itself
  SB_HIP(hipDeviceSynchronize());
  const size_t cells = (size_t)n * d.N;
  SB_HIP(hipMemcpy(h->jgrid.p, tprev, cells * sizeof(float), hipMemcpyHostToDevice));
  DevBuf<float> qb;
  DevBuf<double> tb;
  SB_CHECK(upload(qb, q, cells));
  SB_CHECK(upload(tb, tinf, (size_t)n));
  SB_HIP(hipMemset(d.next_b, 0, sizeof(int)));
  JacArgs j = h->jac;
  j.nb = n; j.q = qb.p; j.tinf = tb.p;
  const int e = launch_sweep_jacobi(d, j, h->info.workgroups, nullptr);
  if (e != (int)hipSuccess) return fail(SB_ERR_HIP, std::string("sb_tap_jacobi: ") + hipGetErrorString((hipError_t)e));
  SB_HIP(hipDeviceSynchronize());
  if (grid_out) SB_HIP(hipMemcpy(grid_out, h->jgrid.p, cells * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<int> nsw((size_t)n);
  SB_HIP(hipMemcpy(nsw.data(), d.nsw, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) {
    if (iterations) iterations[i] = nsw[i] & 0xffff;
    if (converged) converged[i] = nsw[i] >> 16;
  }
  return SB_OK;
}

/* Developer aid (not part of the parity/bench path): 16 int64 cycle stamps, host pointer (16 + 2048 when the handle
   was created under SBSIM_DEBUG_TIMELINE=1). */
int sb_debug_phase_cycles(sb_handle *h, long long *out_host) {
  if (!h || !out_host) return fail(SB_ERR_INVALID, "sb_debug_phase_cycles: null argument");
  if (!h->d.dbg) return fail(SB_ERR_INVALID, "sb_debug_phase_cycles: set SBSIM_PHASE_TIMING=1 before sb_create");
  SB_ON_DEVICE(h->device);
  SB_HIP(hipDeviceSynchronize());
  SB_HIP(hipMemcpy(out_host, h->d.dbg, (16 + (h->d.dbg_timeline ? 2048 : 0)) * sizeof(long long), hipMemcpyDeviceToHost));
  return SB_OK;
}

} // extern "C"
