// step_jacobi.hip -- k_sweep_jacobi: TFSimulator's float32 Jacobi update (simulator/tf_simulator.py:573-853 inside the
// loop of simulator.py:340-371), the finite-difference solver of SB1's shipped configuration (SB_KERNEL_JACOBI,
// sb_create_jacobi; the formulas are in include/sbsim_amd.h above sb_jacobi_desc).
//
// One workgroup owns one building at a time: the first buildings by workgroup index, the rest drawn from the counter
// k_pre zeroes.  Both float32 grids of the iteration live in LDS, row-major and untrimmed (every CV is state: exterior
// CVs enter a step holding the last step's T_inf and feed the first iteration).  Thread t owns CVs t, t + THREADS, ...
// and keeps, per CV, a packed word (LDS slot, class), (M*Tprev)/dt and q in registers for the whole step.  An iteration reads a CV and its four neighbours from one buffer, the CV's class row
// from the LDS class table and writes the other buffer; one barrier per iteration publishes both the grid and the
// workgroup's max|T' - T|.  No ordering: lanes take consecutive CVs, so every LDS access of a wavefront is contiguous.
//
// Bitwise rules: one binary32 rounding per operation, in the reference's order (-ffp-contract=off: no fma
// anywhere in this file); den and the T_inf*h products are precomputed exactly as the reference computes them; num / den
// is float((double)num * (1.0 / (double)den)), which is the correctly rounded binary32 quotient: a binary32 quotient is
// never a rounding midpoint and lies >= 2^-49 (relative) away from one, while the two float64 roundings err by < 2^-52
// (tests/test_jacobi_cpu.py checks it over every shipped plan's denominators).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off.
#include "sb_host.h"
#include "sweep_common.h"

namespace sb {
namespace {

// LDS grid layout: row stride Wp = W + 1, CV (r, c) at (r + 1) * Wp + 1 + c.  The slots around the CVs -- a row above,
// a row below and one column shared by the right end of a row and the left end of the next -- hold T_inf, the
// reference's padding (tf_simulator.py:459-488): every neighbour read is unconditional.
constexpr int kJacRow = 12;    // floats per class row in LDS: k1u k3u k2v k4v | uz vz Tinf*hL Tinf*hR | Tinf*hB Tinf*hT 1/den
constexpr unsigned kSlotMask = (1u << 18) - 1;
constexpr int kMaxN = 20480;   // the largest grid of the instantiations (two buffers: 160 KiB with the padding and table)

__host__ __device__ inline int jac_slots(int H, int W) { return ((H + 2) * (W + 1) + 1 + 3) & ~3; }

template <int THREADS, int K>
__global__ void __launch_bounds__(THREADS) k_sweep_jacobi(Dev a, JacArgs j) {
  constexpr int NW = THREADS / 64;
  extern __shared__ float4 lds4[];
  float *const lds = (float *)lds4;
  float *const tab = lds + 2 * j.n_pad;         // [ncls][kJacRow], 16-byte aligned (n_pad % 4 == 0)
  __shared__ float red[2][NW];                  // per wavefront max|dT| of iterations of either parity
  __shared__ double gred[NW];
  __shared__ int next;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, H = a.H, W = a.W, Wp = W + 1;
  const float thr = (float)a.p.conv_threshold;  // NumPy 2: max_delta (float32) <= threshold compares in float32
  const float dtf = (float)a.p.dt;              // tf.constant(time_step_sec, tf.float32)
  const int limit = a.p.iter_limit;

  // the CVs of this thread (not building-dependent): byte offset of the LDS slot | byte offset of the class row << 18
  unsigned cw[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = tid + k * THREADS;
    const int ic = i < N ? i : 0;
    cw[k] = (unsigned)(ic + ic / W + Wp + 1) * 4u | (unsigned)j.cls[ic] * (kJacRow * 4u) << 18;
  }

  for (int b = blockIdx.x; b < j.nb;) {
    const float tinf = (float)(j.tinf ? j.tinf[b] : a.bld[b].t_now); // tf.constant(ambient_temperature, tf.float32)
    // the class table of this step: the T_inf * h products are the reference's scalar_mul(t_temp_inf, h).  An exterior
    // class is all zeros with 1/den = 1 and its CVs carry c0 = T_inf, q = 0: num = ((0 + 0) + T_inf) + 0, T' = T_inf
    // exactly (apply_exterior_temps) with no select in the loop
    for (int c = tid; c < j.ncls; c += THREADS) {
      const float *g = j.tab + c * SB_JACOBI_COEFS;
      float *t = tab + c * kJacRow;
      const bool ext = g[12] != 0.0f;
      t[0] = ext ? 0.0f : g[0]; t[1] = ext ? 0.0f : g[1]; t[2] = ext ? 0.0f : g[2]; t[3] = ext ? 0.0f : g[3];
      t[4] = ext ? 0.0f : g[4]; t[5] = ext ? 0.0f : g[5];
      t[6] = ext ? 0.0f : tinf * g[8]; t[7] = ext ? 0.0f : tinf * g[9];
      t[8] = ext ? 0.0f : tinf * g[11]; t[9] = ext ? 0.0f : tinf * g[10];
      *(double *)(t + 10) = ext ? 1.0 : j.rden[c];
    }
    // the padding of both buffers: the row above (with the slot before it), the shared column, the row below
    const int npad = 2 * (Wp + 1) + H;
    for (int e = tid; e < npad; e += THREADS) {
      const int slot = e <= Wp ? e : e <= Wp + H ? (e - Wp + 1) * Wp : (H + 1) * Wp + (e - Wp - H - 1);
      lds[slot] = tinf;
      lds[j.n_pad + slot] = tinf;
    }
    // Tprev: the grid at the start of the step; (M*Tprev)/dt and q are constants of the step
    float c0[K], qv[K];
    float *const g0 = j.grid + (size_t)b * N;
    const double *gt = a.gtabg + (size_t)b * a.ts;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = tid + k * THREADS;
      c0[k] = qv[k] = 0.0f;
      if (i < N) {
        const unsigned cls = (cw[k] >> 18) / (kJacRow * 4u);
        const float *g = j.tab + cls * SB_JACOBI_COEFS;
        const float tp = g0[i];
        lds[(cw[k] & kSlotMask) / 4] = tp;
        if (g[12] != 0.0f) {
          c0[k] = tinf;
        } else {
          c0[k] = (g[7] * tp) / dtf;
          qv[k] = j.q ? j.q[(size_t)b * N + i] : (float)gt[cls]; // t_input_q = tf.convert_to_tensor(input_q, tf.float32)
        }
      }
    }
    __syncthreads();

    int it = 0, converged = 0;
    while (it < limit) {
      const float *cur = lds + (it & 1) * j.n_pad;
      float *nxt = lds + ((it + 1) & 1) * j.n_pad;
      float dmax = 0.0f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (tid + k * THREADS < N) {
          // (opaque: the slot and class-row addresses are recomputed here rather than hoisted out of the iteration loop,
          // which would hold ~10 registers per CV)
          const unsigned w = (unsigned)sweep::opaque((int)cw[k]);
          const int p = (int)(w & kSlotMask) / 4;
          const float *t = (const float *)((const char *)tab + (w >> 18));
          const float4 r0 = *(const float4 *)t, r1 = *(const float4 *)(t + 4), r2 = *(const float4 *)(t + 8);
          const float T = cur[p];
          // shift_tensor_left -> T[i][j+1] ("left"), shift_tensor_right -> T[i][j-1] ("right"); above / below are
          // T[i-1][j] / T[i+1][j]
          const float tl = cur[p + 1], tr = cur[p - 1], ta = cur[p - Wp], tb = cur[p + Wp];
          float n1 = r0.x * tl;                 // nt1 = vz*(((k1u*TL + k3u*TR) + Tinf*hL) + Tinf*hR)
          n1 = n1 + r0.y * tr;
          n1 = n1 + r1.z;
          n1 = n1 + r1.w;
          n1 = r1.y * n1;
          float n2 = r0.z * tb;                 // nt2 = uz*(((k2v*Tbelow + k4v*Tabove) + Tinf*hB) + Tinf*hT)
          n2 = n2 + r0.w * ta;
          n2 = n2 + r2.x;
          n2 = n2 + r2.y;
          n2 = r1.x * n2;
          float num = n1 + n2;                  // ((nt1 + nt2) + (M*Tprev)/dt) + q
          num = num + c0[k];
          num = num + qv[k];
          const double rden = __hiloint2double(__float_as_int(r2.w), __float_as_int(r2.z));
          const float tn = (float)((double)num * rden);
          nxt[p] = tn;
          dmax = fmaxf(dmax, fabsf(tn - T));
        }
      }
      const float wm = (float)wave_max((double)dmax);
      if (lane == 0) red[it & 1][wave] = wm;
      __syncthreads();                          // the new grid and every wavefront's max|dT|
      float m = red[it & 1][0];
#pragma unroll
      for (int v = 1; v < NW; ++v) m = fmaxf(m, red[it & 1][v]);
      ++it;
      if (m <= thr) { converged = 1; break; }
    }

    // hand-over to k_post: the grid, zone sums and whole-grid sum in float64, iterations | converged << 16
    const float *fin = lds + (it & 1) * j.n_pad;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = tid + k * THREADS;
      if (i < N) {
        const float v = fin[(cw[k] & kSlotMask) / 4];
        g0[i] = v;
        s += (double)v;
      }
    }
    s = wave_sum(s);
    if (lane == 0) gred[wave] = s;
    for (int z = wave; z < a.Z; z += NW) {      // a zone per wavefront, its cells in a fixed order
      double zs = 0.0;
      for (int e = a.zone_off[z] + lane; e < a.zone_off[z + 1]; e += 64) {
        const int i = a.zone_cells_l[e];
        zs += (double)fin[i + i / W + Wp + 1];
      }
      zs = wave_sum(zs);
      if (lane == 0) a.zsum[(size_t)b * a.Z + z] = zs;
    }
    if (tid == 0) next = (int)gridDim.x + atomicAdd(a.next_b, 1);
    __syncthreads();                            // gred, next; every read of this building's LDS is done
    if (tid == 0) {
      double total = gred[0];
      for (int v = 1; v < NW; ++v) total += gred[v];
      a.gsum[b] = total;
      a.nsw[b] = it | (converged << 16);
    }
    b = next;                                   // (next, gred and red are rewritten only after further barriers)
  }
}

// The instantiations: THREADS x K >= N
template <int THREADS, int K>
struct JacCfg {
  static constexpr int threads = THREADS, cells = THREADS * K;
  static const void *fn() { return (const void *)k_sweep_jacobi<THREADS, K>; }
  static void launch(const Dev &d, const JacArgs &j, int wgs, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((k_sweep_jacobi<THREADS, K>), dim3(wgs), dim3(THREADS), lds, s, d, j);
  }
};
using C0 = JacCfg<512, 4>;
using C1 = JacCfg<512, 8>;
using C2 = JacCfg<512, 16>;
using C3 = JacCfg<1024, 20>;
static_assert(C3::cells == kMaxN, "the largest instantiation holds what two LDS buffers hold");

size_t dyn_bytes(int H, int W, int ncls) { return (size_t)2 * jac_slots(H, W) * sizeof(float) + (size_t)ncls * kJacRow * sizeof(float); }

} // namespace

int sweep_jacobi_path(int H, int W, int ncls, bool force_global) {
  const long long N = (long long)H * W;
  if (!force_global && N >= 1 && N <= kMaxN && sweep_jacobi_lds_bytes(H, W, ncls, 0) <= (size_t)160 * 1024) return 0;
  return sweep_jacobi_g_supported(H, W) ? 2 : -1;
}

int sweep_jacobi_threads(int N) { return N <= C2::cells ? C2::threads : C3::threads; }
int sweep_jacobi_threads(int N, int path) { return path == 2 ? sweep_jacobi_g_threads() : sweep_jacobi_threads(N); }

int sweep_jacobi_slots(int H, int W) { return jac_slots(H, W); }

size_t sweep_jacobi_lds_bytes(int H, int W, int ncls, int path) {
  if (path == 2) return sweep_jacobi_g_lds_bytes();
  const int nw = sweep_jacobi_threads(H * W) / 64;
  return dyn_bytes(H, W, ncls) + (size_t)nw * (2 * sizeof(float) + sizeof(double)) + sizeof(int);
}

int sweep_jacobi_blocks_per_cu(int H, int W, int ncls, int path) {
  if (path == 2) return sweep_jacobi_g_blocks_per_cu();
  const int N = H * W;
  const void *fn = N <= C0::cells ? C0::fn() : N <= C1::cells ? C1::fn() : N <= C2::cells ? C2::fn() : C3::fn();
  int n = 0;
  if (prepare_sweep_jacobi(H, W, ncls, path) != (int)hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, sweep_jacobi_threads(N), dyn_bytes(H, W, ncls)) != hipSuccess)
    return 0;
  return n;
}

int prepare_sweep_jacobi(int H, int W, int ncls, int path) {
  if (path == 2) return (int)hipSuccess;        // (static LDS alone)
  const int N = H * W, bytes = (int)dyn_bytes(H, W, ncls);
  const void *fn = N <= C0::cells ? C0::fn() : N <= C1::cells ? C1::fn() : N <= C2::cells ? C2::fn() : C3::fn();
  return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

int launch_sweep_jacobi(const Dev &d, const JacArgs &j, int workgroups, hipStream_t stream) {
  if (j.path == 2) return launch_sweep_jacobi_g(d, j, workgroups, stream);
  const size_t lds = dyn_bytes(d.H, d.W, j.ncls);
  const int wgs = std::max(1, std::min(workgroups, j.nb));
  if (d.N <= C0::cells) C0::launch(d, j, wgs, lds, stream);
  else if (d.N <= C1::cells) C1::launch(d, j, wgs, lds, stream);
  else if (d.N <= C2::cells) C2::launch(d, j, wgs, lds, stream);
  else C3::launch(d, j, wgs, lds, stream);
  return (int)hipGetLastError();
}

} // namespace sb
