// step_jacobi_global.hip -- k_sweep_jacobi_g: k_sweep_jacobi's step (step_jacobi.hip: TFSimulator's float32 Jacobi
// update, the same contract bit for bit) for floor plans whose two float32 grids do not fit one CU's LDS
// (sb_launch_info.path == 2; sweep_jacobi_path in step_jacobi.hip decides).
//
// One workgroup owns one building at a time: the first buildings by workgroup index, the rest drawn from the counter
// k_pre zeroes.  No workgroup ever waits for another.  Each resident workgroup has a scratch area in global memory
// (JacArgs::scratch): the two grids of the iteration in k_sweep_jacobi's padded layout (row stride W + 1, a T_inf row
// above and below: every neighbour read is unconditional) and (M*Tprev)/dt of every CV, computed once per step.  The
// class table of the step lives in LDS, 16 floats per class; in production q depends on the class alone and sits in
// the class row, sb_tap_jacobi's q is read per CV.  Thread t takes CVs t, t + 1024, ...: a wavefront reads and writes
// 64 consecutive CVs of a row (or the end of one row and the start of the next).  An iteration reads one grid and
// writes the other; the one __syncthreads() per iteration publishes the workgroup's max|T' - T| and, because the
// wavefronts of a workgroup share their CU's vector L1, the iteration's global stores (as in k_sweep_stream).
//
// Bitwise rules: those of step_jacobi.hip's header, unchanged.  The float64 zone sums and the grid sum
// are added in k_sweep_jacobi's order (JacArgs::sum_threads: the thread count of the LDS instantiation for this N), so
// the two kernels hand k_post the same bits.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off.
#include "sb_host.h"

namespace sb {
namespace {

constexpr int kThreads = 1024, kNW = kThreads / 64;
constexpr int kRow = 16;        // floats per class row in LDS: k1u k3u k2v k4v | uz vz Tinf*hL Tinf*hR | Tinf*hB Tinf*hT 1/den | q M exterior -
constexpr int kMaxCls = 255;    // sb_create_jacobi: 1 .. 255 classes
constexpr int kMaxN = 1 << 20;  // CVs per plan: what the int slot arithmetic and a sensible scratch area hold
constexpr int kBatch = 4;       // CVs a thread has in flight: their loads are issued before the first is used

// floats of one workgroup's scratch area: two padded grids of n_pad (= sweep_jacobi_slots) floats and (M*Tprev)/dt
__host__ __device__ inline size_t wg_floats(int n_pad, int N) { return (size_t)2 * n_pad + (size_t)((N + 3) & ~3); }

template <bool TAP>
__global__ void __launch_bounds__(kThreads) k_sweep_jacobi_g(Dev a, JacArgs j) {
  __shared__ float4 tab4[kMaxCls * kRow / 4];
  __shared__ float red[2][kNW];                 // per wavefront max|dT| of iterations of either parity
  __shared__ double gred[kNW];
  __shared__ int next;
  float *const tab = (float *)tab4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, H = a.H, W = a.W, Wp = W + 1;
  const float thr = (float)a.p.conv_threshold;
  const float dtf = (float)a.p.dt;
  const int limit = a.p.iter_limit;
  float *const sc = j.scratch + (size_t)blockIdx.x * wg_floats(j.n_pad, N);
  float *const c0g = sc + 2 * j.n_pad;          // [N] (M*Tprev)/dt; T_inf on exterior CVs
  // a thread's CVs are kThreads apart: dr rows and dc columns, with a carry
  const int r_first = tid / W, c_first = tid - r_first * W, dr = kThreads / W, dc = kThreads - dr * W;

  for (int b = blockIdx.x; b < j.nb;) {
    const float tinf = (float)(j.tinf ? j.tinf[b] : a.bld[b].t_now);
    const double *gt = a.gtabg + (size_t)b * a.ts;
    // the class table of this step (k_sweep_jacobi's, with q, M and the exterior flag): an exterior class is all zeros
    // with 1/den = 1, and its CVs carry c0 = T_inf, q = 0: T' = T_inf exactly with no select in the loop
    for (int c = tid; c < j.ncls; c += kThreads) {
      const float *g = j.tab + c * SB_JACOBI_COEFS;
      float *t = tab + c * kRow;
      const bool ext = g[12] != 0.0f;
      t[0] = ext ? 0.0f : g[0]; t[1] = ext ? 0.0f : g[1]; t[2] = ext ? 0.0f : g[2]; t[3] = ext ? 0.0f : g[3];
      t[4] = ext ? 0.0f : g[4]; t[5] = ext ? 0.0f : g[5];
      t[6] = ext ? 0.0f : tinf * g[8]; t[7] = ext ? 0.0f : tinf * g[9];
      t[8] = ext ? 0.0f : tinf * g[11]; t[9] = ext ? 0.0f : tinf * g[10];
      *(double *)(t + 10) = ext ? 1.0 : j.rden[c];
      t[12] = ext || TAP ? 0.0f : (float)gt[c]; // t_input_q = tf.convert_to_tensor(input_q, tf.float32)
      t[13] = g[7];
      t[14] = ext ? 1.0f : 0.0f;
      t[15] = 0.0f;
    }
    // the padding of both grids: the row above (with the slot before it), the shared column, the row below
    const int npad = 2 * (Wp + 1) + H;
    for (int e = tid; e < npad; e += kThreads) {
      const int slot = e <= Wp ? e : e <= Wp + H ? (e - Wp + 1) * Wp : (H + 1) * Wp + (e - Wp - H - 1);
      sc[slot] = tinf;
      sc[j.n_pad + slot] = tinf;
    }
    __syncthreads();                            // the class table
    // Tprev: the grid at the start of the step; (M*Tprev)/dt is a constant of the step
    float *const g0 = j.grid + (size_t)b * N;
    for (int i = tid, r = r_first, c = c_first; i < N; i += kThreads) {
      const float *t = tab + (int)j.cls[i] * kRow;
      const float tp = g0[i];
      sc[i + r + Wp + 1] = tp;
      c0g[i] = t[14] != 0.0f ? tinf : (t[13] * tp) / dtf;
      c += dc; r += dr;
      if (c >= W) { c -= W; ++r; }
    }
    __syncthreads();

    int it = 0, converged = 0;
    while (it < limit) {
      const float *cur = sc + (it & 1) * j.n_pad;
      float *nxt = sc + ((it + 1) & 1) * j.n_pad;
      float dmax = 0.0f;
      for (int i0 = tid, r = r_first, c = c_first; i0 < N; i0 += kBatch * kThreads) {
        int p[kBatch], cl[kBatch];
        float T[kBatch], tl[kBatch], tr[kBatch], ta[kBatch], tb[kBatch], c0[kBatch], qv[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {      // the loads of the batch (a CV beyond the grid reads CV i0 again)
          const int i = i0 + u * kThreads;
          const bool ok = i < N;
          const int ic = ok ? i : i0;
          p[u] = ok ? i + r + Wp + 1 : -1;
          const int pc = ok ? p[u] : p[0];
          cl[u] = j.cls[ic];
          T[u] = cur[pc];
          // shift_tensor_left -> T[i][j+1] ("left"), shift_tensor_right -> T[i][j-1] ("right"); above / below are
          // T[i-1][j] / T[i+1][j]
          tl[u] = cur[pc + 1]; tr[u] = cur[pc - 1]; ta[u] = cur[pc - Wp]; tb[u] = cur[pc + Wp];
          c0[u] = c0g[ic];
          qv[u] = TAP ? j.q[(size_t)b * N + ic] : 0.0f;
          c += dc; r += dr;
          if (c >= W) { c -= W; ++r; }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const float4 *t = tab4 + cl[u] * (kRow / 4);
          const float4 r0 = t[0], r1 = t[1], r2 = t[2], r3 = t[3];
          float n1 = r0.x * tl[u];              // nt1 = vz*(((k1u*TL + k3u*TR) + Tinf*hL) + Tinf*hR)
          n1 = n1 + r0.y * tr[u];
          n1 = n1 + r1.z;
          n1 = n1 + r1.w;
          n1 = r1.y * n1;
          float n2 = r0.z * tb[u];              // nt2 = uz*(((k2v*Tbelow + k4v*Tabove) + Tinf*hB) + Tinf*hT)
          n2 = n2 + r0.w * ta[u];
          n2 = n2 + r2.x;
          n2 = n2 + r2.y;
          n2 = r1.x * n2;
          float num = n1 + n2;                  // ((nt1 + nt2) + (M*Tprev)/dt) + q
          num = num + c0[u];
          num = num + (TAP ? (r3.z != 0.0f ? 0.0f : qv[u]) : r3.x);
          const double rden = __hiloint2double(__float_as_int(r2.w), __float_as_int(r2.z));
          const float tn = (float)((double)num * rden);
          if (p[u] >= 0) {
            nxt[p[u]] = tn;
            dmax = fmaxf(dmax, fabsf(tn - T[u]));
          }
        }
      }
      const float wm = (float)wave_max((double)dmax);
      if (lane == 0) red[it & 1][wave] = wm;
      __syncthreads();                          // the new grid (global, through the CU's L1) and every wavefront's max|dT|
      float m = red[it & 1][0];
#pragma unroll
      for (int v = 1; v < kNW; ++v) m = fmaxf(m, red[it & 1][v]);
      ++it;
      if (m <= thr) { converged = 1; break; }
    }

    // hand-over to k_post: the grid, zone sums and whole-grid sum in float64 (in k_sweep_jacobi's order: its thread t
    // adds CVs t, t + sum_threads, ..., a wavefront its 64 threads, thread 0 the wavefronts), iterations | converged << 16
    const float *fin = sc + (it & 1) * j.n_pad;
    for (int i = tid, r = r_first, c = c_first; i < N; i += kThreads) {
      g0[i] = fin[i + r + Wp + 1];
      c += dc; r += dr;
      if (c >= W) { c -= W; ++r; }
    }
    const int st = j.sum_threads;
    if (tid < st) {
      double s = 0.0;
      for (int i = tid; i < N; i += st) s += (double)fin[i + i / W + Wp + 1];
      s = wave_sum(s);
      if (lane == 0) gred[wave] = s;
    }
    for (int z = wave; z < a.Z; z += kNW) {     // a zone per wavefront, its cells in a fixed order
      double zs = 0.0;
      for (int e = a.zone_off[z] + lane; e < a.zone_off[z + 1]; e += 64) {
        const int i = a.zone_cells_l[e];
        zs += (double)fin[i + i / W + Wp + 1];
      }
      zs = wave_sum(zs);
      if (lane == 0) a.zsum[(size_t)b * a.Z + z] = zs;
    }
    if (tid == 0) next = (int)gridDim.x + atomicAdd(a.next_b, 1);
    __syncthreads();                            // gred, next; every read of this building's scratch and class table is done
    if (tid == 0) {
      double total = gred[0];
      for (int v = 1; v < st / 64; ++v) total += gred[v];
      a.gsum[b] = total;
      a.nsw[b] = it | (converged << 16);
    }
    b = next;                                   // (next, gred and red are rewritten only after further barriers)
  }
}

} // namespace

bool sweep_jacobi_g_supported(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= kMaxN; }
int sweep_jacobi_g_max_cvs() { return kMaxN; }
int sweep_jacobi_g_threads() { return kThreads; }
size_t sweep_jacobi_g_lds_bytes() {
  return sizeof(float4) * (kMaxCls * kRow / 4) + (size_t)kNW * (2 * sizeof(float) + sizeof(double)) + sizeof(int);
}
size_t sweep_jacobi_g_scratch_floats(int H, int W) { return wg_floats(sweep_jacobi_slots(H, W), H * W); }

int sweep_jacobi_g_blocks_per_cu() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)k_sweep_jacobi_g<false>, kThreads, 0) != hipSuccess) return 0;
  return n;
}

int launch_sweep_jacobi_g(const Dev &d, const JacArgs &j, int workgroups, hipStream_t stream) {
  const int wgs = std::max(1, std::min(workgroups, j.nb));
  if (j.q) hipLaunchKernelGGL(k_sweep_jacobi_g<true>, dim3(wgs), dim3(kThreads), 0, stream, d, j);
  else hipLaunchKernelGGL(k_sweep_jacobi_g<false>, dim3(wgs), dim3(kThreads), 0, stream, d, j);
  return (int)hipGetLastError();
}

} // namespace sb
