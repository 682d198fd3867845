// step_reg.hip -- the sweep kernel whose temperature grid lives in registers.
//
// Layout.  The floor plan is trimmed to the bounding box of its non-exterior cells (the
// exterior-space ring is the constant T_ambient and is handled analytically).  Row R of the
// trimmed grid belongs to one lane; the lane keeps the row in NR registers ("slots"), column
// c in slot (c + l) mod NR where l is the lane's index inside its wavefront.  At sweep step d
// every lane works on slot d mod NR -- the SAME register index in all lanes -- which for lane l
// is column d - l: the anti-diagonal wavefront that reproduces the reference's row-major
// in-place Gauss-Seidel order (simulator.py:302-314).  Neighbours:
//     L = slot d-1 of the lane (updated one step ago)      R = slot d+1 (old)
//     U = slot d-1 of lane l-1 (DPP wave_shr:1, new)        D = slot d+1 of lane l+1 (DPP wave_shl:1, old)
// so the sweep touches no memory for the grid at all.  The sweep is fully unrolled (slot
// indices and lane masks are compile-time constants); per step it reads four coefficients
// (two ds_read2_b64), A = ap*Tprev + g (computed once per step into LDS) and runs 4 DPP
// moves + 4 fp64 FMAs in the association order of step_lds.hip (bit-identical iterates).
//
// Two modes (template parameter P).  Mode 1: one wavefront per building, at most 64 rows.
// Mode 2: two wavefronts per building, at most 128 rows: wave 0 owns the upper rows (in its
// TOP lanes, so that its seam row is lane 63), wave 1 the lower rows (seam row = lane 0).
// The two seam rows are exchanged through LDS once per 8-step chunk; wave 0 counts its
// finished chunks in LDS and wave 1 starts chunk i only once wave 0 has finished chunk
// i + lag (sb_create: seam_lag), which orders every cross-wave read-after-write (wave 0's new
// seam row) and write-after-read (wave 1's old seam row) -- a workgroup barrier per chunk
// costs ~600 cycles on gfx950, a satisfied flag check nothing.  The DPP `old` operand carries
// the seam value into the edge lane.
//
// Plans with one or two rows beyond a wavefront's 64 (tail rows), and the schedule that overlaps
// consecutive sweeps, are k_sweep_roll's (step_roll.hip).
//
// HBM state of a building: [NR][RS] float64, slot-major (one coalesced 8*RS-byte row per
// register), pad cells 0.
#include "step_reg_cfg.h"
#include "sweep_common.h"

namespace sb {
namespace {

using namespace sweep;
using namespace reg; // kPair, lds_slots, waves_per_simd, table_stride, kSeamPad

#ifndef SB_LOOK
#define SB_LOOK 2
#endif
constexpr int kLook = SB_LOOK; // steps between the LDS reads of a step and its arithmetic

struct Co { double bU, bD, bL, bR, A, smU, smD; };
struct Pipe {
  Co co[kLook + 1];
  unsigned long long cw[3]; // class bytes of three consecutive chunks
};

// LDS reads of step PD (issued kLook steps early): coefficients by class, A, seam value.
template <int NR, int P, int PD, int NAR>
__device__ __forceinline__ void prefetch(Pipe &p, const double *tab, const double *Arow,
                                         const double (&Areg)[NAR], const double *seam_in,
                                         const double *seam_in2) {
  const unsigned long long cw = p.cw[(PD / 8) % 3];
  constexpr int kTS = table_stride(NR, P);
  const int c8 = (int)((cw >> (8 * (PD % 8))) & 0xffull) * (kTS / 32); // the class's byte offset into a table column
  const double *bt = (const double *)((const char *)tab + c8);
  Co &o = p.co[PD % (kLook + 1)];
  o.bU = bt[0]; o.bD = bt[kTS]; o.bL = bt[2 * kTS]; o.bR = bt[3 * kTS];
  constexpr int NL = lds_slots(NR, P);
  if constexpr ((PD % NR) < NL) o.A = Arow[PD % NR];
  else o.A = Areg[(PD % NR) - NL];
  if (P == kPair) { // two reads of the same value: each DPP consumes its `old` register
    o.smU = seam_in[PD];
    o.smD = seam_in2[PD];
  }
}

// One Gauss-Seidel update of every lane's current cell.  lp = lane's row index inside its
// wavefront (0x80000000 for lanes without a row): the lane holds a real column at step D
// iff 0 <= D - lp < NR.
template <int NR, int P, int D>
__device__ __forceinline__ void update(double (&e)[NR], const Co &o, int lp, unsigned long long rowmask,
                                       double &dmax) {
  constexpr int r = D % NR, rm = (D + NR - 1) % NR, rp = (D + 1) % NR;
  const double U = wave_shift1<0x138, P == kPair>(e[rm], o.smU);
  const double Dn = wave_shift1<0x130, P == kPair>(e[rp], o.smD);
  double t = fma(o.bD, Dn, o.A);
  t = fma(o.bR, e[rp], t);
  t = fma(o.bL, e[rm], t);
  const double nv = fma(o.bU, U, t);
  constexpr bool need_hi = D < 63;   // lp <= D can fail
  constexpr bool need_lo = D >= NR;  // lp > D - NR can fail
  bool act;
  if (need_hi && need_lo) act = (unsigned)(D - lp) < (unsigned)NR;
  else if (need_hi) act = (unsigned)lp <= (unsigned)D;
  else if (need_lo) act = lp > D - NR;
  else act = __builtin_amdgcn_inverse_ballot_w64(rowmask);
  const double sel = act ? nv : e[r];
  dmax = fmax(dmax, fabs(sel - e[r]));
  e[r] = sel;
}

struct SweepCtx {
  const double *tab, *Arow, *seam_in, *seam_in2; // seam_in2 == seam_in, but the compiler cannot tell
  double *seam_out;
  const unsigned long long *cmap;
  unsigned long long rowmask;
  int lane, lp, nch, edge_off;
  bool edge;
  // P == 2: wave 0 counts its finished chunks in *prog; wave 1 starts chunk i only when wave
  // 0 has finished chunk i + lag (capped at wave 0's last chunk)
  volatile int *prog;
  int role, lag, nch0, prog_base;
};

template <int NR, int P, int CI, int K, int NAR>
__device__ __forceinline__ void chunk_steps(double (&e)[NR], const double (&Areg)[NAR], Pipe &p,
                                            const SweepCtx &x, double &dmax) {
  if constexpr (K < 8 && 8 * CI + K < NR + 63) {
    constexpr int D = 8 * CI + K;
    prefetch<NR, P, D + kLook>(p, x.tab, x.Arow, Areg, x.seam_in, x.seam_in2);
    update<NR, P, D>(e, p.co[D % (kLook + 1)], x.lp, x.rowmask, dmax);
    __builtin_amdgcn_sched_barrier(0);
    chunk_steps<NR, P, CI, K + 1>(e, Areg, p, x, dmax);
  }
}

template <int NR, int P, int CI, int K>
__device__ __forceinline__ void publish(const double (&e)[NR], double *seam_out) {
  if constexpr (K < 8 && 8 * CI + K < NR + 63) {
    seam_out[8 * CI + K] = e[(8 * CI + K) % NR];
    publish<NR, P, CI, K + 1>(e, seam_out);
  }
}

// Wave 1 waits until wave 0's progress counter reaches `target`.  `seen` caches the last
// value read: wave 0 is usually several chunks ahead, so most chunks need no LDS read at all.
__device__ __forceinline__ void wait_progress(volatile int *prog, int target, int &seen) {
  while (seen < target) {
    asm volatile("" ::: "memory");
    seen = __builtin_amdgcn_readfirstlane(*prog);
    if (seen < target) __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");
}

template <int NR, int P, int CI, int NAR>
__device__ __forceinline__ void chunks(double (&e)[NR], const double (&Areg)[NAR], Pipe &p, const SweepCtx &x,
                                       double &dmax, int &seen) {
  constexpr int kMaxCh = (NR + 63 + 7) / 8;
  if constexpr (CI < kMaxCh) {
    if (CI < x.nch) { // wave-uniform
      if (P == kPair && x.role == 1) wait_progress(x.prog, x.prog_base + min(CI + x.lag, x.nch0), seen);
      p.cw[(CI + 2) % 3] = x.cmap[opaque(0) + (CI + 2) * 64];
      chunk_steps<NR, P, CI, 0>(e, Areg, p, x, dmax);
      if (P == kPair) {
        // publish the edge row's new values of this chunk (columns 8*CI-edge_off .. +7)
        const int c0 = 8 * CI - x.edge_off;
        if (c0 + 7 >= 0 && c0 < NR) {
          if (x.edge) publish<NR, P, CI, 0>(e, x.seam_out);
        }
      }
      if (P == kPair) {
        // LDS executes a wavefront's instructions in order: whoever sees the counter sees the
        // seam values written before it, and every LDS read this wave issued so far is done
        asm volatile("" ::: "memory");
        if (x.role == 0 && x.lane == 0) *x.prog = x.prog_base + CI + 1;
        asm volatile("" ::: "memory");
      }
      chunks<NR, P, CI + 1>(e, Areg, p, x, dmax, seen);
    }
  }
}

template <int NR, int P, int NAR>
__device__ __forceinline__ double sweep_reg(double (&e)[NR], const double (&Areg)[NAR], const SweepCtx &xin) {
  double dmax = 0.0;
  int seen = 0;
  // the per-step lane predicates are one v_cmp each; hoisted out of the sweep loop they would
  // be ~150 SGPR pairs spilled to VGPR lanes (2 v_readlane + wait states per step)
  SweepCtx x = xin;
  asm volatile("" : "+v"(x.lp));
  if (P == kPair && x.role == 1) wait_progress(x.prog, x.prog_base + min(x.lag, x.nch0), seen);
  Pipe p;
  p.cw[0] = x.cmap[opaque(0)];
  p.cw[1] = x.cmap[opaque(0) + 64];
  p.cw[2] = 0;
  prefetch<NR, P, 0>(p, x.tab, x.Arow, Areg, x.seam_in, x.seam_in2);
  prefetch<NR, P, 1>(p, x.tab, x.Arow, Areg, x.seam_in, x.seam_in2);
  __builtin_amdgcn_sched_barrier(0);
  chunks<NR, P, 0>(e, Areg, p, x, dmax, seen);
  return dmax;
}

extern __shared__ __attribute__((aligned(16))) double lds[];

template <int NR, int P>
__global__ void __launch_bounds__(P == kPair ? 128 : 64)
    __attribute__((amdgpu_waves_per_eu(waves_per_simd(NR, P), waves_per_simd(NR, P)))) k_sweep_reg(Dev a) {
  const int lane = threadIdx.x & 63;
  const int w = P == kPair ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  constexpr int kASlots = (NR + 7) / 8, kZSlots = (NR + 3) / 4, kMaxCh = (NR + 63 + 7) / 8;
  constexpr int kTS = table_stride(NR, P);

  double *tab = lds;                       // [5][kTS]: bU bD bL bR ap
  double *gtab = lds + 5 * kTS;            // [kTS]
  double *seamD = lds + a.r_seam;          // [pad | NR | pad] old values of wave 1's first row
  double *seamU = seamD + NR + 2 * kSeamPad; // new values of wave 0's last row
  double *A = lds + a.r_A;                 // [RS][AS >= NR]; after the sweeps: zone sums [Z+1][RS]
  double *xchg = lds + a.r_xchg;           // [0..3] max delta (2 sweeps x 2 waves), [4..5] grid sums, [6] progress counter
  // every byte of LDS starts finite: seam / A reads next to the arrays' ends are multiplied by 0
  for (int i = threadIdx.x; i < a.lds_reg_bytes / 8; i += blockDim.x) lds[i] = 0.0;
  __syncthreads();
  for (int i = threadIdx.x; i < 5 * kTS; i += blockDim.x) {
    const int j = i / kTS, c = i - j * kTS;
    tab[i] = c <= a.ncls ? a.ctab[c * 8 + j] : 0.0; // row `ncls` is the pad class: T' = Tprev (ap = 1)
  }
  __syncthreads();

  const sb_params &p = a.p;
  const int lw = a.lw[w], l0 = a.l0[w], rowbase = a.rowbase[w];
  const int lp = lane - l0;
  const bool rowvalid = lp >= 0 && lp < lw;
  const int R = rowbase + (rowvalid ? lp : 0);
  const int RS = a.RS;
  SweepCtx x;
  x.tab = tab;
  x.Arow = A + (size_t)R * a.AS; // odd row stride: the 64 lanes of a ds_read_b64 cover all 32 banks
  constexpr int kNL = lds_slots(NR, P), kNAR = NR - kNL > 0 ? NR - kNL : 1;
  x.cmap = a.cmapS + (size_t)w * (kMaxCh + 3) * 64 + lane;
  x.rowmask = __builtin_amdgcn_ballot_w64(rowvalid);
  x.lane = lane; x.lp = rowvalid ? lp : (int)0x80000000; x.nch = a.nch[w];
  x.edge_off = (P == kPair && w == 0) ? lw - 1 : 0;
  x.edge = P == kPair && lane == (w == 0 ? 63 : 0);
  x.seam_in = (w == 0 ? seamD : seamU) + kSeamPad - x.edge_off;
  x.seam_in2 = x.seam_in + opaque(0);
  x.seam_out = (w == 0 ? seamU : seamD) + kSeamPad - x.edge_off;
  x.prog = (volatile int *)(xchg + 6);
  x.role = w; x.lag = a.lag; x.nch0 = a.nch[0]; x.prog_base = 0;
  const unsigned long long *amap = a.amapS + (size_t)w * kASlots * 64 + lane;
  const unsigned long long *zmap = a.zmapS + (size_t)w * kZSlots * 64 + lane;

// developer aid: cycle stamps of workgroup 0's 11th building (steady state, not the cold start)
#define SB_STAMP(i) do { if (a.dbg && blockIdx.x == 0 && iter == 10 && w == 0 && lane == 0) a.dbg[i] = (long long)__builtin_readcyclecounter(); } while (0)
  // The lane's class bytes by slot (A pass) do not depend on the building: loaded once, they
  // live in AGPRs between their uses (the allocator spills what the sweep does not touch)
  // instead of costing a global round trip per building.  (The two-wavefront mode has no
  // registers to spare and reloads them.)
  constexpr bool kReloadAmap = P == kPair; // no registers to spare
  unsigned long long amapw[kASlots];
  if (!kReloadAmap) {
#pragma unroll
    for (int g = 0; g < kASlots; ++g) amapw[g] = amap[g * 64];
  }

  // The lane's row of the NEXT building is loaded while this building's zone sums are reduced
  // (its registers are free once the row is stored), so the loop never waits on HBM latency.
  double e[NR];
#define SB_LOAD_ROW(bb)                                                                         \
  do {                                                                                          \
    const double *tp_ = a.temp + (size_t)(bb) * a.state_doubles; /* wave-uniform: SGPR base + lane offset */ \
    _Pragma("unroll") for (int j = 0; j < NR; ++j) { /* pad lanes mirror a real row: never updated, never stored */ \
      e[j] = tp_[R];                                                                            \
      tp_ += opaque_s(RS);                                                                      \
    }                                                                                           \
  } while (0)
  // ... and so are the building's small inputs: its g table entry, ambient temperature and
  // the extremes of its exterior ring.
  double nx_g = 0.0, nx_tnow = 0.0, nx_lo = 0.0, nx_hi = 0.0;
#define SB_LOAD_AUX(bb)                                                                         \
  do {                                                                                          \
    nx_tnow = a.bld[(bb)].t_now;                                                                \
    nx_lo = a.scal[(size_t)(bb) * kNScal + 16];                                                 \
    nx_hi = a.scal[(size_t)(bb) * kNScal + 17];                                                 \
    if (w == 0) nx_g = a.gtabg[(size_t)(bb) * kTS + (lane & (kTS - 1))];                        \
  } while (0)
  if ((int)blockIdx.x < a.B) {
    SB_LOAD_ROW(blockIdx.x);
    SB_LOAD_AUX(blockIdx.x);
  }
  // Buildings need different numbers of sweeps, so a static split would leave the last
  // workgroups running alone: after its first building a workgroup draws the next one from a
  // device counter (zeroed before every launch).  In the two-wavefront mode wave 0 draws
  // and hands the index to wave 1 through LDS at the building's first barrier.
  int *draw_slot = (int *)(xchg + 7);
  int iter = 0;
  for (int b = blockIdx.x, bn = 0; b < a.B; b = bn, ++iter) {
    if (w == 0) { // early: the epilogue prefetches building bn
      int nb = 0;
      if (lane == 0) nb = a.sweep_wgs + atomicAdd(a.next_b, 1);
      bn = __builtin_amdgcn_readfirstlane(nb);
      if (P == kPair && lane == 0) *draw_slot = bn;
    }
    SB_STAMP(0);
    double *T = a.temp + (size_t)b * a.state_doubles + R;
    __builtin_amdgcn_sched_barrier(0);
    const double t_now = nx_tnow;
    // exterior-space cells outside the trim box all become t_now in the first sweep
    // (simulator.py:256-258); their largest |delta| follows from their extreme values
    const double ring_d = a.n_ring > 0 ? fmax(fabs(t_now - nx_lo), fabs(t_now - nx_hi)) : 0.0;
    if (w == 0) {
      if (P == kPair && lane == 0) *x.prog = 0;
      if (lane < kTS) gtab[lane] = nx_g;
      if (P == kPair) // old values of wave 1's first row (its lane 0: column c sits in slot c)
        for (int c = lane; c < NR; c += 64)
          seamD[kSeamPad + c] = a.temp[(size_t)b * a.state_doubles + (size_t)c * RS + a.rowbase[1]];
    }
    if (P == kPair) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    if (P == kPair && w == 1) bn = __builtin_amdgcn_readfirstlane(*draw_slot);
    __builtin_amdgcn_sched_barrier(0);
    SB_STAMP(1);
    // A = ap*Tprev + g for every cell of the lane's row (E = Tprev before the first sweep)
    double Areg[kNAR]; // lanes without a row keep finite values (0 * NaN would reach a real row)
#pragma unroll
    for (int k = 0; k < kNAR; ++k) Areg[k] = 0.0;
    if (rowvalid) {
      if (kReloadAmap) {
        const int o = opaque(0);
#pragma unroll
        for (int g = 0; g < kASlots; ++g) amapw[g] = amap[o + g * 64];
      }
      const unsigned long long(&cw)[kASlots] = amapw;
      double *Aw = A + (size_t)R * a.AS;
      // groups of 8, software-pipelined: the table reads of group g+1 are issued before the
      // A values of group g are written (the compiler cannot prove that A and the tables do
      // not alias and would serialise every read behind the previous write)
      constexpr int kGroups = (NR + 7) / 8;
      double ap[2][8], gg[2][8];
      auto fetch = [&](int g, double (&pa)[8], double (&pg)[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int j = min(8 * g + k, NR - 1);
          const int c8 = (int)((cw[j >> 3] >> (8 * (j & 7))) & 0xffull) * (kTS / 32);
          pa[k] = *(const double *)((const char *)(tab + 4 * kTS) + c8);
          pg[k] = *(const double *)((const char *)gtab + c8);
        }
      };
      fetch(0, ap[0], gg[0]);
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        if (g + 1 < kGroups) fetch(g + 1, ap[(g + 1) & 1], gg[(g + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (8 * g + k < NR) {
            const double av = fma(ap[g & 1][k], e[8 * g + k], gg[g & 1][k]);
            if (8 * g + k < kNL) Aw[8 * g + k] = av;
            else Areg[8 * g + k - kNL] = av;
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);
    SB_STAMP(2);

    int n_sweeps = 0, converged = 0;
#pragma nounroll
    for (int it = 0; it < p.iter_limit; ++it) { // simulator.py:348-368
      x.prog_base = it * 32; // the counter only grows within a building's step
      double md = wave_max(sweep_reg<NR, P>(e, Areg, x));
      if (P == kPair) {
        double *xd = xchg + 2 * (it & 1); // double-buffered: wave 0 may finish its next sweep early
        if (lane == 0) xd[w] = md;
        __syncthreads();
        md = fmax(xd[0], xd[1]);
      }
      if (it == 0) md = fmax(md, ring_d);
      ++n_sweeps;
      if (md <= p.conv_threshold) { converged = 1; break; }
    }
    __builtin_amdgcn_sched_barrier(0);
    SB_STAMP(3);
    SB_STAMP(4);

    // grid back to HBM.  Zone sums (A is dead now): every lane adds its cells into its own
    // column of zs[zone][row]; row Z collects every cell outside a zone, so that the sum of all
    // rows is the grid sum.
    double *zs = A;
    const int ZRS = a.ZRS;
    if (rowvalid) {
      unsigned long long zwv[kZSlots]; // zone-sum offsets: loaded while the row is stored
      {
        const int o = opaque(0);
#pragma unroll
        for (int g = 0; g < kZSlots; ++g) zwv[g] = zmap[o + g * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      // one 8-byte store per register straight from e[]: a wider store would have to be
      // assembled in a temporary that the next store overwrites (measured 6x slower)
      double *tp = a.temp + (size_t)b * a.state_doubles;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        tp[R] = e[j];
        tp += opaque_s(RS);
      }
      for (int z = 0; z <= a.Z; ++z) zs[(size_t)z * ZRS + R] = 0.0;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const unsigned off = (unsigned)((zwv[j >> 2] >> (16 * (j & 3))) & 0xffffull);
        __hip_atomic_fetch_add((double *)((char *)zs + off), e[j], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    SB_STAMP(5);
    if (bn < a.B) {
      SB_LOAD_ROW(bn);
      SB_LOAD_AUX(bn);
    }
    __builtin_amdgcn_sched_barrier(0);
    SB_STAMP(6);
    if (P == kPair) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    SB_STAMP(7);

    if (w == 0) { // hand the zone sums, the grid sum and the sweep count to k_post
      // 16 zones x 4 row groups per pass: lane (zone = lane & 15, group = lane >> 4) adds every
      // fourth row of its zone, two xor-shuffles combine the groups
      double gacc = 0.0;
      for (int zb = 0; zb <= a.Z; zb += 16) {
        const int zz = zb + (lane & 15), g = lane >> 4;
        double v = 0.0;
        if (zz <= a.Z)
          for (int r = g; r < RS; r += 4) v += zs[(size_t)zz * ZRS + r];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16 && zz < a.Z) a.zsum[(size_t)b * a.Z + zz] = v;
        if (lane < 16 && zz <= a.Z) gacc += v;
      }
      const double gsum = wave_sum(gacc);
      if (lane == 0) {
        a.gsum[b] = gsum + (double)a.n_ring * t_now;
        a.nsw[b] = n_sweeps | (converged << 16);
      }
      SB_STAMP(8);
      if (a.dbg && blockIdx.x == 0 && iter == 10 && lane == 0) a.dbg[9] = n_sweeps;
    }
    // no barrier here: wave 1 touches no LDS of the next building before the barrier that
    // follows wave 0's g-table load
  }
#undef SB_STAMP
#undef SB_LOAD_ROW
#undef SB_LOAD_AUX
}

struct Variant {
  int NR, P;
  const void *fn;
  void (*launch)(const Dev &, int, hipStream_t);
};

template <int NR, int P>
void launch_variant(const Dev &d, int workgroups, hipStream_t stream) {
  hipLaunchKernelGGL((k_sweep_reg<NR, P>), dim3(workgroups), dim3(P == kPair ? 128 : 64),
                     (size_t)d.lds_reg_bytes, stream, d);
}

#define SB_VARIANT(NR, P) {NR, P, (const void *)k_sweep_reg<NR, P>, launch_variant<NR, P>},
const Variant kVariants[] = {SB_REG_VARIANTS(SB_VARIANT)}; // (step_reg_cfg.h: the list the planner chooses from)
#undef SB_VARIANT

const Variant *find_variant(int NR, int P) {
  for (const Variant &v : kVariants)
    if (v.NR == NR && v.P == P) return &v;
  return nullptr;
}

} // namespace

int prepare_sweep_reg(const Dev &d) {
  const Variant *v = find_variant(d.NR, d.P);
  if (!v) return (int)hipErrorInvalidValue;
  return (int)hipFuncSetAttribute(v->fn, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_reg_bytes);
}

int launch_sweep_reg(const Dev &d, int cus, hipStream_t stream) {
  const Variant *v = find_variant(d.NR, d.P);
  if (!v) return (int)hipErrorInvalidValue;
  (void)cus;
  v->launch(d, d.sweep_wgs, stream); // == min(B, CUs * wg_per_cu)
  return (int)hipGetLastError();
}

} // namespace sb
