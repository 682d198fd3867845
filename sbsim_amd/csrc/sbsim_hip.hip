// sbsim_hip.hip -- the planner and handle creation of the C ABI (include/sbsim_amd.h): which sweep kernel owns a floor
// plan and that kernel's tables (sb_plan_info), the handle's device buffers (sb_create).  The sweep kernels live in the
// step_*.hip files and share sb_device.h; the state kernels and every other entry point live in runtime.hip, the optional
// input generators (occupancy, convection) in generators.hip; sb_host.h holds what the host files share.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (fma only where written).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sb_host.h"

#ifndef SB_EXPERIMENTAL
namespace sb { // the default build's answers for step_stream_ms.hip (sb_host.h, kExperimental)
int launch_sweep_stream_ms(const Dev &, double *, double *, int, hipStream_t) { return (int)hipErrorNotSupported; }
int prepare_sweep_stream_ms(const Dev &, int) { return (int)hipErrorNotSupported; }
int sweep_stream_ms_sweeps() { return 1; }
int sweep_stream_ms_seam_doubles(int, int) { return 0; }
int sweep_stream_ms_xchg_doubles(int) { return 0; }
} // namespace sb
#endif

using namespace sb;

namespace {

bool env_flag(const char *name) {
  const char *e = getenv(name);
  return e && e[0] == '1';
}
int env_int(const char *name, int unset) {
  const char *e = getenv(name);
  return e ? atoi(e) : unset;
}
double env_double(const char *name, double unset) {
  const char *e = getenv(name);
  return e ? atof(e) : unset;
}

// The developer switches, read at the start of every sb_plan_info / sb_create call: the tests
// change them between calls.
struct Knobs {
  bool force_stream = env_flag("SBSIM_FORCE_STREAM_PATH");  // every plan on k_sweep_stream
  bool force_jacobi_global = env_flag("SBSIM_FORCE_JACOBI_GLOBAL"); // sb_create_jacobi: every plan on k_sweep_jacobi_g
  int jacobi_global_wgs = std::max(0, env_int("SBSIM_DEBUG_JACOBI_GLOBAL_WGS", 0)); // k_sweep_jacobi_g: at most this many workgroups (0: what is resident)
  int debug_cus = std::max(0, env_int("SBSIM_DEBUG_CUS", 0)); // launch geometry as on a device of at most this many CUs (0: the device's own; speed only)
  bool force_lds = env_flag("SBSIM_FORCE_LDS_PATH");        // no register kernel: the LDS-grid kernel (else streaming)
  bool band_path = env_flag("SBSIM_BAND_PATH");             // 67..130 rows: k_sweep_band before k_sweep_two
  bool no_two_row = env_flag("SBSIM_NO_TWO_ROW_PATH");      // no k_sweep_two
  bool no_band = env_flag("SBSIM_NO_BAND_PATH");            // no k_sweep_band (unless band_path)
  bool no_two_64 = env_flag("SBSIM_NO_TWO_64");             // k_sweep_two on 76 / 80 slots alone
  bool no_roll_64 = env_flag("SBSIM_NO_ROLL_64");           // k_sweep_roll on 96 slots alone
  bool no_roll_small = env_flag("SBSIM_NO_ROLL_SMALL");     // <= 64 rows stay on k_sweep_reg<NR,1>
  bool two_general = env_flag("SBSIM_TWO_GENERAL");         // k_sweep_two's four-coefficient instantiation
  int two_max_level = std::max(0, env_int("SBSIM_TWO_MAX_LEVEL", 1 << 30)); // k_sweep_two's highest LDS level
  bool two_no_skip = env_flag("SBSIM_TWO_NO_SKIP");         // k_sweep_two measures max|delta| every period
  int lds_pad = env_int("SBSIM_DEBUG_LDS_PAD", 0);          // bytes added to a workgroup's LDS request
  float pred_haste = (float)env_double("SBSIM_DEBUG_PRED_HASTE", 1.0); // k_sweep_two / k_sweep_band's block prediction
  float pred_slack = (float)env_double("SBSIM_DEBUG_PRED_SLACK", 1.0); // (speed only, never the result)
  int pred_first = getenv("SBSIM_DEBUG_PRED_FIRST") ? std::max(1, env_int("SBSIM_DEBUG_PRED_FIRST", 1)) : 0; // 0: unset
  // k_sweep_two: how far ahead the next measurement is placed (speed only; clamped: (int)(skip_kappa * togo) must not overflow)
  float skip_kappa = (float)std::min(100.0, std::max(0.0, env_double("SBSIM_DEBUG_SKIP_KAPPA", 0.9)));
  bool roll_exact = env_int("SBSIM_ROLL_EXACT", 0) != 0;    // k_sweep_roll's float64 instantiation alone
  int force_redo = std::max(0, env_int("SBSIM_DEBUG_FORCE_REDO", 0)); // every m-th building through the redo list
  bool roll_free = env_int("SBSIM_ROLL_FREE", 1) != 0;      // k_sweep_roll: copy-free, measure-free periods where a sweep is proven unfinished
  bool force_generic = env_flag("SBSIM_FORCE_GENERIC_SWEEP"); // the LDS-grid kernel's generic sweep
  bool phase_timing = getenv("SBSIM_PHASE_TIMING") != nullptr;     // cycle stamps (sb_debug_phase_cycles)
  bool debug_timeline = getenv("SBSIM_DEBUG_TIMELINE") != nullptr; // ... plus step_band.hip's time line
  bool stream_ms = kExperimental && env_flag("SBSIM_STREAM_MS");     // streaming plans on k_sweep_stream_ms
  bool stream_roll = kExperimental && env_flag("SBSIM_STREAM_ROLL"); // ... on k_sweep_stream_roll
};

// SBSIM_DEBUG_CUS=n: every per-workgroup buffer and every grid of a handle is sized from sb_handle::cus or from
// sb_launch_info::workgroups, so a smaller count makes the persistent kernels' workgroups draw more buildings each.
int capped_cus(int cus, const Knobs &k) { return k.debug_cus > 0 ? std::min(cus, k.debug_cus) : cus; }

constexpr int kGuardHost = 16; // must match kGuard in step_lds.hip

// ---------------------------------------------------------------- register-path planning
// Host-only: decides whether k_step_reg can own this floor plan and builds its tables.
struct RegPlan {
  bool ok = false;
  std::string why;
  sb_sweep_kernel kernel = SB_KERNEL_LDS; // when ok: the register or streaming kernel this plan is for
  int NR = 0, RS = 0, Ws = 0, r0 = 0, c0 = 0, n_ring = 0, T = 0, state_doubles = 0, ts = 32;
  std::vector<uint8_t> tcls, tcset;
  std::vector<double> csetab; // k_sweep_roll: distinct (bU, bD, bL, bR), the pad set (all zero) last
  std::vector<double> tmul;   // k_sweep_roll: the tail scan's static multipliers (sweep_common.h, tail_pass_static)
  int lw[4] = {0, 0, 0, 0}, l0[2] = {0, 0}, rowbase[2] = {0, 0}, nch[2] = {0, 0};
  int lag = 0, nslots = 0, steps = 0;
  int r_seam = 0, r_A = 0, r_xchg = 0, lds_bytes = 0, wg_per_cu = 0, AS = 0;
  int r_cmap = 0, wave_doubles = 0, waves_per_wg = 1; // k_sweep_roll: four buildings per workgroup share the class words
  int ZRS = 0; // k_sweep_reg, k_sweep_roll: row stride of the zone-sum scratch
  int stream_variant = kStreamPlain; // SB_KERNEL_STREAM: kStreamMs / kStreamRoll (experimental)
  std::vector<unsigned long long> cmapS, amapS, zmapS;
  std::vector<int> cell_state;
  // k_sweep_two (plan_two)
  int two_sym = 0, two_level = 0, tail_set_base = 0, tail_pad_set = 0;
  std::vector<int> zs_off; // [Z + 2] the compact zone-sum scratch: slots of zone z are zs_off[z] .. zs_off[z + 1] - 1
};

constexpr int kRegSeamPad = 8, kLdsCap = 160 * 1024;
constexpr int kLdsGranule = 1280; // LDS is allocated to workgroups in blocks of this many bytes (gfx950)
constexpr int kRegSlots[] = {32, 66, 96};

// wave 1 runs this many 8-step chunks behind wave 0: every seam value crosses at least one
// workgroup barrier between its write and its (2-steps-early) read, in both directions
int seam_lag(int lw0) { return (lw0 + 8) / 8 + 1; }

// The trim box: every cell that is not ambient (T' = T_ambient whatever the neighbours are, simulator.py:256-258), and
// every cell's zone (-1: none).  why: not empty when the register and streaming kernels cannot work inside the box.
struct Trim {
  int x0, x1, y0, y1, Hs, Ws;
  std::vector<int> zone_of;
  std::string why;
};

Trim trim_box(const sb_plan_desc *plan) {
  const int H = plan->H, W = plan->W, ncls = plan->n_classes;
  auto coef = [&](int c, int j) { return plan->class_coef[c * 8 + j]; };
  auto cls_at = [&](int x, int y) { return (int)plan->cell_class[x * W + y]; };
  Trim t{H, -1, W, -1, 0, 0, std::vector<int>((size_t)H * W, -1), ""};
  for (int z = 0; z < plan->Z; ++z)
    for (int i = plan->zone_off[z]; i < plan->zone_off[z + 1]; ++i) t.zone_of[plan->zone_cells[i]] = z;
  std::vector<char> ambient(ncls, 0);
  for (int c = 0; c < ncls; ++c)
    ambient[c] = coef(c, 0) == 0 && coef(c, 1) == 0 && coef(c, 2) == 0 && coef(c, 3) == 0 &&
                 coef(c, 4) == 0 && coef(c, 5) == 1.0 && coef(c, 6) == 0;
  for (int x = 0; x < H; ++x)
    for (int y = 0; y < W; ++y)
      if (!ambient[cls_at(x, y)]) {
        t.x0 = std::min(t.x0, x); t.x1 = std::max(t.x1, x);
        t.y0 = std::min(t.y0, y); t.y1 = std::max(t.y1, y);
      }
  if (t.x1 < 0) { t.why = "no cell inside the building"; return t; }
  t.Hs = t.x1 - t.x0 + 1; t.Ws = t.y1 - t.y0 + 1;
  // nothing may couple to a cell outside the trim box
  for (int y = t.y0; y <= t.y1; ++y)
    if (coef(cls_at(t.x0, y), 0) != 0 || coef(cls_at(t.x1, y), 1) != 0) t.why = "coupling across the trim box";
  for (int x = t.x0; x <= t.x1; ++x)
    if (coef(cls_at(x, t.y0), 2) != 0 || coef(cls_at(x, t.y1), 3) != 0) t.why = "coupling across the trim box";
  return t;
}

// The index of the set v[0 .. width) in `tab` (sets of `width` doubles), appended when it is new.
int intern(std::vector<double> &tab, int width, const double *v) {
  size_t s = 0;
  while (s < tab.size() / width && !std::equal(v, v + width, tab.begin() + width * s)) ++s;
  if (s == tab.size() / width) tab.insert(tab.end(), v, v + width);
  return (int)s;
}

// Appends the classes' distinct neighbour coefficients (bU, bD, bL, bR) to `tab`, then the pad set (all zero: no
// neighbour counts); returns every class's set, the pad class (n_classes) last.
std::vector<int> coefficient_sets(const sb_plan_desc *plan, std::vector<double> &tab) {
  std::vector<int> set_of(plan->n_classes + 1, 0);
  for (int c = 0; c < plan->n_classes; ++c) set_of[c] = intern(tab, 4, plan->class_coef + c * 8);
  set_of[plan->n_classes] = (int)tab.size() / 4;
  tab.insert(tab.end(), 4, 0.0);
  return set_of;
}

// k_sweep_two (step_two.hip): one wavefront, two rows per lane, up to 128 + 2 rows and 80 columns
// inside the exterior ring.  (x0, y0): the trim box's corner; zone_of: zone of every cell or -1.
// Three variants (the kernel's template parameters SYM, DENSE):
//   * general: four coefficients per cell, lane l owns rows 2l, 2l + 1, A's slots 72 / 74 in LDS: two
//     buildings per CU;
//   * sym: every cell of the wavefront rows is two coefficients (bV, bH) with T' = A + bV (U + D) + bH (L + R)
//     -- true of interior control volumes (simulator.py:225-237) and of a rectangular building's edge / corner
//     volumes (:130-142, :176-195) once a missing neighbour reads as zero: a pad column follows the last
//     column in the circular slot order (NR > width), the rows are shifted by one so that lane 0's upper
//     cell is a pad row above row 0 (lane l owns rows 2l - 1, 2l), pad rows follow the last row;
//   * dense = sym with only 46 / 56 of A's slots in LDS (the rest in registers): three buildings per CU.
// The zone-sum scratch that aliases A is compact: one slot per (zone, lane) pair that owns a cell of the
// zone (SB1-synth: 1.1 K slots instead of 127 x 65).
bool plan_two(const sb_plan_desc *plan, int Hs, int Ws, int x0, int y0, const std::vector<int> &zone_of, const Knobs &k, RegPlan &r) {
  const int W = plan->W, Z = plan->Z, ncls = plan->n_classes, N = plan->H * plan->W;
  auto coef = [&](int c, int j) { return plan->class_coef[c * 8 + j]; };
  int NR = 0;
  for (int s : {64, 76, 80}) // the narrowest instantiation that holds the width (SBSIM_NO_TWO_64=1: 76 / 80 alone, the tree before the end of round 4)
    if (!NR && s >= Ws && sweep_two_supported(s) && !(s == 64 && k.no_two_64)) NR = s;
  if (!NR || Hs > 128 + 2) return false;
  int ts = 32;
  while (ts < ncls + 1) ts *= 2;
  if (ts > 256) return false;
  const int pad = ncls;
  auto cell_class = [&](int R, int col) { // trimmed coordinates
    return (R >= 0 && R < Hs && col >= 0 && col < Ws) ? (int)plan->cell_class[(x0 + R) * W + (y0 + col)] : pad;
  };
  // ---- can every wavefront cell do with two coefficients?  (rows shifted by one: 127 wavefront rows)
  bool sym = NR > Ws && Hs <= 127 + 2 && !k.two_general;
  const int Hw_sym = std::min(Hs, 127);
  for (int R = 0; sym && R < Hw_sym; ++R)
    for (int col = 0; sym && col < Ws; ++col) {
      const int c = cell_class(R, col);
      const double bU = coef(c, 0), bD = coef(c, 1), bL = coef(c, 2), bR = coef(c, 3);
      // a missing neighbour reads as zero only outside the grid (pad row / pad column); below the last
      // wavefront row only when no tail row follows
      const bool v_ok = bU == bD || (bU == 0.0 && R == 0) || (bD == 0.0 && R == Hs - 1);
      const bool h_ok = bL == bR || (bL == 0.0 && col == 0) || (bR == 0.0 && col == Ws - 1);
      sym = v_ok && h_ok;
    }
  const int rowoff = sym ? 1 : 0;
  const int Hw = std::min(Hs, 128 - rowoff), T = Hs - Hw, nl = (Hw + rowoff + 1) / 2; // wavefront rows, tail rows, lanes that own rows
  for (int x = x0 + Hw; x < x0 + Hs; ++x)
    for (int y = y0; y < y0 + Ws; ++y)
      if (zone_of[x * W + y] >= 0) return false; // the tail scan adds no zone sums
  // ---- coefficient sets.  general: (bU, bD, bL, bR) for every cell.  sym: (bV, bH) for the wavefront's
  // cells [kSets][2], then (bU, bD, bL, bR) for the tail cells [kSets / 2][4]; the pad sets last.
  const int kSets = sweep_two_set_table();
  std::vector<int> set_of(ncls + 1, 0), tset_of(ncls + 1, 0);
  std::vector<double> wtab, ttab; // the wavefront's table, the tail cells' table
  std::vector<char> in_wave(ncls + 1, 0), in_tail(ncls + 1, 0);
  for (int R = 0; R < Hs; ++R)
    for (int col = 0; col < Ws; ++col) (R < Hw ? in_wave : in_tail)[cell_class(R, col)] = 1;
  for (int c = 0; c < ncls; ++c) {
    const double four[4] = {coef(c, 0), coef(c, 1), coef(c, 2), coef(c, 3)};
    if (sym) {
      if (in_wave[c]) {
        const double two[2] = {four[0] != 0.0 ? four[0] : four[1], four[2] != 0.0 ? four[2] : four[3]};
        set_of[c] = intern(wtab, 2, two);
      }
      if (in_tail[c]) tset_of[c] = intern(ttab, 4, four);
    } else {
      set_of[c] = tset_of[c] = intern(wtab, 4, four);
    }
  }
  const double zeros[4] = {0.0, 0.0, 0.0, 0.0};
  const int wwidth = sym ? 2 : 4;
  wtab.insert(wtab.end(), zeros, zeros + wwidth); // the pad set: no neighbour counts
  set_of[pad] = (int)wtab.size() / wwidth - 1;
  if (sym) {
    ttab.insert(ttab.end(), zeros, zeros + 4);
    tset_of[pad] = (int)ttab.size() / 4 - 1;
    if ((int)wtab.size() / 2 > kSets || (int)ttab.size() / 4 > kSets / 2) return false;
    wtab.resize((size_t)2 * kSets, 0.0);
    r.csetab = wtab;
    r.csetab.insert(r.csetab.end(), ttab.begin(), ttab.end());
  } else {
    tset_of[pad] = set_of[pad];
    if ((int)wtab.size() / 4 > kSets) return false;
    r.csetab = wtab;
  }
  r.two_sym = sym ? 1 : 0;
  r.tail_set_base = sym ? 2 * kSets * 8 : 0;
  r.tail_pad_set = r.tail_set_base + tset_of[pad] * 32;

  // ---- the lanes' cells: register J = 2 * slot + k of lane l is row 2l + k - rowoff, column (slot - l) mod NR
  const int NE = 2 * NR;
  auto row_of = [&](int lane, int k) { return 2 * lane + k - rowoff; };
  auto reg_cell = [&](int lane, int J, int &R, int &col) {
    const int j = J / 2;
    col = ((j - lane) % NR + NR) % NR;
    R = row_of(lane, J & 1);
    return J < NE && R >= 0 && R < Hw && col < Ws;
  };
  // ---- the zone-sum scratch: one slot per (zone, lane) that owns a cell of the zone; zone Z (every cell
  // outside a zone, the tail rows) has a slot for every lane
  std::vector<std::vector<int>> zl(Z + 1);
  {
    std::vector<char> seen((size_t)(Z + 1) * 64, 0);
    for (int lane = 0; lane < 64; ++lane) {
      seen[(size_t)Z * 64 + lane] = 1;
      for (int J = 0; J < NE; ++J) {
        int R, col;
        if (reg_cell(lane, J, R, col) && zone_of[(x0 + R) * W + (y0 + col)] >= 0) seen[(size_t)zone_of[(x0 + R) * W + (y0 + col)] * 64 + lane] = 1;
      }
    }
    for (int z = 0; z <= Z; ++z)
      for (int lane = 0; lane < 64; ++lane)
        if (seen[(size_t)z * 64 + lane]) zl[z].push_back(lane);
  }
  r.zs_off.assign(Z + 2, 0);
  for (int z = 0; z <= Z; ++z) r.zs_off[z + 1] = r.zs_off[z] + (int)zl[z].size();
  const int zs_slots = r.zs_off[Z + 1];
  if (zs_slots > 65535) return false;
  auto zslot = [&](int z, int lane) {
    const auto it = std::lower_bound(zl[z].begin(), zl[z].end(), lane);
    return r.zs_off[z] + (int)(it - zl[z].begin());
  };

  // ---- LDS: [sets 4 kSets][ap g: 2 (ncls + 1), rounded to 8][first tail row][A rows: nl (+ 1 for the idle lanes)]
  // As many buildings per CU as the kernel has a level for (A's other slots stream from L2: step_two.hip).
  auto lds_bytes_for = [&](int level, int &AS, int &r_seam, int &r_A) {
    AS = sweep_two_a_stride(NR, level);
    int off = 4 * kSets + ((2 * (ncls + 1) + 7) & ~7);
    r_seam = off; off += sweep_two_seam_doubles(NR);
    r_A = off; off += std::max((nl < 64 ? nl + 1 : 64) * AS, zs_slots);
    return off * 8;
  };
  auto per_cu = [&](int bytes) { return std::min(4, kLdsCap / ((bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule)); };
  int AS = 0, r_seam = 0, r_A = 0, bytes = 0, level = 0;
  int max_level = sym ? sweep_two_levels() - 1 : 0;
  max_level = std::min(max_level, k.two_max_level);
  for (int lv = 0; lv <= max_level; ++lv) { // the lowest level that holds the most buildings
    int as_, rs_, ra_;
    const int b_ = lds_bytes_for(lv, as_, rs_, ra_);
    if (lv == 0 || per_cu(b_) > per_cu(bytes)) { level = lv; bytes = b_; AS = as_; r_seam = rs_; r_A = ra_; }
  }
  bytes += k.lds_pad;
  r.two_level = level;
  r.r_seam = r_seam; r.r_A = r_A; r.r_xchg = 0; r.AS = AS;
  r.lds_bytes = bytes;
  r.wg_per_cu = per_cu(bytes);
  if (r.wg_per_cu < 1) { r.csetab.clear(); return false; }

  r.NR = NR; r.kernel = SB_KERNEL_TWO_ROWS; r.RS = 64; r.Ws = Ws; r.r0 = x0; r.c0 = y0; r.n_ring = N - Hs * Ws;
  r.T = T; r.ts = ts;
  r.state_doubles = NE * 64 + T * NR;
  r.lw[0] = nl; r.l0[0] = 0; r.rowbase[0] = 0; r.nch[0] = 0;
  r.lag = 0; r.nslots = 0;
  r.steps = NR + nl - 1 + 4 * T;
  const int NW = NR / 4, NWD = (NE + 3) / 4; // step_two.hip: class words of four steps, NR / 4 per lane
  r.cmapS.assign((size_t)NW * 64, 0);
  r.amapS.assign((size_t)NWD * 64, 0);
  r.zmapS.assign((size_t)NWD * 64, 0);
  r.tcls.assign((size_t)std::max(T, 1) * NR, (uint8_t)pad);
  r.tcset.assign((size_t)std::max(T, 1) * NR, (uint8_t)(8 * tset_of[pad]));
  for (int t = 0; t < T; ++t)
    for (int c = 0; c < NR; ++c) {
      r.tcls[(size_t)t * NR + c] = (uint8_t)cell_class(Hw + t, c);
      r.tcset[(size_t)t * NR + c] = (uint8_t)(8 * tset_of[cell_class(Hw + t, c)]);
    }
  for (int lane = 0; lane < 64; ++lane) {
    auto row_class = [&](int k, int col) { // upper / lower cell of the lane at a column of the wavefront rows
      const int R = row_of(lane, k);
      return (R >= 0 && R < Hw && col >= 0 && col < NR) ? cell_class(R, col) : pad;
    };
    for (int wd = 0; wd < NW; ++wd) { // a byte per cell and step: the coefficient sets of the lane's (upper, lower) cell
      unsigned long long word = 0;
      for (int k = 0; k < 4; ++k) { // at step s (of a ramp-up or of any period) the lane works on column (s - lane) mod NR
        const int col = ((4 * wd + k - lane) % NR + NR) % NR;
        word |= (unsigned long long)set_of[row_class(0, col)] << (16 * k);
        word |= (unsigned long long)set_of[row_class(1, col)] << (16 * k + 8);
      }
      r.cmapS[(size_t)wd * 64 + lane] = word;
    }
    for (int g = 0; g < NWD; ++g) { // register J = 2 * slot + k
      unsigned long long aword = 0, zword = 0;
      for (int k = 0; k < 4; ++k) {
        const int J = 4 * g + k;
        int R, col;
        const bool cell = reg_cell(lane, J, R, col);
        aword |= (unsigned long long)((cell ? cell_class(R, col) : pad) * 16) << (16 * k);
        int z = Z; // the dump zone
        if (cell && zone_of[(x0 + R) * W + (y0 + col)] >= 0) z = zone_of[(x0 + R) * W + (y0 + col)];
        zword |= (unsigned long long)zslot(z, lane) << (16 * k);
      }
      r.amapS[(size_t)g * 64 + lane] = aword;
      r.zmapS[(size_t)g * 64 + lane] = zword;
    }
  }
  r.cell_state.assign(N, 0);
  int ring = 0;
  for (int x = 0; x < plan->H; ++x)
    for (int y = 0; y < W; ++y) {
      const int R = x - x0, col = y - y0;
      if (R < 0 || R >= Hs || col < 0 || col >= Ws) { r.cell_state[x * W + y] = -(++ring); continue; }
      if (R >= Hw) { r.cell_state[x * W + y] = NE * 64 + (R - Hw) * NR + col; continue; }
      const int lane = (R + rowoff) >> 1;
      r.cell_state[x * W + y] = (2 * ((col + lane) % NR) + ((R + rowoff) & 1)) * 64 + lane;
    }
  r.ok = true;
  return true;
}

// k_sweep_band (step_band.hip): two to four wavefronts per building, one row per lane (rows 64 w .. 64 w + 63) + at
// most two tail rows, up to 96 columns inside the exterior ring; sweeps overlapped in predicted blocks.
bool plan_band(const sb_plan_desc *plan, int Hs, int Ws, int x0, int y0, const std::vector<int> &zone_of, const Knobs &k, RegPlan &r) {
  const int W = plan->W, Z = plan->Z, ncls = plan->n_classes, N = plan->H * plan->W;
  int NR = 0;
  for (int s : {68, 72, 76, 80, 84, 88, 92, 96}) // the narrowest instantiation that holds the width: a period is NR steps
    if (!NR && s >= Ws && sweep_band_supported(s)) NR = s;
  if (!NR || Hs <= 64) return false;
  // wavefronts: the fewest whose rows + two tail rows hold the plan; a zone cell in a tail row needs one more
  int NWV = 0, T = 0;
  for (int w = 2; w <= sweep_band_max_waves() && !NWV; ++w) {
    if (Hs > 64 * w + 2) continue;
    const int t = std::max(0, Hs - 64 * w);
    bool zone_free = true; // the tail scan adds no zone sums
    for (int x = x0 + Hs - t; x < x0 + Hs; ++x)
      for (int y = y0; y < y0 + Ws; ++y) zone_free = zone_free && zone_of[x * W + y] < 0;
    if (zone_free) { NWV = w; T = t; }
  }
  if (!NWV) return false;
  const int Hw = Hs - T, RS = 64 * NWV;
  int ts = 32;
  while (ts < ncls + 1) ts *= 2;
  if (ts > 256) return false;
  const int pad = ncls;
  r.csetab.clear();
  const std::vector<int> set_of = coefficient_sets(plan, r.csetab);
  if ((int)r.csetab.size() / 4 > sweep_band_set_table()) { r.csetab.clear(); return false; }
  auto cell_class = [&](int R, int col) { // trimmed coordinates
    return (R >= 0 && R < Hs && col >= 0 && col < Ws) ? (int)plan->cell_class[(x0 + R) * W + (y0 + col)] : pad;
  };
  auto zone_at = [&](int R, int col) { // the zone of a wavefront-row cell; Z: none (the dump zone)
    if (R >= Hw || col >= Ws) return Z;
    const int z = zone_of[(x0 + R) * W + (y0 + col)];
    return z >= 0 ? z : Z;
  };
  // ---- the zone-sum scratch: one slot per (zone, row) whose row holds a cell of the zone; zone Z (every
  // cell outside a zone, the tail rows) has a slot for every lane of every wavefront
  std::vector<std::vector<int>> zl(Z + 1);
  for (int R = 0; R < RS; ++R) {
    std::vector<char> seen(Z + 1, 0);
    seen[Z] = 1;
    for (int col = 0; col < Ws && R < Hw; ++col) seen[zone_at(R, col)] = 1;
    for (int z = 0; z <= Z; ++z)
      if (seen[z]) zl[z].push_back(R);
  }
  r.zs_off.assign(Z + 2, 0);
  for (int z = 0; z <= Z; ++z) r.zs_off[z + 1] = r.zs_off[z] + (int)zl[z].size();
  const int zs_slots = r.zs_off[Z + 1];
  if (zs_slots > 65535) { r.csetab.clear(); return false; }
  auto zslot = [&](int z, int R) {
    const auto it = std::lower_bound(zl[z].begin(), zl[z].end(), R);
    return r.zs_off[z] + (int)(it - zl[z].begin());
  };

  const int AS = sweep_band_lds_slots(NR);
  int off = 4 * sweep_band_set_table() + 2 * ts;
  r.r_seam = off; off += sweep_band_seam_doubles(NR, NWV);
  r.r_xchg = off; off += sweep_band_sync_doubles(NWV);
  off = (off + 1) & ~1;
  r.r_A = off; off += std::max(RS * AS, zs_slots); // the zone-sum scratch aliases A
  r.AS = AS;
  r.lds_bytes = off * 8;
  r.lds_bytes += k.lds_pad;
  r.wg_per_cu = std::min(4 / NWV, kLdsCap / ((r.lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule)); // one wavefront per SIMD
  if (r.wg_per_cu < 1) { r.csetab.clear(); r.zs_off.clear(); return false; }

  r.NR = NR; r.kernel = SB_KERNEL_BAND; r.RS = RS; r.Ws = Ws; r.r0 = x0; r.c0 = y0; r.n_ring = N - Hs * Ws;
  r.T = T; r.ts = ts;
  r.state_doubles = NR * RS + T * NR;
  for (int w = 0; w < 4; ++w) r.lw[w] = w < NWV ? std::max(0, std::min(64, Hw - 64 * w)) : 0;
  r.l0[0] = r.l0[1] = 0; r.rowbase[0] = 0; r.rowbase[1] = 64;
  r.nch[0] = r.nch[1] = 0; r.lag = 0; r.nslots = 0;
  r.steps = NR + 4 * T;
  const int NW = NR + 63, NWD = NR / 4;
  std::vector<uint32_t> cw((size_t)NWV * NW * 64, 0);
  r.amapS.assign((size_t)NWV * NWD * 64, 0);
  r.zmapS.assign((size_t)NWV * NWD * 64, 0);
  r.tcls.assign((size_t)std::max(T, 1) * NR, (uint8_t)pad);
  r.tcset.assign((size_t)std::max(T, 1) * NR, (uint8_t)(8 * set_of[pad]));
  for (int t = 0; t < T; ++t)
    for (int c = 0; c < NR; ++c) {
      r.tcls[(size_t)t * NR + c] = (uint8_t)cell_class(Hw + t, c);
      r.tcset[(size_t)t * NR + c] = (uint8_t)(8 * set_of[cell_class(Hw + t, c)]);
    }
  for (int w = 0; w < NWV; ++w)
    for (int lane = 0; lane < 64; ++lane) {
      const int R = 64 * w + lane;
      const bool valid = R < Hw;
      for (int st = 0; st < NW; ++st) { // one word per step: the set offset of the lane's cell
        int col = st - lane;
        if (col >= NR) col -= NR; // rolling periods: the lane is in its next sweep
        const int c = (valid && col >= 0) ? cell_class(R, col) : pad;
        cw[((size_t)w * NW + st) * 64 + lane] = (uint32_t)(set_of[c] * 32);
      }
      for (int g = 0; g < NWD; ++g) {
        unsigned long long aword = 0, zword = 0;
        for (int k = 0; k < 4; ++k) {
          const int j = 4 * g + k, col = ((j - lane) % NR + NR) % NR;
          const bool cell = valid && col < Ws;
          aword |= (unsigned long long)((cell ? cell_class(R, col) : pad) * 16) << (16 * k);
          zword |= (unsigned long long)zslot(cell ? zone_at(R, col) : Z, R) << (16 * k);
        }
        r.amapS[((size_t)w * NWD + g) * 64 + lane] = aword;
        r.zmapS[((size_t)w * NWD + g) * 64 + lane] = zword;
      }
    }
  r.cmapS.assign((cw.size() + 1) / 2, 0);
  std::memcpy(r.cmapS.data(), cw.data(), cw.size() * sizeof(uint32_t));
  r.cell_state.assign(N, 0);
  int ring = 0;
  for (int x = 0; x < plan->H; ++x)
    for (int y = 0; y < W; ++y) {
      const int R = x - x0, col = y - y0;
      if (R < 0 || R >= Hs || col < 0 || col >= Ws) { r.cell_state[x * W + y] = -(++ring); continue; }
      if (R >= Hw) { r.cell_state[x * W + y] = NR * RS + (R - Hw) * NR + col; continue; }
      const int slot = (col + (R & 63)) % NR;
      r.cell_state[x * W + y] = (slot / 2) * 2 * RS + R * 2 + (slot & 1); // state layout [NR / 2][64 W][2]
    }
  r.ok = true;
  return true;
}

// k_sweep_stream (step_stream.hip): the grid stays in global memory; W = ceil(rows / 64) wavefronts per building
// (W <= 16), any width whose seam rows fit in LDS.  For floor plans no other kernel holds.
bool plan_stream(const sb_plan_desc *plan, const Trim &t, const Knobs &k, RegPlan &r, std::string &why) {
  const int H = plan->H, W = plan->W, Z = plan->Z, ncls = plan->n_classes, N = H * W;
  auto cls_at = [&](int x, int y) { return (int)plan->cell_class[x * W + y]; };
  if (!t.why.empty()) { why = t.why; return false; }
  const int x0 = t.x0, y0 = t.y0, Hs = t.Hs, Ws = t.Ws;
  const int NWV = (Hs + 63) / 64;
  if (NWV > 16) { why = "more than 1,024 rows inside the building (try the other orientation)"; return false; }
  const int NS = std::max(72, (Ws + 1) & ~1), RS = 64 * NWV;
  int ts = 32;
  while (ts < ncls + 1) ts *= 2;
  if (ts > 256) { why = "more than 255 cell classes"; return false; }
  const int pad = ncls;
  r.csetab.clear();
  const std::vector<int> set_of = coefficient_sets(plan, r.csetab);
  if ((int)r.csetab.size() / 4 > sweep_stream_set_table()) { why = "more than 31 distinct coefficient sets"; r.csetab.clear(); return false; }
  if (Z > 65534) { why = "too many zones"; r.csetab.clear(); return false; }
  const int ZC = sweep_stream_zone_columns();
  int off = 4 * sweep_stream_set_table() + 2 * ts;
  // step_stream_ms.hip (several sweeps per pass over the grid: a seam row per sweep) -- OPT-IN, SBSIM_STREAM_MS=1: correct
  // (bit-identical iterates, tests/test_gpu_parity.py) but not faster yet (LABNOTES.md 5.4c: 256 registers leave two
  // wavefronts per SIMD, and a step of four sweep slots takes 3.3x a step of step_stream.hip's one).  Needs its LDS to fit
  // and the last wavefront to own the spare rows its bands need (the band of sweep j sits j rows further up).
  {
    const int ms_off = off + sweep_stream_ms_seam_doubles(NS, NWV) + sweep_stream_ms_xchg_doubles(NWV) + (Z + 1) * ZC;
    if (k.stream_ms && ms_off * 8 <= kLdsCap && 64 * NWV - Hs >= sweep_stream_ms_sweeps() - 1 &&
        NWV <= 8) r.stream_variant = kStreamMs; // (its 256 registers: two wavefronts per SIMD, workgroups of at most 8)
  }
  r.r_seam = off; off += r.stream_variant == kStreamMs ? sweep_stream_ms_seam_doubles(NS, NWV) : 2 * NWV * (NS + 8);
  // overlapped sweeps (step_stream.hip's k_sweep_stream_roll, round 5) -- OPT-IN, SBSIM_STREAM_ROLL=1: kStreamRoll.  Exact
  // (tests/test_gpu_parity.py), 9 % faster on R9 forced here, 9 % SLOWER on the 299 x 401 plan it was written for: with three
  // workgroups per CU another workgroup already fills a wavefront's idle steps, and the sweep started in vain is traffic
  if (r.stream_variant == kStreamPlain && k.stream_roll) r.stream_variant = kStreamRoll;
  r.r_xchg = off; off += r.stream_variant == kStreamMs ? sweep_stream_ms_xchg_doubles(NWV) : 32 + 64 * NWV + (r.stream_variant == kStreamRoll ? sweep_stream_roll_xchg_extra_doubles() : 0); // progress, max|delta| parts, the publish scratch
  r.r_A = off; off += (Z + 1) * ZC;
  r.lds_bytes = off * 8;
  if (r.lds_bytes > kLdsCap) { why = "the seam rows (rows / 64 x columns x 16 bytes) and the zone sums do not fit in 160 KiB of LDS"; r.csetab.clear(); return false; }
  // workgroups per CU: LDS, threads (2,048 per CU) and registers (<= 128 per lane: four wavefronts per SIMD)
  r.wg_per_cu = std::max(1, std::min({kLdsCap / ((r.lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule), 32 / NWV, (r.stream_variant == kStreamMs ? 8 : 16) / NWV}));
  r.NR = NS; r.kernel = SB_KERNEL_STREAM; r.RS = RS; r.Ws = Ws; r.r0 = x0; r.c0 = y0; r.n_ring = N - Hs * Ws;
  r.T = 0; r.ts = ts; r.AS = 0;
  r.state_doubles = NS * RS;
  r.lw[0] = std::min(Hs, 64); r.lw[1] = NWV; // lw[1]: wavefronts per building
  r.steps = 64 * (NWV - 1) + NS + 63;
  auto cell_class = [&](int R, int col) {
    return (R >= 0 && R < Hs && col >= 0 && col < Ws) ? cls_at(x0 + R, y0 + col) : pad;
  };
  const std::vector<int> &zone_of = t.zone_of;
  const int NW = NS + 63;
  std::vector<uint32_t> cw((size_t)NWV * NW * 64, 0);
  std::vector<uint16_t> zm((size_t)NWV * NS * 64, (uint16_t)Z);
  for (int w = 0; w < NWV; ++w)
    for (int lane = 0; lane < 64; ++lane) {
      const int R = 64 * w + lane;
      for (int t = 0; t < NW; ++t) {
        const int col = t - lane;
        const int c = (R < Hs && col >= 0 && col < NS) ? cell_class(R, col) : pad;
        cw[((size_t)w * NW + t) * 64 + lane] = (uint32_t)(set_of[c] * 32) | ((uint32_t)(c * 16) << 16);
      }
      for (int s = 0; s < NS; ++s) {
        const int col = ((s - lane) % NS + NS) % NS;
        if (R < Hs && col < Ws && zone_of[(x0 + R) * W + (y0 + col)] >= 0)
          zm[((size_t)w * NS + s) * 64 + lane] = (uint16_t)zone_of[(x0 + R) * W + (y0 + col)];
      }
    }
  r.cmapS.assign((cw.size() + 1) / 2, 0);
  std::memcpy(r.cmapS.data(), cw.data(), cw.size() * sizeof(uint32_t));
  r.zmapS.assign((zm.size() + 3) / 4, 0);
  std::memcpy(r.zmapS.data(), zm.data(), zm.size() * sizeof(uint16_t));
  r.amapS.assign(1, 0);
  r.tcls.assign(1, (uint8_t)0);
  r.tcset.assign(1, (uint8_t)0);
  r.cell_state.assign(N, 0);
  int ring = 0;
  for (int x = 0; x < H; ++x)
    for (int y = 0; y < W; ++y) {
      const int R = x - x0, col = y - y0;
      if (R < 0 || R >= Hs || col < 0 || col >= Ws) { r.cell_state[x * W + y] = -(++ring); continue; }
      r.cell_state[x * W + y] = ((col + (R & 63)) % NS) * RS + R; // state layout [NS][RS]
    }
  r.ok = true;
  return true;
}

// lds_per_cu: buildings per CU the LDS-grid kernel would hold (0: the plan does not fit it).
void plan_reg(const sb_plan_desc *plan, const Trim &t, int lds_per_cu, const Knobs &k, RegPlan &r) {
  const int H = plan->H, W = plan->W, Z = plan->Z, ncls = plan->n_classes, N = H * W;
  auto coef = [&](int c, int j) { return plan->class_coef[c * 8 + j]; };
  auto cls_at = [&](int x, int y) { return (int)plan->cell_class[x * W + y]; };
  if (!t.why.empty()) { r.why = t.why; return; }
  const int x0 = t.x0, x1 = t.x1, y0 = t.y0, y1 = t.y1, Hs = t.Hs, Ws = t.Ws;
  const std::vector<int> &zone_of = t.zone_of;
  // k_sweep_band: two wavefronts, one row per lane, sweeps overlapped in blocks (67..130 rows, <= 80 columns).
  // Measured level with k_sweep_two (profiles/r04_band_vs_two_rows.txt): all four SIMDs run, but four
  // wavefronts share the CU's LDS pipe, every block starts with wavefront 1's 64-step lag and the tail
  // scan sits on wavefront 1's critical path.  Kept, tested, behind SBSIM_BAND_PATH=1.
  if (Hs > 64 + 2 && k.band_path && plan_band(plan, Hs, Ws, x0, y0, zone_of, k, r)) return;
  // k_sweep_two: one wavefront, two rows per lane (67..130 rows, <= 80 columns)
  if (Hs > 64 + 2 && !k.no_two_row && plan_two(plan, Hs, Ws, x0, y0, zone_of, k, r)) return;
  // k_sweep_band again, for what k_sweep_two does not hold: beyond 128 rows (up to 258) three or four wavefronts share a
  // building; 67..130 rows with 81..96 columns two (measured 1.2-2.6x the two-wavefront k_sweep_reg / the LDS-grid
  // kernel on 109 x 92, 113 x 93 and 125 x 97: tools/bench_mid_plans.py)
  if (Hs > 64 + 2 && !k.no_band && plan_band(plan, Hs, Ws, x0, y0, zone_of, k, r)) return;
  auto pick_slots = [&](sb_sweep_kernel kernel) { // narrowest instantiation that holds the width and the class count
    if (kernel == SB_KERNEL_ROLL) {
      for (int s : {64, 72, 80, 88, 96}) // SBSIM_NO_ROLL_64=1: the 96-slot instantiation alone (the tree before round 4's last additions)
        if (s >= Ws && sweep_roll_supported(s) && ncls + 1 <= 32 && !(s < 96 && k.no_roll_64)) return s;
      return 0;
    }
    for (int s : kRegSlots)
      if (s >= Ws && sweep_reg_supported(s, kernel) && ncls + 1 <= sweep_reg_table_stride(s, kernel)) return s;
    return 0;
  };
  // SB_KERNEL_REG: one wavefront; SB_KERNEL_ROLL: one wavefront + one or two tail rows finished by a scan
  // (no zone cell may sit in a tail row); SB_KERNEL_REG_PAIR: two wavefronts.  SB_KERNEL_LDS here: none of them (yet)
  sb_sweep_kernel kernel = Hs <= 64 ? SB_KERNEL_REG : SB_KERNEL_LDS;
  int NR = kernel == SB_KERNEL_REG ? pick_slots(SB_KERNEL_REG) : 0;
  // ... but not on k_sweep_reg<NR,1> (round 1's kernel: a sweep of NR + rows - 1 steps, no overlap) when k_sweep_roll's
  // period is no longer than that: the roll kernel without tail rows, the lanes beyond the plan own pad rows
  // (measured, 65,536 buildings: 47 x 98 / 6 zones 6.8 -> 1.9 ms per step, 62 x 97 4.8 -> 2.5, 49 x 50 8.9 -> 7.6;
  // 25 x 38 and 17 x 25 stay: 3.3 against 4.4, 2.6 against 4.9)
  // (only when the roll kernel's own limits hold -- its zone-sum scratch takes <= 31 zones; its LDS layout always fits: checked
  // HERE, before the switch, so that a plan it cannot take stays on k_sweep_reg<NR,1> instead of falling through to the
  // LDS-grid kernel)
  const int roll_slots = pick_slots(SB_KERNEL_ROLL);
  if (kernel == SB_KERNEL_REG && NR && !k.no_roll_small && roll_slots && Z <= 31 && NR + Hs - 1 >= roll_slots) {
    kernel = SB_KERNEL_ROLL; NR = roll_slots;
  }
  if (kernel == SB_KERNEL_LDS && Hs <= 64 + 2 && roll_slots) {
    bool zone_free = true;
    for (int x = x0 + 64; x <= x1; ++x)
      for (int y = y0; y <= y1; ++y) zone_free = zone_free && zone_of[x * W + y] < 0;
    if (zone_free) { kernel = SB_KERNEL_ROLL; NR = roll_slots; }
  }
  if (kernel == SB_KERNEL_LDS && Hs <= 128) {
    kernel = SB_KERNEL_REG_PAIR; NR = pick_slots(SB_KERNEL_REG_PAIR);
    // a two-wavefront variant that runs one wavefront per SIMD holds two buildings per CU and
    // pays the seam lag: measured no faster than the LDS-grid kernel at two buildings per CU
    if (NR && sweep_reg_waves_per_simd(NR, SB_KERNEL_REG_PAIR) == 1 && lds_per_cu >= 2) {
      r.why = "the LDS-grid kernel holds as many buildings per CU";
      return;
    }
  }
  if (kernel == SB_KERNEL_LDS) { r.why = "more than 128 rows inside the building"; return; }
  if (!NR) { r.why = "no kernel variant for this width and class count"; return; }
  const bool roll = kernel == SB_KERNEL_ROLL, pair = kernel == SB_KERNEL_REG_PAIR;
  const int TS = roll ? 32 : sweep_reg_table_stride(NR, kernel), cscale = 256 / TS; // class byte = class * cscale
  const int nl_slots = roll ? sweep_roll_lds_slots(NR) : sweep_reg_lds_slots(NR, kernel);
  r.ts = TS;
  const int RS = roll ? 64 : Hs;
  // the zone-sum scratch aliases A.  k_sweep_reg: [Z + 1][ZRS = rows | 1] (odd stride: the zone reduce reads 16 zone rows at once),
  // 16-bit byte offsets.  k_sweep_roll: [64 rows][ZRS = (Z + 1) | 1], a slot's offset inside its lane's row is zone * 8:
  // one byte (Z <= 31: every zone has a cell class of its own and the class table holds 32)
  const int ZRS = roll ? ((Z + 1) | 1) : (RS | 1);
  if (roll ? (Z > 31 || ZRS > nl_slots) : ((size_t)(Z + 1) * ZRS > (size_t)RS * nl_slots || (size_t)(Z + 1) * ZRS * 8 > 65535)) {
    r.why = "too many zones for the zone-sum scratch"; // it aliases A
    return;
  }
  r.ZRS = ZRS;
  r.NR = NR; r.kernel = kernel; r.RS = RS; r.Ws = Ws; r.r0 = x0; r.c0 = y0; r.n_ring = N - Hs * Ws;
  r.T = roll ? std::max(0, Hs - 64) : 0;
  r.state_doubles = NR * RS + r.T * NR;
  const int maxch = (NR + 63 + 7) / 8;
  if (roll) {
    r.lw[0] = 64; r.l0[0] = 0; r.rowbase[0] = 0;
    r.nch[0] = (NR + 63 + 7) / 8;
    r.lag = 0; r.nslots = r.nch[0];
    r.steps = NR + 4 * r.T; // overlapped sweeps: NR steps per sweep; a tail row's scan costs about 4 wavefront steps
  } else if (kernel == SB_KERNEL_REG) {
    r.lw[0] = Hs; r.l0[0] = 0; r.rowbase[0] = 0;
    r.nch[0] = (NR + Hs - 1 + 7) / 8;
    r.lag = 0; r.nslots = r.nch[0];
    r.steps = NR + Hs - 1;
  } else {
    int best = -1, best_slots = 1 << 30;
    for (int a0 = Hs - 64; a0 <= 64; ++a0) {
      if (a0 < 1 || Hs - a0 < 1) continue;
      const int n0 = (NR + a0 - 1 + 7) / 8, n1 = (NR + (Hs - a0) - 1 + 7) / 8;
      const int slots = std::max(n0, seam_lag(a0) + n1);
      if (slots < best_slots || (slots == best_slots && std::abs(2 * a0 - Hs) < std::abs(2 * best - Hs))) {
        best = a0; best_slots = slots;
      }
    }
    r.lw[0] = best; r.lw[1] = Hs - best;
    r.l0[0] = 64 - best; r.l0[1] = 0;       // wave 0's rows sit in its top lanes: seam row = lane 63
    r.rowbase[0] = 0; r.rowbase[1] = best;
    r.nch[0] = (NR + r.lw[0] - 1 + 7) / 8; r.nch[1] = (NR + r.lw[1] - 1 + 7) / 8;
    r.lag = seam_lag(best); r.nslots = best_slots;
    r.steps = 8 * (r.lag + r.nch[1]); // critical path: wave 1 starts `lag` chunks late
  }
  // LDS layout (doubles).  A's rows are read lane-per-row at a common column: an odd row
  // stride spreads the 64 lanes over all banks (stride 96 doubles would put them all on one)
  // -- unless the extra column costs a resident building.
  auto layout = [&](int AS) {
    r.AS = AS;
    if (roll) { // step_roll.hip: [coefficient sets | class words] shared, then per wavefront [ap g | first tail row | A]
      r.waves_per_wg = sweep_roll_waves();
      r.r_cmap = 4 * TS;
      r.r_seam = 2 * TS;
      r.r_A = r.r_seam + ((sweep_roll_seam_doubles(NR, r.T) + 1) & ~1); // 16-byte aligned rows
      r.wave_doubles = r.r_A + RS * nl_slots; // rows of AS slots, then [RS][nl_slots - AS]
      r.lds_bytes = (r.r_cmap + (NR / 8) * 64 + sweep_roll_tail_mul_doubles(NR, r.T) + r.waves_per_wg * r.wave_doubles) * 8;
      r.lds_bytes += k.lds_pad;
      r.wg_per_cu = r.lds_bytes <= kLdsCap ? 1 : 0;
      return;
    }
    int off = 5 * TS + TS;
    r.r_seam = off;
    off += pair ? 2 * (NR + 2 * kRegSeamPad) : 0;
    r.r_A = off; off += RS * AS;
    r.r_xchg = off; off += 8;
    r.lds_bytes = off * 8;
    r.lds_bytes += k.lds_pad; // developer knob: fewer buildings per CU
    // workgroups per CU: LDS, and the registers (4 SIMDs x wavefronts per SIMD / wavefronts per building)
    const int by_regs = 4 * sweep_reg_waves_per_simd(NR, kernel) / (pair ? 2 : 1);
    r.wg_per_cu = std::min(by_regs, kLdsCap / ((r.lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule));
  };
  const int nl = nl_slots; // slots of A in LDS (the kernel keeps the rest in registers)
  if (roll) {
    layout(sweep_roll_a_stride(NR)); // 2 mod 4 doubles: 16-byte aligned rows, conflict-free ds_read_b128
  } else {
    layout(nl);
    const int plain = r.wg_per_cu;
    layout(nl | 1);
    if (r.wg_per_cu < plain) layout(nl);
  }
  if (r.wg_per_cu < 1) { r.why = "one building does not fit in LDS"; return; }

  const int pad = ncls;
  // k_sweep_roll: the sweep looks its four neighbour coefficients up by coefficient SET (classes that
  // differ only in ap / g share one): fewer distinct LDS addresses per wavefront read
  std::vector<int> set_of(ncls + 1, 0);
  if (roll) {
    set_of = coefficient_sets(plan, r.csetab);
    if (r.csetab.size() / 4 > 32) { r.why = "more than 32 distinct coefficient sets"; r.ok = false; return; }
  }
  auto cell_class = [&](int R, int col) { // trimmed coordinates
    return (R >= 0 && R < Hs && col >= 0 && col < Ws) ? cls_at(x0 + R, y0 + col) : pad;
  };
  const int aslots = (NR + 7) / 8, zslots = roll ? NR / 8 : (NR + 3) / 4;
  const int nw = pair ? 2 : 1;
  r.cmapS.assign(roll ? (size_t)(NR / 8) * 64 : (size_t)nw * (maxch + 3) * 64, 0);
  r.amapS.assign((size_t)nw * aslots * 64, 0);
  r.zmapS.assign((size_t)nw * zslots * 64, 0);
  r.tcls.assign((size_t)std::max(r.T, 1) * NR, (uint8_t)(8 * pad));
  r.tcset.assign((size_t)std::max(r.T, 1) * NR, (uint8_t)(8 * set_of[pad]));
  for (int t = 0; t < r.T; ++t)
    for (int c = 0; c < NR; ++c) {
      r.tcls[(size_t)t * NR + c] = (uint8_t)(8 * cell_class(64 + t, c));
      r.tcset[(size_t)t * NR + c] = (uint8_t)(8 * set_of[cell_class(64 + t, c)]);
    }
  if (roll && r.T > 0) {
    // The tail scan (sweep_common.h): along a tail row x_c = bL_c x_{c-1} + q_c; lane l >= L0 composes its two
    // columns, six DPP levels scan the lanes.  The multiplicative half of every level does not depend on the
    // temperatures: it is run here, in affine_scan's own order (bit-identical), and the kernel reads what each
    // level multiplies by: `a` entering levels 1..5, 0 where the level has no source lane for the lane.
    const int n = NR / 2, L0 = 64 - n;
    r.tmul.assign((size_t)sweep_roll_tail_mul_doubles(NR, r.T), 0.0);
    auto src_lane = [](int level, int lane) { // the DPP source of affine_scan's levels: row_shr 1 / 2 / 4 / 8, row_bcast:15 (rows 1, 3), row_bcast:31 (rows 2, 3)
      const int row = lane >> 4, i = lane & 15;
      switch (level) {
        case 0: return i >= 1 ? lane - 1 : -1;
        case 1: return i >= 2 ? lane - 2 : -1;
        case 2: return i >= 4 ? lane - 4 : -1;
        case 3: return i >= 8 ? lane - 8 : -1;
        case 4: return (row & 1) ? (row << 4) - 1 : -1;
        default: return row >= 2 ? 31 : -1;
      }
    };
    for (int t = 0; t < r.T; ++t) {
      auto bL = [&](int c) { const int cl = cell_class(64 + t, c); return cl == pad ? 0.0 : coef(cl, 2); };
      double a[64], an[64];
      for (int lane = 0; lane < 64; ++lane) a[lane] = lane >= L0 ? bL(2 * (lane - L0) + 1) * bL(2 * (lane - L0)) : 0.0;
      for (int d = 0; d < 6; ++d) {
        for (int lane = 0; lane < 64; ++lane) {
          const int src = src_lane(d, lane), lp = lane - L0;
          const double A = src >= 0 ? a[lane] : 0.0;
          if (lp >= 0 && (d == 1 || d == 2)) r.tmul[(size_t)4 * n * t + 2 * lp + (d - 1)] = A;
          if (lp >= 0 && (d == 3 || d == 4)) r.tmul[(size_t)4 * n * t + 2 * n + 2 * lp + (d - 3)] = A;
          if (lp >= 0 && d == 5) r.tmul[(size_t)4 * n * r.T + 2 * lp + t] = A;
          an[lane] = a[lane] * (src >= 0 ? a[src] : 1.0);
        }
        std::memcpy(a, an, sizeof(a));
      }
    }
  }
  for (int w = 0; w < nw; ++w)
    for (int lane = 0; lane < 64; ++lane) {
      const int lp = lane - r.l0[w];
      const bool valid = lp >= 0 && lp < r.lw[w];
      const int R = r.rowbase[w] + lp;
      if (roll) {
        // step_roll.hip: one byte per step = the cell's coefficient set (its LDS byte offset is set * 32),
        // eight steps per word; at step s (of the ramp-up or of any period) the lane works on column
        // (s - lane) mod NR
        for (int ch = 0; ch < NR / 8; ++ch) {
          unsigned long long word = 0;
          for (int k = 0; k < 8; ++k) {
            const int col = ((8 * ch + k - lp) % NR + NR) % NR;
            const int c = valid ? cell_class(R, col) : pad;
            word |= (unsigned long long)set_of[c] << (8 * k);
          }
          r.cmapS[(size_t)ch * 64 + lane] = word;
        }
      } else
      for (int ch = 0; ch < maxch + 3; ++ch) {
        unsigned long long word = 0;
        for (int k = 0; k < 8; ++k) {
          int col = 8 * ch + k - lp;
          const int c = valid ? cell_class(R, col) : pad;
          word |= (unsigned long long)(c * cscale) << (8 * k); // stride 32: the byte offset into a table column
        }
        r.cmapS[((size_t)w * (maxch + 3) + ch) * 64 + lane] = word;
      }
      for (int g = 0; g < aslots; ++g) {
        unsigned long long word = 0;
        for (int k = 0; k < 8; ++k) {
          const int j = 8 * g + k;
          const int col = ((j - lp) % NR + NR) % NR;
          const int c = (valid && j < NR) ? cell_class(R, col) : pad;
          word |= (unsigned long long)(c * cscale) << (8 * k);
        }
        r.amapS[((size_t)w * aslots + g) * 64 + lane] = word;
      }
      if (roll) { // step_roll.hip: a byte per slot = zone * 8 (the byte offset inside the lane's row of the scratch), eight slots per word
        for (int g = 0; g < zslots; ++g) {
          unsigned long long word = 0;
          for (int k = 0; k < 8; ++k) {
            const int j = 8 * g + k;
            const int col = ((j - lp) % NR + NR) % NR;
            int z = Z; // dump column
            if (valid && R < Hs && col < Ws) { // (below 64 rows the lanes beyond the plan own pad rows)
              const int zz = zone_of[(x0 + R) * W + (y0 + col)];
              if (zz >= 0) z = zz;
            }
            word |= (unsigned long long)(z * 8) << (8 * k);
          }
          r.zmapS[(size_t)g * 64 + lane] = word;
        }
      } else
      for (int g = 0; g < zslots; ++g) {
        unsigned long long word = 0;
        for (int k = 0; k < 4; ++k) {
          const int j = 4 * g + k;
          const int col = ((j - lp) % NR + NR) % NR;
          int z = Z; // dump row
          if (valid && R < Hs && j < NR && col < Ws) { // (k_sweep_roll below 64 rows: the lanes beyond the plan own pad rows)
            const int zz = zone_of[(x0 + R) * W + (y0 + col)];
            if (zz >= 0) z = zz;
          }
          const unsigned offb = (unsigned)((z * ZRS + (valid ? R : 0)) * 8);
          word |= (unsigned long long)offb << (16 * k);
        }
        r.zmapS[((size_t)w * zslots + g) * 64 + lane] = word;
      }
    }
  r.cell_state.assign(N, 0);
  int ring = 0;
  for (int x = 0; x < H; ++x)
    for (int y = 0; y < W; ++y) {
      if (x < x0 || x > x1 || y < y0 || y > y1) { r.cell_state[x * W + y] = -(++ring); continue; }
      const int R = x - x0, col = y - y0;
      if (roll && R >= 64) { r.cell_state[x * W + y] = NR * 64 + (R - 64) * NR + col; continue; }
      const int w = (pair && R >= r.lw[0]) ? 1 : 0;
      const int lp = R - r.rowbase[w];
      const int slot = (col + lp) % NR;
      if (roll) r.cell_state[x * W + y] = (slot / 2) * 128 + R * 2 + (slot & 1); // step_roll.hip: [NR / 2][64][2]
      else r.cell_state[x * W + y] = slot * RS + R;                                   // state layout [NR][RS]
    }
  r.ok = true;
}

struct LdsPlan { // launch geometry of the LDS-grid kernel
  int pitch, NL, S, nsteps, nbands, fast, ts, off_agtab, off_zscr, off_zmode, off_wtab, lds_wave_doubles;
  unsigned S_magic;
  size_t shared_bytes, wave_bytes;
  bool fits;
};

// per_building (sb_create_materials): the [5][ts] coefficient table is the wavefront's own, not the workgroup's
LdsPlan plan_lds(const sb_plan_desc *plan, bool per_building = false) {
  LdsPlan q{};
  const int H = plan->H, W = plan->W, Z = plan->Z;
  q.pitch = (W + 1) & ~1; // even pitch: skewed ds_read_b64 is bank-conflict free
  q.NL = H * q.pitch;
  q.nbands = (H + 63) / 64;
  // band stride: >= kChunk idle positions between a lane's rows, and with several bands the
  // seam row must be written >= 17 steps before lane 0 prefetches it (S - 63 > 2*kChunk)
  q.S = std::max(W + kChunk, q.nbands > 1 ? 64 + 2 * kChunk : 64);
  q.S_magic = (unsigned)((1ull << 32) / (unsigned)q.S) + 1u;
  const int rows_last = H - (q.nbands - 1) * 64;
  q.nsteps = (q.nbands - 1) * q.S + rows_last + W - 1;
  q.fast = (q.nbands == 1) || (q.S - 63 > 2 * kChunk);
  int off = ((q.NL + 1) & ~1) + 2 * kGuardHost;
  q.ts = plan->n_classes <= 32 ? 32 : (plan->n_classes <= 128 ? 128 : 256);
  q.off_agtab = off; off += q.ts;
  q.off_zscr = off; off += (3 * Z + 1) & ~1;
  q.off_zmode = off; off += ((Z + 1) / 2 + 1) & ~1;
  q.off_wtab = off; off += per_building ? 5 * q.ts : 0;
  q.lds_wave_doubles = off;
  q.shared_bytes = (size_t)(per_building ? 0 : 5 * q.ts) * 8 + (size_t)((Z + 2) >> 1) * 8;
  q.wave_bytes = (size_t)off * 8;
  q.fits = q.shared_bytes + q.wave_bytes <= (size_t)kLdsCap && q.NL < 65535;
  return q;
}

int lds_buildings_per_cu(const LdsPlan &q) {
  return q.fits ? (int)(((size_t)kLdsCap - q.shared_bytes) / q.wave_bytes) : 0;
}

int check_plan(const sb_plan_desc *plan) {
  if (!plan) return fail(SB_ERR_INVALID, "null floor plan");
  if (plan->H < 1 || plan->W < 1 || plan->Z < 0 || plan->n_classes < 1 || plan->n_classes > 255)
    return fail(SB_ERR_INVALID, "sb_create: bad floor-plan dimensions");
  if (!plan->cell_class || !plan->class_coef || !plan->class_zone || !plan->zone_off ||
      (plan->zone_off[plan->Z] > 0 && !plan->zone_cells))
    return fail(SB_ERR_INVALID, "sb_create: null floor-plan table");
  for (int z = 0; z < plan->Z; ++z)
    if (plan->zone_off[z + 1] < plan->zone_off[z] || plan->zone_off[0] != 0)
      return fail(SB_ERR_INVALID, "sb_create: zone offsets must start at 0 and be non-decreasing");
  const int N = plan->H * plan->W;
  for (int i = 0; i < plan->zone_off[plan->Z]; ++i)
    if (plan->zone_cells[i] < 0 || plan->zone_cells[i] >= N)
      return fail(SB_ERR_INVALID, "sb_create: zone cell out of range");
  for (int i = 0; i < N; ++i)
    if (plan->cell_class[i] >= plan->n_classes) return fail(SB_ERR_INVALID, "sb_create: cell class out of range");
  for (int c = 0; c < plan->n_classes; ++c)
    if (plan->class_zone[c] >= plan->Z) return fail(SB_ERR_INVALID, "sb_create: class zone out of range");
  return SB_OK;
}

void fill_launch_info(const sb_plan_desc *plan, const RegPlan &r, const LdsPlan &q, int n_obs, int cus,
                      int n_buildings, sb_launch_info *out, int n_actions = SB_NUM_ACTIONS) {
  const int64_t N = (int64_t)plan->H * plan->W, Z = plan->Z;
  out->algorithmic_bytes_per_env_step = 8ll * N + 24ll * Z + 4ll * n_actions + 4ll * n_obs + 44;
  const int64_t rest = (8 * 4 + 4 * 2) * Z + 16ll * kNScalOut + 4ll * n_actions + 4ll * n_obs + 4;
  out->kernel = r.kernel;
  if (r.kernel == SB_KERNEL_STREAM) { // step_stream.hip: the grid in global memory
    out->path = 2;
    out->waves_per_building = out->waves_per_workgroup = r.lw[1];
    out->workgroups = std::max(1, std::min(n_buildings, cus * r.wg_per_cu));
    out->lds_bytes_per_workgroup = r.lds_bytes;
    out->sweep_steps = r.steps;
    out->state_bytes_per_env_step = 16ll * r.state_doubles + rest;
  } else if (r.kernel != SB_KERNEL_LDS) {
    const int waves = r.kernel == SB_KERNEL_BAND ? r.RS / 64 : r.kernel == SB_KERNEL_REG_PAIR ? 2 : 1;
    out->path = 1;
    out->waves_per_building = waves;
    out->waves_per_workgroup = waves > 1 ? waves : r.waves_per_wg; // SB_KERNEL_ROLL: four buildings per workgroup
    out->workgroups = std::max(1, std::min((n_buildings + r.waves_per_wg - 1) / r.waves_per_wg, cus * r.wg_per_cu));
    out->lds_bytes_per_workgroup = r.lds_bytes;
    out->sweep_steps = r.steps;
    out->state_bytes_per_env_step = 16ll * r.state_doubles + rest;
  } else {
    int wpw = (int)(((size_t)kLdsCap - q.shared_bytes) / q.wave_bytes);
    wpw = std::max(1, std::min(wpw, 16));
    int wg_per_cu = 1;
    if (wpw > 4) { wg_per_cu = std::min(8, wpw / 4); wpw = 4; } // several smaller workgroups once 4 waves fit
    out->path = 0;
    out->waves_per_building = 1;
    out->waves_per_workgroup = wpw;
    out->workgroups = std::max(1, std::min((n_buildings + wpw - 1) / wpw, cus * wg_per_cu));
    out->lds_bytes_per_workgroup = (int32_t)(q.shared_bytes + q.wave_bytes * wpw);
    out->sweep_steps = q.nsteps;
    out->state_bytes_per_env_step = 16ll * N + rest;
  }
}

// Which sweep kernel owns this floor plan (r.kernel): a register kernel (plan_reg), else the LDS-grid kernel, else --
// plans that fit neither -- the streaming kernel.  SBSIM_FORCE_STREAM_PATH=1: the streaming kernel (tests).
int choose_kernel(const sb_plan_desc *plan, const LdsPlan &q, const Knobs &k, RegPlan &r) {
  std::string why;
  const Trim t = trim_box(plan);
  if (k.force_stream) {
    if (!plan_stream(plan, t, k, r, why)) return fail(SB_ERR_TOO_LARGE, "the streaming sweep kernel cannot hold this floor plan: " + why);
    return SB_OK;
  }
  if (!k.force_lds) plan_reg(plan, t, lds_buildings_per_cu(q), k, r);
  if (r.ok) return SB_OK;
  r = RegPlan(); // (kernel = SB_KERNEL_LDS)
  if (q.fits) return SB_OK;
  if (!plan_stream(plan, t, k, r, why))
    return fail(SB_ERR_TOO_LARGE, "no sweep kernel holds this floor plan (the streaming kernel takes up to 1,024 rows in one "
                                  "orientation and rows / 64 x columns <= ~9,000): " + why);
  return SB_OK;
}

// ---------------------------------------------------------------- sb_create, step by step
// Per zone, the action column that drives its VAV damper (-1: none).
struct ActionTable {
  std::vector<int> zone_act;
  int n_damper_actions = 0;
};

// Every argument check of sb_create, before any HIP call.
int check_create_args(const sb_plan_desc *plan, const sb_params *params, const sb_obs_layout *obs, int n_buildings,
                      ActionTable &acts) {
  int rc = check_plan(plan);
  if (rc != SB_OK) return rc;
  if (n_buildings < 1) return fail(SB_ERR_INVALID, "sb_create: n_buildings must be >= 1");
  if (params->dt <= 0 || params->iter_limit < 1)
    return fail(SB_ERR_INVALID, "sb_create: time_step_sec and iteration_limit must be positive");
  if (params->ahu_cool_sp <= params->ahu_heat_sp) // air_handler.py:60-64
    return fail(SB_ERR_INVALID, "cooling_air_temp_setpoint must greater than heating_air_temp_setpoint");
  if (params->n_actions < 1 || params->n_actions > 3 + plan->Z)
    return fail(SB_ERR_INVALID, "sb_create: n_actions must be in 1 .. 3 + zones (one column per settable field)");
  if (!params->act_kind || !params->act_zone || !params->act_lo || !params->act_hi)
    return fail(SB_ERR_INVALID, "sb_create: null action table (sb_params.act_kind / act_zone / act_lo / act_hi)");
  acts.zone_act.assign((size_t)std::max(plan->Z, 1), -1);
  int seen[3] = {0, 0, 0};
  for (int i = 0; i < params->n_actions; ++i) {
    const int kind = params->act_kind[i];
    if (kind < SB_ACT_BOILER_SUPPLY_WATER_SETPOINT || kind > SB_ACT_VAV_SUPPLY_AIR_DAMPER_COMMAND)
      return fail(SB_ERR_INVALID, "sb_create: unknown action kind");
    if (kind == SB_ACT_VAV_SUPPLY_AIR_DAMPER_COMMAND) {
      const int z = params->act_zone[i];
      if (z < 0 || z >= plan->Z) return fail(SB_ERR_INVALID, "sb_create: VAV action for a zone the floor plan does not have");
      // environment.py:591-653 keys its action normalisers by (device, setpoint): a field has one column
      if (acts.zone_act[z] >= 0) return fail(SB_ERR_INVALID, "sb_create: two action columns drive the same VAV damper");
      acts.zone_act[z] = i;
      ++acts.n_damper_actions;
    } else if (seen[kind]++) {
      return fail(SB_ERR_INVALID, "sb_create: two action columns drive the same setpoint");
    }
  }
  if (obs->n_obs < 1) return fail(SB_ERR_INVALID, "sb_create: empty observation layout");
  if (!obs->mean || !obs->sigma || (plan->Z > 0 && !obs->col_zone))
    return fail(SB_ERR_INVALID, "sb_create: null observation-layout table");
  { // every device field is written unguarded by write_obs: its index must be inside the row / the source table
    const int n_fields = obs->n_src ? obs->n_src : obs->n_obs, n_ahu = params->ahu_has_weather ? 9 : 8;
    bool ok = obs->col_ahu >= 0 && obs->col_ahu + n_ahu <= n_fields && obs->col_boiler >= 0 &&
              obs->col_boiler + 3 <= n_fields && obs->col_aux >= 0 && obs->col_aux + SB_NUM_AUX <= obs->n_obs;
    for (int z = 0; z < plan->Z; ++z) ok = ok && obs->col_zone[z] >= 0 && obs->col_zone[z] + 3 <= n_fields;
    if (!ok) return fail(SB_ERR_INVALID, "sb_create: observation columns outside the observation row");
  }
  for (int z = 0; z < plan->Z; ++z) // building.py:579-587: the mean over a zone's air CVs
    if (plan->zone_off[z + 1] == plan->zone_off[z]) return fail(SB_ERR_INVALID, "sb_create: a zone without cells");
  if (obs->n_src) { // optional HistogramReducer
    const int n_dev_fields = 3 * plan->Z + (params->ahu_has_weather ? 9 : 8) + 3;
    if (obs->n_src != n_dev_fields || !obs->src_dest || obs->n_hist < 0 ||
        (obs->n_hist > 0 && (!obs->hist_col || !obs->hist_off || !obs->hist_bins)))
      return fail(SB_ERR_INVALID, "sb_create: inconsistent histogram-reducer layout");
    for (int i = 0; i < obs->n_src; ++i)
      if (obs->src_dest[i] >= obs->n_obs || obs->src_dest[i] < -obs->n_hist)
        return fail(SB_ERR_INVALID, "sb_create: histogram-reducer destination out of range");
    for (int j = 0; j < obs->n_hist; ++j) {
      const int n = obs->hist_off[j + 1] - obs->hist_off[j];
      if (n < 1 || obs->hist_col[j] < 0 || obs->hist_col[j] + n > obs->n_obs)
        return fail(SB_ERR_INVALID, "sb_create: histogram columns out of range");
    }
  }
  return SB_OK;
}

// The register and streaming kernels (RegPlan): launch geometry, tables, the state in their layout.
int setup_reg(sb_handle *h, const sb_plan_desc *plan, const RegPlan &r, const Knobs &k) {
  Dev &d = h->d;
  for (int g = 0; g < d.N; ++g) h->h_state_index[g] = r.cell_state[g];
  d.pitch = d.W; d.NL = d.N; d.ts = r.ts;
  d.NR = r.NR; d.RS = r.RS; d.Ws = r.Ws; d.n_ring = r.n_ring; d.n_ring_f64 = (double)r.n_ring;
  d.T = r.T; d.state_doubles = r.state_doubles; d.AS = r.AS; d.ZRS = r.ZRS ? r.ZRS : (r.RS | 1);
  for (int w = 0; w < 2; ++w) { d.l0[w] = r.l0[w]; d.rowbase[w] = r.rowbase[w]; d.nch[w] = r.nch[w]; }
  for (int w = 0; w < 4; ++w) d.lw[w] = r.lw[w];
  d.lag = r.lag; d.nslots = r.nslots; d.nsteps = r.steps;
  d.lds_reg_bytes = r.lds_bytes; d.wg_per_cu = r.wg_per_cu;
  d.r_seam = r.r_seam; d.r_A = r.r_A; d.r_xchg = r.r_xchg;
  if (h->kernel == SB_KERNEL_ROLL) { d.r_cmap = r.r_cmap; d.lds_wave_doubles = r.wave_doubles; }
  d.pred_haste = k.pred_haste; d.pred_slack = k.pred_slack; // measured (tools/bench_two_rows.py); developer knobs: speed only, never the result
  // measure-free rolling periods (step_two_impl.h, Hist): only when max|delta| provably never grows from one sweep to
  // the next -- every neighbour coefficient >= 0 and every class's four summing to <= 1 (then ||(I - L)^-1 U||_inf <= 1)
  if (h->kernel == SB_KERNEL_TWO_ROWS && !k.two_no_skip) {
    bool mono = true;
    for (int c = 0; c < plan->n_classes; ++c) {
      double sum = 0.0;
      for (int j = 0; j < 4; ++j) { mono = mono && plan->class_coef[c * 8 + j] >= 0.0; sum += plan->class_coef[c * 8 + j]; }
      mono = mono && sum <= 1.0;
    }
    d.two_skip = mono ? 1 : 0;
  }
  d.skip_kappa = k.skip_kappa; // speed only
  d.pred_first = h->kernel == SB_KERNEL_BAND ? 2 : 3; // step_two.hip: periods a first block rolls unseen (+ 1); step_band.hip: its first block aims at the previous step's count - (pred_first - 2) (measured: 2 beats 3 and 4 by 2-4 %; 1: it never rolls unseen)
  if (k.pred_first) d.pred_first = k.pred_first;
  SB_CHECK(upload(h->zone_cells_l, plan->zone_cells, (size_t)plan->zone_off[plan->Z]));
  SB_CHECK(upload(h->cmapS, r.cmapS.data(), r.cmapS.size()));
  SB_CHECK(upload(h->amapS, r.amapS.data(), r.amapS.size()));
  SB_CHECK(upload(h->zmapS, r.zmapS.data(), r.zmapS.size()));
  SB_CHECK(upload(h->cell_state, r.cell_state.data(), r.cell_state.size()));
  SB_CHECK(alloc_zero(h->ring, (size_t)d.B * std::max(r.n_ring, 1)));
  SB_CHECK(upload(h->tcls, r.tcls.data(), r.tcls.size()));
  SB_CHECK(upload(h->tcset, r.tcset.data(), r.tcset.size()));
  SB_CHECK(upload(h->csetab, r.csetab.data(), r.csetab.size()));
  SB_CHECK(upload(h->tmul, r.tmul.data(), r.tmul.size()));
  d.tmulS = h->tmul.p; d.tmul_doubles = (int)r.tmul.size();
  d.tcset = h->tcset.p; d.csetab = h->csetab.p; d.ncset = (int)r.csetab.size() / 4;
  d.csetab_doubles = (int)r.csetab.size();
  d.two_sym = r.two_sym; d.two_level = r.two_level; d.tail_set_base = r.tail_set_base;
  d.tail_pad_set = h->kernel == SB_KERNEL_TWO_ROWS ? r.tail_pad_set : (d.ncset - 1) * 32;
  if (!r.zs_off.empty()) {
    SB_CHECK(upload(h->zs_off, r.zs_off.data(), r.zs_off.size()));
    d.zs_off = h->zs_off.p;
  }
  SB_CHECK(alloc_zero(h->temp, (size_t)d.B * d.state_doubles));
  if (h->kernel == SB_KERNEL_STREAM) {
    SB_CHECK(alloc_zero(h->abuf, (size_t)h->info.workgroups * d.state_doubles)); // A = ap*Tprev + g, one grid per resident workgroup
    if (h->stream_variant != kStreamPlain) SB_CHECK(alloc_zero(h->ebuf, (size_t)h->info.workgroups * d.state_doubles)); // the pass's other grid
  }
  if (h->kernel == SB_KERNEL_TWO_ROWS) { // step_two.hip: the slots of A that stream from L2, one strip per resident workgroup
    SB_CHECK(alloc_zero(h->abuf, (size_t)h->info.workgroups * (size_t)std::max(1, d.NR - sweep_two_lds_slots(d.NR, d.two_level)) * 128));
    d.two_abuf = h->abuf.p;
  }
  if (h->kernel == SB_KERNEL_ROLL) { // step_roll.hip: the list of buildings the fast kernel leaves to the exact one
    SB_CHECK(alloc_zero(h->redo_ctr, 2));
    SB_CHECK(alloc_zero(h->redo_list, (size_t)d.B));
    SB_CHECK(alloc_zero(h->redo_scratch, (size_t)h->info.workgroups * h->info.waves_per_workgroup * d.state_doubles));
    d.redo_ctr = h->redo_ctr.p; d.redo_list = h->redo_list.p; d.redo_scratch = h->redo_scratch.p;
    d.roll_exact = k.roll_exact; d.dbg_redo_mod = k.force_redo; d.roll_free = k.roll_free;
  }
  d.tcls = h->tcls.p;
  d.cmapS = h->cmapS.p; d.amapS = h->amapS.p; d.zmapS = h->zmapS.p; d.cell_state = h->cell_state.p;
  d.ring = h->ring.p;
  return SB_OK;
}

// The LDS-grid kernel (LdsPlan): launch geometry, the padded class grid, zone-sum blocks, the fast sweep's schedule.
int setup_lds(sb_handle *h, const sb_plan_desc *plan, const LdsPlan &q, const Knobs &k) {
  Dev &d = h->d;
  for (int g = 0; g < d.N; ++g) h->h_state_index[g] = kPad + g;
  d.pitch = q.pitch; d.NL = q.NL; d.S = q.S; d.S_magic = q.S_magic; d.nsteps = q.nsteps;
  d.nbands = q.nbands; d.fast = q.fast; d.ts = q.ts;
  if (k.force_generic) d.fast = 0;
  d.off_agtab = q.off_agtab; d.off_zscr = q.off_zscr; d.off_zmode = q.off_zmode; d.off_wtab = q.off_wtab;
  d.lds_wave_doubles = q.lds_wave_doubles;
  std::vector<int> zl((size_t)plan->zone_off[plan->Z]);
  for (size_t i = 0; i < zl.size(); ++i) {
    const int g = plan->zone_cells[i];
    zl[i] = (g / d.W) * d.pitch + g % d.W;
  }
  {
    std::vector<uint8_t> padded((size_t)d.N + 2 * kPad + 8, 0);
    std::memcpy(padded.data() + kPad, plan->cell_class, (size_t)d.N);
    SB_CHECK(upload(h->cls, padded.data(), padded.size()));
  }
  SB_CHECK(upload(h->zone_cells_l, zl.data(), zl.size()));
  { // zone-sum blocks: u16 LDS indices, zones padded to 512 with NL (zero guard cell)
    std::vector<uint16_t> idx;
    std::vector<int> bz;
    for (int z = 0; z < d.Z; ++z) {
      const int c0 = plan->zone_off[z], c1 = plan->zone_off[z + 1];
      std::vector<uint16_t> cells;
      for (int i = c0; i < c1; ++i) cells.push_back((uint16_t)zl[i]);
      while (cells.size() % 512) cells.push_back((uint16_t)d.NL);
      // within a block, element t of lane l is cell t*64+l: one gather instruction touches
      // 64 consecutive cells of the (sorted) zone list -> consecutive LDS addresses, no
      // bank conflicts
      for (size_t b0 = 0; b0 < cells.size(); b0 += 512) {
        for (int l = 0; l < 64; ++l)
          for (int t = 0; t < 8; ++t) idx.push_back(cells[b0 + (size_t)t * 64 + l]);
        bz.push_back(z);
      }
    }
    if (idx.empty()) { idx.assign(512, (uint16_t)d.NL); bz.push_back(0); }
    d.n_zblocks = (int)bz.size();
    SB_CHECK(upload(h->zl16, (const uint4 *)idx.data(), idx.size() / 8));
    SB_CHECK(upload(h->zblk_zone, bz.data(), bz.size()));
  }
  { // fast-sweep schedule (see stage_g): where every lane is during every 8-step chunk
    const int nch = (d.nsteps + kChunk - 1) / kChunk;
    const int nct = ((nch + 1) & ~1) + 6; // the pipeline prefetches up to 5 chunks past the end
    std::vector<int4> sc((size_t)nct * 64);
    std::vector<unsigned long long> mk((size_t)nct * kChunk, 0ull);
    for (int ch = 0; ch < nct; ++ch)
      for (int lane = 0; lane < 64; ++lane) {
        const int v0 = ch * kChunk - lane, vl = v0 + kChunk - 1;
        const int band = vl >= 0 ? vl / d.S : 0;
        const int y0 = v0 - band * d.S;
        const int rr = band * 64 + lane;
        const bool row_ok = vl >= 0 && rr < d.H;
        const int ra = std::min(rr, d.H - 1);
        const int y0a = std::min(std::max(vl >= 0 ? y0 : v0, -kChunk), d.W);
        int4 e;
        e.x = ra * d.pitch + y0a;
        e.y = ra * d.W + y0a;
        e.z = std::min(ra + 1, d.H - 1) * d.pitch + y0a;
        e.w = std::max(ra - 1, 0) * d.pitch + y0a;
        sc[(size_t)ch * 64 + lane] = e;
        for (int k = 0; k < kChunk; ++k)
          if (row_ok && y0 + k >= 0 && y0 + k < d.W) mk[(size_t)ch * kChunk + k] |= 1ull << lane;
      }
    SB_CHECK(upload(h->sched, sc.data(), sc.size()));
    SB_CHECK(upload(h->smask, mk.data(), mk.size()));
  }
  SB_CHECK(alloc_zero(h->temp, (size_t)d.B * d.Np));
  d.cls = h->cls.p; d.zl16 = h->zl16.p; d.zblk_zone = h->zblk_zone.p; d.sched = h->sched.p;
  d.smask = h->smask.p;
  return SB_OK;
}

// The action table, the observation layout and the optional histogram reducer's tables on the device.
int setup_obs_tables(sb_handle *h, const sb_params *params, const sb_obs_layout *obs, const ActionTable &acts) {
  Dev &d = h->d;
  SB_CHECK(upload(h->act_kind, params->act_kind, (size_t)params->n_actions));
  SB_CHECK(upload(h->act_zone, params->act_zone, (size_t)params->n_actions));
  SB_CHECK(upload(h->act_lo, params->act_lo, (size_t)params->n_actions));
  SB_CHECK(upload(h->act_hi, params->act_hi, (size_t)params->n_actions));
  SB_CHECK(upload(h->zone_act, acts.zone_act.data(), acts.zone_act.size()));
  d.act_kind = h->act_kind.p; d.act_zone = h->act_zone.p; d.act_lo = h->act_lo.p; d.act_hi = h->act_hi.p;
  d.zone_act = h->zone_act.p; d.n_damper_actions = acts.n_damper_actions;
  SB_CHECK(upload(h->col_zone, obs->col_zone, (size_t)d.Z));
  const size_t n_norm = (size_t)std::max(obs->n_obs, obs->n_src);
  SB_CHECK(upload(h->obs_mean, obs->mean, n_norm));
  SB_CHECK(upload(h->obs_sigma, obs->sigma, n_norm));
  d.O = obs->n_obs; d.col_ahu = obs->col_ahu; d.col_blr = obs->col_boiler; d.col_aux = obs->col_aux;
  d.col_zone = h->col_zone.p; d.obs_mean = h->obs_mean.p; d.obs_sigma = h->obs_sigma.p;
  d.n_src = obs->n_src; d.n_hist = obs->n_src ? obs->n_hist : 0; d.hist_normalize = obs->hist_normalize;
  if (obs->n_src) { // optional HistogramReducer (layout checked by check_create_args)
    SB_CHECK(upload(h->src_dest, obs->src_dest, (size_t)obs->n_src));
    SB_CHECK(upload(h->hist_col, obs->hist_col, (size_t)obs->n_hist));
    SB_CHECK(upload(h->hist_off, obs->hist_off, (size_t)obs->n_hist + 1));
    SB_CHECK(upload(h->hist_bins, obs->hist_bins, (size_t)(obs->n_hist ? obs->hist_off[obs->n_hist] : 0)));
    d.src_dest = h->src_dest.p; d.hist_col = h->hist_col.p; d.hist_off = h->hist_off.p;
    d.hist_bins = h->hist_bins.p;
  }
  return SB_OK;
}

// What every sweep kernel shares: the class table, the zones, the per-building state and the per-step hand-over.
int setup_state(sb_handle *h, const sb_plan_desc *plan) {
  Dev &d = h->d;
  { // one extra row: the register path's pad class (T' = Tprev: ap = 1, everything else 0)
    std::vector<double> ct((size_t)(d.ncls + 1) * 8, 0.0);
    std::memcpy(ct.data(), plan->class_coef, (size_t)d.ncls * 8 * sizeof(double));
    ct[(size_t)d.ncls * 8 + 4] = 1.0;
    SB_CHECK(upload(h->ctab, ct.data(), ct.size()));
  }
  SB_CHECK(upload(h->czone, plan->class_zone, (size_t)d.ncls));
  SB_CHECK(upload(h->zone_off, plan->zone_off, (size_t)d.Z + 1));
  h->h_zone_off.assign(plan->zone_off, plan->zone_off + d.Z + 1);
  h->h_zone_cells.assign(plan->zone_cells, plan->zone_cells + plan->zone_off[plan->Z]);
  SB_CHECK(alloc_zero(h->zmean, (size_t)d.B * d.Z));
  SB_CHECK(alloc_zero(h->zair, (size_t)d.B * d.Z));
  SB_CHECK(alloc_zero(h->damper, (size_t)d.B * d.Z));
  SB_CHECK(alloc_zero(h->qz, (size_t)d.B * d.Z));
  SB_CHECK(alloc_zero(h->mode, (size_t)d.B * d.Z)); // thermostat.py:66-69: Mode.OFF
  SB_CHECK(alloc_zero(h->scal, (size_t)d.B * kNScal));
  SB_CHECK(alloc_zero(h->bld, (size_t)d.B));
  SB_CHECK(alloc_zero(h->gtabg, (size_t)d.B * d.ts));
  SB_CHECK(alloc_zero(h->zsum, (size_t)d.B * d.Z));
  SB_CHECK(alloc_zero(h->gsum, (size_t)d.B));
  SB_CHECK(alloc_zero(h->nsw, (size_t)d.B));
  SB_CHECK(alloc_zero(h->next_b, 1));
  d.next_b = h->next_b.p;
  // buildings handed out statically before the draw counter: register path = workgroups, LDS-grid path and SB_KERNEL_ROLL = wavefronts
  d.sweep_wgs = (d.reg && h->kernel != SB_KERNEL_ROLL) ? h->info.workgroups : h->info.workgroups * h->info.waves_per_workgroup;
  d.bld = h->bld.p; d.gtabg = h->gtabg.p; d.zsum = h->zsum.p; d.gsum = h->gsum.p; d.nsw = h->nsw.p;
  d.ctab = h->ctab.p; d.czone = h->czone.p; d.zone_off = h->zone_off.p;
  d.zone_cells_l = h->zone_cells_l.p; d.temp = h->temp.p; d.zmean = h->zmean.p;
  d.zair = h->zair.p; d.damper = h->damper.p; d.qz = h->qz.p; d.mode = h->mode.p;
  d.scal = h->scal.p;
  return SB_OK;
}

// Developer aid (SBSIM_PHASE_TIMING): cycle stamps of wave 0's first building; without the buffer there are none.
void setup_debug(sb_handle *h, const Knobs &k) {
  if (!k.phase_timing) return;
  h->d.dbg_timeline = k.debug_timeline ? 1 : 0; // + [2048]: step_band.hip's time line of one building-step (-DSB_PHASE_STAMPS builds)
  if (alloc_zero(h->dbg, 16 + (h->d.dbg_timeline ? 2048 : 0)) == SB_OK) h->d.dbg = h->dbg.p;
}

// The sweep kernel's LDS attribute, then the initial reset -- complete before a caller's own stream touches the state.
int prepare_and_reset(sb_handle *h) {
  const int e = prepare_sweep(h);
  if (e != (int)hipSuccess)
    return fail(SB_ERR_HIP, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") +
                                hipGetErrorString((hipError_t)e));
  SB_CHECK(sb_reset(h, 0.0, nullptr, nullptr)); // on the NULL stream ...
  if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(SB_ERR_HIP, "sb_create: the initial reset failed");
  return SB_OK;
}

// sb_create_jacobi: the plan the shared state sees has the Jacobi classes, with g = diffuser weight * q_zone (gc = 0,
// sc = weight: k_pre's g table then holds the reference's float64 input_q of every class, fma(w, q, 0) = w * q)
int check_jacobi(const sb_plan_desc *plan, const sb_jacobi_desc *jac, std::vector<double> &coef, sb_plan_desc &jp) {
  if (!jac->cell_class || !jac->class_f32 || !jac->class_diffuser || !jac->class_zone)
    return fail(SB_ERR_INVALID, "sb_create_jacobi: null class table");
  if (jac->H != plan->H || jac->W != plan->W) return fail(SB_ERR_INVALID, "sb_create_jacobi: plan and Jacobi tables differ in shape");
  if (jac->n_classes < 1 || jac->n_classes > 255) return fail(SB_ERR_INVALID, "sb_create_jacobi: 1 .. 255 classes");
  for (int c = 0; c < jac->n_classes; ++c)
    if (!(jac->class_f32[c * SB_JACOBI_COEFS + 6] > 0.0f)) return fail(SB_ERR_INVALID, "sb_create_jacobi: a class with den <= 0");
  coef.assign((size_t)jac->n_classes * 8, 0.0);
  for (int c = 0; c < jac->n_classes; ++c) coef[(size_t)c * 8 + 6] = jac->class_diffuser[c];
  jp = *plan;
  jp.n_classes = jac->n_classes; jp.cell_class = jac->cell_class; jp.class_coef = coef.data(); jp.class_zone = jac->class_zone;
  return SB_OK;
}

// sb_create_materials: the structural classes' descriptors against the plan, the plan's own values against the checks
// sb_set_building_materials makes of a row.
int check_struct_desc(const sb_plan_desc *plan, const sb_struct_desc *sd, const sb_params *params) {
  const std::string w = "sb_create_materials: ";
  if (!sd->class_desc || !sd->class_diffuser || !sd->slot_table) return fail(SB_ERR_INVALID, w + "null descriptor table");
  if (sd->n_slots < 1 || sd->n_slots > 255) return fail(SB_ERR_INVALID, w + "n_slots must be in 1 .. 255");
  if (!(sd->dx > 0.0) || !(sd->dx2 > 0.0) || !(sd->zh > 0.0) || !std::isfinite(sd->dx) || !std::isfinite(sd->dx2) ||
      !std::isfinite(sd->zh))
    return fail(SB_ERR_INVALID, w + "dx, dx2 and zh must be positive and finite");
  if (!(sd->h_conv >= 0.0) || !std::isfinite(sd->h_conv)) return fail(SB_ERR_INVALID, w + "h_conv must be finite and >= 0");
  if (!(params->dt > 0.0)) return fail(SB_ERR_INVALID, w + "time_step_sec must be positive");
  for (int i = 0; i < 3 * sd->n_slots; ++i)
    if (!(sd->slot_table[i] > 0.0) || !std::isfinite(sd->slot_table[i]))
      return fail(SB_ERR_INVALID, w + "slot " + std::to_string(i / 3) + ": material values must be positive and finite");
  for (int c = 0; c < plan->n_classes; ++c) {
    const int32_t *e = sd->class_desc + 4 * c;
    if (e[0] < 0 || e[0] >= sd->n_slots || e[1] < 0 || e[1] > 4 || (e[2] & ~15) || (e[3] & ~15))
      return fail(SB_ERR_INVALID, w + "class " + std::to_string(c) + ": bad descriptor");
    if (!(sd->class_diffuser[c] >= 0.0) || !std::isfinite(sd->class_diffuser[c]))
      return fail(SB_ERR_INVALID, w + "class " + std::to_string(c) + ": bad diffuser weight");
  }
  return SB_OK;
}

// sb_create_materials: the descriptors and the buildings' value table on the device, every building's coefficient rows
// from the plan's own values (k_class_coef, runtime.hip).  Sets Dev::ctab_b, which selects k_pre<true> and
// k_sweep_lds<true>.
int setup_materials(sb_handle *h, const sb_plan_desc *plan, const sb_struct_desc *sd) {
  Dev &d = h->d;
  const int M = sd->n_slots, F = 3 * M + 1;
  h->materials = true;
  h->mat_slots = M;
  h->mat_dx = sd->dx; h->mat_dx2 = sd->dx2; h->mat_zh = sd->zh;
  h->mat_default.assign((size_t)F, sd->h_conv); // field kind * M + slot; 3 M: h_conv
  for (int s = 0; s < M; ++s)
    for (int kind = 0; kind < 3; ++kind) h->mat_default[(size_t)kind * M + s] = sd->slot_table[3 * s + kind];
  std::vector<int4> desc((size_t)plan->n_classes);
  for (int c = 0; c < plan->n_classes; ++c)
    desc[c] = make_int4(sd->class_desc[4 * c], sd->class_desc[4 * c + 1], sd->class_desc[4 * c + 2], sd->class_desc[4 * c + 3]);
  SB_CHECK(upload(h->mat_desc, desc.data(), desc.size()));
  SB_CHECK(upload(h->mat_diff, sd->class_diffuser, (size_t)plan->n_classes));
  SB_CHECK(alloc_zero(h->mat_tab, (size_t)F * d.B));
  SB_CHECK(alloc_zero(h->ctab_b, (size_t)d.B * (d.ncls + 1) * 8));
  d.ctab_b = h->ctab_b.p;
  return apply_building_materials(h, std::vector<double>(), nullptr);
}

int materials_too_large(const char *who) {
  return fail(SB_ERR_TOO_LARGE, std::string(who) + ": the floor plan with a coefficient table per wavefront does not fit "
                                                   "one wavefront's share of 160 KiB of LDS (k_sweep_lds)");
}

// sb_create (sd == NULL) and sb_create_materials.
int create_handle(const sb_plan_desc *plan, const sb_struct_desc *sd, const sb_params *params, const sb_obs_layout *obs,
                  int32_t n_buildings, int32_t device, sb_handle **out) {
  const Knobs k;
  if (!plan || !params || !obs || !out) return fail(SB_ERR_INVALID, "sb_create: null argument");
  ActionTable acts;
  SB_CHECK(check_create_args(plan, params, obs, n_buildings, acts));
  if (sd) SB_CHECK(check_struct_desc(plan, sd, params));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(SB_ERR_NO_DEVICE, "sb_create: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(SB_ERR_INVALID, "sb_create: bad device ordinal");
  SB_ON_DEVICE(device);
  hipDeviceProp_t prop;
  SB_HIP(hipGetDeviceProperties(&prop, device));

  RegPlan r; // (kernel = SB_KERNEL_LDS)
  const LdsPlan q = plan_lds(plan, sd != nullptr);
  if (!sd) SB_CHECK(choose_kernel(plan, q, k, r));
  else if (!q.fits) return materials_too_large("sb_create_materials"); // the one kernel that holds coefficient rows per building

  auto h = std::make_unique<sb_handle>(); // (declared after the device guard: an early return frees it on the device)
  h->device = device;
  h->cus = capped_cus(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256, k);
  Dev &d = h->d;
  d.B = n_buildings; d.H = plan->H; d.W = plan->W; d.Z = plan->Z;
  d.N = plan->H * plan->W;
  d.Np = ((d.N + 1) & ~1) + 2 * kPad;
  d.ncls = plan->n_classes;
  d.p = *params;
  d.p.act_kind = d.p.act_zone = nullptr; d.p.act_lo = d.p.act_hi = nullptr; // (host pointers: the device reads Dev::act_*)
  h->kernel = r.kernel; // the selector; the one place the device's copy of it (Dev::reg, P, stream_ms) is written
  h->stream_variant = r.stream_variant;
  d.reg = r.kernel != SB_KERNEL_LDS ? 1 : 0; d.P = r.kernel; d.stream_ms = r.stream_variant;
  fill_launch_info(plan, r, q, obs->n_obs, h->cus, n_buildings, &h->info, params->n_actions);
  h->h_state_index.resize((size_t)d.N);
  SB_CHECK(d.reg ? setup_reg(h.get(), plan, r, k) : setup_lds(h.get(), plan, q, k));
  SB_CHECK(setup_obs_tables(h.get(), params, obs, acts));
  SB_CHECK(setup_state(h.get(), plan));
  if (sd) SB_CHECK(setup_materials(h.get(), plan, sd));
  setup_debug(h.get(), k);
  SB_CHECK(prepare_and_reset(h.get()));
  *out = h.release();
  return SB_OK;
}

} // namespace

extern "C" {

int sb_plan_info(const sb_plan_desc *plan, int32_t n_obs, int32_t n_buildings, sb_launch_info *out) {
  const Knobs k;
  if (!out) return fail(SB_ERR_INVALID, "sb_plan_info: null argument");
  int rc = check_plan(plan);
  if (rc != SB_OK) return rc;
  RegPlan r;
  const LdsPlan q = plan_lds(plan);
  rc = choose_kernel(plan, q, k, r);
  if (rc != SB_OK) return rc;
  fill_launch_info(plan, r, q, n_obs, capped_cus(256, k), std::max(n_buildings, 1), out);
  return SB_OK;
}

int sb_plan_info_materials(const sb_plan_desc *plan, int32_t n_obs, int32_t n_buildings, sb_launch_info *out) {
  const Knobs k;
  if (!out) return fail(SB_ERR_INVALID, "sb_plan_info_materials: null argument");
  const int rc = check_plan(plan);
  if (rc != SB_OK) return rc;
  const RegPlan r; // (kernel = SB_KERNEL_LDS: the one kernel of such a handle)
  const LdsPlan q = plan_lds(plan, true);
  if (!q.fits) return materials_too_large("sb_plan_info_materials");
  fill_launch_info(plan, r, q, n_obs, capped_cus(256, k), std::max(n_buildings, 1), out);
  return SB_OK;
}

int sb_create(const sb_plan_desc *plan, const sb_params *params, const sb_obs_layout *obs,
              int32_t n_buildings, int32_t device, sb_handle **out) {
  return create_handle(plan, nullptr, params, obs, n_buildings, device, out);
}

int sb_create_materials(const sb_plan_desc *plan, const sb_struct_desc *desc, const sb_params *params,
                        const sb_obs_layout *obs, int32_t n_buildings, int32_t device, sb_handle **out) {
  if (!desc) return fail(SB_ERR_INVALID, "sb_create_materials: null argument");
  return create_handle(plan, desc, params, obs, n_buildings, device, out);
}

int sb_create_jacobi(const sb_plan_desc *plan, const sb_jacobi_desc *jac, const sb_params *params,
                     const sb_obs_layout *obs, int32_t n_buildings, int32_t device, sb_handle **out) {
  const Knobs k;
  if (!plan || !jac || !params || !obs || !out) return fail(SB_ERR_INVALID, "sb_create_jacobi: null argument");
  std::vector<double> coef;
  sb_plan_desc jp;
  SB_CHECK(check_jacobi(plan, jac, coef, jp));
  ActionTable acts;
  SB_CHECK(check_create_args(&jp, params, obs, n_buildings, acts));
  const int ncls = jp.n_classes;
  const int path = sweep_jacobi_path(jp.H, jp.W, ncls, k.force_jacobi_global); // 0: k_sweep_jacobi, 2: k_sweep_jacobi_g
  if (path < 0)
    return fail(SB_ERR_TOO_LARGE, "sb_create_jacobi: " + std::to_string((long long)jp.H * jp.W) + " CVs; k_sweep_jacobi_g takes at most " +
                                      std::to_string(sweep_jacobi_g_max_cvs()) + " (k_sweep_jacobi: 20480 CVs in 160 KiB of LDS)");
  const int N = jp.H * jp.W;
  const size_t lds = sweep_jacobi_lds_bytes(jp.H, jp.W, ncls, path);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(SB_ERR_NO_DEVICE, "sb_create_jacobi: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(SB_ERR_INVALID, "sb_create_jacobi: bad device ordinal");
  SB_ON_DEVICE(device);
  hipDeviceProp_t prop;
  SB_HIP(hipGetDeviceProperties(&prop, device));

  auto h = std::make_unique<sb_handle>();
  h->device = device;
  h->cus = capped_cus(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256, k);
  h->kernel = SB_KERNEL_JACOBI;
  Dev &d = h->d;
  d.B = n_buildings; d.H = jp.H; d.W = jp.W; d.Z = jp.Z;
  d.N = N; d.Np = N; d.pitch = d.W; d.NL = N;
  d.ncls = ncls; d.ts = (ncls + 15) & ~15;
  d.p = *params;
  d.p.act_kind = d.p.act_zone = nullptr; d.p.act_lo = d.p.act_hi = nullptr;
  d.reg = 0; d.P = SB_KERNEL_JACOBI;
  { // launch geometry: the workgroups resident at once (the runtime's occupancy for this instantiation: registers, LDS,
    // wavefronts), one building each at a time; more would only start after others retire
    const int threads = sweep_jacobi_threads(N, path);
    const int occ = sweep_jacobi_blocks_per_cu(jp.H, jp.W, ncls, path);
    const int per_cu = std::max(1, occ > 0 ? occ : std::min((int)((size_t)kLdsCap / lds), 32 / (threads / 64)));
    sb_launch_info &li = h->info;
    li.kernel = SB_KERNEL_JACOBI;
    li.path = path;
    li.waves_per_building = li.waves_per_workgroup = threads / 64;
    li.workgroups = std::max(1, std::min(n_buildings, h->cus * per_cu));
    if (path == 2 && k.jacobi_global_wgs > 0) li.workgroups = std::min(li.workgroups, k.jacobi_global_wgs);
    li.lds_bytes_per_workgroup = (int32_t)lds;
    li.sweep_steps = 1; // (no wavefront schedule: every CV of an iteration at once)
    li.algorithmic_bytes_per_env_step = 8ll * N + 24ll * d.Z + 4ll * params->n_actions + 4ll * obs->n_obs + 44;
    li.state_bytes_per_env_step = 8ll * N; // the float32 grid, read once and written once
  }
  h->h_state_index.resize((size_t)N);
  for (int g = 0; g < N; ++g) h->h_state_index[g] = g;
  SB_CHECK(upload(h->zone_cells_l, jp.zone_cells, (size_t)jp.zone_off[jp.Z])); // flat grid indices
  SB_CHECK(setup_obs_tables(h.get(), params, obs, acts));
  SB_CHECK(setup_state(h.get(), &jp));
  std::vector<double> rden((size_t)ncls);
  for (int c = 0; c < ncls; ++c) rden[c] = 1.0 / (double)jac->class_f32[c * SB_JACOBI_COEFS + 6];
  SB_CHECK(upload(h->jcls, jac->cell_class, (size_t)N));
  SB_CHECK(upload(h->jtab, jac->class_f32, (size_t)ncls * SB_JACOBI_COEFS));
  SB_CHECK(upload(h->jrden, rden.data(), rden.size()));
  SB_CHECK(alloc_zero(h->jgrid, (size_t)d.B * N));
  if (path == 2) // k_sweep_jacobi_g: two padded grids and (M*Tprev)/dt per resident workgroup (not zeroed: every slot is written before it is read)
    SB_HIP(hipMalloc((void **)&h->jscratch.p, (size_t)h->info.workgroups * sweep_jacobi_g_scratch_floats(jp.H, jp.W) * sizeof(float)));
  h->jac = JacArgs{h->jgrid.p, h->jcls.p, h->jtab.p, h->jrden.p, ncls, sweep_jacobi_slots(jp.H, jp.W), d.B, nullptr, nullptr,
                   path, sweep_jacobi_threads(N), h->jscratch.p};
  SB_CHECK(prepare_and_reset(h.get()));
  *out = h.release();
  return SB_OK;
}

} // extern "C"
