// planner.cpp -- the launch planner: which sweep kernel owns a floor plan (choose_kernel) and, one function per kernel,
// the tables and LDS offsets that kernel trusts without checking (plan_roll, plan_reg, plan_two, plan_band, plan_stream,
// plan_lds).  Host arithmetic only -- no HIP header: the kernels' numbers come from the step_*_cfg.h headers, which the
// kernels' translation units include too.
#include "planner.h"

#include <cmath>
#include <cstring>

#include "sb_layout.h"
#include "step_band_cfg.h"
#include "step_lds_cfg.h"
#include "step_reg_cfg.h"
#include "step_roll_cfg.h"
#include "step_stream_cfg.h"
#include "step_stream_ms_cfg.h"
#include "step_two_cfg.h"

namespace sb {
namespace {

constexpr int kLdsGranule = 1280; // LDS is allocated to workgroups in blocks of this many bytes (gfx950)
constexpr int kRegSlots[] = {32, 66, 96};

// Workgroups per CU that LDS allows for a request of `bytes`.
int wgs_by_lds(int bytes) { return kLdsCap / ((bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule); }

// Stride of a class table that holds every class and the pad class: 32 .. 256 entries; 0: more than 255 classes.
int class_table_stride(int ncls) {
  int ts = 32;
  while (ts < ncls + 1) ts *= 2;
  return ts > 256 ? 0 : ts;
}

// wave 1 runs this many 8-step chunks behind wave 0: every seam value crosses at least one
// workgroup barrier between its write and its (2-steps-early) read, in both directions
int seam_lag(int lw0) { return (lw0 + 8) / 8 + 1; }

// The trim box: every cell that is not ambient (T' = T_ambient whatever the neighbours are, simulator.py:256-258), and
// every cell's zone (-1: none).  why: not empty when the register and streaming kernels cannot work inside the box.
struct Trim {
  const sb_plan_desc *plan;
  int x0, x1, y0, y1, Hs, Ws;
  std::vector<int> zone_of;
  std::string why;
  bool inside(int R, int col) const { return R >= 0 && R < Hs && col >= 0 && col < Ws; } // trimmed coordinates
  // the class of a cell of the box; outside it the pad class (n_classes)
  int cell_class(int R, int col) const {
    return inside(R, col) ? (int)plan->cell_class[(x0 + R) * plan->W + (y0 + col)] : plan->n_classes;
  }
  int zone(int R, int col) const { return zone_of[(x0 + R) * plan->W + (y0 + col)]; } // of a cell of the box; -1: none
  // no zone cell in rows first .. Hs - 1?  (The tail scan adds no zone sums.)
  bool zone_free_from(int first) const {
    for (int R = first; R < Hs; ++R)
      for (int col = 0; col < Ws; ++col)
        if (zone(R, col) >= 0) return false;
    return true;
  }
};

Trim trim_box(const sb_plan_desc *plan) {
  const int H = plan->H, W = plan->W, ncls = plan->n_classes;
  auto coef = [&](int c, int j) { return plan->class_coef[c * 8 + j]; };
  auto cls_at = [&](int x, int y) { return (int)plan->cell_class[x * W + y]; };
  Trim t{plan, H, -1, W, -1, 0, 0, std::vector<int>((size_t)H * W, -1), ""};
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

// r.cell_state: where every grid cell lives in the building's state.  The exterior ring (outside the trim box) is numbered
// -(ring index + 1) in raster order; a cell of the box gets index(R, col), trimmed coordinates.
template <class F>
void fill_cell_state(const Trim &t, RegPlan &r, F index) {
  const int H = t.plan->H, W = t.plan->W;
  r.cell_state.assign((size_t)H * W, 0);
  int ring = 0;
  for (int x = 0; x < H; ++x)
    for (int y = 0; y < W; ++y) {
      const int R = x - t.x0, col = y - t.y0;
      r.cell_state[x * W + y] = t.inside(R, col) ? index(R, col) : -(++ring);
    }
}

// r.tcls / r.tcset: class (times cls_scale) and coefficient set (times 8) of the T tail rows' cells, rows first .. of the
// box, NR columns each (the pad class beyond the box); one pad row when there is no tail row.
void fill_tail_tables(const Trim &t, RegPlan &r, int T, int NR, int first, int cls_scale, const std::vector<int> &set_of) {
  const int pad = t.plan->n_classes;
  r.tcls.assign((size_t)std::max(T, 1) * NR, (uint8_t)(cls_scale * pad));
  r.tcset.assign((size_t)std::max(T, 1) * NR, (uint8_t)(8 * set_of[pad]));
  for (int tr = 0; tr < T; ++tr)
    for (int c = 0; c < NR; ++c) {
      r.tcls[(size_t)tr * NR + c] = (uint8_t)(cls_scale * t.cell_class(first + tr, c));
      r.tcset[(size_t)tr * NR + c] = (uint8_t)(8 * set_of[t.cell_class(first + tr, c)]);
    }
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
// inside the exterior ring.
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
bool plan_two(const Trim &t, const PlanKnobs &k, RegPlan &r) {
  const sb_plan_desc *plan = t.plan;
  const int Hs = t.Hs, Ws = t.Ws, Z = plan->Z, ncls = plan->n_classes, N = plan->H * plan->W;
  auto coef = [&](int c, int j) { return plan->class_coef[c * 8 + j]; };
  int NR = 0;
  for (int s : two::kSlotCounts) // the narrowest instantiation that holds the width (SBSIM_NO_TWO_64=1: 76 / 80 alone, the tree before the end of round 4)
    if (!NR && s >= Ws && !(s == 64 && k.no_two_64)) NR = s;
  if (!NR || Hs > 128 + 2) return false;
  const int ts = class_table_stride(ncls);
  if (!ts) return false;
  const int pad = ncls;
  // ---- can every wavefront cell do with two coefficients?  (rows shifted by one: 127 wavefront rows)
  bool sym = NR > Ws && Hs <= 127 + 2 && !k.two_general;
  const int Hw_sym = std::min(Hs, 127);
  for (int R = 0; sym && R < Hw_sym; ++R)
    for (int col = 0; sym && col < Ws; ++col) {
      const int c = t.cell_class(R, col);
      const double bU = coef(c, 0), bD = coef(c, 1), bL = coef(c, 2), bR = coef(c, 3);
      // a missing neighbour reads as zero only outside the grid (pad row / pad column); below the last
      // wavefront row only when no tail row follows
      const bool v_ok = bU == bD || (bU == 0.0 && R == 0) || (bD == 0.0 && R == Hs - 1);
      const bool h_ok = bL == bR || (bL == 0.0 && col == 0) || (bR == 0.0 && col == Ws - 1);
      sym = v_ok && h_ok;
    }
  const int rowoff = sym ? 1 : 0;
  const int Hw = std::min(Hs, 128 - rowoff), T = Hs - Hw, nl = (Hw + rowoff + 1) / 2; // wavefront rows, tail rows, lanes that own rows
  if (!t.zone_free_from(Hw)) return false;
  // ---- coefficient sets.  general: (bU, bD, bL, bR) for every cell.  sym: (bV, bH) for the wavefront's
  // cells [kSets][2], then (bU, bD, bL, bR) for the tail cells [kSets / 2][4]; the pad sets last.
  const int kSets = two::kSets;
  std::vector<int> set_of(ncls + 1, 0), tset_of(ncls + 1, 0);
  std::vector<double> wtab, ttab; // the wavefront's table, the tail cells' table
  std::vector<char> in_wave(ncls + 1, 0), in_tail(ncls + 1, 0);
  for (int R = 0; R < Hs; ++R)
    for (int col = 0; col < Ws; ++col) (R < Hw ? in_wave : in_tail)[t.cell_class(R, col)] = 1;
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
        if (reg_cell(lane, J, R, col) && t.zone(R, col) >= 0) seen[(size_t)t.zone(R, col) * 64 + lane] = 1;
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
    AS = two::a_stride_of(two::lds_slots(NR, level));
    int off = 4 * kSets + ((2 * (ncls + 1) + 7) & ~7);
    r_seam = off; off += two::tail_row(NR);
    r_A = off; off += std::max((nl < 64 ? nl + 1 : 64) * AS, zs_slots);
    return off * 8;
  };
  auto per_cu = [&](int bytes) { return std::min(4, wgs_by_lds(bytes)); };
  int AS = 0, r_seam = 0, r_A = 0, bytes = 0, level = 0;
  int max_level = sym ? two::kLevels - 1 : 0;
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

  r.NR = NR; r.kernel = SB_KERNEL_TWO_ROWS; r.RS = 64; r.Ws = Ws; r.r0 = t.x0; r.c0 = t.y0; r.n_ring = N - Hs * Ws;
  r.T = T; r.ts = ts;
  r.state_doubles = NE * 64 + T * NR;
  r.lw[0] = nl; r.l0[0] = 0; r.rowbase[0] = 0; r.nch[0] = 0;
  r.lag = 0; r.nslots = 0;
  r.steps = NR + nl - 1 + 4 * T;
  const int NW = NR / 4, NWD = (NE + 3) / 4; // step_two.hip: class words of four steps, NR / 4 per lane
  r.cmapS.assign((size_t)NW * 64, 0);
  r.amapS.assign((size_t)NWD * 64, 0);
  r.zmapS.assign((size_t)NWD * 64, 0);
  fill_tail_tables(t, r, T, NR, Hw, 1, tset_of);
  for (int lane = 0; lane < 64; ++lane) {
    auto row_class = [&](int k, int col) { // upper / lower cell of the lane at a column of the wavefront rows
      const int R = row_of(lane, k);
      return (R >= 0 && R < Hw && col >= 0 && col < NR) ? t.cell_class(R, col) : pad;
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
        aword |= (unsigned long long)((cell ? t.cell_class(R, col) : pad) * 16) << (16 * k);
        int z = Z; // the dump zone
        if (cell && t.zone(R, col) >= 0) z = t.zone(R, col);
        zword |= (unsigned long long)zslot(z, lane) << (16 * k);
      }
      r.amapS[(size_t)g * 64 + lane] = aword;
      r.zmapS[(size_t)g * 64 + lane] = zword;
    }
  }
  fill_cell_state(t, r, [&](int R, int col) {
    if (R >= Hw) return NE * 64 + (R - Hw) * NR + col;
    const int lane = (R + rowoff) >> 1;
    return (2 * ((col + lane) % NR) + ((R + rowoff) & 1)) * 64 + lane;
  });
  r.ok = true;
  return true;
}

// k_sweep_band (step_band.hip): two to four wavefronts per building, one row per lane (rows 64 w .. 64 w + 63) + at
// most two tail rows, up to 96 columns inside the exterior ring; sweeps overlapped in predicted blocks.
bool plan_band(const Trim &t, const PlanKnobs &k, RegPlan &r) {
  const sb_plan_desc *plan = t.plan;
  const int Hs = t.Hs, Ws = t.Ws, Z = plan->Z, ncls = plan->n_classes, N = plan->H * plan->W;
  int NR = 0;
  for (int s : band::kSlotCounts) // the narrowest instantiation that holds the width: a period is NR steps
    if (!NR && s >= Ws) NR = s;
  if (!NR || Hs <= 64) return false;
  // wavefronts: the fewest whose rows + two tail rows hold the plan; a zone cell in a tail row needs one more
  int NWV = 0, T = 0;
  for (int w = 2; w <= band::kWMax && !NWV; ++w) {
    if (Hs > 64 * w + 2) continue;
    const int tr = std::max(0, Hs - 64 * w);
    if (t.zone_free_from(Hs - tr)) { NWV = w; T = tr; }
  }
  if (!NWV) return false;
  const int Hw = Hs - T, RS = 64 * NWV;
  const int ts = class_table_stride(ncls);
  if (!ts) return false;
  const int pad = ncls;
  r.csetab.clear();
  const std::vector<int> set_of = coefficient_sets(plan, r.csetab);
  if ((int)r.csetab.size() / 4 > band::kSets) { r.csetab.clear(); return false; }
  auto zone_at = [&](int R, int col) { // the zone of a wavefront-row cell; Z: none (the dump zone)
    if (R >= Hw || col >= Ws) return Z;
    const int z = t.zone(R, col);
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

  const int AS = band::lds_slots(NR);
  int off = 4 * band::kSets + 2 * ts;
  r.r_seam = off; off += band::seam_doubles(NR, NWV);
  r.r_xchg = off; off += band::sync_doubles(NWV);
  off = (off + 1) & ~1;
  r.r_A = off; off += std::max(RS * AS, zs_slots); // the zone-sum scratch aliases A
  r.AS = AS;
  r.lds_bytes = off * 8;
  r.lds_bytes += k.lds_pad;
  r.wg_per_cu = std::min(4 / NWV, wgs_by_lds(r.lds_bytes)); // one wavefront per SIMD
  if (r.wg_per_cu < 1) { r.csetab.clear(); r.zs_off.clear(); return false; }

  r.NR = NR; r.kernel = SB_KERNEL_BAND; r.RS = RS; r.Ws = Ws; r.r0 = t.x0; r.c0 = t.y0; r.n_ring = N - Hs * Ws;
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
  fill_tail_tables(t, r, T, NR, Hw, 1, set_of);
  for (int w = 0; w < NWV; ++w)
    for (int lane = 0; lane < 64; ++lane) {
      const int R = 64 * w + lane;
      const bool valid = R < Hw;
      for (int st = 0; st < NW; ++st) { // one word per step: the set offset of the lane's cell
        int col = st - lane;
        if (col >= NR) col -= NR; // rolling periods: the lane is in its next sweep
        const int c = (valid && col >= 0) ? t.cell_class(R, col) : pad;
        cw[((size_t)w * NW + st) * 64 + lane] = (uint32_t)(set_of[c] * 32);
      }
      for (int g = 0; g < NWD; ++g) {
        unsigned long long aword = 0, zword = 0;
        for (int k = 0; k < 4; ++k) {
          const int j = 4 * g + k, col = ((j - lane) % NR + NR) % NR;
          const bool cell = valid && col < Ws;
          aword |= (unsigned long long)((cell ? t.cell_class(R, col) : pad) * 16) << (16 * k);
          zword |= (unsigned long long)zslot(cell ? zone_at(R, col) : Z, R) << (16 * k);
        }
        r.amapS[((size_t)w * NWD + g) * 64 + lane] = aword;
        r.zmapS[((size_t)w * NWD + g) * 64 + lane] = zword;
      }
    }
  r.cmapS.assign((cw.size() + 1) / 2, 0);
  std::memcpy(r.cmapS.data(), cw.data(), cw.size() * sizeof(uint32_t));
  fill_cell_state(t, r, [&](int R, int col) {
    if (R >= Hw) return NR * RS + (R - Hw) * NR + col;
    const int slot = (col + (R & 63)) % NR;
    return (slot / 2) * 2 * RS + R * 2 + (slot & 1); // state layout [NR / 2][64 W][2]
  });
  r.ok = true;
  return true;
}

// k_sweep_stream (step_stream.hip): the grid stays in global memory; W = ceil(rows / 64) wavefronts per building
// (W <= 16), any width whose seam rows fit in LDS.  For floor plans no other kernel holds.
bool plan_stream(const Trim &t, const PlanKnobs &k, RegPlan &r, std::string &why) {
  const sb_plan_desc *plan = t.plan;
  const int Z = plan->Z, ncls = plan->n_classes, N = plan->H * plan->W;
  if (!t.why.empty()) { why = t.why; return false; }
  const int Hs = t.Hs, Ws = t.Ws;
  const int NWV = (Hs + 63) / 64;
  if (NWV > 16) { why = "more than 1,024 rows inside the building (try the other orientation)"; return false; }
  const int NS = std::max(72, (Ws + 1) & ~1), RS = 64 * NWV;
  const int ts = class_table_stride(ncls);
  if (!ts) { why = "more than 255 cell classes"; return false; }
  const int pad = ncls;
  r.csetab.clear();
  const std::vector<int> set_of = coefficient_sets(plan, r.csetab);
  if ((int)r.csetab.size() / 4 > stream::kSets) { why = "more than 31 distinct coefficient sets"; r.csetab.clear(); return false; }
  if (Z > 65534) { why = "too many zones"; r.csetab.clear(); return false; }
  const int ZC = stream::kZC;
  int off = 4 * stream::kSets + 2 * ts;
  // step_stream_ms.hip (several sweeps per pass over the grid: a seam row per sweep) -- OPT-IN, SBSIM_STREAM_MS=1: correct
  // (bit-identical iterates, tests/test_gpu_parity.py) but not faster yet (LABNOTES.md 5.4c: 256 registers leave two
  // wavefronts per SIMD, and a step of four sweep slots takes 3.3x a step of step_stream.hip's one).  Needs its LDS to fit
  // and the last wavefront to own the spare rows its bands need (the band of sweep j sits j rows further up).
  {
    const int ms_off = off + stream_ms::seam_doubles(NS, NWV) + stream_ms::xchg_doubles(NWV) + (Z + 1) * ZC;
    if (k.stream_ms && ms_off * 8 <= kLdsCap && 64 * NWV - Hs >= stream_ms::kS - 1 &&
        NWV <= 8) r.stream_variant = kStreamMs; // (its 256 registers: two wavefronts per SIMD, workgroups of at most 8)
  }
  r.r_seam = off; off += r.stream_variant == kStreamMs ? stream_ms::seam_doubles(NS, NWV) : 2 * NWV * (NS + 8);
  // overlapped sweeps (step_stream.hip's k_sweep_stream_roll, round 5) -- OPT-IN, SBSIM_STREAM_ROLL=1: kStreamRoll.  Exact
  // (tests/test_gpu_parity.py), 9 % faster on R9 forced here, 9 % SLOWER on the 299 x 401 plan it was written for: with three
  // workgroups per CU another workgroup already fills a wavefront's idle steps, and the sweep started in vain is traffic
  if (r.stream_variant == kStreamPlain && k.stream_roll) r.stream_variant = kStreamRoll;
  r.r_xchg = off; off += r.stream_variant == kStreamMs ? stream_ms::xchg_doubles(NWV) : 32 + 64 * NWV + (r.stream_variant == kStreamRoll ? stream::kRollXchgExtra : 0); // progress, max|delta| parts, the publish scratch
  r.r_A = off; off += (Z + 1) * ZC;
  r.lds_bytes = off * 8;
  if (r.lds_bytes > kLdsCap) { why = "the seam rows (rows / 64 x columns x 16 bytes) and the zone sums do not fit in 160 KiB of LDS"; r.csetab.clear(); return false; }
  // workgroups per CU: LDS, threads (2,048 per CU) and registers (<= 128 per lane: four wavefronts per SIMD)
  r.wg_per_cu = std::max(1, std::min({wgs_by_lds(r.lds_bytes), 32 / NWV, (r.stream_variant == kStreamMs ? 8 : 16) / NWV}));
  r.NR = NS; r.kernel = SB_KERNEL_STREAM; r.RS = RS; r.Ws = Ws; r.r0 = t.x0; r.c0 = t.y0; r.n_ring = N - Hs * Ws;
  r.T = 0; r.ts = ts; r.AS = 0;
  r.state_doubles = NS * RS;
  r.lw[0] = std::min(Hs, 64); r.lw[1] = NWV; // lw[1]: wavefronts per building
  r.steps = 64 * (NWV - 1) + NS + 63;
  const int NW = NS + 63;
  std::vector<uint32_t> cw((size_t)NWV * NW * 64, 0);
  std::vector<uint16_t> zm((size_t)NWV * NS * 64, (uint16_t)Z);
  for (int w = 0; w < NWV; ++w)
    for (int lane = 0; lane < 64; ++lane) {
      const int R = 64 * w + lane;
      for (int st = 0; st < NW; ++st) {
        const int col = st - lane;
        const int c = (R < Hs && col >= 0 && col < NS) ? t.cell_class(R, col) : pad;
        cw[((size_t)w * NW + st) * 64 + lane] = (uint32_t)(set_of[c] * 32) | ((uint32_t)(c * 16) << 16);
      }
      for (int s = 0; s < NS; ++s) {
        const int col = ((s - lane) % NS + NS) % NS;
        if (R < Hs && col < Ws && t.zone(R, col) >= 0) zm[((size_t)w * NS + s) * 64 + lane] = (uint16_t)t.zone(R, col);
      }
    }
  r.cmapS.assign((cw.size() + 1) / 2, 0);
  std::memcpy(r.cmapS.data(), cw.data(), cw.size() * sizeof(uint32_t));
  r.zmapS.assign((zm.size() + 3) / 4, 0);
  std::memcpy(r.zmapS.data(), zm.data(), zm.size() * sizeof(uint16_t));
  r.amapS.assign(1, 0);
  r.tcls.assign(1, (uint8_t)0);
  r.tcset.assign(1, (uint8_t)0);
  fill_cell_state(t, r, [&](int R, int col) { return ((col + (R & 63)) % NS) * RS + R; }); // state layout [NS][RS]
  r.ok = true;
  return true;
}

// k_sweep_roll (step_roll.hip): one wavefront, one row per lane (the lanes beyond a plan of fewer than 64 rows own pad
// rows) + at most two tail rows finished by a scan, NR slots; sweeps overlapped, a period is NR steps.
void plan_roll(const Trim &t, int NR, const PlanKnobs &k, RegPlan &r) {
  const sb_plan_desc *plan = t.plan;
  const int Hs = t.Hs, Ws = t.Ws, Z = plan->Z, ncls = plan->n_classes, N = plan->H * plan->W;
  auto coef = [&](int c, int j) { return plan->class_coef[c * 8 + j]; };
  const int TS = 32, RS = 64, nl_slots = roll::lds_slots(NR); // slots of A in LDS (the kernel keeps the rest in registers)
  r.ts = TS;
  // the zone-sum scratch aliases A: [64 rows][ZRS = (Z + 1) | 1], a slot's offset inside its lane's row is zone * 8:
  // one byte (Z <= 31: every zone has a cell class of its own and the class table holds 32)
  const int ZRS = (Z + 1) | 1;
  if (Z > 31 || ZRS > nl_slots) { r.why = "too many zones for the zone-sum scratch"; return; }
  r.ZRS = ZRS;
  r.NR = NR; r.kernel = SB_KERNEL_ROLL; r.RS = RS; r.Ws = Ws; r.r0 = t.x0; r.c0 = t.y0; r.n_ring = N - Hs * Ws;
  r.T = std::max(0, Hs - 64);
  r.state_doubles = NR * RS + r.T * NR;
  r.lw[0] = 64; r.l0[0] = 0; r.rowbase[0] = 0;
  r.nch[0] = (NR + 63 + 7) / 8;
  r.lag = 0; r.nslots = r.nch[0];
  r.steps = NR + 4 * r.T; // overlapped sweeps: NR steps per sweep; a tail row's scan costs about 4 wavefront steps
  // LDS (doubles): [coefficient sets | class words] shared, then per wavefront [ap g | first tail row | A]
  r.AS = roll::a_stride(NR); // 2 mod 4 doubles: 16-byte aligned rows, conflict-free ds_read_b128
  r.waves_per_wg = roll::kWaves;
  r.r_cmap = 4 * TS;
  r.r_seam = 2 * TS;
  r.r_A = r.r_seam + ((roll::tail_row(NR) + 1) & ~1); // 16-byte aligned rows
  r.wave_doubles = r.r_A + RS * nl_slots; // rows of AS slots, then [RS][nl_slots - AS]
  r.lds_bytes = (r.r_cmap + (NR / 8) * 64 + roll::tail_mul_doubles(NR, r.T) + r.waves_per_wg * r.wave_doubles) * 8;
  r.lds_bytes += k.lds_pad;
  r.wg_per_cu = r.lds_bytes <= kLdsCap ? 1 : 0;
  if (r.wg_per_cu < 1) { r.why = "one building does not fit in LDS"; return; }

  const int pad = ncls;
  // the sweep looks its four neighbour coefficients up by coefficient SET (classes that differ only in ap / g share
  // one): fewer distinct LDS addresses per wavefront read
  const std::vector<int> set_of = coefficient_sets(plan, r.csetab);
  if (r.csetab.size() / 4 > 32) { r.why = "more than 32 distinct coefficient sets"; r.ok = false; return; }
  const int aslots = (NR + 7) / 8, zslots = NR / 8;
  r.cmapS.assign((size_t)(NR / 8) * 64, 0);
  r.amapS.assign((size_t)aslots * 64, 0);
  r.zmapS.assign((size_t)zslots * 64, 0);
  fill_tail_tables(t, r, r.T, NR, 64, 8, set_of);
  if (r.T > 0) {
    // The tail scan (sweep_common.h): along a tail row x_c = bL_c x_{c-1} + q_c; lane l >= L0 composes its two
    // columns, six DPP levels scan the lanes.  The multiplicative half of every level does not depend on the
    // temperatures: it is run here, in affine_scan's own order (bit-identical), and the kernel reads what each
    // level multiplies by: `a` entering levels 1..5, 0 where the level has no source lane for the lane.
    const int n = NR / 2, L0 = 64 - n;
    r.tmul.assign((size_t)roll::tail_mul_doubles(NR, r.T), 0.0);
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
    for (int tr = 0; tr < r.T; ++tr) {
      auto bL = [&](int c) { const int cl = t.cell_class(64 + tr, c); return cl == pad ? 0.0 : coef(cl, 2); };
      double a[64], an[64];
      for (int lane = 0; lane < 64; ++lane) a[lane] = lane >= L0 ? bL(2 * (lane - L0) + 1) * bL(2 * (lane - L0)) : 0.0;
      for (int d = 0; d < 6; ++d) {
        for (int lane = 0; lane < 64; ++lane) {
          const int src = src_lane(d, lane), lp = lane - L0;
          const double A = src >= 0 ? a[lane] : 0.0;
          if (lp >= 0 && (d == 1 || d == 2)) r.tmul[(size_t)4 * n * tr + 2 * lp + (d - 1)] = A;
          if (lp >= 0 && (d == 3 || d == 4)) r.tmul[(size_t)4 * n * tr + 2 * n + 2 * lp + (d - 3)] = A;
          if (lp >= 0 && d == 5) r.tmul[(size_t)4 * n * r.T + 2 * lp + tr] = A;
          an[lane] = a[lane] * (src >= 0 ? a[src] : 1.0);
        }
        std::memcpy(a, an, sizeof(a));
      }
    }
  }
  for (int lane = 0; lane < 64; ++lane) { // lane = row; class and zone bytes are byte offsets: class * 8, zone * 8
    // one byte per step = the cell's coefficient set (its LDS byte offset is set * 32), eight steps per word; at step s
    // (of the ramp-up or of any period) the lane works on column (s - lane) mod NR
    for (int ch = 0; ch < NR / 8; ++ch) {
      unsigned long long word = 0;
      for (int k8 = 0; k8 < 8; ++k8) {
        const int col = ((8 * ch + k8 - lane) % NR + NR) % NR;
        word |= (unsigned long long)set_of[t.cell_class(lane, col)] << (8 * k8);
      }
      r.cmapS[(size_t)ch * 64 + lane] = word;
    }
    for (int g = 0; g < aslots; ++g) {
      unsigned long long word = 0;
      for (int k8 = 0; k8 < 8; ++k8) {
        const int j = 8 * g + k8, col = ((j - lane) % NR + NR) % NR;
        word |= (unsigned long long)((j < NR ? t.cell_class(lane, col) : pad) * 8) << (8 * k8);
      }
      r.amapS[(size_t)g * 64 + lane] = word;
    }
    for (int g = 0; g < zslots; ++g) { // a byte per slot: the byte offset inside the lane's row of the scratch
      unsigned long long word = 0;
      for (int k8 = 0; k8 < 8; ++k8) {
        const int col = ((8 * g + k8 - lane) % NR + NR) % NR;
        int z = Z; // dump column
        if (t.inside(lane, col) && t.zone(lane, col) >= 0) z = t.zone(lane, col); // (below 64 rows the lanes beyond the plan own pad rows)
        word |= (unsigned long long)(z * 8) << (8 * k8);
      }
      r.zmapS[(size_t)g * 64 + lane] = word;
    }
  }
  fill_cell_state(t, r, [&](int R, int col) {
    if (R >= 64) return NR * 64 + (R - 64) * NR + col;
    const int slot = (col + R) % NR;
    return (slot / 2) * 128 + R * 2 + (slot & 1); // state layout [NR / 2][64][2]
  });
  r.ok = true;
}

// k_sweep_reg (step_reg.hip): no overlap, no tail rows.  SB_KERNEL_REG: one wavefront, <= 64 rows; SB_KERNEL_REG_PAIR:
// two wavefronts split the rows (<= 128), wave 1 a seam lag behind wave 0.
void plan_reg(const Trim &t, sb_sweep_kernel kernel, int NR, const PlanKnobs &k, RegPlan &r) {
  const sb_plan_desc *plan = t.plan;
  const int Hs = t.Hs, Ws = t.Ws, Z = plan->Z, ncls = plan->n_classes, N = plan->H * plan->W;
  const int nw = kernel == SB_KERNEL_REG_PAIR ? 2 : 1; // wavefronts per building = the kernel's mode P
  const int TS = reg::table_stride(NR, kernel), cscale = 256 / TS; // class byte = class * cscale
  const int nl = reg::lds_slots(NR, kernel); // slots of A in LDS (the kernel keeps the rest in registers)
  r.ts = TS;
  const int RS = Hs;
  // the zone-sum scratch aliases A: [Z + 1][ZRS = rows | 1] (odd stride: the zone reduce reads 16 zone rows at once),
  // 16-bit byte offsets
  const int ZRS = RS | 1;
  if ((size_t)(Z + 1) * ZRS > (size_t)RS * nl || (size_t)(Z + 1) * ZRS * 8 > 65535) {
    r.why = "too many zones for the zone-sum scratch";
    return;
  }
  r.ZRS = ZRS;
  r.NR = NR; r.kernel = kernel; r.RS = RS; r.Ws = Ws; r.r0 = t.x0; r.c0 = t.y0; r.n_ring = N - Hs * Ws;
  r.T = 0;
  r.state_doubles = NR * RS;
  const int maxch = (NR + 63 + 7) / 8;
  if (nw == 1) {
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
    int off = 5 * TS + TS;
    r.r_seam = off;
    off += nw == 2 ? 2 * (NR + 2 * reg::kSeamPad) : 0;
    r.r_A = off; off += RS * AS;
    r.r_xchg = off; off += 8;
    r.lds_bytes = off * 8;
    r.lds_bytes += k.lds_pad; // developer knob: fewer buildings per CU
    // workgroups per CU: LDS, and the registers (4 SIMDs x wavefronts per SIMD / wavefronts per building)
    r.wg_per_cu = std::min(4 * reg::waves_per_simd(NR, kernel) / nw, wgs_by_lds(r.lds_bytes));
  };
  layout(nl);
  const int plain = r.wg_per_cu;
  layout(nl | 1);
  if (r.wg_per_cu < plain) layout(nl);
  if (r.wg_per_cu < 1) { r.why = "one building does not fit in LDS"; return; }

  const int pad = ncls;
  const int aslots = (NR + 7) / 8, zslots = (NR + 3) / 4;
  r.cmapS.assign((size_t)nw * (maxch + 3) * 64, 0);
  r.amapS.assign((size_t)nw * aslots * 64, 0);
  r.zmapS.assign((size_t)nw * zslots * 64, 0);
  fill_tail_tables(t, r, 0, NR, Hs, 8, std::vector<int>(ncls + 1, 0)); // (no tail rows: the pad row alone)
  for (int w = 0; w < nw; ++w)
    for (int lane = 0; lane < 64; ++lane) {
      const int lp = lane - r.l0[w];
      const bool valid = lp >= 0 && lp < r.lw[w];
      const int R = r.rowbase[w] + lp;
      for (int ch = 0; ch < maxch + 3; ++ch) {
        unsigned long long word = 0;
        for (int k8 = 0; k8 < 8; ++k8) {
          const int col = 8 * ch + k8 - lp;
          const int c = valid ? t.cell_class(R, col) : pad;
          word |= (unsigned long long)(c * cscale) << (8 * k8); // stride 32: the byte offset into a table column
        }
        r.cmapS[((size_t)w * (maxch + 3) + ch) * 64 + lane] = word;
      }
      for (int g = 0; g < aslots; ++g) {
        unsigned long long word = 0;
        for (int k8 = 0; k8 < 8; ++k8) {
          const int j = 8 * g + k8;
          const int col = ((j - lp) % NR + NR) % NR;
          const int c = (valid && j < NR) ? t.cell_class(R, col) : pad;
          word |= (unsigned long long)(c * cscale) << (8 * k8);
        }
        r.amapS[((size_t)w * aslots + g) * 64 + lane] = word;
      }
      for (int g = 0; g < zslots; ++g) {
        unsigned long long word = 0;
        for (int k4 = 0; k4 < 4; ++k4) {
          const int j = 4 * g + k4;
          const int col = ((j - lp) % NR + NR) % NR;
          int z = Z; // dump row
          if (valid && j < NR && col < Ws && t.zone(R, col) >= 0) z = t.zone(R, col);
          const unsigned offb = (unsigned)((z * ZRS + (valid ? R : 0)) * 8);
          word |= (unsigned long long)offb << (16 * k4);
        }
        r.zmapS[((size_t)w * zslots + g) * 64 + lane] = word;
      }
    }
  fill_cell_state(t, r, [&](int R, int col) {
    const int w = (nw == 2 && R >= r.lw[0]) ? 1 : 0;
    return ((col + R - r.rowbase[w]) % NR) * RS + R; // state layout [NR][RS]
  });
  r.ok = true;
}

// Which register kernel owns the plan, today's rules in today's order.  k_sweep_two and k_sweep_band decide while they
// plan, so they are tried here (r: their plan when one of them took it); for k_sweep_roll and k_sweep_reg the answer is
// the kernel and its slot count.  why: there is none.
struct RegChoice {
  sb_sweep_kernel kernel = SB_KERNEL_LDS; // SB_KERNEL_LDS: none
  int NR = 0;
  std::string why;
};

RegChoice choose_reg_kernel(const Trim &t, int lds_per_cu, const PlanKnobs &k, RegPlan &r) {
  const int Hs = t.Hs, Ws = t.Ws, Z = t.plan->Z, ncls = t.plan->n_classes;
  RegChoice c;
  // k_sweep_band: two wavefronts, one row per lane, sweeps overlapped in blocks (67..130 rows, <= 80 columns).
  // Measured level with k_sweep_two (profiles/r04_band_vs_two_rows.txt): all four SIMDs run, but four
  // wavefronts share the CU's LDS pipe, every block starts with wavefront 1's 64-step lag and the tail
  // scan sits on wavefront 1's critical path.  Kept, tested, behind SBSIM_BAND_PATH=1.
  if (Hs > 64 + 2 && k.band_path && plan_band(t, k, r)) { c.kernel = SB_KERNEL_BAND; return c; }
  // k_sweep_two: one wavefront, two rows per lane (67..130 rows, <= 80 columns)
  if (Hs > 64 + 2 && !k.no_two_row && plan_two(t, k, r)) { c.kernel = SB_KERNEL_TWO_ROWS; return c; }
  // k_sweep_band again, for what k_sweep_two does not hold: beyond 128 rows (up to 258) three or four wavefronts share a
  // building; 67..130 rows with 81..96 columns two (measured 1.2-2.6x the two-wavefront k_sweep_reg / the LDS-grid
  // kernel on 109 x 92, 113 x 93 and 125 x 97: tools/bench_mid_plans.py)
  if (Hs > 64 + 2 && !k.no_band && plan_band(t, k, r)) { c.kernel = SB_KERNEL_BAND; return c; }
  // the narrowest instantiation that holds the width and the class count
  int roll_slots = 0; // SBSIM_NO_ROLL_64=1: the 96-slot instantiation alone (the tree before round 4's last additions)
  for (int s : roll::kSlotCounts)
    if (!roll_slots && s >= Ws && ncls + 1 <= 32 && !(s < 96 && k.no_roll_64)) roll_slots = s;
  auto reg_slots = [&](sb_sweep_kernel kernel) {
    for (int s : kRegSlots)
      if (s >= Ws && reg::supported(s, kernel) && ncls + 1 <= reg::table_stride(s, kernel)) return s;
    return 0;
  };
  // SB_KERNEL_REG: one wavefront; SB_KERNEL_ROLL: one wavefront + one or two tail rows finished by a scan
  // (no zone cell may sit in a tail row); SB_KERNEL_REG_PAIR: two wavefronts.
  if (Hs <= 64) { c.kernel = SB_KERNEL_REG; c.NR = reg_slots(SB_KERNEL_REG); }
  // ... but not on k_sweep_reg<NR,1> (round 1's kernel: a sweep of NR + rows - 1 steps, no overlap) when k_sweep_roll's
  // period is no longer than that: the roll kernel without tail rows, the lanes beyond the plan own pad rows
  // (measured, 65,536 buildings: 47 x 98 / 6 zones 6.8 -> 1.9 ms per step, 62 x 97 4.8 -> 2.5, 49 x 50 8.9 -> 7.6;
  // 25 x 38 and 17 x 25 stay: 3.3 against 4.4, 2.6 against 4.9)
  // (only when the roll kernel's own limits hold -- its zone-sum scratch takes <= 31 zones; its LDS layout always fits: checked
  // HERE, before the switch, so that a plan it cannot take stays on k_sweep_reg<NR,1> instead of falling through to the
  // LDS-grid kernel)
  if (c.kernel == SB_KERNEL_REG && c.NR && !k.no_roll_small && roll_slots && Z <= 31 && c.NR + Hs - 1 >= roll_slots) {
    c.kernel = SB_KERNEL_ROLL; c.NR = roll_slots;
  }
  if (c.kernel == SB_KERNEL_LDS && Hs <= 64 + 2 && roll_slots && t.zone_free_from(64)) {
    c.kernel = SB_KERNEL_ROLL; c.NR = roll_slots;
  }
  if (c.kernel == SB_KERNEL_LDS && Hs <= 128) {
    c.kernel = SB_KERNEL_REG_PAIR; c.NR = reg_slots(SB_KERNEL_REG_PAIR);
    // a two-wavefront variant that runs one wavefront per SIMD holds two buildings per CU and
    // pays the seam lag: measured no faster than the LDS-grid kernel at two buildings per CU
    if (c.NR && reg::waves_per_simd(c.NR, SB_KERNEL_REG_PAIR) == 1 && lds_per_cu >= 2) {
      c.why = "the LDS-grid kernel holds as many buildings per CU";
      return c;
    }
  }
  if (c.kernel == SB_KERNEL_LDS) c.why = "more than 128 rows inside the building";
  else if (!c.NR) c.why = "no kernel variant for this width and class count";
  return c;
}

// The register kernels.  lds_per_cu: buildings per CU the LDS-grid kernel would hold (0: the plan does not fit it).
void plan_registers(const Trim &t, int lds_per_cu, const PlanKnobs &k, RegPlan &r) {
  if (!t.why.empty()) { r.why = t.why; return; }
  const RegChoice c = choose_reg_kernel(t, lds_per_cu, k, r);
  if (!c.why.empty()) r.why = c.why;
  else if (c.kernel == SB_KERNEL_ROLL) plan_roll(t, c.NR, k, r);
  else if (c.kernel == SB_KERNEL_REG || c.kernel == SB_KERNEL_REG_PAIR) plan_reg(t, c.kernel, c.NR, k, r);
}

// per_building (sb_create_materials): the [5][ts] coefficient table is the wavefront's own, not the workgroup's
LdsPlan plan_lds(const sb_plan_desc *plan, bool per_building) {
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
  int off = ((q.NL + 1) & ~1) + 2 * lds::kGuard;
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

// Which sweep kernel owns this floor plan (r.kernel): a register kernel (plan_registers), else the LDS-grid kernel, else --
// plans that fit neither -- the streaming kernel.  SBSIM_FORCE_STREAM_PATH=1: the streaming kernel (tests).
int choose_kernel(const sb_plan_desc *plan, const LdsPlan &q, const PlanKnobs &k, RegPlan &r) {
  std::string why;
  const Trim t = trim_box(plan);
  if (k.force_stream) {
    if (!plan_stream(t, k, r, why)) return fail(SB_ERR_TOO_LARGE, "the streaming sweep kernel cannot hold this floor plan: " + why);
    return SB_OK;
  }
  if (!k.force_lds) plan_registers(t, q.fits ? (int)(((size_t)kLdsCap - q.shared_bytes) / q.wave_bytes) : 0, k, r);
  if (r.ok) return SB_OK;
  r = RegPlan(); // (kernel = SB_KERNEL_LDS)
  if (q.fits) return SB_OK;
  if (!plan_stream(t, k, r, why))
    return fail(SB_ERR_TOO_LARGE, "no sweep kernel holds this floor plan (the streaming kernel takes up to 1,024 rows in one "
                                  "orientation and rows / 64 x columns <= ~9,000): " + why);
  return SB_OK;
}

// 64-bit FNV-1a.  Vectors: length, then raw bytes (doubles by bit pattern).
struct Fnv {
  uint64_t h = 14695981039346656037ull;
  void bytes(const void *p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  }
  void i64(long long v) { bytes(&v, sizeof v); }
  template <class V>
  void vec(const V &v) {
    i64((long long)v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(v[0]));
  }
};

} // namespace

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

int plan_sweep(const sb_plan_desc *plan, bool per_building, const char *who, const PlanKnobs &k, RegPlan &r, LdsPlan &q) {
  r = RegPlan(); // (kernel = SB_KERNEL_LDS)
  q = plan_lds(plan, per_building);
  if (!per_building) return choose_kernel(plan, q, k, r);
  if (!q.fits) // the one kernel that holds coefficient rows per building
    return fail(SB_ERR_TOO_LARGE, std::string(who) + ": the floor plan with a coefficient table per wavefront does not fit "
                                                     "one wavefront's share of 160 KiB of LDS (k_sweep_lds)");
  return SB_OK;
}

void fill_launch_info(const sb_plan_desc *plan, const RegPlan &r, const LdsPlan &q, int n_obs, int cus,
                      int n_buildings, sb_launch_info *out, int n_actions) {
  const int64_t N = (int64_t)plan->H * plan->W, Z = plan->Z;
  out->algorithmic_bytes_per_env_step = 8ll * N + 24ll * Z + 4ll * n_actions + 4ll * n_obs + 44;
  const int64_t rest = (8 * 4 + 4 * 2) * Z + 16ll * kNScalOut + 4ll * n_actions + 4ll * n_obs + 4;
  out->kernel = r.kernel;
  if (r.kernel != SB_KERNEL_LDS) { // path 2: step_stream.hip, the grid in global memory (r.lw[1] wavefronts); 1: in registers
    const int waves = r.kernel == SB_KERNEL_STREAM ? r.lw[1] : r.kernel == SB_KERNEL_BAND ? r.RS / 64 : r.kernel == SB_KERNEL_REG_PAIR ? 2 : 1;
    out->path = r.kernel == SB_KERNEL_STREAM ? 2 : 1;
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

// The order of hashing is written here, once; it does not follow the structs' declarations.
uint64_t plan_digest(const RegPlan &r, const LdsPlan &q) {
  Fnv f;
  f.i64(r.kernel); f.i64(r.stream_variant);
  for (long long v : {(long long)r.ok, (long long)r.NR, (long long)r.RS, (long long)r.Ws, (long long)r.r0, (long long)r.c0,
                      (long long)r.n_ring, (long long)r.T, (long long)r.state_doubles, (long long)r.ts,
                      (long long)r.lw[0], (long long)r.lw[1], (long long)r.lw[2], (long long)r.lw[3],
                      (long long)r.l0[0], (long long)r.l0[1], (long long)r.rowbase[0], (long long)r.rowbase[1],
                      (long long)r.nch[0], (long long)r.nch[1], (long long)r.lag, (long long)r.nslots, (long long)r.steps,
                      (long long)r.r_seam, (long long)r.r_A, (long long)r.r_xchg, (long long)r.lds_bytes,
                      (long long)r.wg_per_cu, (long long)r.AS, (long long)r.r_cmap, (long long)r.wave_doubles,
                      (long long)r.waves_per_wg, (long long)r.ZRS, (long long)r.two_sym, (long long)r.two_level,
                      (long long)r.tail_set_base, (long long)r.tail_pad_set})
    f.i64(v);
  f.vec(r.tcls); f.vec(r.tcset); f.vec(r.csetab); f.vec(r.tmul);
  f.vec(r.cmapS); f.vec(r.amapS); f.vec(r.zmapS); f.vec(r.cell_state); f.vec(r.zs_off);
  if (r.kernel == SB_KERNEL_LDS)
    for (long long v : {(long long)q.pitch, (long long)q.NL, (long long)q.S, (long long)q.nsteps, (long long)q.nbands,
                        (long long)q.fast, (long long)q.ts, (long long)q.off_agtab, (long long)q.off_zscr,
                        (long long)q.off_zmode, (long long)q.off_wtab, (long long)q.lds_wave_doubles, (long long)q.S_magic,
                        (long long)q.shared_bytes, (long long)q.wave_bytes, (long long)q.fits})
      f.i64(v);
  return f.h;
}

} // namespace sb
