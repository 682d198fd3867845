// sbsim_hip.hip -- handle creation of the C ABI (include/sbsim_amd.h): sb_create and its variants check their arguments, ask
// the planner (planner.cpp: which sweep kernel owns the floor plan, and that kernel's tables) and put the handle's buffers on
// the device; sb_plan_info* are the planner's answers alone.  The sweep kernels live in the step_*.hip files and share
// sb_device.h; the state kernels and every other entry point live in runtime.hip, the optional input generators (occupancy,
// convection) in generators.hip; sb_host.h holds what the host files share.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (fma only where written).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sb_host.h"
#include "step_two_cfg.h"

#ifndef SB_EXPERIMENTAL
namespace sb { // the default build's answers for step_stream_ms.hip (planner.h, kExperimental)
int launch_sweep_stream_ms(const Dev &, double *, double *, int, hipStream_t) { return (int)hipErrorNotSupported; }
int prepare_sweep_stream_ms(const Dev &, int) { return (int)hipErrorNotSupported; }
} // namespace sb
#endif

using namespace sb;

namespace {

// The handle's developer switches, read with the planner's at the start of every sb_create call:
// the tests change them between calls.
struct Knobs {
  PlanKnobs plan;
  bool force_jacobi_global = env_flag("SBSIM_FORCE_JACOBI_GLOBAL"); // sb_create_jacobi: every plan on k_sweep_jacobi_g
  int jacobi_global_wgs = std::max(0, env_int("SBSIM_DEBUG_JACOBI_GLOBAL_WGS", 0)); // k_sweep_jacobi_g: at most this many workgroups (0: what is resident)
  bool two_no_skip = env_flag("SBSIM_TWO_NO_SKIP");         // k_sweep_two measures max|delta| every period
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
};

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
    SB_CHECK(alloc_zero(h->abuf, (size_t)h->info.workgroups * (size_t)std::max(1, d.NR - two::lds_slots(d.NR, d.two_level)) * 128));
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

// The device prologue of every sb_create*: the ordinal is one of the visible devices; *cus: its CU count (SBSIM_DEBUG_CUS
// caps it).  who: the entry's name in the messages.  The caller then moves to the device (SB_ON_DEVICE).
int device_cus(const char *who, int device, const PlanKnobs &k, int *cus) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(SB_ERR_NO_DEVICE, std::string(who) + ": no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(SB_ERR_INVALID, std::string(who) + ": bad device ordinal");
  SB_ON_DEVICE(device);
  hipDeviceProp_t prop;
  SB_HIP(hipGetDeviceProperties(&prop, device));
  *cus = capped_cus(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256, k);
  return SB_OK;
}

// sb_create (sd == NULL) and sb_create_materials.
int create_handle(const sb_plan_desc *plan, const sb_struct_desc *sd, const sb_params *params, const sb_obs_layout *obs,
                  int32_t n_buildings, int32_t device, sb_handle **out) {
  const Knobs k;
  if (!plan || !params || !obs || !out) return fail(SB_ERR_INVALID, "sb_create: null argument");
  ActionTable acts;
  SB_CHECK(check_create_args(plan, params, obs, n_buildings, acts));
  if (sd) SB_CHECK(check_struct_desc(plan, sd, params));
  int cus = 0;
  SB_CHECK(device_cus("sb_create", device, k.plan, &cus));
  SB_ON_DEVICE(device);

  RegPlan r;
  LdsPlan q;
  SB_CHECK(plan_sweep(plan, sd != nullptr, "sb_create_materials", k.plan, r, q));

  auto h = std::make_unique<sb_handle>(); // (declared after the device guard: an early return frees it on the device)
  h->device = device;
  h->cus = cus;
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

// sb_plan_info (per_building false) / sb_plan_info_materials: the planner's answer for a device of 256 CUs
static int plan_info(const char *who, const sb_plan_desc *plan, bool per_building, int32_t n_obs, int32_t n_buildings,
                     sb_launch_info *out) {
  const PlanKnobs k;
  if (!out) return fail(SB_ERR_INVALID, std::string(who) + ": null argument");
  SB_CHECK(check_plan(plan));
  RegPlan r;
  LdsPlan q;
  SB_CHECK(plan_sweep(plan, per_building, who, k, r, q));
  fill_launch_info(plan, r, q, n_obs, capped_cus(256, k), std::max(n_buildings, 1), out);
  return SB_OK;
}

int sb_plan_info(const sb_plan_desc *plan, int32_t n_obs, int32_t n_buildings, sb_launch_info *out) {
  return plan_info("sb_plan_info", plan, false, n_obs, n_buildings, out);
}

int sb_plan_info_materials(const sb_plan_desc *plan, int32_t n_obs, int32_t n_buildings, sb_launch_info *out) {
  return plan_info("sb_plan_info_materials", plan, true, n_obs, n_buildings, out);
}

int sb_debug_plan_digest(const sb_plan_desc *plan, int32_t per_building_tables, uint64_t *out) {
  const PlanKnobs k;
  if (!out) return fail(SB_ERR_INVALID, "sb_debug_plan_digest: null argument");
  *out = 0;
  SB_CHECK(check_plan(plan));
  RegPlan r;
  LdsPlan q;
  SB_CHECK(plan_sweep(plan, per_building_tables != 0, "sb_plan_info_materials", k, r, q));
  *out = plan_digest(r, q);
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
  int cus = 0;
  SB_CHECK(device_cus("sb_create_jacobi", device, k.plan, &cus));
  SB_ON_DEVICE(device);

  auto h = std::make_unique<sb_handle>();
  h->device = device;
  h->cus = cus;
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
