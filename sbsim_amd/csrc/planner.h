// planner.h -- the launch planner (planner.cpp): which sweep kernel owns a floor plan, and every table and LDS offset that
// kernel trusts without checking.  Pure host arithmetic, no HIP: it is built, digested (sb_debug_plan_digest) and run under
// sanitizers (tools/planner_check.cpp) on a CPU.  The kernels' side of each agreement is in the step_*_cfg.h headers.
#ifndef SBSIM_AMD_PLANNER_H_
#define SBSIM_AMD_PLANNER_H_

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "sb_error.h"

// The experimental sweep kernels (step_stream_ms.hip, step_stream.hip's k_sweep_stream_roll: exact, tested, slower than what
// they were meant to replace) are in the library only when it is built with SBSIM_BUILD_EXPERIMENTAL=1 (-DSB_EXPERIMENTAL,
// sbsim_amd/build.py); the default build never plans them.
#ifdef SB_EXPERIMENTAL
constexpr bool kExperimental = true;
#else
constexpr bool kExperimental = false;
#endif

// SB_KERNEL_STREAM's variants (= Dev::stream_ms): k_sweep_stream; the experimental k_sweep_stream_ms, k_sweep_stream_roll
enum { kStreamPlain = 0, kStreamMs = 1, kStreamRoll = 2 };

namespace sb {

inline bool env_flag(const char *name) {
  const char *e = getenv(name);
  return e && e[0] == '1';
}
inline int env_int(const char *name, int unset) {
  const char *e = getenv(name);
  return e ? atoi(e) : unset;
}
inline double env_double(const char *name, double unset) {
  const char *e = getenv(name);
  return e ? atof(e) : unset;
}

// The planner's developer switches, read at the start of every sb_plan_info / sb_create call: the
// tests change them between calls.
struct PlanKnobs {
  bool force_stream = env_flag("SBSIM_FORCE_STREAM_PATH");  // every plan on k_sweep_stream
  bool force_lds = env_flag("SBSIM_FORCE_LDS_PATH");        // no register kernel: the LDS-grid kernel (else streaming)
  bool band_path = env_flag("SBSIM_BAND_PATH");             // 67..130 rows: k_sweep_band before k_sweep_two
  bool no_two_row = env_flag("SBSIM_NO_TWO_ROW_PATH");      // no k_sweep_two
  bool no_band = env_flag("SBSIM_NO_BAND_PATH");            // no k_sweep_band (unless band_path)
  bool no_two_64 = env_flag("SBSIM_NO_TWO_64");             // k_sweep_two on 76 / 80 slots alone
  bool no_roll_64 = env_flag("SBSIM_NO_ROLL_64");           // k_sweep_roll on 96 slots alone
  bool no_roll_small = env_flag("SBSIM_NO_ROLL_SMALL");     // <= 64 rows stay on k_sweep_reg<NR,1>
  bool two_general = env_flag("SBSIM_TWO_GENERAL");         // k_sweep_two's four-coefficient instantiation
  int two_max_level = std::max(0, env_int("SBSIM_TWO_MAX_LEVEL", 1 << 30)); // k_sweep_two's highest LDS level
  int lds_pad = env_int("SBSIM_DEBUG_LDS_PAD", 0);          // bytes added to a workgroup's LDS request
  bool stream_ms = kExperimental && env_flag("SBSIM_STREAM_MS");     // streaming plans on k_sweep_stream_ms
  bool stream_roll = kExperimental && env_flag("SBSIM_STREAM_ROLL"); // ... on k_sweep_stream_roll
  int debug_cus = std::max(0, env_int("SBSIM_DEBUG_CUS", 0)); // launch geometry as on a device of at most this many CUs (0: the device's own; speed only)
};

// SBSIM_DEBUG_CUS=n: every per-workgroup buffer and every grid of a handle is sized from sb_handle::cus or from
// sb_launch_info::workgroups, so a smaller count makes the persistent kernels' workgroups draw more buildings each.
inline int capped_cus(int cus, const PlanKnobs &k) { return k.debug_cus > 0 ? std::min(cus, k.debug_cus) : cus; }

// The plan of a register or streaming kernel: launch geometry and tables (sbsim_hip.hip, setup_reg copies it to the device).
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

struct LdsPlan { // launch geometry of the LDS-grid kernel
  int pitch, NL, S, nsteps, nbands, fast, ts, off_agtab, off_zscr, off_zmode, off_wtab, lds_wave_doubles;
  unsigned S_magic;
  size_t shared_bytes, wave_bytes;
  bool fits;
};

// Every check of a floor plan's tables (SB_ERR_INVALID with its text), shared by sb_plan_info and sb_create.
int check_plan(const sb_plan_desc *plan);
// The plan of a checked floor plan.  q: the LDS-grid kernel's geometry, always (per_building, sb_create_materials: the
// [5][ts] coefficient table is the wavefront's own, not the workgroup's -- and that kernel is the only choice: `who` names
// the caller in SB_ERR_TOO_LARGE's text).  r: which kernel owns the plan (r.kernel; SB_KERNEL_LDS: q's) and, for a register
// or streaming kernel, its tables.  SB_ERR_TOO_LARGE: no kernel holds the plan.
int plan_sweep(const sb_plan_desc *plan, bool per_building, const char *who, const PlanKnobs &k, RegPlan &r, LdsPlan &q);
void fill_launch_info(const sb_plan_desc *plan, const RegPlan &r, const LdsPlan &q, int n_obs, int cus, int n_buildings,
                      sb_launch_info *out, int n_actions = SB_NUM_ACTIONS);
// sb_debug_plan_digest: 64-bit FNV-1a over everything r and q hand the chosen kernel
uint64_t plan_digest(const RegPlan &r, const LdsPlan &q);

} // namespace sb

#endif // SBSIM_AMD_PLANNER_H_
