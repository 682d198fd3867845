// sb_host.h -- what the host-side translation units that use HIP (sbsim_hip.hip: sb_create; runtime.hip: the step
// runtime; generators.hip) share: HIP error reporting, device buffers, the handle behind the C ABI, the sweep-kernel
// dispatch.  (The planner is HIP-free: planner.h, with sb_error.h's fail().)
#ifndef SBSIM_AMD_SB_HOST_H_
#define SBSIM_AMD_SB_HOST_H_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "episode_draw.h"
#include "planner.h"
#include "sb_device.h"

// step_stream.hip's overlapped-sweeps kernel (declared here: sb_device.h is part of the traffic profile's source hash)
namespace sb {
int launch_sweep_stream_roll(const Dev &d, double *abuf, double *ebuf, int waves, hipStream_t stream);
int prepare_sweep_stream_roll(const Dev &d, int waves);
} // namespace sb

// step_jacobi.hip: k_sweep_jacobi (SB_KERNEL_JACOBI), TFSimulator's float32 Jacobi update, both grids in LDS;
// step_jacobi_global.hip: k_sweep_jacobi_g, the same step with the grids in global memory, for plans LDS does not hold.
// Their own arguments besides Dev: Dev carries the step hand-over (Bld::t_now, gtabg, zsum, gsum, nsw, next_b) and the
// zones as for every sweep kernel.
namespace sb {
struct JacArgs {
  float *grid;         // [B][N] the float32 state, row-major in the caller's orientation
  const uint8_t *cls;  // [N] class per CV
  const float *tab;    // [ncls][SB_JACOBI_COEFS] sb_jacobi_desc.class_f32
  const double *rden;  // [ncls] 1.0 / (double)den, correctly rounded (host)
  int ncls;
  int n_pad;           // floats per padded grid buffer (sweep_jacobi_slots: the grid with its T_inf padding)
  int nb;              // buildings of this launch (B; sb_tap_jacobi: its n)
  const float *q;      // sb_tap_jacobi: [nb][N] input_q; NULL: q = (float)gtabg[class]
  const double *tinf;  // sb_tap_jacobi: [nb] T_inf; NULL: Bld::t_now
  int path;            // sweep_jacobi_path's answer: 0 k_sweep_jacobi, 2 k_sweep_jacobi_g
  int sum_threads;     // k_sweep_jacobi_g: sweep_jacobi_threads(N), the thread count whose order the float64 grid sum keeps
  float *scratch;      // k_sweep_jacobi_g: [workgroups][sweep_jacobi_g_scratch_floats] two padded grids and (M*Tprev)/dt
};
// The one rule (sb_launch_info.path): 0 -- k_sweep_jacobi holds the plan (N <= 20,480 and 160 KiB of LDS) and
// force_global is not set; 2 -- k_sweep_jacobi_g; -1 -- neither (more than sweep_jacobi_g_max_cvs() CVs).  The functions
// below that take a path dispatch on its answer.
int sweep_jacobi_path(int H, int W, int ncls, bool force_global);
int sweep_jacobi_threads(int N);                   // threads per workgroup of k_sweep_jacobi's instantiation for N CVs
int sweep_jacobi_threads(int N, int path);         // ... of the kernel of that path
int sweep_jacobi_slots(int H, int W);              // floats of one padded grid buffer
size_t sweep_jacobi_lds_bytes(int H, int W, int ncls, int path); // LDS per workgroup (dynamic + static)
int prepare_sweep_jacobi(int H, int W, int ncls, int path);
int sweep_jacobi_blocks_per_cu(int H, int W, int ncls, int path); // resident workgroups per CU (registers, LDS, waves); 0: unknown
int launch_sweep_jacobi(const Dev &d, const JacArgs &j, int workgroups, hipStream_t stream);
// step_jacobi_global.hip
bool sweep_jacobi_g_supported(int H, int W);
int sweep_jacobi_g_max_cvs();
int sweep_jacobi_g_threads();
size_t sweep_jacobi_g_lds_bytes();
size_t sweep_jacobi_g_scratch_floats(int H, int W); // per resident workgroup
int sweep_jacobi_g_blocks_per_cu();
int launch_sweep_jacobi_g(const Dev &d, const JacArgs &j, int workgroups, hipStream_t stream);
} // namespace sb

#define SB_HIP(call)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(SB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
  } while (0)
// Entry points run on the handle's device and leave the calling thread's current device as
// they found it (a handle on device 1 must not redirect the caller's later torch allocations).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) err = hipSetDevice(device);
    else if (err == hipSuccess) prev = -1; // nothing to restore
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define SB_ON_DEVICE(dev)                                                                    \
  DeviceGuard device_guard_(dev);                                                            \
  if (device_guard_.err != hipSuccess)                                                       \
    return fail(SB_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(device_guard_.err))

template <typename Tp>
struct DevBuf {
  Tp *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

template <typename Tp>
inline void drop(DevBuf<Tp> &buf) { // (the caller has made the device idle where a kernel may still read the buffer)
  if (buf.p) (void)hipFree(buf.p);
  buf.p = nullptr;
}

template <typename Tp>
inline int upload(DevBuf<Tp> &buf, const Tp *src, size_t n) {
  SB_HIP(hipMalloc((void **)&buf.p, std::max<size_t>(n, 1) * sizeof(Tp)));
  if (n) SB_HIP(hipMemcpy(buf.p, src, n * sizeof(Tp), hipMemcpyHostToDevice));
  return SB_OK;
}
template <typename Tp>
inline int alloc_zero(DevBuf<Tp> &buf, size_t n) {
  SB_HIP(hipMalloc((void **)&buf.p, std::max<size_t>(n, 1) * sizeof(Tp)));
  SB_HIP(hipMemset(buf.p, 0, std::max<size_t>(n, 1) * sizeof(Tp)));
  return SB_OK;
}


// A room cell of the convection shuffle (generators.hip).
struct ConvCell {
  int g0;                  // the cell's index in the caller's [H, W] grid: Philox counter, tie-break
  int gh;                  // ... in the handle's grid (which may be the transposed plan)
  int sidx;                // index into the building's state
  int pad;
  unsigned long long mask; // bit k: offset k of the table leads to a cell of the same room
};

// One group's row of sb_occupancy_attach_groups' device table (generators.hip, k_occupancy<CLK, true>): what k_occupancy
// takes from OccArgs' scalars with one configuration.
struct OccGroup {
  int e_arr, l_arr, e_dep, n_occ;
  double p_arr, p_dep;
};

// What the three per-episode attachments (sb_initial_conditions_attach, sb_randomization_attach,
// sb_episode_starts_attach) each keep for their draws (episode_draw.h): one Philox block per (seed, global building,
// episode, tag | field).
struct EpisodeDraws {
  bool attached = false;
  DevBuf<int> episode;  // [B] the number of the building's next episode: 0 at attach, advanced by every reset of the building
  uint64_t seed = 0;
  long long first = 0;  // global index of building 0
};

struct sb_handle {
  sb::Dev d{};
  sb_sweep_kernel kernel = SB_KERNEL_LDS; // which sweep kernel runs (prepare_sweep / launch_sweep); Dev::reg / P / stream_ms follow it
  int stream_variant = kStreamPlain;      // SB_KERNEL_STREAM: kStreamPlain / kStreamMs / kStreamRoll
  int device = 0, cus = 256;
  bool was_reset = false; // the first sb_reset also sets the construction-time device state
  int steps_since_reset = 0; // how far a reset rewinds the clock (the boiler's action age, scal[19])
  void *counters_zeroed_on = (void *)(uintptr_t)1; // the stream on which k_pre has zeroed the sweep kernel's draw counters since the last sweep launch (1: none)
  sb_launch_info info{};
  sb_reward_config reward{};  // sb_set_reward_function: which k_post runs (kind 0: the regret, the default) and its constants
  DevBuf<uint8_t> cls, tcls, tcset;
  DevBuf<double> abuf; // step_stream.hip: A = ap*Tprev + g of the buildings in flight
  DevBuf<double> ebuf; // step_stream_ms.hip: the scratch grid a pass writes when it reads the building's state (per resident workgroup)
  DevBuf<double> redo_scratch; // step_roll.hip: see Dev
  DevBuf<int> redo_ctr, redo_list, zs_off;
  DevBuf<int> act_kind, act_zone, zone_act; // the action vector's tables (sb_params.act_*) on the device
  DevBuf<double> act_lo, act_hi;
  DevBuf<double> tmul; // step_roll.hip: the tail scan's static multipliers
  DevBuf<double> bp;   // sb_set_building_params: [SB_NUM_BUILDING_PARAMS][B] (Dev::bp points here while a table is set)
  DevBuf<double> ctab, csetab, temp, zmean, zair, damper, qz, scal, obs_mean, obs_sigma, ring, gtabg, zsum, gsum,
      hist_bins;
  DevBuf<int> czone, zone_off, zone_cells_l, mode, col_zone, zblk_zone, cell_state, nsw, next_b, src_dest,
      hist_col, hist_off;
  DevBuf<sb::Bld> bld;
  DevBuf<uint4> zl16;
  DevBuf<int4> sched;
  DevBuf<unsigned long long> smask, cmapS, amapS, zmapS;
  DevBuf<long long> dbg;
  // host copies for the optional generators
  std::vector<int> h_zone_off, h_zone_cells, h_state_index; // state index of every grid cell (< 0: exterior ring)
  // sb_convection_attach
  DevBuf<int> conv_local, conv_off; // per grid cell: index in its room's list; the offset table as linear steps
  DevBuf<int> conv_by_rank;         // whole-room shuffle: list index of the room's cell with raster rank r
  bool conv_whole_room = false;
  bool conv_wide = false, conv_transposed = false; // a window of more than 64 offsets: rejection sampling
  int conv_wide_d = 0;
  DevBuf<short> conv_room;          // per grid cell: its room (-1: none)
  DevBuf<ConvCell> conv_cells;
  DevBuf<unsigned short> conv_partner; // per room cell: its valid offsets' target cells (list indices), conv_pw entries per cell
  int conv_pw = 1;
  double conv_p = 0.0;
  int conv_n_off = 0, conv_max_room = 0;
  uint64_t conv_seed = 0;
  long long conv_first = 0;
  uint32_t conv_calls = 0;
  bool conv_attached = false;
  // sb_convection_attach_seeded (conv_seeded.hip): the buildings' Mersenne Twisters, [B][625]; the tables above are shared
  DevBuf<uint32_t> conv_rng;
  bool conv_seeded = false;
  DevBuf<uint32_t> occ_state; // sb_occupancy_attach
  sb_occupancy_config occ{};
  uint32_t occ_queries = 0;
  bool occ_attached = false;
  // sb_occupancy_attach_groups: a configuration per group of buildings (occ then holds group 0's: the shared seed, first
  // building and time step); occ_n_groups == 0: the one configuration of sb_occupancy_attach
  DevBuf<OccGroup> occ_groups;      // [occ_n_groups]
  DevBuf<uint16_t> occ_group_of;    // [B] the building's group
  int occ_n_groups = 0;
  // sb_clock_attach / sb_clock_seek: the table of instants, the buildings' offsets, the position of the next step
  DevBuf<double> clock_rows;        // [clock_n_rows][SB_CLOCK_FIELDS]; NULL: no clock
  DevBuf<int> clock_offs;           // [B] the attached offsets
  DevBuf<int> clock_eff;            // [B] the effective offsets (ClockView::offs): attached offset - the building's restart position
  std::vector<int> h_clock_offs;    // [B] host copy of the attached offsets
  int clock_n_rows = 0, clock_max_off = 0; // clock_max_off: the largest EFFECTIVE offset (sb_clock_seek's bound)
  int clock_pos = -1, clock_prev = -1; // pos < 0: never sought
  // sb_reset_buildings: episodes per building.  The host shadow of every building's restart position (empty: all 0), the
  // largest of them (sb_clock_seek: pos >= it), and whether some building was reset by itself since the last sb_reset
  std::vector<int> restart_pos;
  int max_restart = 0;
  bool own_prev = false;
  bool ep_dirty = false;            // ep_start may hold non-zero entries: a partial reset since the last sb_reset
  DevBuf<int> ep_start;             // [B] the handle's steps_since_reset at the building's own last reset (allocated by the first sb_reset_buildings)
  DevBuf<uint8_t> ep_mask;          // [B] the mask of the call in flight (allocated by the first sb_reset_buildings / sb_observe_buildings)
  // sb_create_materials: the structural classes' descriptors, the buildings' values and their coefficient rows
  bool materials = false;
  int mat_slots = 0;                // M
  std::vector<double> mat_default;  // [3 M + 1] the plan's own value of every field (kind * M + slot; 3 M: h_conv)
  double mat_dx = 0.0, mat_dx2 = 0.0, mat_zh = 0.0;
  DevBuf<int4> mat_desc;            // [ncls] {slot, neighbour count, present mask, half-factor mask}
  DevBuf<double> mat_diff;          // [ncls] diffuser weight
  DevBuf<double> mat_tab;           // [3 M + 1][B] the values in force
  DevBuf<double> ctab_b;            // [B][ncls + 1][8] (Dev::ctab_b)
  // sb_spatial_attach (spatial.hip): k_spatial's index tables (spatial.h) on the device, and the scalars that go with them
  bool sp_attached = false;
  int sp_map_h = 0, sp_map_w = 0, sp_tile_len = 0, sp_tile_wave = 0; // map_h == 0: zone statistics only
  int sp_state_len = 0;             // elements of a building's state (the source indices' first range)
  int sp_stage_bytes = 0;           // > 0: the state is staged in this much LDS per workgroup; 0: gathered from global memory
  DevBuf<int> sp_tile_src, sp_tile_off, sp_tile_cnt, sp_zone_off, sp_zone_src;
  // sb_initial_conditions_attach (runtime.hip): the start temperatures' arrays and the buildings' episode counters
  EpisodeDraws ic_draws;            // (attached: launch_reset runs the conditions' kernels)
  int ic_n_grids = 0;               // K; 0: no grids
  DevBuf<double> ic_grids;          // [K][N] in the handle's orientation
  DevBuf<int> ic_grid_of;           // [B]; NULL: every building grid 0
  DevBuf<double> ic_base, ic_offset; // [B] initial_temp, offset; NULL: absent
  bool ic_jitter = false;
  double ic_lo = 0.0, ic_hi = 0.0;
  // sb_randomization_attach (randomize.hip): the fields' descriptors and choice tables, their base rows, the counters
  EpisodeDraws rz_draws;
  int rz_n_fields = 0;
  bool rz_materials = false;        // some field is a material field: a redraw re-folds the coefficient rows
  bool rz_own_bp = false;           // the attach allocated the parameter table (the handle had none): detach drops it
  DevBuf<unsigned char> rz_desc;    // [n_fields] sb::RandField, then the choice tables (doubles)
  size_t rz_choices_at = 0;         // byte offset of the choice tables in rz_desc
  DevBuf<double> rz_base;           // [n_fields][B] the rows in force at attach
  std::vector<double> rz_base_bp;   // host: [SB_NUM_BUILDING_PARAMS][B] the whole table at attach (sb_params' values without one)
  std::vector<double> rz_base_mat;  // host: [3 M + 1][B] likewise; empty on a handle without materials
  // sb_clock_set_offsets: the offsets a building takes at its next reset where they differ from h_clock_offs, which then
  // holds the larger of the two (empty: none pending)
  std::vector<int> h_clock_next;
  // sb_episode_starts_attach (episode_starts.hip): the fields, their choice tables, the base values, the counters
  EpisodeDraws es_draws;            // attached: a reset launches k_episode_starts ...
  bool es_restoring = false;        // ... which writes the base values: detached, until every building was reset once
  bool es_offsets = false;          // SB_START_OFFSET is (or, restoring, was) drawn: h_clock_offs holds the largest possible offsets
  sb::StartField es_field[SB_START_FIELDS] = {};
  int es_relative = 0;
  DevBuf<double> es_choices;        // the fields' choice tables, one after the other
  DevBuf<int> es_base_offs;         // [B] the offsets given to sb_clock_attach
  DevBuf<double> es_base_lohi;      // [B][2] the caller's weather array at attach
  DevBuf<double> es_base_shift;     // [B] likewise
  std::vector<int> es_h_base_offs;  // host copy of es_base_offs
  std::vector<uint8_t> es_pending;  // restoring: the buildings not reset since the detach
  double *es_lohi = nullptr, *es_shift = nullptr; // the caller's arrays
  // sb_episode_metrics_attach (episode_metrics.hip): the buildings' episode totals
  EpisodeDraws em_draws;            // attached: sb_step launches k_episode_metrics, a reset k_episode_metrics_close (no draws: the flag alone)
  DevBuf<double> em_running;        // [SB_EM_FIELDS][B] the episodes in progress
  DevBuf<double> em_completed;      // [SB_EM_FIELDS][B] every building's last closed episode
  DevBuf<float> em_info;            // [B][SB_INFO_STRIDE] k_post's info rows when sb_step is given none
  // sb_telemetry_attach (telemetry.hip): the buildings scored against recorded zone temperatures
  EpisodeDraws tl_draws;            // attached: sb_step launches k_telemetry, a reset k_telemetry_close (no draws: the flag alone)
  DevBuf<double> tl_running, tl_completed;           // [SB_TL_FIELDS][B]
  DevBuf<double> tl_zone_running, tl_zone_completed; // [SB_TL_ZONE_FIELDS][Z][B] with per_zone, else null
  DevBuf<double> tl_traces, tl_weights;              // [n_traces][n_rows][Z] the recording; [Z] the zone weights
  DevBuf<float> tl_actions;                          // [n_traces][n_rows][n_actions] the recorded setpoints, or null
  DevBuf<int> tl_trace_of, tl_first_row;             // [B]
  int tl_n_traces = 0, tl_n_rows = 0;
  // SB_KERNEL_JACOBI (sb_create_jacobi): the float32 grid and the class tables; jac.grid etc. point into them
  DevBuf<float> jgrid, jtab, jscratch; // (jscratch: k_sweep_jacobi_g's per-workgroup grids)
  DevBuf<double> jrden;
  DevBuf<uint8_t> jcls;
  sb::JacArgs jac{};
};


// The handle's clock as the kernels take it (sb_clock_attach / sb_clock_seek); rows == NULL without one.  Refused: a clock
// never sought, or sought below a building's restart position (sb_reset_buildings: that building's row would lie before
// its offset, or before the table).
inline int handle_clock_view(const sb_handle *h, const char *who, sb::ClockView *out) {
  *out = sb::ClockView{};
  if (!h->clock_rows.p) return SB_OK;
  if (h->clock_pos < 0) return fail(SB_ERR_INVALID, std::string(who) + ": the handle has a clock that was never sought (sb_clock_seek)");
  if (h->clock_pos < h->max_restart)
    return fail(SB_ERR_INVALID, std::string(who) + ": a building restarts at position " + std::to_string(h->max_restart) +
                                    " (sb_reset_buildings), the clock is at " + std::to_string(h->clock_pos) + ": sb_clock_seek first");
  // (drawn offsets, sb_episode_starts_attach: a reset moves the building's rows, as a reset of its own does)
  const bool own_prev = h->own_prev || (h->es_draws.attached && h->es_offsets);
  *out = sb::ClockView{h->clock_rows.p, h->clock_eff.p, h->clock_pos, h->clock_prev, h->clock_n_rows, own_prev ? 1 : 0};
  return SB_OK;
}

// runtime.hip: the one dispatch on sb_handle::kernel -- the sweep kernel's LDS attribute (sb_create), its launch (sb_step)
int prepare_sweep(const sb_handle *h);
int launch_sweep(const sb_handle *h, hipStream_t stream);

// runtime.hip: uploads the buildings' values (tab: [3 M + 1][B]; empty: the plan's own in every row) and runs k_class_coef
// on `stream`, and waits for both
int apply_building_materials(sb_handle *h, const std::vector<double> &tab, hipStream_t stream);

// runtime.hip: k_class_coef on `stream` from the values in force (mat_tab); mask (DEVICE [B]) != NULL: the masked form,
// which re-folds the rows of the buildings with mask[b] != 0 and touches no other
int launch_class_coef(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream);
// runtime.hip: the names sb_set_building_params / sb_set_building_materials use in their messages
const char *building_param_name(int k);
std::string material_field_name(int f, int M);

// episode_draw.hip: what the per-episode attachments share on the host.
// The device is idle on return; a capture in progress refuses the synchronisation (SB_ERR_INVALID, `who` in front).
int idle_device(const std::string &who);
// The grid of a draw kernel over n items: kDrawThreads per workgroup, at most kDrawBlocksPerCu workgroups per CU (the
// kernels take the grid stride beyond), at least one.
constexpr int kDrawThreads = 256, kDrawBlocksPerCu = 8; // (_ffi.py: SB_RAND_THREADS, SB_RAND_BLOCKS_PER_CU)
int draw_blocks(const sb_handle *h, size_t n);
// One distribution of a sb_rand_field / sb_start_field, checked and taken apart.
struct DistIn {
  int kind;                     // sb_rand_kind, or SB_RAND_UNIFORM_INT
  double lo, hi;
  int step, n_choices;
  const double *choices;
};
struct DistWords {              // where the callers' messages differ, and what one of them checks beyond the other
  const char *unknown_head, *unknown_tail; // a kind outside `kinds`: "<field>: <head><kind><tail>"
  bool (*value_ok)(double);     // a further check on SB_RAND_UNIFORM_INT's bounds and on every choice; NULL: none
  const char *bounds_text, *choice_text; // ... "<field>: <bounds_text>", "<field>: choice <j> <choice_text>"
};
struct DistOut {
  double lo, hi;                // SB_RAND_UNIFORM
  int choice_off, choice_len;   // SB_RAND_CHOICE: the field's entries of `choices`, which parse_dist appended
  int ilo, step, k;             // SB_RAND_UNIFORM_INT
  double dmin, dmax;            // the smallest and the largest possible draw
};
// `at`: the entry point and the field's name, in front of every message; kinds: bit k set -- the field takes kind k.
int parse_dist(const std::string &at, const DistIn &in, unsigned kinds, const DistWords &w, std::vector<double> &choices, DistOut *out);
// The *_episodes_get / *_episodes_set entry points: the null checks, SB_ERR_UNSUPPORTED ("<who>: <missing_text>") when
// `draws` is not attached, and the stream-ordered device-to-device copy of the [B] counters.
int episodes_get(sb_handle *h, EpisodeDraws sb_handle::*draws, const char *who, const char *missing_text, int32_t *out_dev, hipStream_t stream);
int episodes_set(sb_handle *h, EpisodeDraws sb_handle::*draws, const char *who, const char *missing_text, const int32_t *in_dev, hipStream_t stream);
// Their check by itself (sb_episode_metrics_get / _set share it): SB_ERR_INVALID for a null handle or !have_array,
// SB_ERR_UNSUPPORTED when `draws` is not attached.
int draws_attached(const sb_handle *h, EpisodeDraws sb_handle::*draws, const char *who, const char *missing_text, bool have_array);

// episode_metrics.hip: k_episode_metrics behind k_post (sb_step's POST phase; info_dev: the rows k_post wrote), and the
// latch at the top of a reset, in front of the redraws below (mask_dev NULL: every building).  Stream-ordered launches
// only.  Only called while em_draws.attached.
int sb_episode_metrics_step(sb_handle *h, const float *reward_dev, const float *info_dev, hipStream_t stream);
int sb_episode_metrics_close(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream);

// telemetry.hip: k_telemetry behind k_post (and behind k_episode_metrics), and the latch at the top of a reset, next to
// the one above.  Stream-ordered launches only.  Only called while tl_draws.attached.
int sb_telemetry_step(sb_handle *h, hipStream_t stream);
int sb_telemetry_close(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream);

// randomize.hip: the redraw at the top of a reset (sb_reset: mask_dev NULL, every building; sb_reset_buildings: its
// device mask), stream-ordered launches only.  Only called while a randomisation is attached.
int sb_randomization_redraw(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream);

// runtime.hip: the bounds sb_clock_seek checks (clock_max_off, max_restart), from the host shadows
void episode_bounds(sb_handle *h);
// episode_starts.hip: the draw at the top of a reset, after sb_randomization_redraw (mask_dev as there), one stream-ordered
// launch; and the host shadow's part once the reset is queued (mask_host NULL: sb_reset).  Only called while es_draws.attached.
int sb_episode_starts_redraw(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream);
void sb_episode_starts_after_reset(sb_handle *h, const uint8_t *mask_host);
// episode_starts.hip: forgets an attachment with the clock its offsets belonged to (drop_clock; the device is idle)
void sb_episode_starts_forget(sb_handle *h);

// generators.hip: the convection shuffle between the sweep and the reward (sb_step)
int sb_launch_convection(sb_handle *h, hipStream_t stream);
// conv_seeded.hip: the seeded shuffle in its place.  In force after sb_convection_attach_seeded until either attach call
// replaces or detaches it: sb_convection_attach leaves conv_first >= 0 and conv_attached set, the seeded attach -1 and clear.
int sb_launch_convection_seeded(sb_handle *h, hipStream_t stream);
inline bool seeded_in_force(const sb_handle *h) { return h->conv_seeded && !h->conv_attached && h->conv_first < 0; }

#endif // SBSIM_AMD_SB_HOST_H_
