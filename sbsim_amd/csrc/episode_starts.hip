// episode_starts.hip -- sb_episode_starts_attach: a start time and weather per building, drawn at every episode start, on
// the device (include/sbsim_amd.h states the semantics; episode_draw.h the draw).  A reset of a handle with the
// attachment launches k_episode_starts before its reset kernel: the drawn offset into the buffer the reset kernel reads
// as the attached offsets, the weather values into the caller's arrays, the counter advanced, all by the one thread
// that owns the building.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (one rounding per operation: the draw is restated in NumPy).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "episode_draw.h"
#include "sb_host.h"

using namespace sb;

namespace {

// StartField::present beyond 0 / 1: a field an earlier attachment drew and this one does not -- every reset writes its
// base value, so the building returns to it at its next reset.
constexpr int kPresentBase = 2;

enum StartMode {
  kDraw = 0,        // a reset: the draw of episode e, then e + 1
  kMaterialise = 1, // sb_episode_starts_episodes_set: the values in force for counters t -- the draw of t - 1, the base at 0
  kRestore = 2      // detached: the base values
};

struct StartArgs {
  StartField f[SB_START_FIELDS];
  const double *choices;
  const int *base_offs;     // [B] the offsets given to sb_clock_attach
  const double *base_lohi;  // [B][2] the caller's array at attach
  const double *base_shift; // [B]
  int *offs;                // [B] the offsets in force: what the reset kernel reads as the attached offsets
  int *eff;                 // [B] the effective offsets
  double *lohi, *shift;     // the caller's arrays
  int *episode;             // [B]
  const uint8_t *mask;      // [B] the buildings that are reset; NULL: every building
  uint64_t seed;
  long long first;
  int B, relative, mode;
};

// One thread per building, the building the fast index: a wavefront writes 64 neighbours of every array.
__global__ void __launch_bounds__(kDrawThreads) k_episode_starts(StartArgs a) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < a.B; b += gridDim.x * blockDim.x) {
    if (a.mask && !a.mask[b]) continue;
    int e = a.mode == kRestore ? 0 : a.episode[b];
    const bool base = a.mode == kRestore || (a.mode == kMaterialise && before_first_episode(e));
    auto based = [&](int i) { return base || a.f[i].present == kPresentBase; };
    if (a.mode == kMaterialise) e = episode_in_force(e);
    const uint64_t gb = (uint64_t)(a.first + b);
    if (a.f[SB_START_OFFSET].present) {
      int off = a.base_offs[b];
      if (!based(SB_START_OFFSET)) {
        const int d = start_offset_draw(a.f[SB_START_OFFSET], a.choices, a.seed, gb, (uint32_t)e);
        off = a.relative ? off + d : d;
      }
      // the effective offset: a masked reset's kernel writes it (offset - restart_pos); sb_reset restarts at 0; a
      // materialised offset keeps the building's restart position
      if (a.mode == kMaterialise) a.eff[b] += off - a.offs[b];
      else if (!a.mask) a.eff[b] = off;
      a.offs[b] = off;
    }
    if (a.f[SB_START_WEATHER_LOW].present)
      a.lohi[2 * (size_t)b] = based(SB_START_WEATHER_LOW) ? a.base_lohi[2 * (size_t)b]
                                   : start_draw(a.f[SB_START_WEATHER_LOW], a.choices, a.seed, gb, (uint32_t)e);
    if (a.f[SB_START_WEATHER_HIGH].present)
      a.lohi[2 * (size_t)b + 1] = based(SB_START_WEATHER_HIGH) ? a.base_lohi[2 * (size_t)b + 1]
                                       : start_draw(a.f[SB_START_WEATHER_HIGH], a.choices, a.seed, gb, (uint32_t)e);
    if (a.f[SB_START_WEATHER_SHIFT].present)
      a.shift[b] = based(SB_START_WEATHER_SHIFT) ? a.base_shift[b] : start_draw(a.f[SB_START_WEATHER_SHIFT], a.choices, a.seed, gb, (uint32_t)e);
    if (a.mode == kDraw) a.episode[b] = next_episode(e);
  }
}

int launch_starts(sb_handle *h, const uint8_t *mask, int mode, hipStream_t stream) {
  StartArgs a{};
  for (int i = 0; i < SB_START_FIELDS; ++i) a.f[i] = h->es_field[i];
  a.choices = h->es_choices.p;
  a.base_offs = h->es_base_offs.p;
  a.base_lohi = h->es_base_lohi.p;
  a.base_shift = h->es_base_shift.p;
  a.offs = h->clock_offs.p;
  a.eff = h->clock_eff.p;
  a.lohi = h->es_lohi;
  a.shift = h->es_shift;
  a.episode = h->es_draws.episode.p;
  a.mask = mask;
  a.seed = h->es_draws.seed;
  a.first = h->es_draws.first;
  a.B = h->d.B;
  a.relative = h->es_relative;
  a.mode = mode;
  hipLaunchKernelGGL(k_episode_starts, dim3(draw_blocks(h, (size_t)h->d.B)), dim3(kDrawThreads), 0, stream, a);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

const char *const kFieldNames[SB_START_FIELDS] = {"offsets", "weather_low", "weather_high", "weather_shift"};

// An offset, bound or choice: a whole number of rows a timeline may have.
bool whole_rows(double v) { return v >= 0.0 && v <= (double)SB_CLOCK_MAX_ROWS && v == std::floor(v); }

const char *const kNoStarts = "the handle has no episode starts (sb_episode_starts_attach)";

// Largest offset building b may have while the attachment draws: the attached one, or the largest draw.
int largest_offset(const sb_handle *h, int b, int max_draw, int relative) {
  const int base = h->es_h_base_offs[(size_t)b];
  return relative ? base + max_draw : std::max(base, max_draw);
}

} // namespace

int sb_episode_starts_redraw(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream) {
  return launch_starts(h, mask_dev, h->es_restoring ? kRestore : kDraw, stream);
}

void sb_episode_starts_after_reset(sb_handle *h, const uint8_t *mask_host) {
  if (!h->es_restoring) return; // (drawing: the shadow holds the largest possible offsets, whichever were drawn)
  const size_t B = (size_t)h->d.B;
  bool left = false;
  for (size_t b = 0; b < B; ++b) {
    if (!mask_host || mask_host[b]) {
      h->es_pending[b] = 0;
      if (h->es_offsets) h->h_clock_offs[b] = h->es_h_base_offs[b];
    }
    left = left || h->es_pending[b];
  }
  if (h->es_offsets) episode_bounds(h);
  if (!left) h->es_draws.attached = h->es_restoring = h->es_offsets = false; // (the buffers go with the next attach or the handle)
}

void sb_episode_starts_forget(sb_handle *h) {
  h->es_draws.attached = h->es_restoring = h->es_offsets = false;
  drop(h->es_choices); drop(h->es_draws.episode); drop(h->es_base_offs); drop(h->es_base_lohi); drop(h->es_base_shift);
  h->es_h_base_offs.clear();
  h->es_pending.clear();
  h->es_lohi = h->es_shift = nullptr;
}

extern "C" {

int sb_episode_starts_attach(sb_handle *h, const sb_episode_starts *es) {
  const std::string who = "sb_episode_starts_attach: ";
  if (!h || !es) return fail(SB_ERR_INVALID, who + "null argument");
  const int B = h->d.B;
  if (es->first_building < 0) return fail(SB_ERR_INVALID, who + "first_building must be >= 0");
  // the fields by themselves
  StartField fld[SB_START_FIELDS] = {};
  std::vector<double> choices;
  double dmin[SB_START_FIELDS] = {}, dmax[SB_START_FIELDS] = {};
  bool any = false;
  for (int i = 0; i < SB_START_FIELDS; ++i) {
    const sb_start_field &f = es->field[i];
    if (!f.present) continue;
    any = true;
    const std::string name = kFieldNames[i];
    StartField &d = fld[i];
    d.present = 1;
    d.d = RandField{i, 0, 0, f.kind, 0, 0, 0, 0, 0.0, 0.0};
    const bool offset = i == SB_START_OFFSET;
    DistOut o;
    SB_CHECK(parse_dist(who + name, DistIn{f.kind, f.lo, f.hi, f.step, f.n_choices, f.choices},
                        1u << (offset ? SB_RAND_UNIFORM_INT : SB_RAND_UNIFORM) | 1u << SB_RAND_CHOICE,
                        DistWords{"distribution ", " is unknown or not one this field takes", offset ? whole_rows : nullptr,
                                  "lo and hi must be whole numbers of rows in 0 .. 2^22", "must be a whole number of rows in 0 .. 2^22"},
                        choices, &o));
    d.d.lo = o.lo; d.d.hi = o.hi; d.d.choice_off = o.choice_off; d.d.choice_len = o.choice_len;
    d.ilo = o.ilo; d.step = o.step; d.k = o.k;
    dmin[i] = o.dmin; dmax[i] = o.dmax;
  }
  if (!any) return fail(SB_ERR_INVALID, who + "no field is present (sb_episode_starts_detach returns to the handle without)");
  const bool inherit = h->es_draws.attached;
  double *const lohi_dev = es->weather_lohi_dev ? es->weather_lohi_dev : inherit ? h->es_lohi : nullptr;
  double *const shift_dev = es->weather_offset_dev ? es->weather_offset_dev : inherit ? h->es_shift : nullptr;
  if (inherit)
    for (int i = 0; i < SB_START_FIELDS; ++i)
      if (h->es_field[i].present && !fld[i].present) {
        fld[i].present = kPresentBase;
        fld[i].d.id = i;
      }
  const bool lohi = fld[SB_START_WEATHER_LOW].present || fld[SB_START_WEATHER_HIGH].present;
  if (lohi && !lohi_dev) return fail(SB_ERR_INVALID, who + "weather_low / weather_high need weather_lohi_dev");
  if (fld[SB_START_WEATHER_SHIFT].present && !shift_dev)
    return fail(SB_ERR_INVALID, who + "weather_shift needs weather_offset_dev");
  if (fld[SB_START_OFFSET].present && !h->clock_rows.p)
    return fail(SB_ERR_UNSUPPORTED, who + "offsets: the handle has no clock (sb_clock_attach first)");
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device(who));
  // the base values: those of an attachment this one replaces, else what is in force
  std::vector<int> base_offs;
  if (fld[SB_START_OFFSET].present) {
    if (inherit && h->es_offsets) base_offs = h->es_h_base_offs;
    else base_offs = h->h_clock_next.empty() ? h->h_clock_offs : h->h_clock_next;
    const int max_draw = (int)dmax[SB_START_OFFSET]; // (a field that only returns to its base: 0)
    for (int b = 0; b < B; ++b) {
      const long long top = es->relative ? (long long)base_offs[(size_t)b] + max_draw : std::max(base_offs[(size_t)b], max_draw);
      if (top > (long long)h->clock_n_rows - 2)
        return fail(SB_ERR_INVALID, who + "offsets: building " + std::to_string(b) + ": the largest possible offset " +
                                        std::to_string(top) + " leaves no two rows of the table's " + std::to_string(h->clock_n_rows));
    }
  }
  std::vector<double> base_lohi, base_shift;
  if (lohi) {
    base_lohi.resize((size_t)B * 2);
    const double *src = inherit && h->es_base_lohi.p && h->es_lohi == lohi_dev ? h->es_base_lohi.p : lohi_dev;
    SB_HIP(hipMemcpy(base_lohi.data(), src, base_lohi.size() * sizeof(double), hipMemcpyDeviceToHost));
    const bool dl = fld[SB_START_WEATHER_LOW].present == 1, dh = fld[SB_START_WEATHER_HIGH].present == 1;
    for (int b = 0; b < B; ++b) {
      const double lo_max = dl ? dmax[SB_START_WEATHER_LOW] : base_lohi[2 * (size_t)b];
      const double hi_min = dh ? dmin[SB_START_WEATHER_HIGH] : base_lohi[2 * (size_t)b + 1];
      if ((dl || dh) && lo_max > hi_min)
        return fail(SB_ERR_INVALID, who + (dl ? "weather_low" : "weather_high") + ": building " + std::to_string(b) + ": low can be " +
                                        std::to_string(lo_max) + ", above a high of " + std::to_string(hi_min));
    }
  }
  if (fld[SB_START_WEATHER_SHIFT].present) {
    base_shift.resize((size_t)B);
    const double *src = inherit && h->es_base_shift.p && h->es_shift == shift_dev ? h->es_base_shift.p : shift_dev;
    SB_HIP(hipMemcpy(base_shift.data(), src, base_shift.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  // nothing refused: from here on the handle changes
  drop(h->es_choices); drop(h->es_draws.episode); drop(h->es_base_offs); drop(h->es_base_lohi); drop(h->es_base_shift);
  SB_CHECK(upload(h->es_choices, choices.data(), choices.size()));
  SB_CHECK(alloc_zero(h->es_draws.episode, (size_t)B));
  if (!base_offs.empty()) SB_CHECK(upload(h->es_base_offs, base_offs.data(), base_offs.size()));
  if (!base_lohi.empty()) SB_CHECK(upload(h->es_base_lohi, base_lohi.data(), base_lohi.size()));
  if (!base_shift.empty()) SB_CHECK(upload(h->es_base_shift, base_shift.data(), base_shift.size()));
  for (int i = 0; i < SB_START_FIELDS; ++i) h->es_field[i] = fld[i];
  h->es_relative = es->relative ? 1 : 0;
  h->es_lohi = lohi_dev;
  h->es_shift = shift_dev;
  h->es_draws.seed = es->seed;
  h->es_draws.first = es->first_building;
  h->es_h_base_offs = base_offs;
  h->es_pending.clear();
  h->es_offsets = fld[SB_START_OFFSET].present != 0;
  h->es_restoring = false;
  h->es_draws.attached = true;
  if (h->es_offsets) { // the host shadow: the largest offset every building may have from here on
    h->h_clock_next.clear();
    const int max_draw = (int)dmax[SB_START_OFFSET];
    for (int b = 0; b < B; ++b) h->h_clock_offs[(size_t)b] = std::max(h->h_clock_offs[(size_t)b], largest_offset(h, b, max_draw, h->es_relative));
    episode_bounds(h);
  }
  return SB_OK;
}

int sb_episode_starts_detach(sb_handle *h) {
  if (!h) return fail(SB_ERR_INVALID, "sb_episode_starts_detach: null handle");
  if (!h->es_draws.attached || h->es_restoring) return SB_OK;
  h->es_restoring = true; // every building's next reset writes its base values; the counters mean nothing from here on
  h->es_pending.assign((size_t)h->d.B, 1);
  return SB_OK;
}

// (restoring: detached, the counters mean nothing)
int sb_episode_starts_episodes_get(sb_handle *h, int32_t *out_dev, void *stream) {
  const char *who = "sb_episode_starts_episodes_get";
  if (h && out_dev && h->es_restoring) return fail(SB_ERR_UNSUPPORTED, std::string(who) + ": " + kNoStarts);
  return episodes_get(h, &sb_handle::es_draws, who, kNoStarts, out_dev, (hipStream_t)stream);
}

int sb_episode_starts_episodes_set(sb_handle *h, const int32_t *in_dev, void *stream) {
  const char *who = "sb_episode_starts_episodes_set";
  if (h && in_dev && h->es_restoring) return fail(SB_ERR_UNSUPPORTED, std::string(who) + ": " + kNoStarts);
  SB_CHECK(episodes_set(h, &sb_handle::es_draws, who, kNoStarts, in_dev, (hipStream_t)stream));
  SB_ON_DEVICE(h->device);
  return launch_starts(h, nullptr, kMaterialise, (hipStream_t)stream); // the values in force for these counters
}

int sb_episode_starts_values_get(sb_handle *h, int32_t *offsets_dev, int32_t *effective_dev, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_episode_starts_values_get: null handle");
  if (!h->clock_rows.p) return fail(SB_ERR_UNSUPPORTED, "sb_episode_starts_values_get: the handle has no clock (sb_clock_attach)");
  SB_ON_DEVICE(h->device);
  const size_t n = (size_t)h->d.B * sizeof(int32_t);
  if (offsets_dev) SB_HIP(hipMemcpyAsync(offsets_dev, h->clock_offs.p, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (effective_dev) SB_HIP(hipMemcpyAsync(effective_dev, h->clock_eff.p, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SB_OK;
}

int sb_clock_set_offsets(sb_handle *h, const int32_t *offsets_host, void *stream) {
  const std::string who = "sb_clock_set_offsets: ";
  if (!h || !offsets_host) return fail(SB_ERR_INVALID, who + "null argument");
  if (!h->clock_rows.p) return fail(SB_ERR_UNSUPPORTED, who + "the handle has no clock (sb_clock_attach first)");
  if (h->es_draws.attached && h->es_offsets)
    return fail(SB_ERR_INVALID, who + "the attached episode starts draw the offsets (sb_episode_starts_detach, then a reset of every building, first)");
  const int B = h->d.B;
  for (int b = 0; b < B; ++b) {
    if (offsets_host[b] < 0) return fail(SB_ERR_INVALID, who + "building " + std::to_string(b) + ": negative offset " + std::to_string(offsets_host[b]));
    if (offsets_host[b] > h->clock_n_rows - 2)
      return fail(SB_ERR_INVALID, who + "building " + std::to_string(b) + ": offset " + std::to_string(offsets_host[b]) +
                                      " leaves no two rows of the table's " + std::to_string(h->clock_n_rows));
  }
  SB_ON_DEVICE(h->device);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  SB_HIP(hipStreamIsCapturing((hipStream_t)stream, &cap));
  if (cap != hipStreamCaptureStatusNone) return fail(SB_ERR_INVALID, who + "not while the stream is being captured into a graph");
  SB_HIP(hipMemcpyAsync(h->clock_offs.p, offsets_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream));
  SB_HIP(hipStreamSynchronize((hipStream_t)stream)); // (the host array may go away on return)
  h->h_clock_next.assign(offsets_host, offsets_host + B);
  for (int b = 0; b < B; ++b) h->h_clock_offs[(size_t)b] = std::max(h->h_clock_offs[(size_t)b], (int)offsets_host[b]);
  episode_bounds(h);
  return SB_OK;
}

} // extern "C"
