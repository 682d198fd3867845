// episode_draw.hip -- what the three per-episode attachments share on the host (sb_host.h declares it): the idle-device
// guard of an attach, the draw kernels' grid, the check of one distribution, the copies behind *_episodes_get / _set and their
// attachment check (which sb_episode_metrics_get / _set use too).
// Host code only: the draws themselves are episode_draw.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sb_host.h"

int idle_device(const std::string &who) {
  if (const hipError_t e = hipDeviceSynchronize(); e != hipSuccess) {
    const bool capturing = e == hipErrorStreamCaptureUnsupported || e == hipErrorStreamCaptureImplicit;
    return fail(capturing ? SB_ERR_INVALID : SB_ERR_HIP, who + (capturing ? "not while a stream is being captured into a graph"
                                                                          : hipGetErrorString(e)));
  }
  return SB_OK;
}

int draw_blocks(const sb_handle *h, size_t n) {
  return (int)std::max<size_t>(1, std::min<size_t>((n + kDrawThreads - 1) / kDrawThreads, (size_t)h->cus * kDrawBlocksPerCu));
}

int parse_dist(const std::string &at, const DistIn &in, unsigned kinds, const DistWords &w, std::vector<double> &choices, DistOut *out) {
  *out = DistOut{};
  const bool taken = in.kind >= 0 && in.kind < 32 && ((kinds >> in.kind) & 1u);
  if (taken && (in.kind == SB_RAND_UNIFORM || in.kind == SB_RAND_UNIFORM_INT)) {
    if (!(std::isfinite(in.lo) && std::isfinite(in.hi))) return fail(SB_ERR_INVALID, at + ": lo and hi must be finite");
    if (in.lo > in.hi) return fail(SB_ERR_INVALID, at + ": lo " + std::to_string(in.lo) + " > hi " + std::to_string(in.hi));
    if (in.kind == SB_RAND_UNIFORM) {
      out->lo = out->dmin = in.lo;
      out->hi = out->dmax = in.hi;
      return SB_OK;
    }
    if (w.value_ok && !(w.value_ok(in.lo) && w.value_ok(in.hi))) return fail(SB_ERR_INVALID, at + ": " + w.bounds_text);
    if (in.step < 1) return fail(SB_ERR_INVALID, at + ": step must be >= 1, got " + std::to_string(in.step));
    const long long k = ((long long)in.hi - (long long)in.lo) / in.step + 1;
    if (k > SB_START_MAX_K) return fail(SB_ERR_INVALID, at + ": K = " + std::to_string(k) + " is more than 2^22");
    out->ilo = (int)in.lo;
    out->step = in.step;
    out->k = (int)k;
    out->dmin = in.lo;
    out->dmax = (double)(out->ilo + out->step * (out->k - 1));
    return SB_OK;
  }
  if (taken && in.kind == SB_RAND_CHOICE) {
    if (in.n_choices < 1 || in.n_choices > SB_RAND_MAX_CHOICES || !in.choices)
      return fail(SB_ERR_INVALID, at + ": a choice needs 1 .. 65,536 values, got " + std::to_string(in.n_choices));
    for (int j = 0; j < in.n_choices; ++j) {
      if (!std::isfinite(in.choices[j])) return fail(SB_ERR_INVALID, at + ": choice " + std::to_string(j) + " is not finite");
      if (w.value_ok && !w.value_ok(in.choices[j])) return fail(SB_ERR_INVALID, at + ": choice " + std::to_string(j) + " " + w.choice_text);
    }
    out->choice_off = (int)choices.size();
    out->choice_len = in.n_choices;
    choices.insert(choices.end(), in.choices, in.choices + in.n_choices);
    out->dmin = *std::min_element(in.choices, in.choices + in.n_choices);
    out->dmax = *std::max_element(in.choices, in.choices + in.n_choices);
    return SB_OK;
  }
  return fail(SB_ERR_INVALID, at + ": " + w.unknown_head + std::to_string(in.kind) + w.unknown_tail);
}

int draws_attached(const sb_handle *h, EpisodeDraws sb_handle::*draws, const char *who, const char *missing_text, bool have_array) {
  if (!h || !have_array) return fail(SB_ERR_INVALID, std::string(who) + ": null argument");
  if (!(h->*draws).attached) return fail(SB_ERR_UNSUPPORTED, std::string(who) + ": " + missing_text);
  return SB_OK;
}

namespace {

int episodes_copy(sb_handle *h, EpisodeDraws sb_handle::*draws, const char *who, const char *missing_text, int32_t *out_dev,
                  const int32_t *in_dev, hipStream_t stream) {
  SB_CHECK(draws_attached(h, draws, who, missing_text, out_dev || in_dev));
  const EpisodeDraws &d = h->*draws;
  SB_ON_DEVICE(h->device);
  const size_t bytes = (size_t)h->d.B * sizeof(int32_t);
  if (out_dev) SB_HIP(hipMemcpyAsync(out_dev, d.episode.p, bytes, hipMemcpyDeviceToDevice, stream));
  else SB_HIP(hipMemcpyAsync(d.episode.p, in_dev, bytes, hipMemcpyDeviceToDevice, stream));
  return SB_OK;
}

} // namespace

int episodes_get(sb_handle *h, EpisodeDraws sb_handle::*draws, const char *who, const char *missing_text, int32_t *out_dev, hipStream_t stream) {
  return episodes_copy(h, draws, who, missing_text, out_dev, nullptr, stream);
}

int episodes_set(sb_handle *h, EpisodeDraws sb_handle::*draws, const char *who, const char *missing_text, const int32_t *in_dev, hipStream_t stream) {
  return episodes_copy(h, draws, who, missing_text, nullptr, in_dev, stream);
}
