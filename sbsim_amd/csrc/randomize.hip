// randomize.hip -- sb_randomization_attach: per-building parameters and materials re-drawn at every episode start, on the
// device (include/sbsim_amd.h states the semantics; episode_draw.h the draw).  A reset of a handle with a randomisation
// launches, before its reset kernel: k_randomize (the drawn values of the resetting buildings into the two tables),
// k_rand_advance (their counters) and, with material fields, the masked k_class_coef (runtime.hip).
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

// One thread per (building, randomised field), the building the fast index: a wavefront writes 64 neighbours of one row.
// materialise (sb_randomization_episodes_set): the rows in force for counters t -- values(b, t - 1), the base row at 0.
__global__ void __launch_bounds__(kDrawThreads) k_randomize(const RandField *fields, const double *choices, const double *base, int nf,
                                                            int B, double *bp, double *mat, const uint8_t *mask, const int *episode,
                                                            uint64_t seed, long long first, int materialise) {
  const size_t n = (size_t)B * nf;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int f = (int)(i / B), b = (int)(i - (size_t)f * B);
    if (mask && !mask[b]) continue;
    const RandField fd = fields[f];
    const double b0 = base[i];
    int e = episode[b];
    const bool drawn = !materialise || !before_first_episode(e);
    if (materialise) e = episode_in_force(e);
    double v = b0;
    if (drawn) v = rand_value(fd, rand_draw(fd, choices, seed, (uint64_t)(first + b), (uint32_t)e), b0);
    (fd.material ? mat : bp)[(size_t)fd.row * B + b] = v;
  }
}

// After k_randomize (whose threads of a building all read the counter): the resetting buildings' next episode.
__global__ void __launch_bounds__(kDrawThreads) k_rand_advance(int *episode, const uint8_t *mask, int B) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x)
    if (!mask || mask[b]) episode[b] = next_episode(episode[b]);
}

// sb_params' value of every field in every building's row (a handle without a table).
struct ParamRow { double v[SB_NUM_BUILDING_PARAMS]; };
__global__ void __launch_bounds__(kDrawThreads) k_fill_params(ParamRow r, int B, double *out) {
  const size_t n = (size_t)B * SB_NUM_BUILDING_PARAMS;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = r.v[i / B];
}

int fill_params(const sb_handle *h, double *out, hipStream_t stream) {
  ParamRow r;
  for (int k = 0; k < SB_NUM_BUILDING_PARAMS; ++k) r.v[k] = param_field(h->d.p, k);
  hipLaunchKernelGGL(k_fill_params, dim3(draw_blocks(h, (size_t)h->d.B * SB_NUM_BUILDING_PARAMS)), dim3(kDrawThreads), 0, stream, r, h->d.B, out);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

int launch_randomize(sb_handle *h, const uint8_t *mask, int materialise, hipStream_t stream) {
  const RandField *fields = (const RandField *)h->rz_desc.p;
  const double *choices = (const double *)(h->rz_desc.p + h->rz_choices_at);
  hipLaunchKernelGGL(k_randomize, dim3(draw_blocks(h, (size_t)h->d.B * h->rz_n_fields)), dim3(kDrawThreads), 0, stream, fields, choices,
                     h->rz_base.p, h->rz_n_fields, h->d.B, h->bp.p, h->mat_tab.p, mask, h->rz_draws.episode.p, h->rz_draws.seed,
                     h->rz_draws.first, materialise);
  SB_HIP(hipGetLastError());
  return SB_OK;
}

std::string field_name(const sb_handle *h, int id) {
  return id < SB_RAND_MATERIAL ? building_param_name(id) : material_field_name(id - SB_RAND_MATERIAL, h->mat_slots);
}

// Both tables back to the rows of the attach, the buffers dropped.  The device is idle.
int drop_randomization(sb_handle *h) {
  if (!h->rz_draws.attached) return SB_OK;
  if (h->rz_own_bp) { // the handle had no table: back to sb_params' values through Dev::bp == NULL
    h->d.bp = nullptr;
    if (h->bp.p) SB_HIP(hipFree(h->bp.p));
    h->bp.p = nullptr;
  } else if (h->bp.p) {
    SB_HIP(hipMemcpy(h->bp.p, h->rz_base_bp.data(), h->rz_base_bp.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (h->materials && h->rz_materials) {
    SB_HIP(hipMemcpy(h->mat_tab.p, h->rz_base_mat.data(), h->rz_base_mat.size() * sizeof(double), hipMemcpyHostToDevice));
    SB_CHECK(launch_class_coef(h, nullptr, nullptr));
    SB_HIP(hipDeviceSynchronize());
  }
  drop(h->rz_desc); drop(h->rz_base); drop(h->rz_draws.episode);
  h->rz_base_bp.clear(); h->rz_base_bp.shrink_to_fit();
  h->rz_base_mat.clear(); h->rz_base_mat.shrink_to_fit();
  h->rz_draws.attached = h->rz_materials = h->rz_own_bp = false;
  h->rz_n_fields = 0;
  return SB_OK;
}

} // namespace

int sb_randomization_redraw(sb_handle *h, const uint8_t *mask_dev, hipStream_t stream) {
  SB_CHECK(launch_randomize(h, mask_dev, 0, stream));
  hipLaunchKernelGGL(k_rand_advance, dim3(draw_blocks(h, (size_t)h->d.B)), dim3(kDrawThreads), 0, stream, h->rz_draws.episode.p, mask_dev, h->d.B);
  SB_HIP(hipGetLastError());
  if (h->rz_materials) SB_CHECK(launch_class_coef(h, mask_dev, stream));
  return SB_OK;
}

extern "C" {

int sb_randomization_attach(sb_handle *h, const sb_rand_field *fields, int32_t n_fields, uint64_t seed, int64_t first_building) {
  const std::string who = "sb_randomization_attach: ";
  if (!h || !fields) return fail(SB_ERR_INVALID, who + "null argument");
  const int B = h->d.B, M = h->mat_slots, F = h->materials ? 3 * M + 1 : 0;
  if (n_fields <= 0 || n_fields > SB_NUM_BUILDING_PARAMS + F)
    return fail(SB_ERR_INVALID, who + "n_fields must be in 1 .. the number of per-building fields (sb_randomization_detach returns to the handle without)");
  if (first_building < 0) return fail(SB_ERR_INVALID, who + "first_building must be >= 0");
  // the fields by themselves
  std::vector<RandField> desc((size_t)n_fields);
  std::vector<double> choices;
  std::vector<double> dmin((size_t)n_fields), dmax((size_t)n_fields);
  std::vector<int> param_at(SB_NUM_BUILDING_PARAMS, -1), mat_at((size_t)F, -1); // the field's index in `fields`
  bool any_param = false, any_mat = false;
  for (int i = 0; i < n_fields; ++i) {
    const sb_rand_field &f = fields[i];
    const bool material = f.id >= SB_RAND_MATERIAL;
    if (material && !h->materials)
      return fail(SB_ERR_UNSUPPORTED, who + "material field " + std::to_string(f.id - SB_RAND_MATERIAL) + ": the handle has one "
                                          "coefficient table for every building (sb_create / sb_create_jacobi); create it with sb_create_materials");
    const int row = material ? f.id - SB_RAND_MATERIAL : f.id;
    if (row < 0 || row >= (material ? F : (int)SB_NUM_BUILDING_PARAMS)) return fail(SB_ERR_INVALID, who + "unknown field " + std::to_string(f.id));
    const std::string name = field_name(h, f.id);
    int &at = material ? mat_at[row] : param_at[row];
    if (at >= 0) return fail(SB_ERR_INVALID, who + "field " + name + " named twice");
    at = i;
    (material ? any_mat : any_param) = true;
    RandField &d = desc[i];
    d = RandField{f.id, row, material ? 1 : 0, f.kind, f.scale ? 1 : 0, 0, 0, 0, 0.0, 0.0};
    DistOut o;
    SB_CHECK(parse_dist(who + name, DistIn{f.kind, f.lo, f.hi, 0, f.n_choices, f.choices}, 1u << SB_RAND_UNIFORM | 1u << SB_RAND_CHOICE,
                        DistWords{"unknown distribution ", "", nullptr, nullptr, nullptr}, choices, &o));
    d.lo = o.lo; d.hi = o.hi; d.choice_off = o.choice_off; d.choice_len = o.choice_len;
    dmin[i] = o.dmin; dmax[i] = o.dmax;
  }
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device(who));
  // the base rows: those of an attachment this one replaces, else the tables in force
  std::vector<double> base_bp, base_mat;
  const bool had_table = h->rz_draws.attached ? !h->rz_own_bp : h->bp.p != nullptr;
  if (h->rz_draws.attached) {
    base_bp = h->rz_base_bp;
    base_mat = h->rz_base_mat;
  } else {
    base_bp.resize((size_t)SB_NUM_BUILDING_PARAMS * B);
    if (h->bp.p) SB_HIP(hipMemcpy(base_bp.data(), h->bp.p, base_bp.size() * sizeof(double), hipMemcpyDeviceToHost));
    else
      for (int k = 0; k < SB_NUM_BUILDING_PARAMS; ++k) std::fill_n(base_bp.begin() + (size_t)k * B, B, param_field(h->d.p, k));
    if (h->materials) {
      base_mat.resize((size_t)F * B);
      SB_HIP(hipMemcpy(base_mat.data(), h->mat_tab.p, base_mat.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  // every possible draw against the rows' checks: the closed range of every field, per building (scale: around its base)
  std::vector<double> plo(SB_NUM_BUILDING_PARAMS), phi(SB_NUM_BUILDING_PARAMS);
  static const int positive[] = {SB_BP_VAV_MAX_AIR_FLOW, SB_BP_AHU_EFF, SB_BP_AHU_MAX_FLOW, SB_BP_BLR_PUMP_EFF,
                                 SB_BP_BLR_CONV, SB_BP_BLR_LEN, SB_BP_BLR_RADIUS, SB_BP_BLR_INS_K, SB_BP_BLR_INS_THICK};
  for (int b = 0; b < B; ++b) {
    const std::string at = who + "building " + std::to_string(b) + ": ";
    auto range = [&](int i, double base, double *lo, double *hi) {
      const double x = desc[i].scale ? base * dmin[i] : dmin[i], y = desc[i].scale ? base * dmax[i] : dmax[i];
      *lo = std::min(x, y);
      *hi = std::max(x, y);
      return std::isfinite(x) && std::isfinite(y);
    };
    for (int f = 0; f < F; ++f) {
      if (mat_at[f] < 0) continue;
      double lo, hi;
      if (!range(mat_at[f], base_mat[(size_t)f * B + b], &lo, &hi)) return fail(SB_ERR_INVALID, at + material_field_name(f, M) + " can be drawn not finite");
      if (f < 3 * M && !(lo > 0.0)) return fail(SB_ERR_INVALID, at + material_field_name(f, M) + " must be positive, and can be drawn as " + std::to_string(lo));
      if (f == 3 * M && lo < 0.0) return fail(SB_ERR_INVALID, at + material_field_name(f, M) + " must not be negative, and can be drawn as " + std::to_string(lo));
    }
    if (!any_param) continue;
    for (int k = 0; k < SB_NUM_BUILDING_PARAMS; ++k) {
      plo[k] = phi[k] = base_bp[(size_t)k * B + b];
      if (param_at[k] >= 0 && !range(param_at[k], plo[k], &plo[k], &phi[k]))
        return fail(SB_ERR_INVALID, at + building_param_name(k) + " can be drawn not finite");
    }
    auto drawn = [&](std::initializer_list<int> ks) { return std::any_of(ks.begin(), ks.end(), [&](int k) { return param_at[k] >= 0; }); };
    for (const int k : positive)
      if (param_at[k] >= 0 && !(plo[k] > 0.0))
        return fail(SB_ERR_INVALID, at + building_param_name(k) + " must be positive, and can be drawn as " + std::to_string(plo[k]));
    if (drawn({SB_BP_W_PROD, SB_BP_W_COST, SB_BP_W_CARBON}) && !(plo[SB_BP_W_PROD] + plo[SB_BP_W_COST] + plo[SB_BP_W_CARBON] > 0.0))
      return fail(SB_ERR_INVALID, at + "w_prod + w_cost + w_carbon must be positive at their smallest draws");
    if (drawn({SB_BP_AHU_HEAT_SP, SB_BP_AHU_COOL_SP}) && plo[SB_BP_AHU_COOL_SP] <= phi[SB_BP_AHU_HEAT_SP]) // air_handler.py:60-64
      return fail(SB_ERR_INVALID, at + (param_at[SB_BP_AHU_HEAT_SP] >= 0 ? "ahu_heat_sp" : "ahu_cool_sp") +
                                      ": the largest possible ahu_heat_sp " + std::to_string(phi[SB_BP_AHU_HEAT_SP]) +
                                      " must be below the smallest possible ahu_cool_sp " + std::to_string(plo[SB_BP_AHU_COOL_SP]));
    if (drawn({SB_BP_COMFORT_LO, SB_BP_COMFORT_HI}) && phi[SB_BP_COMFORT_LO] > plo[SB_BP_COMFORT_HI]) // setpoint_schedule.py:66-75
      return fail(SB_ERR_INVALID, at + "comfort_lo: comfort_temp_window[0] can be drawn above comfort_temp_window[1]");
    if (drawn({SB_BP_ECO_LO, SB_BP_ECO_HI}) && phi[SB_BP_ECO_LO] > plo[SB_BP_ECO_HI])
      return fail(SB_ERR_INVALID, at + "eco_lo: eco_temp_window[0] can be drawn above eco_temp_window[1]");
  }
  // nothing refused: from here on the handle changes
  SB_CHECK(drop_randomization(h));
  if (any_param && !h->bp.p) { // as sb_set_building_params: a table selects the per-building code paths
    SB_HIP(hipMalloc((void **)&h->bp.p, base_bp.size() * sizeof(double)));
    SB_CHECK(fill_params(h, h->bp.p, nullptr));
    SB_HIP(hipDeviceSynchronize());
    h->d.bp = h->bp.p;
    h->rz_own_bp = !had_table;
  }
  std::vector<double> base((size_t)n_fields * B);
  for (int i = 0; i < n_fields; ++i) {
    const std::vector<double> &src = desc[i].material ? base_mat : base_bp;
    std::copy_n(src.begin() + (size_t)desc[i].row * B, B, base.begin() + (size_t)i * B);
  }
  const size_t desc_bytes = desc.size() * sizeof(RandField);
  std::vector<unsigned char> blob(desc_bytes + std::max<size_t>(choices.size(), 1) * sizeof(double));
  std::memcpy(blob.data(), desc.data(), desc_bytes);
  if (!choices.empty()) std::memcpy(blob.data() + desc_bytes, choices.data(), choices.size() * sizeof(double));
  SB_CHECK(upload(h->rz_desc, blob.data(), blob.size()));
  SB_CHECK(upload(h->rz_base, base.data(), base.size()));
  SB_CHECK(alloc_zero(h->rz_draws.episode, (size_t)B));
  h->rz_choices_at = desc_bytes;
  h->rz_base_bp = std::move(base_bp);
  h->rz_base_mat = std::move(base_mat);
  h->rz_n_fields = n_fields;
  h->rz_materials = any_mat;
  h->rz_draws.seed = seed;
  h->rz_draws.first = first_building;
  h->rz_draws.attached = true;
  return SB_OK;
}

int sb_randomization_detach(sb_handle *h) {
  if (!h) return fail(SB_ERR_INVALID, "sb_randomization_detach: null handle");
  if (!h->rz_draws.attached) return SB_OK;
  SB_ON_DEVICE(h->device);
  SB_CHECK(idle_device("sb_randomization_detach: "));
  return drop_randomization(h);
}

static const char *const kNoRandomization = "the handle has no randomisation (sb_randomization_attach)";

int sb_randomization_episodes_get(sb_handle *h, int32_t *out_dev, void *stream) {
  return episodes_get(h, &sb_handle::rz_draws, "sb_randomization_episodes_get", kNoRandomization, out_dev, (hipStream_t)stream);
}

int sb_randomization_episodes_set(sb_handle *h, const int32_t *in_dev, void *stream) {
  SB_CHECK(episodes_set(h, &sb_handle::rz_draws, "sb_randomization_episodes_set", kNoRandomization, in_dev, (hipStream_t)stream));
  SB_ON_DEVICE(h->device);
  SB_CHECK(launch_randomize(h, nullptr, 1, (hipStream_t)stream)); // the rows in force for these counters
  if (h->rz_materials) SB_CHECK(launch_class_coef(h, nullptr, (hipStream_t)stream));
  return SB_OK;
}

int sb_get_building_params(sb_handle *h, double *out_dev, void *stream) {
  if (!h || !out_dev) return fail(SB_ERR_INVALID, "sb_get_building_params: null argument");
  SB_ON_DEVICE(h->device);
  if (!h->d.bp) return fill_params(h, out_dev, (hipStream_t)stream);
  SB_HIP(hipMemcpyAsync(out_dev, h->d.bp, (size_t)SB_NUM_BUILDING_PARAMS * h->d.B * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SB_OK;
}

int sb_get_building_materials(sb_handle *h, double *out_dev, void *stream) {
  if (!h || !out_dev) return fail(SB_ERR_INVALID, "sb_get_building_materials: null argument");
  if (!h->materials)
    return fail(SB_ERR_UNSUPPORTED, "sb_get_building_materials: the handle has no materials per building (sb_create_materials)");
  SB_ON_DEVICE(h->device);
  SB_HIP(hipMemcpyAsync(out_dev, h->mat_tab.p, (size_t)(3 * h->mat_slots + 1) * h->d.B * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SB_OK;
}

} // extern "C"
