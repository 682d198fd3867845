"""ctypes binding of the C ABI in include/sbsim_amd.h (host code stays Python; HIP does the work).

There is deliberately no fallback: if the shared library is missing or no MI355X is
visible the constructors raise.  Nothing in this package imports ``oracle``."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SBSIM_LIB") or os.path.join(_HERE, "libsbsim_amd.so")

SB_NUM_ACTIONS = 2     # the SB1 action set; sb_params.n_actions is the width of an action row
SB_ACTION_KEEP = -3.0e38   # sb_step_in.actions_native: this column leaves its field alone
SB_NUM_AUX = 7
SB_ABI_VERSION = 8   # include/sbsim_amd.h
# sb_action_kind
SB_ACT_BOILER_SUPPLY_WATER_SETPOINT, SB_ACT_AHU_SUPPLY_AIR_HEATING_SETPOINT = 0, 1
SB_ACT_AHU_SUPPLY_AIR_COOLING_SETPOINT, SB_ACT_VAV_SUPPLY_AIR_DAMPER_COMMAND = 2, 3
SB_INFO_STRIDE = 24
SB_NUM_SCALARS = 16

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)


class PlanDesc(C.Structure):
  _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("Z", C.c_int32), ("n_classes", C.c_int32),
              ("cell_class", C.POINTER(C.c_uint8)), ("class_coef", _dp), ("class_zone", _ip),
              ("zone_off", _ip), ("zone_cells", _ip)]


PARAM_FIELDS = [
    ("dt", C.c_double), ("conv_threshold", C.c_double), ("iter_limit", C.c_int32),
    ("ahu_has_weather", C.c_int32),
    ("vav_max_air_flow", C.c_double), ("vav_max_water_flow", C.c_double),
    ("ahu_recirc", C.c_double), ("ahu_heat_sp", C.c_double), ("ahu_cool_sp", C.c_double),
    ("ahu_dp", C.c_double), ("ahu_eff", C.c_double), ("ahu_max_flow", C.c_double),
    ("blr_setpoint", C.c_double), ("blr_head", C.c_double), ("blr_pump_eff", C.c_double),
    ("blr_heating_rate", C.c_double), ("blr_cooling_rate", C.c_double),
    ("blr_conv", C.c_double), ("blr_len", C.c_double), ("blr_radius", C.c_double),
    ("blr_capacity", C.c_double), ("blr_ins_k", C.c_double), ("blr_ins_thick", C.c_double),
    ("comfort_lo", C.c_double), ("comfort_hi", C.c_double), ("eco_lo", C.c_double),
    ("eco_hi", C.c_double),
    ("max_prod", C.c_double), ("min_prod", C.c_double), ("max_elec", C.c_double),
    ("max_gas", C.c_double), ("prod_delta", C.c_double), ("prod_stiff", C.c_double),
    ("w_prod", C.c_double), ("w_cost", C.c_double), ("w_carbon", C.c_double),
    ("n_actions", C.c_int32), ("act_kind", C.POINTER(C.c_int32)), ("act_zone", C.POINTER(C.c_int32)),
    ("act_lo", C.POINTER(C.c_double)), ("act_hi", C.POINTER(C.c_double)),
]


class Params(C.Structure):
  _fields_ = PARAM_FIELDS


# enum sb_building_param: the double fields of sb_params from vav_max_air_flow to w_carbon, in declaration order (what
# sb_set_building_params sets per building); index = the enum value
BUILDING_PARAM_FIELDS = tuple(name for name, _ in PARAM_FIELDS[PARAM_FIELDS.index(("vav_max_air_flow", C.c_double)):
                                                                PARAM_FIELDS.index(("w_carbon", C.c_double)) + 1])
SB_NUM_BUILDING_PARAMS = len(BUILDING_PARAM_FIELDS)   # 32


class ObsLayout(C.Structure):
  _fields_ = [("n_obs", C.c_int32), ("col_ahu", C.c_int32), ("col_boiler", C.c_int32),
              ("col_aux", C.c_int32), ("col_zone", _ip), ("mean", _dp), ("sigma", _dp),
              ("n_src", C.c_int32), ("n_hist", C.c_int32), ("src_dest", _ip), ("hist_col", _ip),
              ("hist_off", _ip), ("hist_bins", _dp), ("hist_normalize", C.c_int32)]


class StepIn(C.Structure):
  _fields_ = [("t_amb_now", C.c_double), ("t_amb_next", C.c_double), ("t_amb_dev", C.c_void_p),
              ("weather_lohi_dev", C.c_void_p), ("weather_f_now", C.c_double), ("weather_f_next", C.c_double),
              ("weather_times_dev", C.c_void_p), ("weather_tempf_dev", C.c_void_p), ("weather_offset_dev", C.c_void_p),
              ("weather_n", C.c_int32), ("weather_t_now", C.c_double), ("weather_t_next", C.c_double),
              ("comfort_now", C.c_int32), ("comfort_prev", C.c_int32),
              ("comfort_next", C.c_int32), ("has_action", C.c_int32), ("reject_dev", C.c_void_p), ("actions_native", C.c_int32),
              ("occupancy", C.c_double), ("occupancy_dev", C.c_void_p),
              ("occupancy_bz_dev", C.c_void_p), ("num_occupants_dev", C.c_void_p), ("occupancy_norm", C.c_double),
              ("e_price", C.c_double), ("e_carbon", C.c_double),
              ("g_price", C.c_double), ("g_carbon", C.c_double),
              ("aux", C.c_float * SB_NUM_AUX)]


class OccupancyConfig(C.Structure):
  _fields_ = [("zone_assignment", C.c_int32), ("earliest_arrival_hour", C.c_int32),
              ("latest_arrival_hour", C.c_int32), ("earliest_departure_hour", C.c_int32),
              ("latest_departure_hour", C.c_int32), ("time_step_sec", C.c_double),
              ("seed", C.c_uint64), ("first_building", C.c_int64)]


class TapBld(C.Structure):   # sb_tap_bld
  _fields_ = [("t_now", C.c_double), ("t_next", C.c_double), ("heat_sp", C.c_double), ("cool_sp", C.c_double),
              ("blr_sp", C.c_double), ("t_sa", C.c_double), ("ahu_flow", C.c_double), ("blr_flow", C.c_double),
              ("blr_return", C.c_double), ("ahu_count", C.c_int32), ("blr_count", C.c_int32),
              ("tank", C.c_double), ("tank_change", C.c_double), ("duration", C.c_double), ("rejected", C.c_int32)]


class PbTime(C.Structure):
  _fields_ = [("seconds", C.c_int64), ("nanos", C.c_int32)]


class LaunchInfo(C.Structure):
  _fields_ = [("waves_per_workgroup", C.c_int32), ("workgroups", C.c_int32),
              ("lds_bytes_per_workgroup", C.c_int32), ("sweep_steps", C.c_int32),
              ("algorithmic_bytes_per_env_step", C.c_int64),
              ("state_bytes_per_env_step", C.c_int64),
              ("path", C.c_int32), ("waves_per_building", C.c_int32),
              ("kernel", C.c_int32), ("reserved", C.c_int32)]


SB_STATE_NUM_SCALARS = 20   # doubles per row of sb_state_view.scal


class StateView(C.Structure):   # sb_state_view: DEVICE pointers of one snapshot
  _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("grid", C.c_void_p), ("zone", C.c_void_p),
              ("mode", C.c_void_p), ("scal", C.c_void_p), ("nsw", C.c_void_p), ("occ", C.c_void_p)]


class StateClock(C.Structure):   # sb_state_clock
  _fields_ = [("occ_queries", C.c_uint32), ("conv_calls", C.c_uint32), ("steps_since_reset", C.c_int32),
              ("was_reset", C.c_int32)]


SB_REWARD_REGRET, SB_REWARD_SETPOINT_ENERGY_CARBON = 0, 1   # sb_reward_kind


class RewardConfig(C.Structure):   # sb_reward_config
  _fields_ = [("kind", C.c_int32), ("energy_cost_weight", C.c_double), ("carbon_cost_weight", C.c_double),
              ("carbon_cost_factor", C.c_double), ("normalizer_shift", C.c_double), ("normalizer_scale", C.c_double)]


# enum sb_clock_field: the fields of one row of sb_clock_attach's table, in order
CLOCK_FIELDS = ("t_amb", "weather_f", "weather_t", "comfort") + tuple(f"aux{i}" for i in range(SB_NUM_AUX)) + (
    "occupancy", "e_price", "e_carbon", "g_price", "g_carbon", "occ_hour", "occ_workday", "occ_hour5", "occ_workday5")
SB_CLOCK_FIELDS = len(CLOCK_FIELDS)   # 20
SB_CLOCK_MAX_ROWS = 1 << 22

SB_JACOBI_COEFS = 16   # floats per class row of sb_jacobi_desc.class_f32


class JacobiDesc(C.Structure):   # sb_jacobi_desc
  _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n_classes", C.c_int32), ("reserved", C.c_int32),
              ("cell_class", C.POINTER(C.c_uint8)), ("class_f32", _fp), ("class_diffuser", _dp), ("class_zone", _ip)]


class StructDesc(C.Structure):   # sb_struct_desc
  _fields_ = [("n_slots", C.c_int32), ("reserved", C.c_int32), ("class_desc", _ip), ("class_diffuser", _dp),
              ("slot_table", _dp), ("h_conv", C.c_double), ("dx", C.c_double), ("dx2", C.c_double), ("zh", C.c_double)]


class InitialConditionsDesc(C.Structure):   # sb_initial_conditions (HOST pointers)
  _fields_ = [("grids", _dp), ("n_grids", C.c_int32), ("has_jitter", C.c_int32), ("grid_of", _ip), ("initial_temp", _dp),
              ("offset", _dp), ("jitter_lo", C.c_double), ("jitter_hi", C.c_double), ("seed", C.c_uint64),
              ("first_building", C.c_int64)]


class RandField(C.Structure):   # sb_rand_field (choices: a HOST pointer)
  _fields_ = [("id", C.c_int32), ("kind", C.c_int32), ("scale", C.c_int32), ("n_choices", C.c_int32),
              ("lo", C.c_double), ("hi", C.c_double), ("choices", _dp)]


class StartField(C.Structure):   # sb_start_field (choices: a HOST pointer)
  _fields_ = [("present", C.c_int32), ("kind", C.c_int32), ("n_choices", C.c_int32), ("step", C.c_int32),
              ("lo", C.c_double), ("hi", C.c_double), ("choices", _dp)]


class EpisodeStartsDesc(C.Structure):   # sb_episode_starts (the two weather arrays: DEVICE pointers)
  _fields_ = [("field", StartField * 4), ("relative", C.c_int32), ("reserved", C.c_int32),
              ("weather_lohi_dev", C.c_void_p), ("weather_offset_dev", C.c_void_p), ("seed", C.c_uint64),
              ("first_building", C.c_int64)]


class Telemetry(C.Structure):   # sb_telemetry (HOST pointers)
  _fields_ = [("traces", _dp), ("trace_of", _ip), ("first_row", _ip), ("zone_weights", _dp), ("actions", C.POINTER(C.c_float)),
              ("n_traces", C.c_int32), ("n_rows", C.c_int32), ("n_actions", C.c_int32), ("per_zone", C.c_int32)]


# sb_sweep_kernel
SWEEP_KERNELS = {0: "k_sweep_lds", 1: "k_sweep_reg", 2: "k_sweep_reg (two wavefronts)", 3: "k_sweep_roll", 4: "k_sweep_two",
                 5: "k_sweep_band", 6: "k_sweep_stream", 7: "k_sweep_jacobi"}
SB_KERNEL_JACOBI = 7


EXPORTS = ("sb_abi_version", "sb_has_experimental_kernels", "sb_last_error", "sb_plan_info", "sb_create", "sb_destroy", "sb_get_launch_info",
           "sb_reset", "sb_observe", "sb_observe_occupancy", "sb_occupancy_attach", "sb_occupancy_peek", "sb_convection_attach", "sb_step", "sb_step_phases", "sb_get_temps", "sb_set_temps", "sb_get_zone_temps",
           "sb_get_scalars", "sb_get_modes", "sb_get_zone_power", "sb_debug_phase_cycles",
           "sb_floorplan_padded_shape", "sb_floorplan_preprocess", "sb_floorplan_diffusers", "sb_debug_numpy_choice", "sb_pb_reward_info", "sb_pb_reward_response",
           "sb_pb_observation_response", "sb_pb_action_response", "sb_shard_append", "sb_pb_device_info",
           "sb_pb_zone_info", "sb_pb_variable_info", "sb_record_append", "sb_tap_pre", "sb_tap_post",
           "sb_state_save", "sb_state_load", "sb_create_jacobi", "sb_tap_jacobi", "sb_set_building_params",
           "sb_set_reward_function", "sb_create_materials", "sb_plan_info_materials", "sb_set_building_materials",
           "sb_get_building_coef", "sb_clock_attach", "sb_clock_seek", "sb_clock_detach", "sb_observe_step_in",
           "sb_debug_plan_digest", "sb_reset_buildings", "sb_observe_buildings", "sb_occupancy_attach_groups",
           "sb_spatial_shape", "sb_spatial_attach", "sb_spatial",
           "sb_convection_attach_seeded", "sb_convection_rng_get", "sb_convection_rng_set", "sb_convection_apply",
           "sb_initial_conditions_attach", "sb_initial_conditions_detach", "sb_initial_conditions_episodes_get",
           "sb_initial_conditions_episodes_set",
           "sb_randomization_attach", "sb_randomization_detach", "sb_randomization_episodes_get",
           "sb_randomization_episodes_set", "sb_get_building_params", "sb_get_building_materials",
           "sb_episode_starts_attach", "sb_episode_starts_detach", "sb_episode_starts_episodes_get",
           "sb_episode_starts_episodes_set", "sb_episode_starts_values_get", "sb_clock_set_offsets",
           "sb_episode_metrics_attach", "sb_episode_metrics_detach", "sb_episode_metrics_get", "sb_episode_metrics_set",
           "sb_telemetry_attach", "sb_telemetry_detach", "sb_telemetry_get", "sb_telemetry_set", "sb_telemetry_zone_get",
           "sb_telemetry_zone_set", "sb_telemetry_actions")
# entries a library of ABI 8 may predate (load() binds them when present; state_entry() / jacobi_entry() raise without them)
STATE_ENTRIES = ("sb_state_save", "sb_state_load")
JACOBI_ENTRIES = ("sb_create_jacobi", "sb_tap_jacobi")
BUILDING_PARAM_ENTRIES = ("sb_set_building_params",)
REWARD_ENTRIES = ("sb_set_reward_function",)
CLOCK_ENTRIES = ("sb_clock_attach", "sb_clock_seek", "sb_clock_detach", "sb_observe_step_in")
PLAN_DIGEST_ENTRIES = ("sb_debug_plan_digest",)
EPISODES_ENTRIES = ("sb_reset_buildings", "sb_observe_buildings")
OCCUPANCY_ENTRIES = ("sb_occupancy_attach_groups",)
SPATIAL_ENTRIES = ("sb_spatial_shape", "sb_spatial_attach", "sb_spatial")
CONVECTION_SEEDED_ENTRIES = ("sb_convection_attach_seeded", "sb_convection_rng_get", "sb_convection_rng_set", "sb_convection_apply")
SB_CONV_RNG_WORDS = 625                  # a building's row of the seeded generators: MT19937's 624 words, then the index
SB_CONV_SEEDED_MAX_WORKGROUPS = 4096     # k_convect_seeded's grid cap (conv_seeded.hip): buildings beyond it take the grid stride
INITIAL_CONDITIONS_ENTRIES = ("sb_initial_conditions_attach", "sb_initial_conditions_detach",
                              "sb_initial_conditions_episodes_get", "sb_initial_conditions_episodes_set")
SB_INITIAL_CONDITIONS_TAG = 0xC1C00000   # include/sbsim_amd.h: the last counter word of the start temperatures' draws
RANDOMIZATION_ENTRIES = ("sb_randomization_attach", "sb_randomization_detach", "sb_randomization_episodes_get",
                         "sb_randomization_episodes_set", "sb_get_building_params", "sb_get_building_materials")
SB_RANDOMIZATION_TAG = 0xE9150000        # include/sbsim_amd.h: the redraws' last counter word is this | the field's id
SB_RAND_MATERIAL = 0x100                 # id of material field f: SB_RAND_MATERIAL + f
SB_RAND_MAX_CHOICES = 65536
SB_RAND_UNIFORM, SB_RAND_CHOICE = 0, 1   # sb_rand_kind
SB_RAND_BLOCKS_PER_CU, SB_RAND_THREADS = 8, 256   # the draw kernels' grid cap (sb_host.h: draw_blocks): work beyond it takes the grid stride
EPISODE_STARTS_ENTRIES = ("sb_episode_starts_attach", "sb_episode_starts_detach", "sb_episode_starts_episodes_get",
                          "sb_episode_starts_episodes_set", "sb_episode_starts_values_get", "sb_clock_set_offsets")
SB_EPISODE_STARTS_TAG = 0xE5A70000       # include/sbsim_amd.h: the starts' last counter word is this | sb_start_field_id
SB_RAND_UNIFORM_INT = 2                  # sb_start_field's third kind
SB_START_MAX_K = 1 << 22
SB_START_OFFSET, SB_START_WEATHER_LOW, SB_START_WEATHER_HIGH, SB_START_WEATHER_SHIFT = range(4)   # sb_start_field_id
SB_STARTS_BLOCKS_PER_CU, SB_STARTS_THREADS = SB_RAND_BLOCKS_PER_CU, SB_RAND_THREADS   # k_episode_starts' grid: the same rule
EPISODE_METRICS_ENTRIES = ("sb_episode_metrics_attach", "sb_episode_metrics_detach", "sb_episode_metrics_get",
                           "sb_episode_metrics_set")
SB_EM_FIELDS = 20                        # include/sbsim_amd.h: doubles per building of the episode totals (sb_episode_metric)
EPISODE_METRIC_NAMES = (
    "episode", "steps", "rejected_steps", "return", "accepted_return", "electrical_energy", "natural_gas_energy",
    "electricity_energy_cost", "natural_gas_energy_cost", "carbon_emitted", "total_occupancy", "productivity_regret",
    "normalized_productivity_regret", "normalized_energy_cost", "normalized_carbon_emission", "productivity_reward",
    "sweeps", "unconverged_steps", "zone_temp_min", "zone_temp_max")
TELEMETRY_ENTRIES = ("sb_telemetry_attach", "sb_telemetry_detach", "sb_telemetry_get", "sb_telemetry_set",
                     "sb_telemetry_zone_get", "sb_telemetry_zone_set", "sb_telemetry_actions")
SB_TL_FIELDS = 13                        # include/sbsim_amd.h: doubles per building of the telemetry scores (sb_telemetry_score)
SB_TL_ZONE_FIELDS = 4                    # ... and per zone of the per-zone tables
TELEMETRY_SCORE_NAMES = (
    "episode", "steps", "samples", "missing", "sum_err", "sum_abs_err", "sum_sq_err", "max_abs_err", "max_abs_row",
    "max_abs_zone", "weighted_abs_err", "weighted_sq_err", "weight_sum")
TELEMETRY_ZONE_SCORE_NAMES = ("samples", "sum_err", "sum_abs_err", "sum_sq_err")
MATERIALS_ENTRIES = ("sb_create_materials", "sb_plan_info_materials", "sb_set_building_materials", "sb_get_building_coef")

_lib = None


class SbsimError(RuntimeError):
  pass


def load():
  """Loads libsbsim_amd.so; raises if it has not been built (no silent fallback)."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise SbsimError(
        f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950).  sbsim_amd has no CPU fallback.")
  # torch FIRST: it ships its own HIP runtime, and the device memory this library works on is torch's.  Loaded before torch,
  # the library binds the system's libamdhip64 instead -- a second runtime in the process that sees no device
  # (`sb_create: no HIP device visible` after __graft_entry__.build() and smoke() in one process)
  import torch  # noqa: F401
  L = C.CDLL(LIB_PATH)
  vp = C.c_void_p
  L.sb_abi_version.restype = C.c_int
  if L.sb_abi_version() != SB_ABI_VERSION:   # a stale library would read these structs with another layout
    raise SbsimError(f"{LIB_PATH} has ABI version {L.sb_abi_version()}, this package needs {SB_ABI_VERSION}: "
                     "rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
  L.sb_last_error.restype = C.c_char_p
  if hasattr(L, "sb_has_experimental_kernels"):   # (has_experimental_kernels() asks for a rebuild without it)
    L.sb_has_experimental_kernels.argtypes = []
    L.sb_has_experimental_kernels.restype = C.c_int
  L.sb_create.argtypes = [C.POINTER(PlanDesc), C.POINTER(Params), C.POINTER(ObsLayout),
                          C.c_int32, C.c_int32, C.POINTER(vp)]
  L.sb_plan_info.argtypes = [C.POINTER(PlanDesc), C.c_int32, C.c_int32, C.POINTER(LaunchInfo)]
  L.sb_destroy.argtypes = [vp]
  L.sb_destroy.restype = None
  L.sb_get_launch_info.argtypes = [vp, C.POINTER(LaunchInfo)]
  L.sb_reset.argtypes = [vp, C.c_double, vp, vp]
  L.sb_observe.argtypes = [vp, C.POINTER(C.c_float), C.c_double, vp, vp, vp]
  L.sb_observe_occupancy.argtypes = [vp, C.POINTER(C.c_float), C.c_double, vp, vp, C.c_double, vp, vp]
  L.sb_occupancy_attach.argtypes = [vp, C.POINTER(OccupancyConfig)]
  L.sb_occupancy_peek.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
  L.sb_convection_attach.argtypes = [vp, C.c_double, C.c_int32, C.c_uint64, C.c_int64, C.c_int32]
  L.sb_step.argtypes = [vp, vp, C.POINTER(StepIn), vp, vp, vp, vp]
  L.sb_step_phases.argtypes = [vp, vp, C.POINTER(StepIn), vp, vp, vp, vp, C.c_int32]
  for name in ("sb_get_temps", "sb_set_temps", "sb_get_zone_temps", "sb_get_scalars", "sb_get_modes",
               "sb_get_zone_power"):
    getattr(L, name).argtypes = [vp, vp, vp]
  L.sb_debug_phase_cycles.argtypes = [vp, C.POINTER(C.c_longlong)]
  L.sb_tap_pre.argtypes = [vp, C.c_int32, _dp, _ip, _dp, _fp, C.POINTER(StepIn), C.POINTER(TapBld), _dp, _dp, _ip]
  L.sb_tap_post.argtypes = [vp, C.c_int32, C.POINTER(TapBld), _dp, C.c_double, C.c_int32, C.POINTER(StepIn), _fp, _fp]
  cpp, fp_ = C.POINTER(C.c_char_p), C.POINTER(C.c_float)
  L.sb_pb_reward_info.argtypes = [PbTime, PbTime, C.c_char_p, C.c_char_p, C.c_int32, cpp, fp_, C.c_int32, cpp, fp_,
                                  C.c_int32, cpp, fp_, vp, C.c_int64]
  L.sb_pb_reward_response.argtypes = [fp_, PbTime, PbTime, vp, C.c_int64]
  L.sb_pb_observation_response.argtypes = [PbTime, C.c_int32, cpp, cpp, fp_, vp, vp, C.c_int64]
  L.sb_pb_action_response.argtypes = [PbTime, PbTime, C.c_int32, cpp, cpp, fp_, vp, vp, C.c_int64]
  for name in ("sb_pb_reward_info", "sb_pb_reward_response", "sb_pb_observation_response", "sb_pb_action_response"):
    getattr(L, name).restype = C.c_int64
  L.sb_shard_append.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, vp, C.c_int64]
  ip_ = C.POINTER(C.c_int32)
  L.sb_pb_device_info.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, cpp, ip_,
                                  C.c_int32, cpp, ip_, vp, C.c_int64]
  L.sb_pb_zone_info.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_float, C.c_int32, cpp, C.c_int32, C.c_int32,
                                vp, C.c_int64]
  L.sb_pb_device_info.restype = L.sb_pb_zone_info.restype = C.c_int64
  L.sb_record_append.argtypes = [C.c_char_p, vp, C.c_int64, C.c_int32]
  L.sb_pb_variable_info.argtypes = [C.c_char_p, C.c_int32, PbTime, C.c_int32, PbTime, C.c_int32, fp_, vp, C.c_int64]
  L.sb_pb_variable_info.restype = C.c_int64
  L.sb_floorplan_padded_shape.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
  L.sb_floorplan_preprocess.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, C.POINTER(C.c_int32)]
  L.sb_floorplan_diffusers.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
  L.sb_debug_numpy_choice.argtypes = [C.c_uint32, C.c_int64, C.c_int64, vp]
  if all(hasattr(L, name) for name in STATE_ENTRIES):
    L.sb_state_save.argtypes = [vp, vp, C.c_int32, C.POINTER(StateView), C.POINTER(StateClock), C.c_int32, vp]
    L.sb_state_load.argtypes = [vp, vp, C.POINTER(StateView), C.POINTER(StateClock), C.c_int32, vp]
  if all(hasattr(L, name) for name in JACOBI_ENTRIES):
    L.sb_create_jacobi.argtypes = [C.POINTER(PlanDesc), C.POINTER(JacobiDesc), C.POINTER(Params), C.POINTER(ObsLayout),
                                   C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sb_tap_jacobi.argtypes = [vp, C.c_int32, _fp, _fp, _dp, _fp, _ip, _ip]
  if all(hasattr(L, name) for name in BUILDING_PARAM_ENTRIES):
    L.sb_set_building_params.argtypes = [vp, C.c_int32, vp, vp, vp]
  if all(hasattr(L, name) for name in REWARD_ENTRIES):
    L.sb_set_reward_function.argtypes = [vp, C.POINTER(RewardConfig)]
  if all(hasattr(L, name) for name in MATERIALS_ENTRIES):
    L.sb_create_materials.argtypes = [C.POINTER(PlanDesc), C.POINTER(StructDesc), C.POINTER(Params), C.POINTER(ObsLayout),
                                      C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sb_plan_info_materials.argtypes = [C.POINTER(PlanDesc), C.c_int32, C.c_int32, C.POINTER(LaunchInfo)]
    L.sb_set_building_materials.argtypes = [vp, C.c_int32, vp, vp, vp]
    L.sb_get_building_coef.argtypes = [vp, vp, vp]
  if all(hasattr(L, name) for name in CLOCK_ENTRIES):
    L.sb_clock_attach.argtypes = [vp, vp, C.c_int32, C.c_int32, vp]
    L.sb_clock_seek.argtypes = [vp, C.c_int32, C.c_int32]
    L.sb_clock_detach.argtypes = [vp]
    L.sb_observe_step_in.argtypes = [vp, C.POINTER(StepIn), vp, vp]
  if all(hasattr(L, name) for name in EPISODES_ENTRIES):
    L.sb_reset_buildings.argtypes = [vp, vp, C.c_int32, C.c_double, vp, vp]
    L.sb_observe_buildings.argtypes = [vp, vp, C.POINTER(StepIn), vp, vp]
  if all(hasattr(L, name) for name in OCCUPANCY_ENTRIES):
    L.sb_occupancy_attach_groups.argtypes = [vp, C.POINTER(OccupancyConfig), C.c_int32, vp]
  if all(hasattr(L, name) for name in SPATIAL_ENTRIES):
    L.sb_spatial_shape.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sb_spatial_attach.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.sb_spatial.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
  if all(hasattr(L, name) for name in CONVECTION_SEEDED_ENTRIES):
    L.sb_convection_attach_seeded.argtypes = [vp, C.c_double, C.c_int32, C.POINTER(C.c_uint64), C.c_int32]
    L.sb_convection_rng_get.argtypes = [vp, vp, vp]
    L.sb_convection_rng_set.argtypes = [vp, vp, vp]
    L.sb_convection_apply.argtypes = [vp, vp]
  if all(hasattr(L, name) for name in INITIAL_CONDITIONS_ENTRIES):
    L.sb_initial_conditions_attach.argtypes = [vp, C.POINTER(InitialConditionsDesc)]
    L.sb_initial_conditions_detach.argtypes = [vp]
    L.sb_initial_conditions_episodes_get.argtypes = [vp, vp, vp]
    L.sb_initial_conditions_episodes_set.argtypes = [vp, vp, vp]
  if all(hasattr(L, name) for name in RANDOMIZATION_ENTRIES):
    L.sb_randomization_attach.argtypes = [vp, C.POINTER(RandField), C.c_int32, C.c_uint64, C.c_int64]
    L.sb_randomization_detach.argtypes = [vp]
    for name in RANDOMIZATION_ENTRIES[2:]:
      getattr(L, name).argtypes = [vp, vp, vp]
  if all(hasattr(L, name) for name in EPISODE_STARTS_ENTRIES):
    L.sb_episode_starts_attach.argtypes = [vp, C.POINTER(EpisodeStartsDesc)]
    L.sb_episode_starts_detach.argtypes = [vp]
    L.sb_episode_starts_episodes_get.argtypes = [vp, vp, vp]
    L.sb_episode_starts_episodes_set.argtypes = [vp, vp, vp]
    L.sb_episode_starts_values_get.argtypes = [vp, vp, vp, vp]
    L.sb_clock_set_offsets.argtypes = [vp, vp, vp]
  if all(hasattr(L, name) for name in EPISODE_METRICS_ENTRIES):
    L.sb_episode_metrics_attach.argtypes = [vp]
    L.sb_episode_metrics_detach.argtypes = [vp]
    L.sb_episode_metrics_get.argtypes = [vp, vp, vp, vp]
    L.sb_episode_metrics_set.argtypes = [vp, vp, vp, vp]
  if all(hasattr(L, name) for name in TELEMETRY_ENTRIES):
    L.sb_telemetry_attach.argtypes = [vp, C.POINTER(Telemetry)]
    L.sb_telemetry_detach.argtypes = [vp]
    for name in ("sb_telemetry_get", "sb_telemetry_set", "sb_telemetry_zone_get", "sb_telemetry_zone_set"):
      getattr(L, name).argtypes = [vp, vp, vp, vp]
    L.sb_telemetry_actions.argtypes = [vp, vp, vp]
  if all(hasattr(L, name) for name in PLAN_DIGEST_ENTRIES):
    L.sb_debug_plan_digest.argtypes = [C.POINTER(PlanDesc), C.c_int32, C.POINTER(C.c_uint64)]
  _lib = L
  return L


def entry(name: str):
  """The entry `name` of the loaded library.  A library built before it existed (same ABI version) gets the usual
  request to rebuild -- an SbsimError, not ctypes' bare AttributeError."""
  L = load()
  if not hasattr(L, name):
    raise SbsimError(f"{LIB_PATH} has no {name}: rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
  return getattr(L, name)


def state_entry(name: str):
  """The state-snapshot entry `name` (sb_state_save, sb_state_load): see entry()."""
  return entry(name)


def jacobi_entry(name: str):
  """The Jacobi-solver entry `name` (sb_create_jacobi, sb_tap_jacobi): see entry()."""
  return entry(name)


def reward_entry(name: str):
  """The reward-function entry `name` (sb_set_reward_function): see entry()."""
  return entry(name)


def materials_entry(name: str):
  """The per-building-materials entry `name` (sb_create_materials, sb_plan_info_materials, sb_set_building_materials,
  sb_get_building_coef): see entry()."""
  return entry(name)


def clock_entry(name: str):
  """The per-building-calendar entry `name` (sb_clock_attach, sb_clock_seek, sb_clock_detach, sb_observe_step_in): see
  entry()."""
  return entry(name)


def occupancy_entry(name: str):
  """The occupancy-groups entry `name` (sb_occupancy_attach_groups): see entry()."""
  return entry(name)


def episodes_entry(name: str):
  """The per-building-episodes entry `name` (sb_reset_buildings, sb_observe_buildings): see entry()."""
  return entry(name)


def spatial_entry(name: str):
  """The spatial-outputs entry `name` (sb_spatial_shape, sb_spatial_attach, sb_spatial): see entry()."""
  return entry(name)


def convection_seeded_entry(name: str):
  """The seeded-convection entry `name` (sb_convection_attach_seeded, sb_convection_rng_get, sb_convection_rng_set,
  sb_convection_apply): see entry()."""
  return entry(name)


def initial_conditions_entry(name: str):
  """The start-temperatures entry `name` (sb_initial_conditions_attach, sb_initial_conditions_detach,
  sb_initial_conditions_episodes_get, sb_initial_conditions_episodes_set): see entry()."""
  return entry(name)


def randomization_entry(name: str):
  """The episode-randomisation entry `name` (sb_randomization_attach, sb_randomization_detach,
  sb_randomization_episodes_get, sb_randomization_episodes_set, sb_get_building_params, sb_get_building_materials): see
  entry()."""
  return entry(name)


def episode_starts_entry(name: str):
  """The episode-starts entry `name` (sb_episode_starts_attach, sb_episode_starts_detach, sb_episode_starts_episodes_get,
  sb_episode_starts_episodes_set, sb_episode_starts_values_get, sb_clock_set_offsets): see entry()."""
  return entry(name)


def episode_metrics_entry(name: str):
  """The episode-totals entry `name` (sb_episode_metrics_attach, sb_episode_metrics_detach, sb_episode_metrics_get,
  sb_episode_metrics_set): see entry()."""
  return entry(name)


def telemetry_entry(name: str):
  """The telemetry entry `name` (one of TELEMETRY_ENTRIES): see entry()."""
  return entry(name)


def has_experimental_kernels() -> bool:
  """sb_has_experimental_kernels(): whether the library was built with SBSIM_BUILD_EXPERIMENTAL=1 (see entry())."""
  return bool(entry("sb_has_experimental_kernels")())


def check(rc: int, what: str) -> None:
  if rc != 0:
    msg = load().sb_last_error()
    raise SbsimError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
