"""Vectorised drop-in for sbsim's RL environment: ``reset()`` / ``step(action)`` over B buildings.

Mirrors ``smart_control/environment/environment.py`` ``Environment`` (a TF-Agents
``PyEnvironment``) for the simulator-backed configuration of
``configs/resources/sb1/sim_config.gin``, with a leading batch axis:

    reference                                   here
    ---------                                   ----
    Environment._reset()  (:1165-1212)          BatchedEnvironment.reset()
    Environment._step(a)  (:1228-1370)          BatchedEnvironment.step(a)      a: [B, A] in [-1, 1]
    action_spec()/observation_spec() (:1215-1221)   same names; shapes without the batch axis
    steps_per_episode (:522), current_simulation_timestamp (:816), discount_factor

Every step is one call through the C ABI (include/sbsim_amd.h: sb_step = three HIP kernel
launches on the current torch stream); observations, rewards and actions stay in HBM as torch
tensors.  Calendar,
weather, occupancy and tariffs are resolved on the host once per step (all buildings share
the simulator clock) by ``sbsim_amd.host_inputs``.  Episode bookkeeping follows
``environment.py:427-435,1311-1368``: an episode is N transitions plus one terminal step;
a ``step`` after termination resets.  Action rejection (``RejectionSimulatorBuilding``)
and metrics writing are out of scope.
"""
from __future__ import annotations

import collections
import copy
import ctypes as C
import dataclasses
import datetime as dt
import hashlib
import math
import operator
import os
import pickle
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ffi, host_inputs
from .floorplan import CompiledPlan, FloorPlan, Materials

TimeStep = collections.namedtuple("TimeStep", ["step_type", "reward", "discount", "observation"])
STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2   # tf_agents.trajectories.time_step.StepType


@dataclasses.dataclass(frozen=True)
class ArraySpec:
  shape: Tuple[int, ...]
  dtype: np.dtype
  name: str
  minimum: Optional[float] = None
  maximum: Optional[float] = None


# air_handler.py:66-95, boiler.py:69-79, vav.py:54-64: observable fields in sorted order.
_AHU_FIELDS = ("cooling_request_count", "differential_pressure_setpoint",
               "discharge_fan_speed_percentage_command", "outside_air_flowrate_sensor",
               "outside_air_temperature_sensor", "supply_air_cooling_temperature_setpoint",
               "supply_air_flowrate_sensor", "supply_air_heating_temperature_setpoint",
               "supply_fan_speed_percentage_command")
_BOILER_FIELDS = ("heating_request_count", "supply_water_setpoint",
                  "supply_water_temperature_sensor")
_VAV_FIELDS = ("supply_air_damper_percentage_command", "supply_air_flowrate_setpoint",
               "zone_air_temperature_sensor")
_AUX_FIELDS = ("hod_cos_000", "hod_sin_000", "dow_cos_000", "dow_sin_000",
               "comfort_mode_now", "comfort_mode_soon", "num_occupants")
ACTION_NAMES = ("supply_water_setpoint", "supply_air_heating_temperature_setpoint")
# settable fields of the simulated devices (boiler.py:81-85, air_handler.py:97-104, vav.py:65-69) -> sb_action_kind
ACTION_KINDS = {
    "supply_water_setpoint": _ffi.SB_ACT_BOILER_SUPPLY_WATER_SETPOINT,
    "supply_air_heating_temperature_setpoint": _ffi.SB_ACT_AHU_SUPPLY_AIR_HEATING_SETPOINT,
    "supply_air_cooling_temperature_setpoint": _ffi.SB_ACT_AHU_SUPPLY_AIR_COOLING_SETPOINT,
    "supply_air_damper_percentage_command": _ffi.SB_ACT_VAV_SUPPLY_AIR_DAMPER_COMMAND,
}
ACTION_REJECTION_REWARD = float("-inf")   # environment.py:52
# sim_config.gin:164: the SB1 configuration's clock starts at a tz-aware UTC time, which the schedule
# converts to US/Pacific.  BatchedEnvironment's default start is the NAIVE 2023-07-06 07:00 of the
# reference's test scenarios and of BASELINE.json configs[0..1]; a naive time stamp is taken as UTC
# wall clock whatever `time_zone` says (setpoint_schedule.py:100-106).
SB1_START_TIMESTAMP = dt.datetime(2023, 7, 6, 7, 0, 0, tzinfo=dt.timezone.utc)


@dataclasses.dataclass
class SimConfig:
  """Scalar configuration: the constructor arguments of the reference's Simulator, Hvac
  devices, SetpointSchedule and SetpointEnergyCarbonRegretFunction.  ``sb1()`` gives
  ``configs/resources/sb1/sim_config.gin:23-250``."""
  time_step_sec: float = 300.0
  convergence_threshold: float = 0.1
  iteration_limit: int = 100
  cv_size_cm: float = 10.0
  floor_height_cm: float = 300.0
  initial_temp: float = 294.0
  materials: Materials = dataclasses.field(default_factory=Materials.sb1)
  # schedule
  morning_start_hour: int = 6
  evening_start_hour: int = 19
  comfort_temp_window: Tuple[float, float] = (294.0, 297.0)
  eco_temp_window: Tuple[float, float] = (289.0, 298.0)
  schedule_holidays: Tuple[int, ...] = ()
  time_zone: str = "US/Pacific"
  # devices
  vav_max_air_flow_rate: float = 0.035
  vav_reheat_max_water_flow_rate: float = 0.03
  ahu_recirculation: float = 0.3
  ahu_heating_air_temp_setpoint: float = 285.0
  ahu_cooling_air_temp_setpoint: float = 298.0
  ahu_fan_differential_pressure: float = 10000.0
  ahu_fan_efficiency: float = 0.9
  ahu_max_air_flow_rate: float = 8.67
  ahu_has_weather_sensor: bool = True
  boiler_reheat_water_setpoint: float = 360.0
  boiler_water_pump_differential_head: float = 6.0
  boiler_water_pump_efficiency: float = 0.98
  boiler_heating_rate: float = 0.5
  boiler_cooling_rate: float = 0.1
  boiler_convection_coefficient: float = 5.6
  boiler_tank_length: float = 2.0
  boiler_tank_radius: float = 0.5
  boiler_water_capacity: float = 1.5
  boiler_insulation_conductivity: float = 0.067
  boiler_insulation_thickness: float = 0.06
  # reward
  max_productivity_personhour_usd: float = 300.0
  min_productivity_personhour_usd: float = 100.0
  max_electricity_rate: float = 160000.0
  max_natural_gas_rate: float = 400000.0
  productivity_midpoint_delta: float = 0.5
  productivity_decay_stiffness: float = 4.3
  productivity_weight: float = 0.2
  energy_cost_weight: float = 0.4
  carbon_emission_weight: float = 0.4
  # action normalisation (bounded_action_normalizer.py; sim_config.gin:229-237)
  action_ranges: Tuple[Tuple[float, float], ...] = ((310.0, 355.0), (285.0, 300.0))
  # the action vector (environment.py:278-307,591-653: one column per (device, setpoint) of the
  # ActionConfig that has a normalizer): setpoint names, and the zone index for a VAV field.
  # Default: the SB1 set of sim_config.gin:239-242.  `action_ranges[i]` is column i's native range.
  action_names: Tuple[str, ...] = ACTION_NAMES
  action_zones: Tuple[int, ...] = ()

  @staticmethod
  def sb1() -> "SimConfig":
    return SimConfig()

  def schedule(self) -> host_inputs.SetpointSchedule:
    return host_inputs.SetpointSchedule(
        self.morning_start_hour, self.evening_start_hour, self.comfort_temp_window,
        self.eco_temp_window, set(self.schedule_holidays), self.time_zone)

  def to_params(self) -> _ffi.Params:
    p = _ffi.Params()
    p.dt, p.conv_threshold, p.iter_limit = self.time_step_sec, self.convergence_threshold, self.iteration_limit
    p.ahu_has_weather = int(self.ahu_has_weather_sensor)
    p.vav_max_air_flow, p.vav_max_water_flow = self.vav_max_air_flow_rate, self.vav_reheat_max_water_flow_rate
    p.ahu_recirc, p.ahu_heat_sp, p.ahu_cool_sp = (self.ahu_recirculation, self.ahu_heating_air_temp_setpoint,
                                                  self.ahu_cooling_air_temp_setpoint)
    p.ahu_dp, p.ahu_eff, p.ahu_max_flow = (self.ahu_fan_differential_pressure, self.ahu_fan_efficiency,
                                           self.ahu_max_air_flow_rate)
    p.blr_setpoint, p.blr_head, p.blr_pump_eff = (self.boiler_reheat_water_setpoint,
                                                  self.boiler_water_pump_differential_head,
                                                  self.boiler_water_pump_efficiency)
    p.blr_heating_rate, p.blr_cooling_rate = self.boiler_heating_rate, self.boiler_cooling_rate
    p.blr_conv, p.blr_len, p.blr_radius = (self.boiler_convection_coefficient, self.boiler_tank_length,
                                           self.boiler_tank_radius)
    p.blr_capacity, p.blr_ins_k, p.blr_ins_thick = (self.boiler_water_capacity,
                                                    self.boiler_insulation_conductivity,
                                                    self.boiler_insulation_thickness)
    p.comfort_lo, p.comfort_hi = self.comfort_temp_window
    p.eco_lo, p.eco_hi = self.eco_temp_window
    p.max_prod, p.min_prod = self.max_productivity_personhour_usd, self.min_productivity_personhour_usd
    p.max_elec, p.max_gas = self.max_electricity_rate, self.max_natural_gas_rate
    p.prod_delta, p.prod_stiff = self.productivity_midpoint_delta, self.productivity_decay_stiffness
    p.w_prod, p.w_cost, p.w_carbon = self.productivity_weight, self.energy_cost_weight, self.carbon_emission_weight
    n = len(self.action_names)
    if n != len(self.action_ranges) or n < 1:
      raise ValueError("one native range per action, at least one action")
    for name in self.action_names:
      if name not in ACTION_KINDS:   # simulator_building.py:236-251: REJECTED_NOT_ENABLED_OR_AVAILABLE at run time
        raise ValueError(f"{name!r} is not a settable field of the simulated devices")
    p.n_actions = n
    # host arrays the struct points at (sb_create copies them; they live as long as the Params object)
    kinds = (C.c_int32 * n)(*[ACTION_KINDS[name] for name in self.action_names])
    zones = (C.c_int32 * n)(*[self.action_zones[i] if i < len(self.action_zones) else 0 for i in range(n)])
    los = (C.c_double * n)(*[float(lo) for lo, _ in self.action_ranges])
    his = (C.c_double * n)(*[float(hi) for _, hi in self.action_ranges])
    p.act_kind, p.act_zone = C.cast(kinds, C.POINTER(C.c_int32)), C.cast(zones, C.POINTER(C.c_int32))
    p.act_lo, p.act_hi = C.cast(los, C.POINTER(C.c_double)), C.cast(his, C.POINTER(C.c_double))
    p._keep_alive = (kinds, zones, los, his)
    return p


# Observation normalisation constants of sim_config.gin:252-590 that apply to simulated
# devices: field name -> (sample_mean, sample_variance).  Unknown fields get (0, 1)
# (observation_normalizer.py:57-66).
SB1_OBSERVATION_NORMALIZATION: Dict[str, Tuple[float, float]] = {
    "differential_pressure_setpoint": (83810.269540, 14889040.603647),
    "outside_air_flowrate_sensor": (3.701930, 20.300565),
    "outside_air_temperature_sensor": (291.244931, 12.904175),
    "supply_air_flowrate_sensor": (177.520026, 50499.153481),
    "supply_fan_speed_percentage_command": (26.543748, 575.094979),
    "supply_water_setpoint": (310.0, 2500.0),
    "supply_water_temperature_sensor": (321.520315, 658.413066),
    "zone_air_temperature_sensor": (190.0, 408.113303),
}


def observation_field_names(zone_names: Sequence[str], ahu_has_weather: bool,
                            ahu_id: str = "air_handler_id", boiler_id: str = "boiler_id"):
  """environment.py:543-553,783-813: (device_id, field) sorted, then auxiliary features.
  Returns (names, col_ahu, col_boiler, col_zone[Z], col_aux)."""
  devices = [(ahu_id, "ahu", -1), (boiler_id, "blr", -1)]
  devices += [(f"vav_{z}", "vav", i) for i, z in enumerate(zone_names)]
  names, col_ahu, col_blr, col_zone = [], -1, -1, [0] * len(zone_names)
  for dev_id, kind, zi in sorted(devices, key=lambda d: d[0]):
    if kind == "ahu":
      col_ahu = len(names)
      fields = [f for f in _AHU_FIELDS if ahu_has_weather or f != "outside_air_temperature_sensor"]
    elif kind == "blr":
      col_blr = len(names)
      fields = _BOILER_FIELDS
    else:
      col_zone[zi] = len(names)
      fields = _VAV_FIELDS
    names += [f"{dev_id}/{f}" for f in fields]
  col_aux = len(names)
  names += list(_AUX_FIELDS)
  return names, col_ahu, col_blr, col_zone, col_aux


def histogram_reducer_layout(source_names: Sequence[str],
                             histogram_parameters: Sequence[Tuple[str, Sequence[float]]]):
  """Output layout of the observation HistogramReducer (utils/histogram_reducer.py:204-471) in
  the field order of ``Environment._get_observation_spec_histogram_reducer``
  (environment.py:731-777): devices sorted by id, fields sorted; a reduced measurement
  contributes one column per bin (``<measurement>_h_<bin:.2f>``) where it is first met, every
  other field passes through.  ``source_names`` are the device fields ("device/field") in that
  sorted order.  Returns (names, src_dest, hist_col, hist_off, hist_bins)."""
  bins = {}
  for name, values in histogram_parameters:
    b = [float(v) for v in values]
    if len(b) < 1 or any(b[i] >= b[i + 1] for i in range(len(b) - 1)):
      raise ValueError(f"histogram bins of {name} must be ascending")
    bins[name] = b
  names: list = []
  src_dest = [0] * len(source_names)
  feature_index, hist_col, hist_off, hist_bins = {}, [], [0], []
  for i, full in enumerate(source_names):
    _, meas = full.split("/", 1)
    if meas in bins:
      if meas not in feature_index:
        feature_index[meas] = len(hist_col)
        hist_col.append(len(names))
        hist_bins += bins[meas]
        hist_off.append(len(hist_bins))
        names += [f"{meas}_h_{v:.2f}" for v in bins[meas]]
      src_dest[i] = -(feature_index[meas] + 1)
    else:
      src_dest[i] = len(names)
      names.append(full)
  return names, src_dest, hist_col, hist_off, hist_bins


@dataclasses.dataclass
class SimState:
  """A snapshot of a ``BatchedSimulator``'s buildings (sb_state_save): device tensors of ``n`` rows in a form that does
  not depend on the state layout, the sweep kernel or the orientation the library chose, the handle's counters
  (``clock``: occupancy queries, convection calls, steps since the last reset, reset once), with the seeded convection
  (``convection_attach_seeded``) the generators of every building slot (``conv_rng``; a snapshot of ``rows`` carries
  none: a forked building keeps its own slot's stream), and a fingerprint of what the rows mean -- floor plan and zone
  count, the compiled plan tables, ``SimConfig.to_params()``, the device generators attached and their ``first_building``.  ``BatchedSimulator.load_state`` refuses another fingerprint."""
  grid: torch.Tensor              # [n, H*W] float64, the caller's orientation
  zone: torch.Tensor              # [n, 4, Z] float64: zone means, VAV zone-air temperature, damper, zone heat input
  mode: torch.Tensor              # [n, Z] int32: thermostat mode | reheat valve << 8
  scal: torch.Tensor              # [n, 20] float64
  nsw: torch.Tensor               # [n] int32: sweeps | converged << 16 of the last step
  occ: Optional[torch.Tensor]     # [n, Z] int32 (occupant bits) when device occupancy is attached
  clock: Tuple[int, int, int, int]
  fingerprint: Tuple
  conv_rng: Optional[torch.Tensor] = None   # [B, 625] int32 (bit patterns): the seeded convection generators of every slot

  @property
  def n(self) -> int:
    return int(self.grid.shape[0])

  def tensors(self) -> Dict[str, Optional[torch.Tensor]]:
    return dict(grid=self.grid, zone=self.zone, mode=self.mode, scal=self.scal, nsw=self.nsw, occ=self.occ)

  def view(self) -> _ffi.StateView:
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    v = _ffi.StateView()
    v.n = self.n
    v.grid, v.zone, v.mode, v.scal, v.nsw, v.occ = (ptr(self.grid), ptr(self.zone), ptr(self.mode), ptr(self.scal),
                                                     ptr(self.nsw), ptr(self.occ))
    return v

  def state_dict(self) -> dict:
    d = {k: (None if t is None else t.cpu()) for k, t in self.tensors().items()}
    d.update(clock=list(self.clock), fingerprint=list(self.fingerprint))
    if self.conv_rng is not None:   # (only with the seeded convection: older readers see the dict they know)
      d["conv_rng"] = self.conv_rng.cpu()
    return d

  @staticmethod
  def from_state_dict(d: Mapping, device) -> "SimState":
    if not isinstance(d, Mapping) or "fingerprint" not in d or "clock" not in d:
      raise ValueError("not a SimState state_dict: fingerprint or clock missing")
    to = lambda t: None if t is None else t.to(device).contiguous()
    return SimState(to(d["grid"]), to(d["zone"]), to(d["mode"]), to(d["scal"]), to(d["nsw"]), to(d.get("occ")),
                    tuple(int(x) for x in d["clock"]), _as_fingerprint(d["fingerprint"]), to(d.get("conv_rng")))


def _as_fingerprint(f) -> Tuple:
  return tuple(_as_fingerprint(x) if isinstance(x, (list, tuple)) else x for x in f)


def _sha(*arrays) -> str:
  h = hashlib.sha256()
  for a in arrays:
    a = np.ascontiguousarray(a)
    h.update(str((a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
  return h.hexdigest()


SOLVERS = ("gauss_seidel", "jacobi_fp32")   # BatchedSimulator / BatchedEnvironment(solver=...)


class BatchedSimulator:
  """Thin owner of the C-ABI handle: B building instances of one floor plan on one GPU.

  Counterpart of ``SimulatorBuilding`` + ``Simulator`` + reward function for the batched
  path (simulator_building.py:44-315); tensors in, tensors out."""

  def __init__(self, plan: FloorPlan, config: SimConfig, n_buildings: int, h_conv: float,
               device: int = 0,
               observation_normalization: Optional[Mapping[str, Tuple[float, float]]] = None,
               zone_names: Optional[Sequence[str]] = None, orientation: str = "auto",
               histogram_parameters: Optional[Sequence[Tuple[str, Sequence[float]]]] = None,
               normalize_reduce: bool = False, solver: str = "gauss_seidel",
               building_materials: Optional[host_inputs.BuildingMaterials] = None):
    """``solver``: "gauss_seidel" -- SimulatorFlexibleGeometries' float64 sweep (simulator.py:278-371), the library's
    own kernels; "jacobi_fp32" -- TFSimulator's float32 Jacobi update (tf_simulator.py:502-853), the solver of SB1's
    shipped sim_config.gin, on k_sweep_jacobi (grid in the caller's orientation only; no snapshots, no convection).
    ``building_materials``: a ``host_inputs.BuildingMaterials`` makes a handle whose buildings have materials and a
    convection coefficient of their own (sb_create_materials: structural classes, k_sweep_lds with a coefficient table
    per building; ``set_building_materials`` changes the rows later).  None, the default, is the handle without."""
    if solver not in SOLVERS:
      raise ValueError(f"solver must be one of {SOLVERS}")
    if building_materials is not None:
      if not isinstance(building_materials, host_inputs.BuildingMaterials):
        raise ValueError("building_materials must be a host_inputs.BuildingMaterials (or None)")
      if solver == "jacobi_fp32":
        raise ValueError("building_materials is not implemented for solver='jacobi_fp32' (its float32 class table is one "
                         "per batch); use solver='gauss_seidel'")
    if solver == "jacobi_fp32" and orientation not in ("auto", "rows"):
      raise ValueError("solver='jacobi_fp32' keeps the caller's orientation (transposing would move TFSimulator's "
                       "swapped horizontal neighbours to the other axis): orientation must be 'auto' or 'rows'")
    self.solver = solver
    self._lib = _ffi.load()
    if not torch.cuda.is_available():
      raise _ffi.SbsimError("sbsim_amd needs a HIP device (MI355X); there is no CPU path")
    self.plan, self.config, self.B, self.device = plan, config, int(n_buildings), int(device)
    self._h_conv = float(h_conv)
    self._occ_attached = self._conv_attached = None   # the arguments of the device generators (SimState fingerprint)
    self._conv_seeded = False      # convection_attach_seeded is in force: SimState carries the generators (conv_rng)
    self._building_params = None   # set_building_params: the per-building table in force (None: the config's values)
    self._reward_function = None   # set_reward_function: None -- the default regret function of the SimConfig
    self._materials_handle = building_materials is not None   # sb_create_materials made the handle
    self._building_materials = None   # set_building_materials: the rows in force (None: the plan's own values)
    self._clock_offsets = None   # clock_attach: the buildings' offsets into the timeline (None: one clock for the batch)
    self._calendars = None   # clock_attach(calendar_of=...): hashes of the concatenated rows and of calendar_of
    self._episode_starts = None   # episode_starts_attach: the host_inputs.EpisodeStarts in force
    self._spatial = (False, None)   # spatial_attach: (attached, the map's shape or None); configuration, not state
    self._initial_conditions = None   # initial_conditions_attach: the host_inputs.InitialConditions in force
    self._randomization = None   # randomization_attach: the host_inputs.EpisodeRandomization in force
    self._randomization_base = None   # ... and the rows in force when it was attached, by name
    self._episode_metrics = False   # episode_metrics_attach: episode totals are kept (not state: no fingerprint entry)
    self._telemetry = None   # telemetry_attach: the host_inputs.Telemetry in force (not state either)
    self._fingerprint = None
    self.n_actions = len(config.action_names)
    H0, W0 = plan.shape
    if orientation not in ("auto", "rows", "columns"):
      raise ValueError("orientation must be 'auto', 'rows' or 'columns'")
    self.Z, self.H, self.W = plan.n_zones, H0, W0
    zone_names = list(zone_names or plan.zone_names or [f"room_{i + 1}" for i in range(self.Z)])
    self.zone_names = zone_names
    (source_names, col_ahu, col_blr, col_zone, n_src) = observation_field_names(
        zone_names, config.ahu_has_weather_sensor)
    aux_names, source_names = source_names[n_src:], source_names[:n_src]
    # optional HistogramReducer (environment.py:731-777,1032-1071): device-side binning
    if histogram_parameters:
      out_names, src_dest, hist_col, hist_off, hist_bins = histogram_reducer_layout(
          source_names, histogram_parameters)
    else:
      out_names, src_dest, hist_col, hist_off, hist_bins = list(source_names), None, [], [0], []
    col_aux = len(out_names)
    self.field_names = out_names + list(aux_names)
    self.source_names = source_names
    self.O = len(self.field_names)

    def describe(p: FloorPlan):
      cp = p.compile(config.time_step_sec, h_conv)
      keep = dict(cls=np.ascontiguousarray(cp.cell_class), coef=np.ascontiguousarray(cp.class_coef),
                  czone=np.ascontiguousarray(cp.class_zone), zoff=np.ascontiguousarray(cp.zone_off),
                  zcells=np.ascontiguousarray(cp.zone_cells))
      desc = _ffi.PlanDesc(cp.H, cp.W, cp.Z, cp.n_classes,
                           keep["cls"].ctypes.data_as(C.POINTER(C.c_uint8)),
                           keep["coef"].ctypes.data_as(_ffi._dp), keep["czone"].ctypes.data_as(_ffi._ip),
                           keep["zoff"].ctypes.data_as(_ffi._ip), keep["zcells"].ctypes.data_as(_ffi._ip))
      info = _ffi.LaunchInfo()
      rc = self._lib.sb_plan_info(C.byref(desc), self.O, self.B, C.byref(info))
      return cp, keep, desc, (rc, info)

    # device-side orientation (internal to the library; reset()/temps() convert, so callers
    # always see the reference's [H, W] layout): the library reports, per orientation, which
    # step kernel it would use, how many wavefront steps one sweep takes and on how many wavefronts
    if orientation == "auto" and os.environ.get("SBSIM_ORIENTATION") in ("rows", "columns") and solver == "gauss_seidel":
      orientation = os.environ["SBSIM_ORIENTATION"]   # (developer knob)
    if solver == "jacobi_fp32":
      self.transposed = False
      self.compiled, keep, pd_, jd = self._describe_jacobi(plan, config.time_step_sec, h_conv)
    elif self._materials_handle:
      # always k_sweep_lds: the orientation with fewer wavefront steps per sweep (rows on a tie, as below) among those
      # whose grid, with the coefficient table per wavefront, fits in LDS (sb_plan_info_materials).
      # The slots are numbered once, in the caller's orientation: a table's [B, M] columns mean plan.material_slots()
      # whichever orientation the device runs (the transposed plan's own raster order can differ)
      slot_ids, self._slot_table = plan.material_slots()
      building_materials.check_plan(self.B, len(self._slot_table))
      plan_info = _ffi.materials_entry("sb_plan_info_materials")
      chosen = None
      for tr in sorted({"rows": [False], "columns": [True], "auto": [False, True]}[orientation],
                       key=lambda tr: FloorPlan.sweep_steps(*(plan.shape[::-1] if tr else plan.shape))):
        cand = self._describe_structural(plan.transposed() if tr else plan, config.time_step_sec, h_conv,
                                         (slot_ids.T if tr else slot_ids, self._slot_table))
        rc = plan_info(C.byref(cand[2]), self.O, self.B, C.byref(_ffi.LaunchInfo()))
        if rc == 0:
          chosen = (tr, cand)
          break
        if rc != -4:   # (SB_ERR_TOO_LARGE: the other orientation may fit)
          _ffi.check(rc, "sb_plan_info_materials")
      if chosen is None:
        raise ValueError("building_materials needs k_sweep_lds, which cannot hold this floor plan: "
                         + (self._lib.sb_last_error() or b"").decode())
      self.transposed, (self.compiled, keep, pd_, sd_) = chosen
    else:
      cands = {"rows": [False], "columns": [True], "auto": [False, True]}[orientation]
      best = None
      for tr in cands:
        cand = describe(plan.transposed() if tr else plan)
        rc, info = cand[3]
        # SIMD steps per building-sweep: a kernel that spreads a building over two wavefronts holds half as many
        pref = {1: 0, 0: 1, 2: 2}.get(info.path, 3) if rc == 0 else 9   # registers, then LDS, then the streaming kernel
        key = (rc != 0, pref, info.sweep_steps * max(info.waves_per_building, 1) if rc == 0 else 0)
        if best is None or key < best[0]:
          best = (key, tr, cand)
      self.transposed = best[1]
      self.compiled, keep, pd_, _ = best[2]
    norm = dict(observation_normalization or {})
    mean = np.zeros(max(self.O, n_src))     # by source index
    sigma = np.ones(max(self.O, n_src))
    for i, name in enumerate(source_names):
      mu, var = norm.get(name.split("/", 1)[1], (0.0, 1.0))
      # ContinuousVariableInfo fields are proto floats (smart_control_normalization.proto)
      mu, var = float(np.float32(mu)), float(np.float32(var))
      mean[i] = mu
      sigma[i] = math.sqrt(var) if var > 0.0 else 0.0
    self._keep = dict(keep, colz=np.asarray(col_zone, dtype=np.int32), mean=mean, sigma=sigma)
    self._keep.update(src_dest=np.asarray(src_dest if src_dest is not None else [0], dtype=np.int32),
                      hist_col=np.asarray(hist_col or [0], dtype=np.int32),
                      hist_off=np.asarray(hist_off, dtype=np.int32),
                      hist_bins=np.asarray(hist_bins or [0.0], dtype=np.float64))
    kp = self._keep
    ol = _ffi.ObsLayout(self.O, col_ahu, col_blr, col_aux, kp["colz"].ctypes.data_as(_ffi._ip),
                        mean.ctypes.data_as(_ffi._dp), sigma.ctypes.data_as(_ffi._dp),
                        n_src if src_dest is not None else 0, len(hist_col),
                        kp["src_dest"].ctypes.data_as(_ffi._ip), kp["hist_col"].ctypes.data_as(_ffi._ip),
                        kp["hist_off"].ctypes.data_as(_ffi._ip), kp["hist_bins"].ctypes.data_as(_ffi._dp),
                        1 if normalize_reduce else 0)
    params = config.to_params()
    h = C.c_void_p()
    with torch.cuda.device(self.device):
      if solver == "jacobi_fp32":
        _ffi.check(_ffi.jacobi_entry("sb_create_jacobi")(C.byref(pd_), C.byref(jd), C.byref(params), C.byref(ol), self.B,
                                                         self.device, C.byref(h)), "sb_create_jacobi")
      elif self._materials_handle:
        _ffi.check(_ffi.materials_entry("sb_create_materials")(C.byref(pd_), C.byref(sd_), C.byref(params), C.byref(ol),
                                                               self.B, self.device, C.byref(h)), "sb_create_materials")
      else:
        _ffi.check(self._lib.sb_create(C.byref(pd_), C.byref(params), C.byref(ol), self.B, self.device,
                                       C.byref(h)), "sb_create")
    self._h = h
    self.tdev = torch.device("cuda", self.device)
    info = _ffi.LaunchInfo()
    _ffi.check(self._lib.sb_get_launch_info(self._h, C.byref(info)), "sb_get_launch_info")
    self.launch_info = {f[0]: getattr(info, f[0]) for f in _ffi.LaunchInfo._fields_}
    self.sweep_events = None   # a list: step() appends (start, end) HIP events of every sweep-kernel launch (bench.py)
    if building_materials is not None:
      self.set_building_materials(building_materials)

  @staticmethod
  def _describe_structural(plan: FloorPlan, dt: float, h_conv: float, slots):
    """FloorPlan.compile_structural's tables (material slots numbered by ``slots``) as sb_create_materials' arguments."""
    sp = plan.compile_structural(dt, slots)
    keep = dict(cls=np.ascontiguousarray(sp.cell_class), coef=np.ascontiguousarray(sp.class_coef(h_conv=h_conv)),
                czone=np.ascontiguousarray(sp.class_zone), zoff=np.ascontiguousarray(sp.zone_off),
                zcells=np.ascontiguousarray(sp.zone_cells), cdesc=np.ascontiguousarray(sp.class_desc),
                cdiff=np.ascontiguousarray(sp.class_diffuser), slots=np.ascontiguousarray(sp.slot_table))
    pd_ = _ffi.PlanDesc(sp.H, sp.W, sp.Z, sp.n_classes, keep["cls"].ctypes.data_as(C.POINTER(C.c_uint8)),
                        keep["coef"].ctypes.data_as(_ffi._dp), keep["czone"].ctypes.data_as(_ffi._ip),
                        keep["zoff"].ctypes.data_as(_ffi._ip), keep["zcells"].ctypes.data_as(_ffi._ip))
    sd = _ffi.StructDesc(sp.n_slots, 0, keep["cdesc"].ctypes.data_as(_ffi._ip), keep["cdiff"].ctypes.data_as(_ffi._dp),
                         keep["slots"].ctypes.data_as(_ffi._dp), float(h_conv), sp.dx, sp.dx ** 2, sp.zh)
    return sp, keep, pd_, sd

  @staticmethod
  def _describe_jacobi(plan: FloorPlan, dt: float, h_conv: float):
    """FloorPlan.compile_jacobi's tables as sb_create_jacobi's arguments (the plan descriptor carries the zones)."""
    jp = plan.compile_jacobi(dt, h_conv)
    keep = dict(cls=np.ascontiguousarray(jp.cell_class), f32=np.ascontiguousarray(jp.class_f32),
                diff=np.ascontiguousarray(jp.class_diffuser), czone=np.ascontiguousarray(jp.class_zone),
                coef=np.zeros((jp.n_classes, 8)), zoff=np.ascontiguousarray(jp.zone_off),
                zcells=np.ascontiguousarray(jp.zone_cells))
    keep["coef"][:, 6] = jp.class_diffuser
    pd_ = _ffi.PlanDesc(jp.H, jp.W, jp.Z, jp.n_classes, keep["cls"].ctypes.data_as(C.POINTER(C.c_uint8)),
                        keep["coef"].ctypes.data_as(_ffi._dp), keep["czone"].ctypes.data_as(_ffi._ip),
                        keep["zoff"].ctypes.data_as(_ffi._ip), keep["zcells"].ctypes.data_as(_ffi._ip))
    jd = _ffi.JacobiDesc(jp.H, jp.W, jp.n_classes, 0, keep["cls"].ctypes.data_as(C.POINTER(C.c_uint8)),
                         keep["f32"].ctypes.data_as(_ffi._fp), keep["diff"].ctypes.data_as(_ffi._dp),
                         keep["czone"].ctypes.data_as(_ffi._ip))
    return jp, keep, pd_, jd

  def _refuse_on_jacobi(self, what: str) -> None:
    if self.solver == "jacobi_fp32":
      raise ValueError(f"{what} is not implemented for solver='jacobi_fp32' (the Jacobi path keeps a float32 grid the "
                       "snapshot format and the convection shuffle do not handle yet); use solver='gauss_seidel'")

  def tap_jacobi(self, tprev: np.ndarray, q: np.ndarray, tinf: np.ndarray):
    """sb_tap_jacobi: one finite_differences_timestep of TFSimulator on buildings 0 .. n-1 from prescribed float32
    grids Tprev [n, H, W], float32 input_q [n, H, W] and T_inf [n].  Returns (grid [n, H, W] float32, iterations [n],
    converged [n]).  Overwrites those buildings' grids: not inside a rollout."""
    if self.solver != "jacobi_fp32":
      raise ValueError("tap_jacobi needs solver='jacobi_fp32'")
    n = int(tprev.shape[0])
    tp = np.ascontiguousarray(tprev, dtype=np.float32).reshape(n, -1)
    qq = np.ascontiguousarray(q, dtype=np.float32).reshape(n, -1)
    ti = np.ascontiguousarray(tinf, dtype=np.float64).reshape(n)
    grid = np.zeros_like(tp)
    iters, conv = np.zeros(n, np.int32), np.zeros(n, np.int32)
    torch.cuda.synchronize(self.tdev)
    with torch.cuda.device(self.device):
      _ffi.check(_ffi.jacobi_entry("sb_tap_jacobi")(
          self._h, n, tp.ctypes.data_as(_ffi._fp), qq.ctypes.data_as(_ffi._fp), ti.ctypes.data_as(_ffi._dp),
          grid.ctypes.data_as(_ffi._fp), iters.ctypes.data_as(_ffi._ip), conv.ctypes.data_as(_ffi._ip)), "sb_tap_jacobi")
    return grid.reshape(n, self.H, self.W), iters, conv

  def close(self) -> None:
    if getattr(self, "_h", None):
      self._lib.sb_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def _stream(self) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(self.tdev).cuda_stream)

  # ---- Simulator.reset() ----
  def _refuse_two_bases(self, initial_temp: Optional[float]) -> None:
    ic = self._initial_conditions
    if initial_temp is not None and ic is not None and ic.has_base:
      raise ValueError("initial_temp given while the attached initial conditions hold "
                       + ("reset_temp_values" if ic.n_grids else "initial_temp") + ": two bases for the same cells "
                       "(initial_conditions_detach, or leave initial_temp out)")

  def reset(self, initial_temp: Optional[float] = None, temps: Optional[torch.Tensor] = None) -> None:
    """sb_reset.  ``temps``: every cell's value, float64 [B, H*W]; otherwise the attached initial conditions
    (``initial_conditions_attach``), otherwise ``initial_temp`` (None: the SimConfig's) in every cell."""
    self._refuse_two_bases(initial_temp)
    ptr = None
    if temps is not None:
      if temps.dtype != torch.float64 or tuple(temps.shape) != (self.B, self.H * self.W) or not temps.is_contiguous():
        raise ValueError("temps must be a contiguous float64 [B, H*W] tensor")
      if self.transposed:
        temps = temps.view(self.B, self.H, self.W).transpose(1, 2).contiguous()
      ptr = C.c_void_p(temps.data_ptr())
    t0 = self.config.initial_temp if initial_temp is None else float(initial_temp)
    _ffi.check(self._lib.sb_reset(self._h, t0, ptr, self._stream()), "sb_reset")

  def occupancy_attach(self, zone_assignment: int, hours: Sequence[int], time_step_sec: float, seed: int,
                       first_building: int = 0) -> None:
    """sb_occupancy_attach: one RandomizedArrivalDepartureOccupancy per building on the device."""
    cfg = _ffi.OccupancyConfig(int(zone_assignment), int(hours[0]), int(hours[1]), int(hours[2]), int(hours[3]),
                               float(time_step_sec), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_building))
    _ffi.check(self._lib.sb_occupancy_attach(self._h, C.byref(cfg)), "sb_occupancy_attach")
    self._occ_attached = (int(zone_assignment), tuple(int(x) for x in hours[:4]), float(time_step_sec),
                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_building))

  def occupancy_attach_groups(self, configs: Sequence, group_of) -> None:
    """sb_occupancy_attach_groups: ``occupancy_attach`` with one configuration per group of buildings.  ``configs``: per
    group ``(zone_assignment, hours, time_step_sec, seed, first_building)`` as ``occupancy_attach`` takes them (seed,
    first_building and time_step_sec the same in every group); ``group_of``: integers [B], building b's group.
    ValueError for what the library refuses, its message naming the group or the building."""
    fn = _ffi.occupancy_entry("sb_occupancy_attach_groups")
    groups = [(int(z), tuple(int(x) for x in hours[:4]), float(step), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first))
              for z, hours, step, seed, first in configs]
    g = np.asarray(group_of)
    if g.shape != (self.B,) or g.dtype == bool or not np.issubdtype(g.dtype, np.integer):
      raise ValueError(f"group_of must be integers of shape [{self.B}] (one group per building)")
    g = np.ascontiguousarray(g, dtype=np.int32)
    cfgs = (_ffi.OccupancyConfig * max(len(groups), 1))(*[
        _ffi.OccupancyConfig(z, hours[0], hours[1], hours[2], hours[3], step, seed, first)
        for z, hours, step, seed, first in groups])
    with torch.cuda.device(self.device):
      rc = fn(self._h, cfgs, len(groups), g.ctypes.data_as(C.c_void_p))
    if rc == -1:   # SB_ERR_INVALID
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_occupancy_attach_groups")
    self._occ_attached = ("groups", tuple(groups), _sha(g))

  def convection_attach(self, p: float, distance: int, seed: int, first_building: int = 0) -> None:
    """sb_convection_attach: StochasticConvectionSimulator(p, distance, seed) after every FD update
    (stochastic_convection_simulator.py:62-145), counter-based draws per building."""
    self._refuse_on_jacobi("the convection shuffle")
    _ffi.check(self._lib.sb_convection_attach(self._h, float(p), int(distance), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              int(first_building), int(self.transposed)), "sb_convection_attach")
    if (p == 0.0 or distance == 0) and self._conv_seeded:   # (the C entry's detach form leaves a seeded generator in force)
      seeds = np.zeros(self.B, np.uint64)
      _ffi.check(_ffi.convection_seeded_entry("sb_convection_attach_seeded")(
          self._h, 0.0, 0, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(self.transposed)), "sb_convection_attach_seeded")
    self._conv_seeded = False
    self._conv_attached = (None if p == 0.0 or distance == 0
                           else (float(p), int(distance), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_building)))

  def convection_attach_seeded(self, p: float, distance: int, seeds) -> None:
    """sb_convection_attach_seeded: the reference's seeded shuffle per building, draw for draw -- building b is the
    reference process that called random.seed(seeds[b]) (``seeds``: an integer s, building b gets s + b, or an integer
    array [B]; see ``host_inputs.SeededStochasticConvectionSimulator``).  Replaces a counter-based generator; p == 0 or
    distance == 0 detaches.  ValueError, the attachment left as it was: bad seeds, a window of more than 64 offsets
    (distance >= 20, or -1 with p < 1), a room of more than 2047 cells, solver='jacobi_fp32'."""
    seeds = host_inputs.SeededStochasticConvectionSimulator(p, distance, seeds).seeds_for(self.B)
    if self.solver == "jacobi_fp32":
      raise ValueError("the seeded convection shuffle is not implemented for solver='jacobi_fp32'; the host mode replays it "
                       "(host_convection.SeededHostConvection)")
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    with torch.cuda.device(self.device):
      rc = _ffi.convection_seeded_entry("sb_convection_attach_seeded")(
          self._h, float(p), int(distance), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(self.transposed))
    if rc == -5:   # SB_ERR_UNSUPPORTED
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_convection_attach_seeded")
    detached = p == 0.0 or distance == 0
    self._conv_seeded = not detached
    # (the seeds are where the streams started, not where they are: the snapshot carries the streams themselves)
    self._conv_attached = None if detached else ("seeded", float(p), int(distance))

  def convection_rng(self) -> torch.Tensor:
    """sb_convection_rng_get: the buildings' generators, int32 [B, 625] on the device (bit patterns of MT19937's 624
    words and the index of the next word: ``random.Random(seed).getstate()[1]`` as uint32)."""
    out = torch.empty((self.B, _ffi.SB_CONV_RNG_WORDS), dtype=torch.int32, device=self.tdev)
    _ffi.check(_ffi.convection_seeded_entry("sb_convection_rng_get")(self._h, C.c_void_p(out.data_ptr()), self._stream()),
               "sb_convection_rng_get")
    return out

  def set_convection_rng(self, t: torch.Tensor) -> None:
    """sb_convection_rng_set: the buildings' generators <- t (int32 [B, 625] on the device, contiguous).  An index word
    above 624 counts as 624."""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (self.B, _ffi.SB_CONV_RNG_WORDS)
        or t.device != self.tdev or not t.is_contiguous()):
      raise ValueError(f"the generators must be a contiguous int32 [{self.B}, {_ffi.SB_CONV_RNG_WORDS}] tensor on {self.tdev}")
    _ffi.check(_ffi.convection_seeded_entry("sb_convection_rng_set")(self._h, C.c_void_p(t.data_ptr()), self._stream()),
               "sb_convection_rng_set")

  def convection_apply(self) -> None:
    """sb_convection_apply: one convection pass on the current grids with the attached generator of either kind (what a
    step runs after its finite-difference update) -- a test tap; the zone means are not recomputed."""
    _ffi.check(_ffi.convection_seeded_entry("sb_convection_apply")(self._h, self._stream()), "sb_convection_apply")

  def occupancy_peek(self, local_hour: int, is_work_day: bool, count: Optional[torch.Tensor] = None,
                     total: Optional[torch.Tensor] = None) -> None:
    """sb_occupancy_peek: advances every occupant once; count [B, Z] / total [B] float32."""
    for t, shape in ((count, (self.B, self.Z)), (total, (self.B,))):
      if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
        raise ValueError(f"occupancy output must be a contiguous float32 {shape} tensor")
    _ffi.check(self._lib.sb_occupancy_peek(
        self._h, int(local_hour), int(bool(is_work_day)), C.c_void_p(count.data_ptr()) if count is not None else None,
        C.c_void_p(total.data_ptr()) if total is not None else None, self._stream()), "sb_occupancy_peek")

  # ---- a calendar per building (sb_clock_attach / sb_clock_seek) ----
  def clock_attach(self, rows: np.ndarray, offsets: np.ndarray, calendar_of: Optional[np.ndarray] = None) -> None:
    """sb_clock_attach: ``rows`` float64 [n_rows, SB_CLOCK_FIELDS] (``host_inputs.Timeline.rows``), ``offsets`` int32 [B].
    The library copies both; ``clock_seek`` before the first step, observation or occupancy query.  Configuration of the
    buildings' slots, as ``set_building_params``: snapshots do not carry it, a forked building keeps its slot's offset.
    ``calendar_of``: the table is a ``host_inputs.CalendarTimeline``'s, several calendars one after the other, and this
    is its ``calendar_of`` -- the snapshot fingerprint then carries the rows and the buildings' calendars."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    if rows.ndim != 2 or offsets.shape != (self.B,):
      raise ValueError(f"clock_attach needs rows [n_rows, {_ffi.SB_CLOCK_FIELDS}] and offsets [{self.B}]")
    with torch.cuda.device(self.device):
      rc = _ffi.clock_entry("sb_clock_attach")(self._h, rows.ctypes.data_as(C.c_void_p), int(rows.shape[0]),
                                               int(rows.shape[1]), offsets.ctypes.data_as(C.c_void_p))
    if rc in (-1, -4):   # SB_ERR_INVALID, SB_ERR_TOO_LARGE
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_clock_attach")
    if self._clock_offsets is not None:   # (a new table: the library drops the starts with the clock it replaces)
      self._episode_starts = None
    self._clock_offsets = offsets.copy()
    self._calendars = None if calendar_of is None else (_sha(rows), _sha(np.ascontiguousarray(calendar_of, dtype=np.int32)))

  def clock_seek(self, pos: int, prev_pos: int = -1) -> None:
    """sb_clock_seek: the position of the next step, observation and occupancy query (a host value: no device work);
    prev_pos: the position of the previous thermostat update, -1 for none."""
    rc = _ffi.clock_entry("sb_clock_seek")(self._h, int(pos), int(prev_pos))
    if rc == -1:
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_clock_seek")

  def clock_detach(self) -> None:
    with torch.cuda.device(self.device):
      _ffi.check(_ffi.clock_entry("sb_clock_detach")(self._h), "sb_clock_detach")
    if self._clock_offsets is not None:   # (the library drops the starts with the clock)
      self._episode_starts = None
    self._clock_offsets = self._calendars = None

  def observe_step_in(self, step_in: _ffi.StepIn, out: torch.Tensor) -> torch.Tensor:
    """sb_observe_step_in: the observation with its inputs in a StepIn (the weather forms per building; with a clock,
    every building's own row)."""
    _ffi.check(_ffi.clock_entry("sb_observe_step_in")(self._h, C.byref(step_in), C.c_void_p(out.data_ptr()), self._stream()),
               "sb_observe_step_in")
    return out

  # ---- episodes per building (sb_reset_buildings / sb_observe_buildings) ----
  def _host_mask(self, mask) -> np.ndarray:
    """A building mask as the library takes it: uint8 [B] on the host.  bool or uint8, numpy or torch; a device tensor is
    copied to the host, which synchronises with the device."""
    if isinstance(mask, torch.Tensor):
      if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"mask must be bool or uint8, got {mask.dtype}")
      m = mask.detach().cpu().numpy()
    else:
      m = np.asarray(mask)
      if m.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        raise ValueError(f"mask must be bool or uint8, got dtype {m.dtype}")
    if m.shape != (self.B,):
      raise ValueError(f"mask must have shape [{self.B}] (one flag per building), got {tuple(m.shape)}")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)

  def reset_buildings(self, mask, restart_pos: int = 0, initial_temp: Optional[float] = None,
                      temps: Optional[torch.Tensor] = None) -> None:
    """sb_reset_buildings: ``reset`` for the buildings of ``mask`` alone (bool or uint8 [B], numpy or torch -- a device
    tensor is copied to the host, which synchronises); not one bit of another building's state changes.  ``restart_pos``:
    with a clock attached, the batch position of the reset buildings' next step (``clock_seek`` there before it).
    ``temps``: the full [B, H*W] array, of which only the masked rows are read.  The call synchronises with the current
    stream; not while that stream is being captured.  ValueError: a mask of the wrong shape or dtype (before any
    launch), and what the library refuses (before the first ``reset``, a negative restart_pos, a restart that leaves a
    building without two rows of the table)."""
    fn = _ffi.episodes_entry("sb_reset_buildings")
    self._refuse_two_bases(initial_temp)
    m = self._host_mask(mask)
    ptr = None
    if temps is not None:
      if temps.dtype != torch.float64 or tuple(temps.shape) != (self.B, self.H * self.W) or not temps.is_contiguous():
        raise ValueError("temps must be a contiguous float64 [B, H*W] tensor")
      if self.transposed:
        temps = temps.view(self.B, self.H, self.W).transpose(1, 2).contiguous()
      ptr = C.c_void_p(temps.data_ptr())
    t0 = self.config.initial_temp if initial_temp is None else float(initial_temp)
    with torch.cuda.device(self.device):
      rc = fn(self._h, m.ctypes.data_as(C.c_void_p), int(restart_pos), t0, ptr, self._stream())
    if rc == -1:   # SB_ERR_INVALID
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_reset_buildings")

  def observe_buildings(self, mask, step_in: _ffi.StepIn, out: torch.Tensor) -> torch.Tensor:
    """sb_observe_buildings: ``observe_step_in`` for the buildings of ``mask`` (as ``reset_buildings`` takes it): their
    rows of ``out`` (float32 [B, O]) are written, every other row and building is left alone."""
    fn = _ffi.episodes_entry("sb_observe_buildings")
    m = self._host_mask(mask)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (self.B, self.O)
        or not out.is_contiguous() or out.device != self.tdev):
      raise ValueError(f"out must be a contiguous float32 [{self.B}, {self.O}] tensor on {self.tdev}")
    with torch.cuda.device(self.device):
      rc = fn(self._h, m.ctypes.data_as(C.c_void_p), C.byref(step_in), C.c_void_p(out.data_ptr()), self._stream())
    if rc == -1:
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_observe_buildings")
    return out

  def observe(self, aux: Sequence[float], t_amb, out: Optional[torch.Tensor] = None,
              num_occupants: Optional[torch.Tensor] = None, occupancy_norm: float = 0.0) -> torch.Tensor:
    """t_amb: one ambient temperature, or a float64 [B] device tensor (per-building weather).
    num_occupants: optional float32 [B] device tensor (per-building occupancy feature)."""
    out = out if out is not None else torch.empty((self.B, self.O), dtype=torch.float32, device=self.tdev)
    a = (C.c_float * _ffi.SB_NUM_AUX)(*[float(x) for x in aux])
    per_b = None
    if isinstance(t_amb, torch.Tensor):
      if t_amb.dtype != torch.float64 or tuple(t_amb.shape) != (self.B,):
        raise ValueError("per-building t_amb must be a float64 [B] tensor")
      per_b, t_amb = C.c_void_p(t_amb.contiguous().data_ptr()), 0.0
    _ffi.check(self._lib.sb_observe_occupancy(
        self._h, a, float(t_amb), per_b, C.c_void_p(num_occupants.data_ptr()) if num_occupants is not None else None,
        float(occupancy_norm), C.c_void_p(out.data_ptr()), self._stream()), "sb_observe")
    return out

  def step(self, actions: Optional[torch.Tensor], step_in: _ffi.StepIn, obs: torch.Tensor,
           reward: torch.Tensor, info: Optional[torch.Tensor] = None, phases: int = 7) -> None:
    """One Environment._step for every building (sb_step).  `phases` selects a subset of its
    three launches (1 = device algebra before the sweep, 2 = sweep kernel, 4 = reward /
    observation) -- a measurement aid; a step is complete once all three ran in order."""
    if actions is not None:
      if actions.dtype != torch.float32 or tuple(actions.shape) != (self.B, self.n_actions):
        raise ValueError(f"actions must be float32 [{self.B}, {self.n_actions}]")
      if not actions.is_contiguous():
        actions = actions.contiguous()
    args = (self._h, C.c_void_p(actions.data_ptr()) if actions is not None else None, C.byref(step_in),
            C.c_void_p(obs.data_ptr()) if obs is not None else None, C.c_void_p(reward.data_ptr()),
            C.c_void_p(info.data_ptr()) if info is not None else None, self._stream())
    if self.sweep_events is not None and phases == 7:
      # measurement aid (bench.py): the step's three launches one by one, HIP events around the sweep kernel on its stream
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      _ffi.check(self._lib.sb_step_phases(*args, 1), "sb_step")
      e0.record()
      _ffi.check(self._lib.sb_step_phases(*args, 2), "sb_step")
      e1.record()
      _ffi.check(self._lib.sb_step_phases(*args, 4), "sb_step")
      self.sweep_events.append((e0, e1))
      return
    _ffi.check(self._lib.sb_step_phases(*args, int(phases)), "sb_step")

  # ---- per-building parameters (sb_set_building_params) ----
  def set_building_params(self, params: Optional[host_inputs.BuildingParams]) -> None:
    """Per-building HVAC, setpoint-window and reward parameters (``host_inputs.BuildingParams``, one row per building;
    None clears the table: every building back to the SimConfig's values).  Checked on the host, then ordered on the
    current stream and synchronised with it; not while that stream is being captured into a graph.  A row belongs to
    the building's slot, not to its state: snapshots do not carry it and a forked building keeps its own row.  It
    applies from the next reset, step or observation; a reset sets the AHU and boiler setpoints from it."""
    fn = _ffi.entry("sb_set_building_params")
    if self._randomization is not None:
      raise ValueError("set_building_params: an episode randomisation is attached, which owns the rows (randomization_detach first)")
    if params is None:
      _ffi.check(fn(self._h, 0, None, None, self._stream()), "sb_set_building_params")
      self._building_params = None
      return
    if not isinstance(params, host_inputs.BuildingParams):
      raise ValueError("set_building_params needs a host_inputs.BuildingParams (or None)")
    if params.n_buildings != self.B:
      raise ValueError(f"BuildingParams has {params.n_buildings} rows, the simulator {self.B} buildings")
    params.validate(self.config)
    fields, values = params.c_table()
    with torch.cuda.device(self.device):
      _ffi.check(fn(self._h, int(fields.shape[0]), fields.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p),
                    self._stream()), "sb_set_building_params")
    self._building_params = params

  def building_params(self) -> Dict[str, np.ndarray]:
    """The parameters every building runs with: SimConfig field name -> float64 [B] ([B, 2] for the windows)."""
    return host_inputs.effective_building_params(self._building_params, self.config, self.B)

  # ---- per-building materials (sb_set_building_materials) ----
  def set_building_materials(self, materials: Optional[host_inputs.BuildingMaterials]) -> None:
    """Per-building conductivity, heat capacity and density of the plan's material slots and convection coefficient
    (``host_inputs.BuildingMaterials``; None: every building back to the plan's own values), on a simulator created with
    ``building_materials``.  The device computes every building's coefficient rows (k_class_coef) on the current stream
    and the call synchronises with it; not while that stream is being captured into a graph.  Configuration of the
    building's slot, as ``set_building_params``: snapshots do not carry it, a forked building keeps its own row, and
    it applies from the next step."""
    if not self._materials_handle:
      raise ValueError("set_building_materials needs a simulator created with building_materials=... (its floor plan is "
                       "compiled into structural classes and runs on k_sweep_lds)")
    fn = _ffi.materials_entry("sb_set_building_materials")
    if self._randomization is not None:
      raise ValueError("set_building_materials: an episode randomisation is attached, which owns the rows (randomization_detach first)")
    if materials is None:
      with torch.cuda.device(self.device):
        _ffi.check(fn(self._h, 0, None, None, self._stream()), "sb_set_building_materials")
      self._building_materials = None
      return
    if not isinstance(materials, host_inputs.BuildingMaterials):
      raise ValueError("set_building_materials needs a host_inputs.BuildingMaterials (or None)")
    M = len(self._slot_table)
    materials.check_plan(self.B, M)
    fields, values = materials.c_table(M)
    with torch.cuda.device(self.device):
      rc = fn(self._h, int(fields.shape[0]), fields.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p),
              self._stream())
    if rc == -1:   # SB_ERR_INVALID
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_set_building_materials")
    self._building_materials = materials

  def building_materials(self) -> Dict[str, np.ndarray]:
    """The materials every building runs with: conductivity / heat_capacity / density float64 [B, M] by material slot
    (``FloorPlan.material_slots()``), convection_coefficient [B]."""
    table = self._slot_table if self._materials_handle else self.plan.material_slots()[1]
    return host_inputs.effective_building_materials(self._building_materials, table, self._h_conv, self.B)

  def building_coef(self) -> torch.Tensor:
    """sb_get_building_coef: every building's coefficient rows in force, float64 [B, n_classes, 8] (bU bD bL bR ap gc sc
    pad; classes of ``self.compiled``, the device's orientation)."""
    if not self._materials_handle:
      raise ValueError("building_coef needs a simulator created with building_materials=...")
    return self._get(_ffi.materials_entry("sb_get_building_coef"), (self.B, self.compiled.n_classes, 8), torch.float64)

  # ---- the reward function (sb_set_reward_function) ----
  def set_reward_function(self, reward_function: Optional[host_inputs.SetpointEnergyCarbonReward]) -> None:
    """The reward every building's step returns from the next step on: a ``host_inputs.SetpointEnergyCarbonReward``
    (the reference's absolute reward in dollars; info columns 8..12 then hold its RewardResponse fields, 13..23 are 0),
    or None for the default, the SimConfig's regret function.  Works with both solvers and with a per-building table
    (whose productivity and window rows keep applying).  A host value of the handle: no upload, no synchronisation."""
    fn = _ffi.reward_entry("sb_set_reward_function")
    if reward_function is None:
      _ffi.check(fn(self._h, None), "sb_set_reward_function")
      self._reward_function = None
      return
    if not isinstance(reward_function, host_inputs.SetpointEnergyCarbonReward):
      raise ValueError("set_reward_function needs a host_inputs.SetpointEnergyCarbonReward (or None: the regret function)")
    cfg = _ffi.RewardConfig(*reward_function.as_tuple())
    try:
      _ffi.check(fn(self._h, C.byref(cfg)), "sb_set_reward_function")
    except _ffi.SbsimError as e:   # SB_ERR_INVALID: the reference's ValueError
      raise ValueError(str(e)) from None
    self._reward_function = reward_function

  @property
  def reward_function(self) -> Optional[host_inputs.SetpointEnergyCarbonReward]:
    """The reward function in force (None: the default regret function)."""
    return self._reward_function

  # ---- the three per-episode attachments: one path into the library ----
  def _draws_call(self, name: str, *args, value_errors=(-1, -5)) -> None:
    """The library's entry ``name`` on this simulator's device.  A return code in ``value_errors`` (-1 SB_ERR_INVALID,
    -5 SB_ERR_UNSUPPORTED) raises ValueError with the library's message, any other failure ``_ffi.SbsimError``."""
    with torch.cuda.device(self.device):
      rc = _ffi.entry(name)(self._h, *args)
    if rc in value_errors:
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, name)

  def _episodes_get(self, name: str, value_errors=(-5,)) -> torch.Tensor:
    out = torch.empty((self.B,), dtype=torch.int32, device=self.tdev)
    self._draws_call(name, C.c_void_p(out.data_ptr()), self._stream(), value_errors=value_errors)
    return out

  def _episodes_set(self, name: str, t: torch.Tensor, value_errors=(-5,)) -> None:
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (self.B,) or t.device != self.tdev
        or not t.is_contiguous()):
      raise ValueError(f"the episode numbers must be a contiguous int32 [{self.B}] tensor on {self.tdev}")
    self._draws_call(name, C.c_void_p(t.data_ptr()), self._stream(), value_errors=value_errors)

  # ---- start temperatures per building (sb_initial_conditions_attach) ----
  def initial_conditions_attach(self, ic: host_inputs.InitialConditions) -> None:
    """sb_initial_conditions_attach: from now on every reset without ``temps`` -- ``reset``, ``reset_buildings`` -- takes
    its cells from ``ic`` (``ic.start_temps(b, e)``, e the building's own episode number: 0 now, incremented by every
    reset of the building).  The library copies the arrays (the grids transposed here when the device runs the plan
    transposed); the call synchronises the device, not under stream capture.  Configuration of the slots plus one
    counter: snapshots carry neither (``initial_condition_episodes`` is how a checkpoint keeps the counters)."""
    if not isinstance(ic, host_inputs.InitialConditions):
      raise ValueError("initial_conditions_attach needs a host_inputs.InitialConditions (initial_conditions_detach clears them)")
    ic.check(self.B, (self.H, self.W))
    d = _ffi.InitialConditionsDesc()
    keep = []
    if ic.reset_temp_values is not None:
      g = ic.reset_temp_values.transpose(0, 2, 1) if self.transposed else ic.reset_temp_values
      g = np.ascontiguousarray(g, dtype=np.float64)
      keep.append(g)
      d.grids, d.n_grids = g.ctypes.data_as(_ffi._dp), int(g.shape[0])
    for name, ptr_t, dtype in (("grid_of", _ffi._ip, np.int32), ("initial_temp", _ffi._dp, np.float64),
                               ("offset", _ffi._dp, np.float64)):
      a = getattr(ic, name)
      if a is not None:
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        setattr(d, name, a.ctypes.data_as(ptr_t))
    if ic.jitter is not None:
      d.has_jitter, d.jitter_lo, d.jitter_hi, d.seed = 1, ic.jitter[0], ic.jitter[1], ic.jitter[2]
    d.first_building = ic.first_building
    self._draws_call("sb_initial_conditions_attach", C.byref(d), value_errors=(-1,))
    self._initial_conditions = ic

  def initial_conditions_detach(self) -> None:
    """sb_initial_conditions_detach: the resets fill from ``initial_temp`` again, with the kernels of a handle that never
    had conditions."""
    self._draws_call("sb_initial_conditions_detach", value_errors=())
    self._initial_conditions = None

  @property
  def initial_conditions(self) -> Optional[host_inputs.InitialConditions]:
    return self._initial_conditions

  def initial_condition_episodes(self) -> torch.Tensor:
    """sb_initial_conditions_episodes_get: int32 [B] on the device, the number of every building's NEXT episode.
    ``save_state`` / ``load_state`` leave the counters alone; a checkpoint keeps them with this pair."""
    return self._episodes_get("sb_initial_conditions_episodes_get")

  def set_initial_condition_episodes(self, t: torch.Tensor) -> None:
    """sb_initial_conditions_episodes_set: the counters <- t (int32 [B] on the device, contiguous)."""
    self._episodes_set("sb_initial_conditions_episodes_set", t)

  # ---- parameters and materials re-drawn per episode (sb_randomization_attach) ----
  def _randomization_bases(self):
    """The rows a randomisation attached now would take as its base: those of the attachment it replaces, else the rows
    in force (parameters by SimConfig field; materials None on a simulator created without ``building_materials``)."""
    if self._randomization_base is not None:
      return self._randomization_base
    return self.building_params(), (self.building_materials() if self._materials_handle else None)

  def randomization_attach(self, er: host_inputs.EpisodeRandomization) -> None:
    """sb_randomization_attach: from now on every reset of a building -- ``reset``, ``reset_buildings``, the autoreset --
    first writes ``er.values(b, e, base)`` into the building's rows of the two per-building tables and re-folds its
    coefficient rows, e the building's own episode number: 0 now, incremented by every reset of the building; base: the
    rows in force now.  Checked on the host first (``er.check``); the call synchronises the device, not under stream
    capture.  While attached, ``set_building_params`` / ``set_building_materials`` are refused, and
    ``building_params()`` / ``building_materials()`` keep returning the base rows (``building_param_rows()`` /
    ``building_material_rows()`` are the rows in force)."""
    if not isinstance(er, host_inputs.EpisodeRandomization):
      raise ValueError("randomization_attach needs a host_inputs.EpisodeRandomization (randomization_detach clears it)")
    if torch.cuda.is_current_stream_capturing():   # (the library's hipDeviceSynchronize would refuse, and invalidate the capture)
      raise ValueError("randomization_attach: not while the stream is being captured into a graph (the call synchronises the device)")
    bases = self._randomization_bases()
    er.check(self.B, bases[0], bases[1], self.solver)
    arr, keep = er.c_fields(len(self._slot_table) if self._materials_handle else None)
    self._draws_call("sb_randomization_attach", arr, len(er.fields), er.seed, er.first_building)
    del keep
    self._randomization, self._randomization_base = er, bases

  def randomization_detach(self) -> None:
    """sb_randomization_detach: both tables back to the rows of the attach, bit for bit, the coefficient rows re-folded;
    the resets launch what they launched before."""
    if torch.cuda.is_current_stream_capturing():
      raise ValueError("randomization_detach: not while the stream is being captured into a graph (the call synchronises the device)")
    self._draws_call("sb_randomization_detach", value_errors=())
    self._randomization = self._randomization_base = None

  @property
  def randomization(self) -> Optional[host_inputs.EpisodeRandomization]:
    return self._randomization

  def randomization_base(self) -> Dict[str, np.ndarray]:
    """The rows in force when the randomisation was attached, by name: what ``EpisodeRandomization.values`` takes as
    ``base``."""
    if self._randomization is None:
      raise ValueError("randomization_base: no episode randomisation is attached")
    return dict(self._randomization_base[0], **(self._randomization_base[1] or {}))

  def _rows_out(self, name: str, n_rows: int) -> torch.Tensor:
    out = torch.empty((n_rows, self.B), dtype=torch.float64, device=self.tdev)
    self._draws_call(name, C.c_void_p(out.data_ptr()), self._stream(), value_errors=(-5,))
    return out

  def building_param_rows(self) -> torch.Tensor:
    """sb_get_building_params: the parameter rows in force on the device, float64 [SB_NUM_BUILDING_PARAMS, B] (row k:
    ``_ffi.BUILDING_PARAM_FIELDS[k]``; the SimConfig's values without a table).  Stream-ordered."""
    return self._rows_out("sb_get_building_params", _ffi.SB_NUM_BUILDING_PARAMS)

  def building_material_rows(self) -> torch.Tensor:
    """sb_get_building_materials: the material rows in force, float64 [3 M + 1, B] (row kind * M + slot; 3 M: the
    convection coefficient), on a simulator created with ``building_materials``.  Stream-ordered."""
    if not self._materials_handle:
      raise ValueError("building_material_rows needs a simulator created with building_materials=...")
    return self._rows_out("sb_get_building_materials", 3 * len(self._slot_table) + 1)

  def randomization_episodes(self) -> torch.Tensor:
    """sb_randomization_episodes_get: int32 [B] on the device, the number of every building's NEXT episode.  Snapshots
    carry neither the rows nor the counters: a checkpoint keeps the counters with this pair."""
    return self._episodes_get("sb_randomization_episodes_get")

  def set_randomization_episodes(self, t: torch.Tensor) -> None:
    """sb_randomization_episodes_set: the counters <- t (int32 [B] on the device, contiguous), and the rows in force
    <- ``values(b, t[b] - 1)`` (the base row where t[b] == 0), coefficient rows included."""
    self._episodes_set("sb_randomization_episodes_set", t)

  # ---- a start time and weather per building, drawn per episode (sb_episode_starts_attach) ----
  def episode_starts_attach(self, es: host_inputs.EpisodeStarts, weather_lohi: Optional[torch.Tensor] = None,
                            weather_offset: Optional[torch.Tensor] = None) -> None:
    """sb_episode_starts_attach: from now on every reset of a building -- ``reset``, ``reset_buildings``, the autoreset --
    first writes ``es.values(b, e, base_offsets)`` into the building's clock offset and its entries of the two weather
    arrays, e the building's own episode number: 0 now, incremented by every reset of the building.  ``weather_lohi``
    (float64 [B, 2]) / ``weather_offset`` (float64 [B]): the device tensors passed in every StepIn, which the library
    writes in place; the caller keeps them alive.  Offsets need a clock (``clock_attach`` first).  The call synchronises
    the device, not under stream capture."""
    if not isinstance(es, host_inputs.EpisodeStarts):
      raise ValueError("episode_starts_attach needs a host_inputs.EpisodeStarts (episode_starts_detach clears it)")
    if torch.cuda.is_current_stream_capturing():   # (the library's hipDeviceSynchronize would refuse, and invalidate the capture)
      raise ValueError("episode_starts_attach: not while the stream is being captured into a graph (the call synchronises the device)")
    for name, t, shape in (("weather_lohi", weather_lohi, (self.B, 2)), ("weather_offset", weather_offset, (self.B,))):
      if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != shape
                            or t.device != self.tdev or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float64 {list(shape)} tensor on {self.tdev}")
    desc, keep = es.c_desc(0 if weather_lohi is None else weather_lohi.data_ptr(),
                           0 if weather_offset is None else weather_offset.data_ptr())
    self._draws_call("sb_episode_starts_attach", C.byref(desc))
    del keep
    self._episode_starts = es

  def episode_starts_detach(self) -> None:
    """sb_episode_starts_detach: from its next reset on, every building is back on its attached offset and the weather
    entries of the attach, bit for bit; the episode in progress finishes where it is."""
    self._draws_call("sb_episode_starts_detach")
    self._episode_starts = None

  @property
  def episode_starts(self) -> Optional[host_inputs.EpisodeStarts]:
    return self._episode_starts

  def episode_start_episodes(self) -> torch.Tensor:
    """sb_episode_starts_episodes_get: int32 [B] on the device, the number of every building's NEXT episode (this
    feature's own counter).  Snapshots carry neither the values nor the counters: a checkpoint keeps the counters with
    this pair."""
    return self._episodes_get("sb_episode_starts_episodes_get", value_errors=(-1, -5))

  def set_episode_start_episodes(self, t: torch.Tensor) -> None:
    """sb_episode_starts_episodes_set: the counters <- t (int32 [B] on the device, contiguous), and the values in force
    <- ``values(b, t[b] - 1)`` (the attached values where t[b] == 0)."""
    self._episodes_set("sb_episode_starts_episodes_set", t, value_errors=(-1, -5))

  def clock_offsets_in_force(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """sb_episode_starts_values_get: (offsets, effective offsets), int32 [B] each, stream-ordered copies -- the buildings'
    attached offsets as the last draw or ``clock_set_offsets`` left them, and what the kernels index (offset minus the
    building's restart position)."""
    offs = torch.empty((self.B,), dtype=torch.int32, device=self.tdev)
    eff = torch.empty_like(offs)
    self._draws_call("sb_episode_starts_values_get", C.c_void_p(offs.data_ptr()), C.c_void_p(eff.data_ptr()), self._stream())
    return offs, eff

  def clock_set_offsets(self, offsets: np.ndarray) -> None:
    """sb_clock_set_offsets: new attached offsets (int32 [B], inside the table), each taken by its building at its next
    reset; the episodes in progress keep their rows.  Refused while attached episode starts draw the offsets."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    if offsets.shape != (self.B,):
      raise ValueError(f"clock_set_offsets needs offsets [{self.B}]")
    self._draws_call("sb_clock_set_offsets", offsets.ctypes.data_as(C.c_void_p), self._stream())
    self._clock_offsets = offsets.copy()

  # ---- episode totals per building (sb_episode_metrics_attach) ----
  EPISODE_METRIC_NAMES = _ffi.EPISODE_METRIC_NAMES

  def episode_metrics_attach(self) -> None:
    """sb_episode_metrics_attach: from now on every step adds to each building's running row of episode totals (return,
    energy, cost, carbon, ...: ``EPISODE_METRIC_NAMES``, include/sbsim_amd.h states each), and every reset of a building
    that has stepped closes its episode into its completed row.  One more launch per step, on tables allocated here;
    attaching again re-initialises them.  The call synchronises the device, not under stream capture.  Not part of a
    snapshot: ``episode_metrics`` / ``completed_episodes`` / ``episode_metrics_set`` are how a checkpoint keeps them."""
    self._draws_call("sb_episode_metrics_attach")
    self._episode_metrics = True

  def episode_metrics_detach(self) -> None:
    """sb_episode_metrics_detach: the tables go; the simulator launches what it launched before the attach."""
    self._draws_call("sb_episode_metrics_detach")
    self._episode_metrics = False

  @property
  def episode_metrics_attached(self) -> bool:
    return self._episode_metrics

  def _episode_metrics_get(self, running: bool) -> torch.Tensor:
    out = torch.empty((self.B, _ffi.SB_EM_FIELDS), dtype=torch.float64, device=self.tdev)
    ptr = C.c_void_p(out.data_ptr())
    self._draws_call("sb_episode_metrics_get", ptr if running else None, None if running else ptr, self._stream())
    return out

  def episode_metrics(self) -> torch.Tensor:
    """sb_episode_metrics_get: the running rows, float64 [B, 20] on the device (columns: ``EPISODE_METRIC_NAMES``), a
    stream-ordered copy -- the totals of every building's episode in progress.  ValueError without an attachment."""
    return self._episode_metrics_get(True)

  def completed_episodes(self) -> torch.Tensor:
    """sb_episode_metrics_get: the completed rows, float64 [B, 20] on the device -- the totals of every building's last
    closed episode (``episode`` -1, no steps: none closed since the attach)."""
    return self._episode_metrics_get(False)

  def episode_metrics_set(self, running: Optional[torch.Tensor], completed: Optional[torch.Tensor]) -> None:
    """sb_episode_metrics_set: puts back what ``episode_metrics()`` / ``completed_episodes()`` returned (either may be
    None, not both), bit for bit."""
    ptrs = []
    for t in (running, completed):
      if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self.tdev
                            or tuple(t.shape) != (self.B, _ffi.SB_EM_FIELDS) or not t.is_contiguous()):
        raise ValueError(f"episode metrics must be contiguous float64 [{self.B}, {_ffi.SB_EM_FIELDS}] tensors on {self.tdev}")
      ptrs.append(C.c_void_p(t.data_ptr()) if t is not None else None)
    self._draws_call("sb_episode_metrics_set", ptrs[0], ptrs[1], self._stream())

  # ---- every building scored against recorded zone temperatures (sb_telemetry_attach) ----
  TELEMETRY_SCORE_NAMES = _ffi.TELEMETRY_SCORE_NAMES
  TELEMETRY_ZONE_SCORE_NAMES = _ffi.TELEMETRY_ZONE_SCORE_NAMES

  def telemetry_attach(self, tel: host_inputs.Telemetry) -> None:
    """sb_telemetry_attach: from now on every step compares each building's post-update zone means with its row of the
    recording ``tel`` and adds to its running row of scores (``TELEMETRY_SCORE_NAMES``, include/sbsim_amd.h states
    each), and every reset of a building that has stepped closes its episode into its completed row.  One more launch
    per step, on tables allocated here; the library copies the arrays; attaching again replaces the recording and
    re-initialises the tables.  The call synchronises the device, not under stream capture.  Not part of a snapshot:
    ``telemetry_scores`` / ``completed_telemetry_scores`` / ``telemetry_set`` are how a checkpoint keeps them."""
    if not isinstance(tel, host_inputs.Telemetry):
      raise ValueError("telemetry_attach needs a host_inputs.Telemetry (telemetry_detach clears it)")
    tel.check(self.B, self.Z, self.n_actions)
    d = _ffi.Telemetry()
    traces = np.ascontiguousarray(tel.zone_temps, dtype=np.float64)
    keep = [traces]
    d.traces, d.n_traces, d.n_rows = traces.ctypes.data_as(_ffi._dp), tel.n_traces, tel.n_rows
    for name, ptr_t, dtype in (("trace_of", _ffi._ip, np.int32), ("first_row", _ffi._ip, np.int32),
                               ("zone_weights", _ffi._dp, np.float64), ("actions", C.POINTER(C.c_float), np.float32)):
      a = getattr(tel, name)
      if a is not None:
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        setattr(d, name, a.ctypes.data_as(ptr_t))
    d.n_actions, d.per_zone = tel.n_actions, int(tel.per_zone)
    self._draws_call("sb_telemetry_attach", C.byref(d))
    self._telemetry = tel

  def telemetry_detach(self) -> None:
    """sb_telemetry_detach: the tables and the recording go; the simulator launches what it launched before the attach."""
    self._draws_call("sb_telemetry_detach")
    self._telemetry = None

  @property
  def telemetry(self) -> Optional[host_inputs.Telemetry]:
    return self._telemetry

  def _telemetry_get(self, running: bool, zone: bool) -> torch.Tensor:
    shape = (self.B, self.Z, _ffi.SB_TL_ZONE_FIELDS) if zone else (self.B, _ffi.SB_TL_FIELDS)
    out = torch.empty(shape, dtype=torch.float64, device=self.tdev)
    ptr = C.c_void_p(out.data_ptr())
    self._draws_call("sb_telemetry_zone_get" if zone else "sb_telemetry_get", ptr if running else None, None if running else ptr,
                     self._stream())
    return out

  def telemetry_scores(self) -> torch.Tensor:
    """sb_telemetry_get: the running rows, float64 [B, 13] on the device (columns: ``TELEMETRY_SCORE_NAMES``), a
    stream-ordered copy -- the scores of every building's episode in progress.  ValueError without an attachment."""
    return self._telemetry_get(True, False)

  def completed_telemetry_scores(self) -> torch.Tensor:
    """sb_telemetry_get: the completed rows, float64 [B, 13] -- the scores of every building's last closed episode
    (``episode`` -1, no steps: none closed since the attach)."""
    return self._telemetry_get(False, False)

  def telemetry_zone_scores(self) -> torch.Tensor:
    """sb_telemetry_zone_get: the running per-zone rows, float64 [B, Z, 4] (``TELEMETRY_ZONE_SCORE_NAMES``).  ValueError
    without an attachment, or one without ``per_zone``."""
    return self._telemetry_get(True, True)

  def completed_telemetry_zone_scores(self) -> torch.Tensor:
    """sb_telemetry_zone_get: the completed per-zone rows, float64 [B, Z, 4]."""
    return self._telemetry_get(False, True)

  def telemetry_set(self, running: Optional[torch.Tensor] = None, completed: Optional[torch.Tensor] = None,
                    zone_running: Optional[torch.Tensor] = None, zone_completed: Optional[torch.Tensor] = None) -> None:
    """sb_telemetry_set / sb_telemetry_zone_set: puts back what the four readers returned, bit for bit; any may be None,
    not all."""
    if all(t is None for t in (running, completed, zone_running, zone_completed)):
      raise ValueError("telemetry_set needs at least one table")
    for name, shape, pair in (("sb_telemetry_set", (self.B, _ffi.SB_TL_FIELDS), (running, completed)),
                              ("sb_telemetry_zone_set", (self.B, self.Z, _ffi.SB_TL_ZONE_FIELDS), (zone_running, zone_completed))):
      ptrs = []
      for t in pair:
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self.tdev
                              or tuple(t.shape) != shape or not t.is_contiguous()):
          raise ValueError(f"telemetry tables must be contiguous float64 {list(shape)} tensors on {self.tdev}")
        ptrs.append(C.c_void_p(t.data_ptr()) if t is not None else None)
      if ptrs[0] is not None or ptrs[1] is not None:
        self._draws_call(name, ptrs[0], ptrs[1], self._stream())

  def telemetry_actions(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sb_telemetry_actions: the recorded setpoints of every building's next step, float32 [B, A] on the device -- row
    ``first_row[b] + steps_b`` of the building's trace, the last row past the end of the recording.  ValueError without an
    attachment or without recorded actions."""
    if out is None:
      out = torch.empty((self.B, self.n_actions), dtype=torch.float32, device=self.tdev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != self.tdev
          or tuple(out.shape) != (self.B, self.n_actions) or not out.is_contiguous()):
      raise ValueError(f"out must be a contiguous float32 [{self.B}, {self.n_actions}] tensor on {self.tdev}")
    self._draws_call("sb_telemetry_actions", C.c_void_p(out.data_ptr()), self._stream())
    return out

  # ---- state snapshots (sb_state_save / sb_state_load) ----
  def state_fingerprint(self) -> Tuple:
    """What a SimState of this simulator means: plan shape and zones, a hash of the compiled plan tables (in the
    caller's orientation) and of SimConfig.to_params(), the attached device generators -- and, when it is not the
    default, the reward function (its kind and constants: the reward a restored batch replays).  Not the layout, the
    orientation or the sweep kernel: a snapshot moves between them."""
    if self._fingerprint is None:
      if self._materials_handle:   # the structural tables (caller's orientation): the coefficients are the rows', not the plan's
        sp = self.plan.compile_structural(self.config.time_step_sec)
        tables = (sp.cell_class, sp.class_desc, sp.class_diffuser, sp.class_zone, sp.zone_off, sp.zone_cells)
      else:
        cp = self.plan.compile(self.config.time_step_sec, self._h_conv)
        tables = (cp.cell_class, cp.class_coef, cp.class_zone, cp.zone_off, cp.zone_cells)
      prm = self.config.to_params()
      vals = []
      for name, ctype in _ffi.PARAM_FIELDS:
        v = getattr(prm, name)
        vals.append(repr([v[i] for i in range(prm.n_actions)]) if name.startswith("act_") else repr(v))
      params_hash = hashlib.sha256(repr(vals).encode()).hexdigest()
      self._fingerprint = ((self.H, self.W, self.Z), _sha(*tables), params_hash)
    fp = self._fingerprint + (self._occ_attached, self._conv_attached)
    if self._reward_function is not None:   # (the default adds nothing: checkpoints from before the option still load)
      fp += (("reward_function",) + self._reward_function.as_tuple(),)
    if self._materials_handle:   # (a table is configuration, not state: the marker says which class map the state means)
      fp += (("building_materials",),)
    if self._clock_offsets is not None:   # (the offsets stay with the slots; a snapshot restores where they are the same)
      fp += (("clock", _sha(self._clock_offsets)),)
    if self._calendars is not None:   # (only with calendars: checkpoints from before them still load)
      fp += (("calendars",) + self._calendars,)
    if self._initial_conditions is not None:   # (configuration of the slots: a snapshot restores where it is the same)
      fp += (("initial_conditions", self._initial_conditions.digest()),)
    if self._randomization is not None:   # (likewise; the rows and the counters are not in a snapshot)
      fp += (("episode_randomization", self._randomization.digest()),)
    if self._episode_starts is not None:   # (likewise; the values and the counters are not in a snapshot)
      fp += (("episode_starts", self._episode_starts.digest()),)
    return fp

  def save_state(self, rows: Optional[torch.Tensor] = None) -> SimState:
    """Snapshot of every building (``rows`` None) or of buildings ``rows`` (int32 / int64 [n] on the device; row i of
    the snapshot holds building rows[i]).  Stream-ordered on the current stream."""
    self._refuse_on_jacobi("save_state")
    pick, n = None, self.B
    if rows is not None:
      pick = self._check_index(rows, None, 0, self.B, "rows")
      n = int(pick.shape[0])
    dev = self.tdev
    st = SimState(torch.empty((n, self.H * self.W), dtype=torch.float64, device=dev),
                  torch.empty((n, 4, self.Z), dtype=torch.float64, device=dev),
                  torch.empty((n, self.Z), dtype=torch.int32, device=dev),
                  torch.empty((n, _ffi.SB_STATE_NUM_SCALARS), dtype=torch.float64, device=dev),
                  torch.empty((n,), dtype=torch.int32, device=dev),
                  torch.empty((n, self.Z), dtype=torch.int32, device=dev) if self._occ_attached else None,
                  (0, 0, 0, 0), self.state_fingerprint())
    clk = _ffi.StateClock()
    _ffi.check(_ffi.state_entry("sb_state_save")(
        self._h, None if pick is None else C.c_void_p(pick.data_ptr()), n, C.byref(st.view()), C.byref(clk),
        int(self.transposed), self._stream()), "sb_state_save")
    st.clock = (clk.occ_queries, clk.conv_calls, clk.steps_since_reset, clk.was_reset)
    if self._conv_seeded and rows is None:   # the slots' streams (rows: a fork's source rows -- streams stay with the slots)
      st.conv_rng = self.convection_rng()
    return st

  def load_state(self, state: SimState, pick: Optional[torch.Tensor] = None, clock: bool = True) -> None:
    """Building b <- row pick[b] of ``state`` (pick: int32 / int64 [B] on the device, < 0 keeps building b; None:
    row b, state.n == B).  clock: also set the handle's counters (occupancy / convection draws, steps since reset) to
    the snapshot's -- a restore; False for a fork, whose counters go on.  Raises ValueError for a state of another
    fingerprint, or a pick of the wrong shape, dtype, device or range, before anything is launched."""
    self._refuse_on_jacobi("load_state")
    if not isinstance(state, SimState):
      raise ValueError("load_state needs a SimState")
    if state.fingerprint != self.state_fingerprint():
      raise ValueError("this SimState belongs to another floor plan, configuration or generator set: "
                       f"{state.fingerprint} != {self.state_fingerprint()}")
    n = state.n
    shapes = dict(grid=(n, self.H * self.W), zone=(n, 4, self.Z), mode=(n, self.Z),
                  scal=(n, _ffi.SB_STATE_NUM_SCALARS), nsw=(n,), occ=(n, self.Z))
    dtypes = dict(grid=torch.float64, zone=torch.float64, scal=torch.float64, mode=torch.int32, nsw=torch.int32,
                  occ=torch.int32)
    for k, t in state.tensors().items():
      if t is None:
        continue
      if (tuple(t.shape) != shapes[k] or t.dtype != dtypes[k] or t.device != self.tdev or not t.is_contiguous()
          or t.data_ptr() % 16):
        raise ValueError(f"SimState.{k}: expected a contiguous {dtypes[k]} {shapes[k]} tensor on {self.tdev}")
    if pick is None:
      if n != self.B:
        raise ValueError(f"a SimState of {n} rows loads into {self.B} buildings only with a pick")
    else:
      pick = self._check_index(pick, self.B, -(1 << 31), n, "pick")
    restore_rng = self._conv_seeded and clock and pick is None   # (a fork leaves every slot's stream in place)
    if restore_rng:
      if state.conv_rng is None:
        raise ValueError("this SimState carries no convection generators (conv_rng), the simulator has the seeded convection "
                         "attached: a restore would not replay")
      t = state.conv_rng
      if (tuple(t.shape) != (self.B, _ffi.SB_CONV_RNG_WORDS) or t.dtype != torch.int32 or t.device != self.tdev
          or not t.is_contiguous()):
        raise ValueError(f"SimState.conv_rng: expected a contiguous int32 [{self.B}, {_ffi.SB_CONV_RNG_WORDS}] tensor on {self.tdev}")
    clk = _ffi.StateClock(*state.clock) if clock else None
    _ffi.check(_ffi.state_entry("sb_state_load")(
        self._h, None if pick is None else C.c_void_p(pick.data_ptr()), C.byref(state.view()),
        C.byref(clk) if clk is not None else None, int(self.transposed), self._stream()), "sb_state_load")
    if restore_rng:
      self.set_convection_rng(state.conv_rng)

  def _check_index(self, t: torch.Tensor, length: Optional[int], lo: int, hi: int, what: str) -> torch.Tensor:
    """A device index vector, checked on the host: int32 / int64, 1-D (of `length`), values in [lo, hi) (lo < 0: a
    negative value is allowed and means "none").  Returns it as contiguous int32."""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
      raise ValueError(f"{what} must be an int32 or int64 tensor")
    if t.dim() != 1 or (length is not None and t.shape[0] != length) or t.shape[0] == 0:
      raise ValueError(f"{what} must be a non-empty 1-D tensor" + (f" of {length}" if length is not None else ""))
    if t.device != self.tdev:
      raise ValueError(f"{what} must be on {self.tdev}")
    if int(t.max()) >= hi or int(t.min()) < lo:
      raise ValueError(f"{what} out of range: its values must be below {hi}" + ("" if lo < 0 else f" and >= {lo}"))
    return t.to(torch.int32).contiguous()

  # ---- parity taps ----
  def _get(self, fn, shape, dtype):
    out = torch.empty(shape, dtype=dtype, device=self.tdev)
    _ffi.check(fn(self._h, C.c_void_p(out.data_ptr()), self._stream()), fn.__name__)
    return out

  def temps(self) -> torch.Tensor:
    if self.transposed:
      t = self._get(self._lib.sb_get_temps, (self.B, self.W, self.H), torch.float64)
      return t.transpose(1, 2).contiguous()
    return self._get(self._lib.sb_get_temps, (self.B, self.H, self.W), torch.float64)

  def set_temps(self, temps: torch.Tensor) -> None:
    """sb_set_temps: building.temp <- temps ([B, H, W] float64 on the device) between two steps; every
    device state stays (what Building.apply_convection does to the reference's array, building.py:891-893)."""
    self._refuse_on_jacobi("set_temps")
    if temps.dtype != torch.float64 or tuple(temps.shape) != (self.B, self.H, self.W):
      raise ValueError(f"temps must be float64 [{self.B}, {self.H}, {self.W}]")
    t = temps.transpose(1, 2).contiguous() if self.transposed else temps.contiguous()
    _ffi.check(self._lib.sb_set_temps(self._h, C.c_void_p(t.data_ptr()), self._stream()), "sb_set_temps")

  def zone_temps(self) -> torch.Tensor:
    return self._get(self._lib.sb_get_zone_temps, (self.B, self.Z), torch.float64)

  def scalars(self) -> torch.Tensor:
    return self._get(self._lib.sb_get_scalars, (self.B, _ffi.SB_NUM_SCALARS), torch.float64)

  def modes(self) -> torch.Tensor:
    return self._get(self._lib.sb_get_modes, (self.B, self.Z), torch.int32)

  def zone_power(self) -> torch.Tensor:
    return self._get(self._lib.sb_get_zone_power, (self.B, self.Z), torch.float64)

  # ---- spatial outputs (sb_spatial_attach / sb_spatial) ----
  def spatial_attach(self, pool: Optional[Tuple[int, int]] = None) -> None:
    """sb_spatial_attach: builds the index tables of ``zone_temp_stats`` / ``temperature_map`` / ``spatial``.
    ``pool``: (pool_h, pool_w) of the pooled map on the caller's [H, W] grid; None: zone statistics only.  Attaching again
    replaces the tables.  Not state: it enters neither ``state_fingerprint()`` nor a ``SimState``."""
    attach = _ffi.spatial_entry("sb_spatial_attach")
    if pool is None:
      ph = pw = 0
      shape = None
    else:
      try:
        ph, pw = (operator.index(x) for x in pool)
      except (TypeError, ValueError):
        raise ValueError("pool must be (pool_h, pool_w), two integers >= 1, or None") from None
      if ph < 1 or pw < 1 or ph >= 1 << 31 or pw >= 1 << 31:
        raise ValueError("pool must be (pool_h, pool_w), two integers >= 1, or None")
      mh, mw = C.c_int32(), C.c_int32()
      _ffi.check(_ffi.spatial_entry("sb_spatial_shape")(self.H, self.W, ph, pw, C.byref(mh), C.byref(mw)), "sb_spatial_shape")
      shape = (mh.value, mw.value)
    with torch.cuda.device(self.device):
      _ffi.check(attach(self._h, ph, pw, int(self.transposed)), "sb_spatial_attach")
    self._spatial = (True, shape)

  @property
  def map_shape(self) -> Optional[Tuple[int, int]]:
    """(map_h, map_w) of ``temperature_map`` as attached, or None (no pool, or nothing attached)."""
    return self._spatial[1]

  def spatial(self, rows: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None,
              map_out: Optional[torch.Tensor] = None, stats: bool = True, map: Optional[bool] = None):  # pylint: disable=redefined-builtin
    """sb_spatial: ONE launch on the current stream.  Returns (zone statistics [n, Z, 3] float64 {min, max, mean},
    pooled map [n, map_h, map_w] float32); row i is building rows[i] (int32 / int64 [n] on the device), or building i
    (``rows`` None, n == B).  ``stats`` / ``map`` False leave that output out (None in its place); ``map`` defaults to
    "a pool is attached".  ``stats_out`` / ``map_out``: the tensors to write (contiguous, of that shape and dtype, on
    the device); rows of a repeated pick are written more than once, with the same values.  ValueError before any launch
    for rows of the wrong dtype, shape, device or range, for outputs that do not fit, and for a map without a pool."""
    fn = _ffi.spatial_entry("sb_spatial")
    attached, shape = self._spatial
    if not attached:
      raise ValueError("spatial outputs need spatial_attach() first")
    if map is None:
      map = shape is not None or map_out is not None
    if map and shape is None:
      raise ValueError("temperature_map needs a pool size: spatial_attach(pool=(pool_h, pool_w))")
    if not stats and not map:
      raise ValueError("spatial: nothing asked for (stats and map both off)")
    pick, n = None, self.B
    if rows is not None:
      pick = self._check_index(rows, None, 0, self.B, "rows")
      n = int(pick.shape[0])
    outs = []
    for want, out, shp, dtype, what in ((stats, stats_out, (n, self.Z, 3), torch.float64, "stats_out"),
                                        (map, map_out, (n,) + (shape or (0, 0)), torch.float32, "map_out")):
      if not want:
        if out is not None:
          raise ValueError(f"{what} given, but that output is off")
        outs.append(None)
        continue
      if out is None:
        out = torch.empty(shp, dtype=dtype, device=self.tdev)
      elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != shp or out.dtype != dtype or out.device != self.tdev
            or not out.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous {dtype} {shp} tensor on {self.tdev}")
      outs.append(out)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = fn(self._h, ptr(pick), n, ptr(outs[0]), ptr(outs[1]), self._stream())
    if rc == -1:   # SB_ERR_INVALID (before sb_reset, ...)
      raise ValueError((self._lib.sb_last_error() or b"").decode())
    _ffi.check(rc, "sb_spatial")
    return outs[0], outs[1]

  def zone_temp_stats(self, rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Building.get_zone_temp_stats for every zone (building.py:564-577): [n, Z, 3] float64 {min, max, mean}."""
    return self.spatial(rows, stats_out=out, stats=True, map=False)[0]

  def temperature_map(self, rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The grid pooled by the attached (pool_h, pool_w): [n, map_h, map_w] float32 tile means."""
    return self.spatial(rows, map_out=out, stats=False, map=True)[1]


@dataclasses.dataclass
class EnvSnapshot:
  """``BatchedEnvironment.snapshot()``: the simulator's ``SimState``, the environment's host clock, deep copies of its
  stateful host models (a shared ``RandomizedArrivalDepartureOccupancy`` draws from its ``np.random.RandomState``
  every step) and copies of the current TimeStep and info.  ``state_dict()`` / ``from_state_dict`` give a form
  ``torch.save`` / ``torch.load`` (``weights_only`` too) take, so that another process can restore it into an environment of the
  same floor plan and configuration; the host models travel pickled inside it -- load checkpoints you trust."""
  sim: SimState
  host: Dict              # _now, _step_count, _episode_count, _episode_ended, _needs_reset, _prev_thermostat_ts
  rejected: Optional[torch.Tensor]   # the per-building rejection flags of the last step that had any (or None)
  models: Dict            # attribute name -> deep copy of a stateful host model
  observation: torch.Tensor
  reward: torch.Tensor
  info: Optional[torch.Tensor]

  def state_dict(self) -> dict:
    cpu = lambda t: None if t is None else t.cpu()
    enc = lambda v: (["datetime", v.isoformat()] if isinstance(v, dt.datetime) else v)
    return dict(kind="sbsim_amd.EnvSnapshot", sim=self.sim.state_dict(), host={k: enc(v) for k, v in self.host.items()},
                rejected=cpu(self.rejected), models=pickle.dumps(self.models), observation=cpu(self.observation),
                reward=cpu(self.reward), info=cpu(self.info), fingerprint=list(self.sim.fingerprint))

  @staticmethod
  def from_state_dict(d: Mapping, device) -> "EnvSnapshot":
    if not isinstance(d, Mapping) or d.get("kind") != "sbsim_amd.EnvSnapshot" or "sim" not in d:
      raise ValueError("not an EnvSnapshot state_dict")
    if "fingerprint" not in d or _as_fingerprint(d["fingerprint"]) != _as_fingerprint(d["sim"].get("fingerprint", ())):
      raise ValueError("EnvSnapshot state_dict: fingerprint missing or not that of its simulator state")
    dec = lambda v: (dt.datetime.fromisoformat(v[1]) if isinstance(v, (list, tuple)) and len(v) == 2
                     and v[0] == "datetime" else v)
    to = lambda t: None if t is None else t.to(device).contiguous()
    return EnvSnapshot(SimState.from_state_dict(d["sim"], device), {k: dec(v) for k, v in d["host"].items()},
                       to(d["rejected"]), pickle.loads(d["models"]), to(d["observation"]), to(d["reward"]), to(d["info"]))


class BatchedEnvironment:
  """B lock-stepped sbsim environments behind ``reset()`` / ``step(action)``.

  ``start_timestamp``: naive by default (see SB1_START_TIMESTAMP for the SB1 configuration's own).
  The TimeStep tensors returned by ``reset`` / ``step`` are the environment's own device buffers and
  are overwritten by the next call: clone what must outlive a step (replay buffers, n-step returns)."""

  def __init__(self, plan: FloorPlan, n_buildings: int, config: Optional[SimConfig] = None,
               weather=None, occupancy=None, start_timestamp=dt.datetime(2023, 7, 6, 7, 0, 0),
               num_days_in_episode: float = 3, discount_factor: float = 1.0, device: int = 0,
               observation_normalization: Optional[Mapping[str, Tuple[float, float]]] = None,
               occupancy_normalization_constant: float = 0.0, holiday_calendar="us",
               electricity_energy_cost=None, natural_gas_energy_cost=None, collect_info: bool = False,
               observation_histogram_parameters: Optional[Sequence[Tuple[str, Sequence[float]]]] = None,
               normalize_reduce: bool = False, convection_simulator=None, solver: str = "gauss_seidel",
               building_params: Optional[host_inputs.BuildingParams] = None,
               reward_function: Optional[host_inputs.SetpointEnergyCarbonReward] = None,
               building_materials: Optional[host_inputs.BuildingMaterials] = None, start_offsets=None,
               per_building_episodes: bool = False, episode_steps=None,
               calendars: Optional[Sequence[host_inputs.Calendar]] = None, calendar_of=None,
               spatial: Optional[host_inputs.SpatialOutputs] = None,
               initial_conditions: Optional[host_inputs.InitialConditions] = None,
               episode_randomization: Optional[host_inputs.EpisodeRandomization] = None,
               episode_starts: Optional[host_inputs.EpisodeStarts] = None, max_start_offset: Optional[int] = None,
               episode_metrics: bool = False, telemetry: Optional[host_inputs.Telemetry] = None):
    """``telemetry``: a ``host_inputs.Telemetry`` -- every building is scored against recorded zone temperatures on the
    device: ``telemetry_scores()`` the running rows, ``completed_telemetry_scores()`` each building's
    last closed episode, float64 [B, 13] with the columns ``TELEMETRY_SCORE_NAMES``, the per-zone readers with
    ``per_zone``, ``telemetry_actions()`` the recorded setpoints of every building's next step.  Works with and without
    ``per_building_episodes`` and ``collect_info``; not together with ``episode_starts`` (the rows follow a building's
    step count, not a drawn start).  None (the default): nothing of this is built or launched.
    ``episode_metrics``: True -- every building's episode totals are kept on the device:
    ``episode_metrics()`` the running rows, ``completed_episodes()`` each building's last closed episode, float64
    [B, 20] with the columns ``EPISODE_METRIC_NAMES``; works with and without ``collect_info``.  False (the default):
    nothing of this is built or launched.
    ``max_start_offset``: the largest row ``set_start_offsets`` may move a building to; the timeline is built to hold
    an episode that starts there (and the environment runs on the device clock).  None: the largest of ``start_offsets``.
    ``episode_starts``: a ``host_inputs.EpisodeStarts`` -- a start time (a row of the timeline) and weather per
    building, drawn anew at every reset of a building, on the device (``set_episode_starts`` between
    episodes, ``episode_start_values()`` the values in force).  Such an environment always runs on the device clock.
    None (the default): nothing of this is built or launched.
    ``episode_randomization``: a ``host_inputs.EpisodeRandomization`` -- per-building parameters and materials drawn
    anew at every reset of a building, on the device (``set_episode_randomization`` between episodes,
    ``randomized_values()`` the values in force).  None (the default): nothing of this is built or launched.
    ``initial_conditions``: a ``host_inputs.InitialConditions`` -- start temperatures per building (recorded grids,
    a number per building, an offset, a draw per episode), attached before the first ``reset()`` and used by every reset
    of a building: ``reset()``, the autoreset of ``per_building_episodes``, ``reset_buildings(mask)`` (INTEGRATION.md
    4o; ``set_initial_conditions`` between episodes).  None (the default): every cell starts at
    ``SimConfig.initial_temp``, and nothing of this is built or launched.
    ``spatial``: a ``host_inputs.SpatialOutputs`` -- ``temperature_map`` and / or ``zone_temp_stats`` of the state
    the returned observation describes, refreshed with one launch per call; with
    ``per_building_episodes`` also ``final_temperature_map`` / ``final_zone_temp_stats``, written like
    ``final_observation``.  None (the default): the attributes are None and nothing is built or launched.
    ``calendars`` / ``calendar_of``: several calendars in one batch.  ``calendars``: a list of K
    ``host_inputs.Calendar`` -- setpoint schedule, occupancy model, tariffs, a shared weather and the start date, each
    the environment's own where left None; ``calendar_of``: an integer array [B], building b's index into it.  Building
    b then lives at ``calendars[calendar_of[b]]``'s start ``+ (start_offsets[b] + step) * step_interval`` (zeros without
    ``start_offsets``) with that calendar's models; ``current_simulation_timestamp`` stays the batch's base clock.
    Device occupancy generators (``BatchedRandomizedArrivalDepartureOccupancy``) are every calendar's model or none's,
    with one seed, first_building and time_step_sec.  ValueError before anything is created for what
    ``host_inputs.check_calendars`` refuses.
    ``per_building_episodes`` / ``episode_steps``: episodes per building with same-step autoreset (INTEGRATION.md
    4k).  ``episode_steps``: an integer array [B], building b's step returns LAST when its own step count has reached
    ``episode_steps[b]`` (1 .. ``steps_per_episode``); giving it implies the flag, the flag alone gives every building
    ``steps_per_episode``.  ``step()`` then resets the buildings whose episode just ended on the device and returns
    their first observation of the new episode (their last one: ``final_observation``); ``reset_buildings(mask)`` ends
    episodes early.  Both left out (the default): nothing of this is built.
    ``start_offsets``: None -- every building lives at ``start_timestamp + step * step_interval``; an integer array
    [B] of whole step intervals (>= 0) -- building b lives at ``start_timestamp + (start_offsets[b] + step) *
    step_interval``: its own calendar (time features, setpoint schedule, tariffs, occupancy, weather) on the batch's one
    episode clock (``current_simulation_timestamps()``).
    ``solver``: the finite-difference solver (BatchedSimulator): "gauss_seidel" (default) or "jacobi_fp32"
    (TFSimulator, SB1's shipped configuration; no convection_simulator, snapshot, restore or fork).
    ``building_params``: per-building plant, setpoint and reward parameters (``set_building_params``).
    ``building_materials``: per-building materials and convection coefficient (``set_building_materials``); such an
    environment runs on k_sweep_lds, not with solver="jacobi_fp32", and its floor plan must fit that kernel.
    ``reward_function``: None -- the reference's SetpointEnergyCarbonRegretFunction with the SimConfig's arguments;
    a ``host_inputs.SetpointEnergyCarbonReward`` -- its SetpointEnergyCarbonRewardFunction (``set_reward_function``)."""
    if discount_factor <= 0 or discount_factor > 1:
      raise ValueError("Discount factor must be in (0,1]")   # environment.py:454-455
    if solver == "jacobi_fp32" and convection_simulator is not None:
      raise ValueError("a convection_simulator is not implemented for solver='jacobi_fp32'")
    if isinstance(convection_simulator, host_inputs.SeededStochasticConvectionSimulator):
      seeds = convection_simulator.seeds_for(int(n_buildings))   # (checked here: nothing is created for seeds of another shape)
    if initial_conditions is not None:   # (likewise)
      if not isinstance(initial_conditions, host_inputs.InitialConditions):
        raise ValueError("initial_conditions must be a host_inputs.InitialConditions (or None)")
      initial_conditions.check(int(n_buildings), tuple(plan.shape))
    self.per_building_episodes = bool(per_building_episodes) or episode_steps is not None
    if self.per_building_episodes and isinstance(occupancy, host_inputs.BatchedRandomizedArrivalDepartureOccupancy):
      raise ValueError("per_building_episodes: BatchedRandomizedArrivalDepartureOccupancy is not supported -- each of its "
                       "queries advances every building's occupants, so the observation of the buildings that restart "
                       "would draw for all the others too")
    self.config = config or SimConfig.sb1()
    self.weather = weather or host_inputs.WeatherController(273.0, 283.0, convection_coefficient=100.0)
    self.occupancy = occupancy or host_inputs.StepFunctionOccupancy(
        dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1, holiday_calendar=holiday_calendar)
    self.schedule = self.config.schedule()
    self.electricity = electricity_energy_cost or host_inputs.ElectricityEnergyCost(
        holiday_calendar=holiday_calendar)
    self.gas = natural_gas_energy_cost or host_inputs.NaturalGasEnergyCost()
    self.discount_factor = float(discount_factor)
    self._start_timestamp = host_inputs.as_datetime(start_timestamp)
    self._occ_norm = float(occupancy_normalization_constant)
    h_conv = self.weather.get_air_convection_coefficient(self._start_timestamp)
    self.calendars = self.calendar_of = None
    occupancy_groups = None   # the calendars' device occupancy generators (one per calendar), or None
    if calendars is not None or calendar_of is not None:
      if calendars is None:
        raise ValueError("calendar_of needs calendars: the list of host_inputs.Calendar it indexes")
      self.calendar_of = host_inputs.check_calendars(calendars, calendar_of, int(n_buildings), self.weather, self.occupancy,
                                                     self._start_timestamp, self.config.comfort_temp_window,
                                                     self.config.eco_temp_window)
      self.calendars = list(calendars)
      occupancy_groups = host_inputs.device_occupancy_groups(self.calendars, self.occupancy)
      if occupancy_groups is not None and self.per_building_episodes:
        raise ValueError("per_building_episodes: BatchedRandomizedArrivalDepartureOccupancy is not supported -- each of its "
                         "queries advances every building's occupants, so the observation of the buildings that restart "
                         "would draw for all the others too")
      if start_offsets is not None:   # (checked here: nothing is created for offsets the timeline would refuse)
        start_offsets = host_inputs.check_start_offsets(start_offsets, int(n_buildings))
    if episode_randomization is not None:   # (checked here: nothing is created for a randomisation the library would refuse)
      if not isinstance(episode_randomization, host_inputs.EpisodeRandomization):
        raise ValueError("episode_randomization must be a host_inputs.EpisodeRandomization (or None)")
      if building_params is not None and not isinstance(building_params, host_inputs.BuildingParams):
        raise ValueError("building_params must be a host_inputs.BuildingParams (or None)")
      episode_randomization.check(
          int(n_buildings), host_inputs.effective_building_params(building_params, self.config, int(n_buildings)),
          None if building_materials is None else host_inputs.effective_building_materials(
              building_materials, plan.material_slots()[1], h_conv, int(n_buildings)), solver)
    if max_start_offset is not None and (isinstance(max_start_offset, bool) or not isinstance(max_start_offset, (int, np.integer))
                                         or not 0 <= max_start_offset <= (1 << 22)):
      raise ValueError(f"max_start_offset must be an integer >= 0 (and at most 2^22), got {max_start_offset!r}")
    if telemetry is not None:   # (before anything is built)
      if not isinstance(telemetry, host_inputs.Telemetry):
        raise ValueError("telemetry must be a host_inputs.Telemetry (or None)")
      if episode_starts is not None:
        raise ValueError("telemetry together with episode_starts: the recording's rows follow a building's step count, not a "
                         "drawn start time")
    if episode_starts is not None:   # (likewise)
      if not isinstance(episode_starts, host_inputs.EpisodeStarts):
        raise ValueError("episode_starts must be a host_inputs.EpisodeStarts (or None)")
      episode_starts.check(int(n_buildings), self.weather, calendars)
      if start_offsets is not None and calendars is None:
        start_offsets = host_inputs.check_start_offsets(start_offsets, int(n_buildings))
    self.sim = BatchedSimulator(plan, self.config, n_buildings, h_conv, device,
                                observation_normalization,
                                histogram_parameters=observation_histogram_parameters,
                                normalize_reduce=normalize_reduce, solver=solver, building_materials=building_materials)
    self.batch_size = self.sim.B
    if building_params is not None:
      self.sim.set_building_params(building_params)
    if reward_function is not None:
      self.sim.set_reward_function(reward_function)
    if initial_conditions is not None:
      self.sim.initial_conditions_attach(initial_conditions)
    if episode_randomization is not None:
      self.sim.randomization_attach(episode_randomization)
    self._weather_lohi = self._weather_replay = None
    if isinstance(self.weather, host_inputs.BatchedReplayWeather):
      if self.weather.offsets_sec.shape[0] != self.batch_size:
        raise ValueError("BatchedReplayWeather needs one offset per building")
      td = lambda a: torch.tensor(a, dtype=torch.float64, device=self.sim.tdev).contiguous()
      self._weather_replay = (td(self.weather.times), td(self.weather.temps_f), td(self.weather.offsets_sec))
    if isinstance(self.weather, host_inputs.BatchedSinusoidWeather):
      if self.weather.low.shape[0] != self.batch_size:
        raise ValueError("BatchedSinusoidWeather needs one (low, high) pair per building")
      self._weather_lohi = torch.tensor(np.stack([self.weather.low, self.weather.high], axis=1),
                                        dtype=torch.float64, device=self.sim.tdev).contiguous()
    if isinstance(convection_simulator, host_inputs.SeededStochasticConvectionSimulator):
      c = convection_simulator
      self.sim.convection_attach_seeded(c.p, c.distance, seeds)
    elif convection_simulator is not None:   # simulator_flexible_floor_plan.py:71,156
      c = convection_simulator
      self.sim.convection_attach(c.p, c.distance, c.seed or 0, getattr(c, "first_building", 0))
    self._occ_count = self._occ_total = None
    if occupancy_groups is not None or (self.calendars is None and isinstance(
        self.occupancy, host_inputs.BatchedRandomizedArrivalDepartureOccupancy)):
      if occupancy_groups is not None:   # a generator per calendar: the building's group is its calendar
        self.sim.occupancy_attach_groups([(o.zone_assignment, o.hours, o.time_step_sec, o.seed or 0, o.first_building)
                                          for o in occupancy_groups], self.calendar_of)
      else:
        o = self.occupancy   # per-building occupants live on the device
        self.sim.occupancy_attach(o.zone_assignment, o.hours, o.time_step_sec, o.seed or 0, o.first_building)
      self._occ_count = torch.zeros((self.batch_size, self.sim.Z), dtype=torch.float32, device=self.sim.tdev)
      self._occ_total = torch.zeros((self.batch_size,), dtype=torch.float32, device=self.sim.tdev)
    self._step_interval = dt.timedelta(seconds=self.config.time_step_sec)
    # environment.py:427-435
    self._num_timesteps_in_episode = int(dt.timedelta(days=num_days_in_episode) / self._step_interval)
    self.start_offsets = self.timeline = self._cursor = None
    self._offsets_moved = False   # drawn starts or set_start_offsets: the offsets in force are the device's from then on
    if self.calendars is not None:   # several calendars: their row tables one after the other, always on the clock path
      self.timeline = host_inputs.CalendarTimeline(self.calendars, self.calendar_of, self._models(), self._start_timestamp,
                                                   start_offsets, self._num_timesteps_in_episode)
      self.start_offsets = self.timeline.start_offsets
      self.sim.clock_attach(self.timeline.rows, self.timeline.offsets, calendar_of=self.calendar_of)
      self._cursor = host_inputs.ClockCursor()
    elif start_offsets is not None or episode_starts is not None or max_start_offset is not None:
      # a calendar per building: the table of instants, built once, and the offsets into it (episode_starts: all zero
      # without start_offsets, the table sized for the largest draw)
      self.start_offsets = (None if start_offsets is None
                            else host_inputs.check_start_offsets(start_offsets, self.batch_size))
      offsets = np.zeros(self.batch_size, dtype=np.int32) if self.start_offsets is None else self.start_offsets
      self.timeline = host_inputs.Timeline(self._models(), self._start_timestamp, offsets,
                                           self._num_timesteps_in_episode, episode_starts=episode_starts,
                                           max_offset=max_start_offset)
      self.sim.clock_attach(self.timeline.rows, offsets)
      self._cursor = host_inputs.ClockCursor()
    self.episode_steps = self.final_observation = None
    if self.per_building_episodes:
      self._setup_episodes(episode_steps)
    if episode_starts is not None:
      self._attach_starts(episode_starts)
    self.has_episode_metrics = bool(episode_metrics)
    if self.has_episode_metrics:
      self.sim.episode_metrics_attach()
    self.has_telemetry = telemetry is not None
    if self.has_telemetry:
      self.sim.telemetry_attach(telemetry)
    self._action_spec = ArraySpec((self.sim.n_actions,), np.dtype(np.float32), "action", -1.0, 1.0)
    self._observation_spec = ArraySpec((self.sim.O,), np.dtype(np.float32), "observation")
    self.field_names = self.sim.field_names
    dev = self.sim.tdev
    self._obs = torch.zeros((self.batch_size, self.sim.O), dtype=torch.float32, device=dev)
    self._reward = torch.zeros((self.batch_size,), dtype=torch.float32, device=dev)
    self._info = (torch.zeros((self.batch_size, _ffi.SB_INFO_STRIDE), dtype=torch.float32, device=dev)
                  if collect_info else None)
    self._discount = torch.full((self.batch_size,), self.discount_factor, dtype=torch.float32, device=dev)
    self._zero = torch.zeros((self.batch_size,), dtype=torch.float32, device=dev)
    if self.per_building_episodes:
      self.final_observation = torch.zeros_like(self._obs)   # [B, O]: a building's row is written when its episode ends
      self._step_type = torch.zeros((self.batch_size,), dtype=torch.int32, device=dev)   # per building, kept between calls
      self._disc = torch.ones((self.batch_size,), dtype=torch.float32, device=dev)
      # the previous thermostat update stays per building on the device (scal[18]), as after a first rejection
      self._no_reject = torch.zeros((self.batch_size,), dtype=torch.uint8, device=dev)
    self.spatial = None
    self.temperature_map = self.zone_temp_stats = self.final_temperature_map = self.final_zone_temp_stats = None
    if spatial is not None:
      self._setup_spatial(spatial)
    self._episode_ended = False
    self._step_count = 0
    self._episode_count = 0
    self._prev_thermostat_ts = None   # Thermostat._previous_timestamp survives reset()
    self._now = self._start_timestamp
    self._needs_reset = True

  # ---- specs / properties (environment.py:522-540,1215-1221) ----
  def action_spec(self) -> ArraySpec:
    return self._action_spec

  def observation_spec(self) -> ArraySpec:
    return self._observation_spec

  @property
  def batched(self) -> bool:
    return True

  @property
  def steps_per_episode(self) -> int:
    return self._num_timesteps_in_episode

  @property
  def current_simulation_timestamp(self) -> dt.datetime:
    return self._now

  @property
  def info(self) -> Optional[torch.Tensor]:
    return self._info

  # ---- episode totals per building (episode_metrics=True) ----
  EPISODE_METRIC_NAMES = _ffi.EPISODE_METRIC_NAMES

  def _need_episode_metrics(self) -> None:
    if not self.has_episode_metrics:
      raise ValueError("the environment was built without episode_metrics=True")

  def episode_metrics(self) -> torch.Tensor:
    """The running rows: float64 [B, 20] on the device, the totals of every building's episode in progress."""
    self._need_episode_metrics()
    return self.sim.episode_metrics()

  def completed_episodes(self) -> torch.Tensor:
    """The completed rows: float64 [B, 20] on the device, the totals of every building's last closed episode (closed by
    the reset that followed it: ``reset()``, the autoreset inside ``step()``, ``reset_buildings``)."""
    self._need_episode_metrics()
    return self.sim.completed_episodes()

  # ---- every building scored against recorded zone temperatures (telemetry=...) ----
  TELEMETRY_SCORE_NAMES = _ffi.TELEMETRY_SCORE_NAMES
  TELEMETRY_ZONE_SCORE_NAMES = _ffi.TELEMETRY_ZONE_SCORE_NAMES

  def _need_telemetry(self) -> None:
    if not self.has_telemetry:
      raise ValueError("the environment was built without telemetry=...")

  def telemetry_scores(self) -> torch.Tensor:
    """The running rows: float64 [B, 13] on the device, the scores of every building's episode in progress."""
    self._need_telemetry()
    return self.sim.telemetry_scores()

  def completed_telemetry_scores(self) -> torch.Tensor:
    """The completed rows: float64 [B, 13] on the device, the scores of every building's last closed episode (closed by
    the reset that followed it: ``reset()``, the autoreset inside ``step()``, ``reset_buildings``)."""
    self._need_telemetry()
    return self.sim.completed_telemetry_scores()

  def telemetry_zone_scores(self) -> torch.Tensor:
    """The running per-zone rows: float64 [B, Z, 4] (``Telemetry(per_zone=True)``)."""
    self._need_telemetry()
    return self.sim.telemetry_zone_scores()

  def completed_telemetry_zone_scores(self) -> torch.Tensor:
    """The completed per-zone rows: float64 [B, Z, 4]."""
    self._need_telemetry()
    return self.sim.completed_telemetry_zone_scores()

  def telemetry_actions(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The recorded setpoints of every building's next step: float32 [B, A] on the device, ready for ``step``."""
    self._need_telemetry()
    return self.sim.telemetry_actions(out)

  def current_simulation_timestamps(self) -> List[dt.datetime]:
    """Every building's own instant: ``current_simulation_timestamp`` (the batch's base clock) moved by the building's
    start offset; without ``start_offsets``, the base clock B times.  With ``calendars``: the building's instant on its
    own calendar (its calendar's start, its start offset, its position)."""
    if self.calendars is not None:
      pos = (self._cursor.positions() if self.per_building_episodes
             else np.full(self.batch_size, int(round((self._now - self._start_timestamp) / self._step_interval))))
      return [self.timeline.instant(b, int(pos[b])) for b in range(self.batch_size)]
    if self._offsets_moved:   # drawn, or given by set_start_offsets for the next reset: those in force live on the device
      # (the effective offset: the episode's own offset minus the building's restart position; a building keeps it
      # until its next reset, whatever set_start_offsets has given it for then)
      eff = self.sim.clock_offsets_in_force()[1].cpu().numpy().astype(np.int64)
      return [self._start_timestamp + int(r) * self._step_interval for r in eff + self._cursor.pos]
    if self.per_building_episodes:   # every building's own episode position on its own calendar
      offs = np.zeros(self.batch_size, dtype=np.int64) if self.start_offsets is None else self.start_offsets
      return [self._start_timestamp + int(r) * self._step_interval for r in self._cursor.rows(offs)["now"]]
    if self.start_offsets is None:
      return [self._now] * self.batch_size
    return [self._now + int(o) * self._step_interval for o in self.start_offsets]

  def episode_positions(self) -> np.ndarray:
    """Every building's position in its own episode (the steps it has taken since its last reset), int64 [B]."""
    if not self.per_building_episodes:
      return np.full(self.batch_size, int(round((self._now - self._start_timestamp) / self._step_interval)), dtype=np.int64)
    return self._cursor.positions().astype(np.int64)

  # ---- host-side step inputs ----
  def _models(self) -> host_inputs.StepModels:
    """The host models in force (``restore`` may have replaced a stateful one) as the step-input functions take them."""
    return host_inputs.StepModels(self.weather, self.schedule, self.occupancy, self.electricity, self.gas,
                                  self._step_interval, tuple(self.sim.zone_names[:self.sim.Z]), self._occ_norm)

  def _aux(self, ts: dt.datetime):
    """environment.py:916-956 auxiliary features at the observation time."""
    if self._occ_total is not None:   # per building, on the device: overrides aux[6]
      t5 = ts - dt.timedelta(minutes=5)
      self.sim.occupancy_peek(*host_inputs.occupancy_clock(self.occupancy, t5), None, self._occ_total)
    return host_inputs.aux_features(self._models(), ts)

  def _device_inputs(self, si: _ffi.StepIn) -> None:
    """The fields of a StepIn that do not depend on the instant: the per-building weather's device tables."""
    if self._weather_replay is not None:   # per-building replay weather, interpolated on the device
      tt, tf, off = self._weather_replay
      si.weather_times_dev, si.weather_tempf_dev, si.weather_offset_dev = tt.data_ptr(), tf.data_ptr(), off.data_ptr()
      si.weather_n = int(tt.shape[0])
    elif isinstance(self.weather, host_inputs.BatchedSinusoidWeather):   # per-building weather, on the device
      si.weather_lohi_dev = self._weather_lohi.data_ptr()

  def make_step_in(self, ts: dt.datetime, has_action: bool = True) -> _ffi.StepIn:
    """The step's host-resolved inputs at ``ts`` (sb_step_in): ``host_inputs.step_inputs``, built from the functions a
    ``Timeline`` row is built from, and the device occupancy's two queries."""
    nxt = ts + self._step_interval
    si = _ffi.StepIn()
    self._device_inputs(si)
    d = host_inputs.step_inputs(self._models(), ts, self._prev_thermostat_ts)
    for name in host_inputs.STEP_INPUT_SCALARS:
      setattr(si, name, d[name])
    si.has_action = int(has_action)
    for i, v in enumerate(d["aux"]):
      si.aux[i] = float(v)
    # the reference asks the occupancy model in this order (environment.py:1310-1330):
    # _get_observation (num_occupants), then _get_reward (reward_info) -- it matters for the
    # randomized model, whose every query advances the occupants
    if self._occ_count is not None:
      self.sim.occupancy_peek(*host_inputs.occupancy_clock(self.occupancy, nxt - dt.timedelta(minutes=5)), None, self._occ_total)
      self.sim.occupancy_peek(*host_inputs.occupancy_clock(self.occupancy, nxt), self._occ_count, None)
      si.occupancy_bz_dev = self._occ_count.data_ptr()
      si.num_occupants_dev = self._occ_total.data_ptr()
      si.occupancy_norm = self._occ_norm
    elif isinstance(d["occupancy"], list):   # one shared randomized instance: per-zone values, same for every building
      self._occ_zone = torch.tensor(d["occupancy"], dtype=torch.float64, device=self.sim.tdev)
      si.occupancy_dev = self._occ_zone.data_ptr()
    else:
      si.occupancy = d["occupancy"]
    self._occ_host = d["occupancy"]   # what the step's RewardInfo holds (episode_writer.py)
    return si

  def _clock_step_in(self, has_action: bool = True) -> _ffi.StepIn:
    """A step's StepIn under a calendar per building: what does not depend on the instant; the library reads the rest from
    every building's own rows at the position sought.  The device occupancy is asked in make_step_in's order."""
    si = _ffi.StepIn()
    self._device_inputs(si)
    si.has_action = int(has_action)
    self.sim.clock_seek(*self._cursor.seek_args())
    if self._occ_count is not None:
      self.sim.occupancy_peek(1, 0, None, self._occ_total)   # the next row's t - 5 min pair: num_occupants' query
      self.sim.occupancy_peek(1, 1, self._occ_count, None)   # ... its t pair: the reward's query
      si.occupancy_bz_dev = self._occ_count.data_ptr()
      si.num_occupants_dev = self._occ_total.data_ptr()
      si.occupancy_norm = self._occ_norm
    return si

  # ---- PyEnvironment API ----
  def reset(self) -> TimeStep:
    """environment.py:1165-1212."""
    self.sim.reset()
    self._now = self._start_timestamp
    self._episode_ended = False
    self._episode_count += 1
    self._step_count = 0
    self._needs_reset = False
    if self._cursor is not None:   # every building's observation at its own instant: the rows at position 0
      self._cursor.reset()
      self.sim.clock_seek(*self._cursor.seek_args())
      si = _ffi.StepIn()
      self._device_inputs(si)
      if self._occ_total is not None:
        self.sim.occupancy_peek(0, 0, None, self._occ_total)   # this row's t - 5 min pair
        si.num_occupants_dev, si.occupancy_norm = self._occ_total.data_ptr(), self._occ_norm
      self.sim.observe_step_in(si, self._obs)
    else:
      if isinstance(self.weather, (host_inputs.BatchedSinusoidWeather, host_inputs.BatchedReplayWeather)):
        t_amb = torch.tensor(self.weather.temps(self._now), dtype=torch.float64, device=self.sim.tdev)
      else:
        t_amb = self.weather.get_current_temp(self._now)
      self.sim.observe(self._aux(self._now), t_amb, self._obs, self._occ_total, self._occ_norm)
    self._refresh_spatial()
    if self.per_building_episodes:   # the per-building TimeStep buffers: what reset_buildings() returns for the others
      self._step_type.fill_(STEP_FIRST)
      self._reward.zero_()
      self._disc.fill_(1.0)
      return TimeStep(self._step_type, self._reward, self._disc, self._obs)
    first = torch.full((self.batch_size,), STEP_FIRST, dtype=torch.int32, device=self.sim.tdev)
    return TimeStep(first, self._zero, torch.ones_like(self._discount), self._obs)

  def step(self, action: torch.Tensor, rejected: Optional[torch.Tensor] = None) -> TimeStep:
    """environment.py:1228-1370.  ``rejected``: optional bool / uint8 [B] on the device -- buildings
    whose BaseBuilding.request_action raised (environment.py:1266-1309; RejectionSimulatorBuilding):
    they skip setup_step_sim and the actions, step and observe like the others, and return the
    reward ``ACTION_REJECTION_REWARD`` (-inf).

    The returned TimeStep's tensors are the environment's own buffers: the next ``step`` / ``reset``
    overwrites them (clone what you keep across steps)."""
    if self._needs_reset or self._episode_ended:
      return self.reset()
    if self.per_building_episodes:
      return self._step_episodes(action, rejected)
    si = self.make_step_in(self._now) if self._cursor is None else self._clock_step_in()
    if rejected is not None:
      if tuple(rejected.shape) != (self.batch_size,) or rejected.device != self.sim.tdev:
        raise ValueError(f"rejected must be a [{self.batch_size}] tensor on {self.sim.tdev}")
      self._rejected = rejected.to(torch.uint8).contiguous()
      si.reject_dev = self._rejected.data_ptr()
    elif getattr(self, "_rejected", None) is not None:
      # once buildings may skip thermostat updates, "the previous update" stays per building on the
      # device (scal[18]): the host's comfort_prev assumes every building updated at the last step
      if getattr(self, "_no_reject", None) is None:
        self._no_reject = torch.zeros((self.batch_size,), dtype=torch.uint8, device=self.sim.tdev)
      si.reject_dev = self._no_reject.data_ptr()
    self.sim.step(action, si, self._obs, self._reward, self._info)
    self._refresh_spatial()
    self._prev_thermostat_ts = self._now
    self._now = self._now + self._step_interval
    if self._cursor is not None:
      self._cursor.advance()
    self._episode_ended = self._step_count >= self._num_timesteps_in_episode   # :1366-1368
    dev = self.sim.tdev
    if self._episode_ended:
      last = torch.full((self.batch_size,), STEP_LAST, dtype=torch.int32, device=dev)
      return TimeStep(last, self._reward, self._zero, self._obs)
    self._step_count += 1
    mid = torch.full((self.batch_size,), STEP_MID, dtype=torch.int32, device=dev)
    return TimeStep(mid, self._reward, self._discount, self._obs)

  # ---- episodes per building ----
  def _setup_episodes(self, episode_steps) -> None:
    """The constructor's part for per_building_episodes: the lengths, the cursor, and a clock in any case (all-zero
    offsets without start_offsets; with calendars, the CalendarTimeline attached already) -- the library moves a building's
    rows when it restarts."""
    self.episode_steps = (np.full(self.batch_size, self._num_timesteps_in_episode, dtype=np.int64) if episode_steps is None
                          else host_inputs.check_episode_steps(episode_steps, self.batch_size, self._num_timesteps_in_episode))
    if self.timeline is None:
      offsets = np.zeros(self.batch_size, dtype=np.int32)
      self.timeline = host_inputs.Timeline(self._models(), self._start_timestamp, offsets, self._num_timesteps_in_episode)
      self.sim.clock_attach(self.timeline.rows, offsets)
    self._cursor = host_inputs.EpisodeCursor(self.batch_size)

  def _restart(self, ended: np.ndarray) -> None:
    """The buildings of ``ended`` (bool [B]) start a new episode at the next position: reset on the device, their
    calendars moved, their first observation written into the observation buffer."""
    self.sim.reset_buildings(ended, restart_pos=self._cursor.pos)
    self._cursor.restart(ended)
    self.sim.clock_seek(*self._cursor.seek_args())
    si = _ffi.StepIn()
    self._device_inputs(si)
    self.sim.observe_buildings(ended, si, self._obs)

  def _step_episodes(self, action: torch.Tensor, rejected: Optional[torch.Tensor]) -> TimeStep:
    """``step`` with episodes per building, same-step autoreset: every building steps; those whose episode just ended
    leave their last observation in ``final_observation``, are reset, and return the first observation of their new
    episode with this step's reward, LAST and discount 0."""
    si = self._clock_step_in()
    if rejected is not None:
      if tuple(rejected.shape) != (self.batch_size,) or rejected.device != self.sim.tdev:
        raise ValueError(f"rejected must be a [{self.batch_size}] tensor on {self.sim.tdev}")
      self._rejected = rejected.to(torch.uint8).contiguous()
      si.reject_dev = self._rejected.data_ptr()
    else:
      si.reject_dev = self._no_reject.data_ptr()
    self.sim.step(action, si, self._obs, self._reward, self._info)
    self._prev_thermostat_ts = self._now
    self._now = self._now + self._step_interval
    self._cursor.advance()
    ended = self._cursor.ended(self.episode_steps)
    self._step_type.fill_(STEP_MID)
    self._disc.fill_(self.discount_factor)
    if ended.any():
      last = torch.from_numpy(ended).to(self.sim.tdev)
      self._step_type.masked_fill_(last, STEP_LAST)
      self._disc.masked_fill_(last, 0.0)
      self.final_observation.copy_(torch.where(last[:, None], self._obs, self.final_observation))
      self._final_spatial(last)
      self._restart(ended)
    self._refresh_spatial()
    return TimeStep(self._step_type, self._reward, self._disc, self._obs)

  def reset_buildings(self, mask) -> TimeStep:
    """Ends the episodes of the buildings of ``mask`` (bool or uint8 [B], numpy or torch) now, between two steps: they
    are reset on the device and get FIRST, reward 0, discount 1 and the first observation of their new episode; the
    other buildings keep the step type, reward, discount and observation of their last step.  ValueError before the
    first ``reset()`` and on an environment without ``per_building_episodes``."""
    if not self.per_building_episodes:
      raise ValueError("reset_buildings needs an environment created with per_building_episodes=True (or episode_steps)")
    if self._needs_reset:
      raise ValueError("reset_buildings: reset() first (no building has an episode yet)")
    m = self.sim._host_mask(mask) != 0
    if m.any():
      first = torch.from_numpy(m).to(self.sim.tdev)
      self._restart(m)
      self._refresh_spatial()
      self._step_type.masked_fill_(first, STEP_FIRST)
      self._reward.masked_fill_(first, 0.0)
      self._disc.masked_fill_(first, 1.0)
    return TimeStep(self._step_type, self._reward, self._disc, self._obs)

  def _refuse_with_episodes(self, what: str) -> None:
    if self.per_building_episodes:
      raise ValueError(f"{what} is not supported with per_building_episodes: the per-building episode positions are not in "
                       "the snapshot (sb_state_view)")


  def set_building_params(self, params: Optional[host_inputs.BuildingParams]) -> None:
    """BatchedSimulator.set_building_params between steps; the usual place is just before ``reset()``, which sets
    the AHU and boiler setpoints of the new episode from the new rows."""
    self.sim.set_building_params(params)

  def building_params(self) -> Dict[str, np.ndarray]:
    return self.sim.building_params()

  def set_building_materials(self, materials: Optional[host_inputs.BuildingMaterials]) -> None:
    """BatchedSimulator.set_building_materials between steps (an environment created with ``building_materials``): the
    new rows apply from the next step; None returns every building to the plan's own values."""
    self.sim.set_building_materials(materials)

  def building_materials(self) -> Dict[str, np.ndarray]:
    return self.sim.building_materials()

  def set_reward_function(self, reward_function: Optional[host_inputs.SetpointEnergyCarbonReward]) -> None:
    """BatchedSimulator.set_reward_function: the reward of the steps from now on (None: the default regret function)."""
    self.sim.set_reward_function(reward_function)

  def set_initial_conditions(self, initial_conditions: Optional[host_inputs.InitialConditions]) -> None:
    """The start temperatures of the resets from now on (between episodes; None: ``SimConfig.initial_temp`` in every
    cell again).  New conditions start every building's episode count at 0."""
    if initial_conditions is None:
      self.sim.initial_conditions_detach()
    else:
      self.sim.initial_conditions_attach(initial_conditions)

  @property
  def initial_conditions(self) -> Optional[host_inputs.InitialConditions]:
    return self.sim.initial_conditions

  def set_episode_randomization(self, episode_randomization: Optional[host_inputs.EpisodeRandomization]) -> None:
    """The randomisation of the resets from now on (between episodes; None: the rows return to those of the attach and
    stay).  A new one starts every building's episode count at 0, with the same base rows."""
    if episode_randomization is None:
      self.sim.randomization_detach()
    else:
      self.sim.randomization_attach(episode_randomization)

  @property
  def episode_randomization(self) -> Optional[host_inputs.EpisodeRandomization]:
    return self.sim.randomization

  # ---- a start time and weather per building ----
  def _attach_starts(self, es: host_inputs.EpisodeStarts) -> None:
    self.sim.episode_starts_attach(es, self._weather_lohi, None if self._weather_replay is None else self._weather_replay[2])
    self._offsets_moved = self._offsets_moved or es.has_offsets

  def set_episode_starts(self, episode_starts: Optional[host_inputs.EpisodeStarts]) -> None:
    """The starts of the resets from now on (between episodes; None: every building returns to its attached offset and
    the weather of the attach at its next reset, and stays).  New starts begin every building's episode count at 0 and
    inherit the attached values.  The timeline was built by the constructor: an environment created without
    ``episode_starts`` has none that is sized for draws, and new starts must fit the table there is (ValueError)."""
    if episode_starts is None:
      self.sim.episode_starts_detach()
      return
    if not isinstance(episode_starts, host_inputs.EpisodeStarts):
      raise ValueError("episode_starts must be a host_inputs.EpisodeStarts (or None)")
    episode_starts.check(self.batch_size, self.weather, self.calendars)
    if self._cursor is None:
      raise ValueError("set_episode_starts: this environment was created without a device clock; create it with "
                       "episode_starts=... (or start_offsets / per_building_episodes)")
    # the constructor's checks on the table there is: its size, and a replay trace over the worst draw
    if self.calendars is None:   # (with calendars no offset is drawn, ``check`` above, and the table is not a Timeline)
      self.timeline.check_starts(episode_starts, self.weather, self.start_offsets)
    self._attach_starts(episode_starts)

  @property
  def episode_starts(self) -> Optional[host_inputs.EpisodeStarts]:
    return self.sim.episode_starts

  def episode_start_values(self) -> Dict[str, torch.Tensor]:
    """The values in force, on the device: "offsets" -> int32 [B] (every building's attached offset, drawn or not; on
    an environment with a device clock), and with the matching weather class "weather_low" / "weather_high" /
    "weather_shift" -> float64 [B].  Copies, ordered on the current stream."""
    out: Dict[str, torch.Tensor] = {}
    if self._cursor is not None:
      out["offsets"] = self.sim.clock_offsets_in_force()[0]
    if self._weather_lohi is not None:
      out["weather_low"], out["weather_high"] = self._weather_lohi[:, 0].clone(), self._weather_lohi[:, 1].clone()
    if self._weather_replay is not None:
      out["weather_shift"] = self._weather_replay[2].clone()
    return out

  def _refuse_owned(self, what: str, *fields: str) -> None:
    es = self.sim.episode_starts
    owned = [] if es is None else [f for f in fields if f in es.fields]
    if owned:
      raise ValueError(f"{what}: the attached episode_starts draw {owned[0]} (set_episode_starts(None) first)")

  def set_start_offsets(self, start_offsets) -> None:
    """The host route to a new start time: integer rows [B] (>= 0, inside the timeline), building b's from its next
    reset on; the episodes in progress keep their rows.  ValueError on an environment without a device clock, and while
    attached ``episode_starts`` draw the offsets."""
    self._refuse_owned("set_start_offsets", "offsets")
    if self._cursor is None or self.calendars is not None:
      raise ValueError("set_start_offsets needs an environment with one timeline on the device clock (start_offsets, "
                       "per_building_episodes or episode_starts; not calendars)")
    offs = host_inputs.check_start_offsets(start_offsets, self.batch_size)
    self.sim.clock_set_offsets(offs)
    self.start_offsets = offs   # (the attached offsets; ``current_simulation_timestamps`` asks the device for those in force)
    self._offsets_moved = True

  def set_weather(self, low_temps=None, high_temps=None, offsets_sec=None) -> None:
    """The host route to new weather per building, from the next step on: ``low_temps`` / ``high_temps`` (float [B]
    each, either may be left out) of a ``BatchedSinusoidWeather``, ``offsets_sec`` of a ``BatchedReplayWeather``.  The
    host model and the device array both take the values.  ValueError for the wrong weather class, low > high, values
    that are not finite, and while attached ``episode_starts`` draw that field.  (After ``set_episode_starts(None)`` a
    building's next reset still writes the weather of the attach: call this once every building has been reset.)"""
    def arr(name, a):
      a = np.ascontiguousarray(a, dtype=np.float64)
      if a.shape != (self.batch_size,):
        raise ValueError(f"{name} must have shape [{self.batch_size}], got {a.shape}")
      if not np.isfinite(a).all():
        raise ValueError(f"{name}: building {int(np.argmin(np.isfinite(a)))} is not finite")
      return a
    if offsets_sec is not None:
      if self._weather_replay is None or low_temps is not None or high_temps is not None:
        raise ValueError("set_weather(offsets_sec=...) needs weather=BatchedReplayWeather(...), and no low_temps / high_temps")
      self._refuse_owned("set_weather", "weather_shift")
      a = arr("offsets_sec", offsets_sec)
      self.weather.offsets_sec = a
      self._weather_replay[2].copy_(torch.from_numpy(a))
      return
    if self._weather_lohi is None or (low_temps is None and high_temps is None):
      raise ValueError("set_weather(low_temps=..., high_temps=...) needs weather=BatchedSinusoidWeather(...)")
    self._refuse_owned("set_weather", *(f for f, v in (("weather_low", low_temps), ("weather_high", high_temps)) if v is not None))
    low = self.weather.low if low_temps is None else arr("low_temps", low_temps)
    high = self.weather.high if high_temps is None else arr("high_temps", high_temps)
    lo_now, hi_now = low, high
    es = self.sim.episode_starts
    if es is not None and (low_temps is None or high_temps is None) and {"weather_low", "weather_high"} & set(es.fields):
      # the other value in force may be a drawn one, which only the device has (a copy that waits for the stream; with
      # both values given, or nothing drawn, the host model answers)
      column = 1 if high_temps is None else 0
      other = self._weather_lohi[:, column].cpu().numpy()
      lo_now, hi_now = (low, other) if column == 1 else (other, high)
    if (lo_now > hi_now).any():
      raise ValueError(f"set_weather: building {int(np.argmax(lo_now > hi_now))}: low above high")
    self.weather.low, self.weather.high = low, high
    if low_temps is not None:
      self._weather_lohi[:, 0].copy_(torch.from_numpy(low))
    if high_temps is not None:
      self._weather_lohi[:, 1].copy_(torch.from_numpy(high))

  def randomized_values(self) -> Dict[str, torch.Tensor]:
    """The values in force of the randomised fields, on the device (e.g. as privileged input of a critic): SimConfig
    field -> float64 [B] ([B, 2] for a window), material kind -> [B, M], "convection_coefficient" -> [B].  Copies,
    ordered on the current stream."""
    er = self.sim.randomization
    if er is None:
      raise ValueError("randomized_values: no episode randomisation is attached")
    out: Dict[str, torch.Tensor] = {}
    if er.has_params:
      rows = self.sim.building_param_rows()
      index = {name: k for k, name in enumerate(_ffi.BUILDING_PARAM_FIELDS)}
      for name in dict.fromkeys(f.name.partition("[")[0] for f in er.fields if f.param is not None):
        ks = [index[c] for c in host_inputs.BUILDING_PARAM_NAMES[name]]
        out[name] = rows[ks[0]].clone() if len(ks) == 1 else rows[ks].t().contiguous()
    if er.has_materials:
      rows = self.sim.building_material_rows()
      M = (rows.shape[0] - 1) // 3
      for kind in dict.fromkeys(f.material[0] for f in er.fields if f.material is not None):
        if kind == 3:
          out["convection_coefficient"] = rows[3 * M].clone()
        else:
          out[host_inputs._MATERIAL_KINDS[kind]] = rows[kind * M:(kind + 1) * M].t().contiguous()
    return out

  # ---- snapshots ----
  _HOST_CLOCK = ("_now", "_step_count", "_episode_count", "_episode_ended", "_needs_reset", "_prev_thermostat_ts")

  def _stateful_models(self) -> Dict:
    """Host models whose answers depend on what they answered before (the device-side occupancy keeps its state on
    the device: it is in the SimState)."""
    out = {}
    if (isinstance(self.occupancy, host_inputs.RandomizedArrivalDepartureOccupancy)
        and self._occ_count is None):
      out["occupancy"] = self.occupancy
    return out

  def snapshot(self) -> EnvSnapshot:
    """Everything ``restore`` needs to put this environment back where it is now: the simulator state of every
    building, the host clock and episode bookkeeping, stateful host models, the current TimeStep and info."""
    self._refuse_with_episodes("snapshot()")
    self.sim._refuse_on_jacobi("snapshot()")
    if self._needs_reset:
      raise ValueError("snapshot() needs a current TimeStep: reset() first")
    clone = lambda t: None if t is None else t.clone()
    return EnvSnapshot(self.sim.save_state(), {k: getattr(self, k) for k in self._HOST_CLOCK},
                       clone(getattr(self, "_rejected", None)),
                       {k: copy.deepcopy(v) for k, v in self._stateful_models().items()},
                       self._obs.clone(), self._reward.clone(), clone(self._info))

  def _timestep(self) -> TimeStep:
    """The TimeStep that reset() / step() returned last, rebuilt from the host clock and the current buffers."""
    dev = self.sim.tdev
    if self._episode_ended:
      return TimeStep(torch.full((self.batch_size,), STEP_LAST, dtype=torch.int32, device=dev), self._reward,
                      self._zero, self._obs)
    if self._step_count == 0:
      return TimeStep(torch.full((self.batch_size,), STEP_FIRST, dtype=torch.int32, device=dev), self._zero,
                      torch.ones_like(self._discount), self._obs)
    return TimeStep(torch.full((self.batch_size,), STEP_MID, dtype=torch.int32, device=dev), self._reward,
                    self._discount, self._obs)

  def restore(self, snap: EnvSnapshot) -> TimeStep:
    """Puts the environment back to ``snap`` (of this environment, or of one of the same floor plan, configuration
    and batch size) and returns the TimeStep that was current then.  The simulator's draw counters rewind with it,
    so the device occupancy and convection draw what they drew after the snapshot: a restored batch replays exactly."""
    self._refuse_with_episodes("restore()")
    self.sim._refuse_on_jacobi("restore()")
    if not isinstance(snap, EnvSnapshot):
      raise ValueError("restore needs an EnvSnapshot")
    if tuple(snap.observation.shape) != tuple(self._obs.shape) or (snap.info is None) != (self._info is None):
      raise ValueError("this EnvSnapshot belongs to an environment of another batch size, observation or info layout")
    models = {k: copy.deepcopy(v) for k, v in snap.models.items()}
    if set(models) != set(self._stateful_models()):
      raise ValueError(f"this EnvSnapshot carries host models {sorted(models)}, the environment has "
                       f"{sorted(self._stateful_models())}")
    self.sim.load_state(snap.sim)   # (checks the fingerprint before anything changes)
    for k, v in snap.host.items():
      setattr(self, k, v)
    for k, v in models.items():
      setattr(self, k, v)
    if self._cursor is not None:   # the restored clock, as positions on the timeline (the next step re-seeks)
      at = lambda t: None if t is None else int(round((t - self._start_timestamp) / self._step_interval))
      self._cursor = host_inputs.ClockCursor(at(self._now), at(self._prev_thermostat_ts))
    if snap.rejected is not None:
      self._rejected = snap.rejected.clone()
    elif getattr(self, "_rejected", None) is not None:
      self._rejected = None
    self._obs.copy_(snap.observation)
    self._reward.copy_(snap.reward)
    if self._info is not None:
      self._info.copy_(snap.info)
    self._refresh_spatial()   # (not in the snapshot: recomputed from the restored state)
    return self._timestep()

  def fork(self, src: torch.Tensor) -> None:
    """Building b takes building src[b]'s current state (src: int64 [B] on the device; repeats and aliasing allowed):
    one save of the distinct source buildings and one load with a pick.  The clock does not move; the current
    observation, reward and info rows follow their buildings.  With ``start_offsets`` or ``calendars`` the thermostats'
    previous update is the source building's, like the rest of its state, not the row of the slot's calendar.  Random
    streams: the device occupancy and convection draw by (seed, global building, counter), so a forked building keeps
    its own slot's stream -- forked replicas of one building diverge under those stochastic models and stay identical
    without them."""
    self._refuse_with_episodes("fork()")
    self.sim._refuse_on_jacobi("fork()")
    if not isinstance(src, torch.Tensor) or src.dtype != torch.int64 or tuple(src.shape) != (self.batch_size,):
      raise ValueError(f"src must be an int64 [{self.batch_size}] tensor")
    if src.device != self.sim.tdev:
      raise ValueError(f"src must be on {self.sim.tdev}")
    if int(src.min()) < 0 or int(src.max()) >= self.batch_size:
      raise ValueError(f"src out of range [0, {self.batch_size})")
    uniq, inv = torch.unique(src, return_inverse=True)
    state = self.sim.save_state(rows=uniq)
    self.sim.load_state(state, pick=inv, clock=False)
    if self._cursor is not None and getattr(self, "_rejected", None) is None:
      # The previous thermostat update is state (scal[18], Thermostat._previous_timestamp): a forked building's is its
      # source's, which the row of its own slot's calendar does not know.  From here on k_pre reads scal[18], as after a
      # first rejection -- a step after a fork must not depend on whether `rejected` was ever passed.
      self._rejected = torch.zeros((self.batch_size,), dtype=torch.uint8, device=self.sim.tdev)
    self._obs.copy_(self._obs[src])
    self._reward.copy_(self._reward[src])
    if self._info is not None:
      self._info.copy_(self._info[src])
    self._refresh_spatial()

  # ---- spatial outputs ----
  def _setup_spatial(self, spatial: host_inputs.SpatialOutputs) -> None:
    """The constructor's part for ``spatial``: the index tables on the device and the output tensors."""
    if not isinstance(spatial, host_inputs.SpatialOutputs):
      raise ValueError("spatial must be a host_inputs.SpatialOutputs (or None)")
    self.sim.spatial_attach(spatial.pool)
    self.spatial = spatial
    dev, B = self.sim.tdev, self.batch_size
    if spatial.pool is not None:
      self.temperature_map = torch.zeros((B,) + self.sim.map_shape, dtype=torch.float32, device=dev)
    if spatial.zone_stats:
      self.zone_temp_stats = torch.zeros((B, self.sim.Z, 3), dtype=torch.float64, device=dev)
    if self.per_building_episodes:   # [B, ...]: a building's row is written when its episode ends, as final_observation's
      self.final_temperature_map = None if self.temperature_map is None else torch.zeros_like(self.temperature_map)
      self.final_zone_temp_stats = None if self.zone_temp_stats is None else torch.zeros_like(self.zone_temp_stats)

  def _refresh_spatial(self) -> None:
    """One sb_spatial launch on the current stream: the outputs of the state the current observation describes."""
    if self.spatial is not None:
      self.sim.spatial(None, stats_out=self.zone_temp_stats, map_out=self.temperature_map,
                       stats=self.zone_temp_stats is not None, map=self.temperature_map is not None)

  def _final_spatial(self, last: torch.Tensor) -> None:
    """Before the buildings of ``last`` (bool [B] on the device) are reset: one picked launch, their rows of final_*."""
    if self.spatial is None:
      return
    rows = torch.nonzero(last).reshape(-1)
    stats, tmap = self.sim.spatial(rows, stats=self.zone_temp_stats is not None, map=self.temperature_map is not None)
    if stats is not None:
      self.final_zone_temp_stats.index_copy_(0, rows, stats)
    if tmap is not None:
      self.final_temperature_map.index_copy_(0, rows, tmap)

  def close(self) -> None:
    self.sim.close()


class MixedBatchedEnvironment:
  """One vectorised environment over SEVERAL floor-plan classes (BASELINE.json configs[2]: a batch mixed over
  floor plans with different zone counts): the same ``reset()`` / ``step(action)`` -> TimeStep contract as
  ``BatchedEnvironment`` over the concatenated batch.

      env = MixedBatchedEnvironment([(plan_a, 21845), (plan_b, 21845), (plan_c, 21845)], holiday_calendar="us")
      ts = env.reset()
      ts = env.step(actions)            # actions [B_total, n_actions] in HBM, buildings in class order

  Inside: one ``BatchedEnvironment`` (one library handle, the sweep kernel the planner picks for that plan)
  per class, each on its own HIP stream, so that the classes' launches overlap on the chip; ``step`` makes
  every class stream wait for the caller's stream (the actions) and the caller's stream wait for every class.
  The classes share the simulator clock and the episode length, so they step and end together.

  Observations: a class's observation row has ``3 * zones + 19`` fields, so rows differ in width.  The
  mixed observation is ``[B_total, max width]``; a building's row holds its class's fields first (the layout
  of ``BatchedEnvironment.field_names`` of its class, ``self.envs[k].field_names``) and zeros after
  ``self.observation_widths[k]``; ``self.class_of_building`` ([B_total] int32 in HBM) and ``self.slices``
  say which class a building belongs to.  Every keyword argument goes to each class's ``BatchedEnvironment``
  (``solver`` may also be a sequence: one finite-difference solver per class);
  a seeded per-building generator among them (``convection_simulator``, randomized ``occupancy``) gets its
  ``first_building`` moved to the class's first GLOBAL building on this rank, so every building of the mixed batch
  draws from its own stream whatever the sharding.

  Several GPUs (``rank``, ``world``): the counts in ``classes`` are the GLOBAL ones and every class
  is block-partitioned over the ranks on its own (``sbsim_amd.distributed.class_shard_ranges``), so each rank
  holds the same class mix -- the classes need very different numbers of sweeps per step, a rank with only the
  large class would set the pace.  ``self.class_totals`` / ``self.class_ranges`` say which global buildings of
  each class this rank holds; ``distributed.gather_returns_by_class`` puts per-building results back into
  global (class-major) order."""

  def __init__(self, classes: Sequence[Tuple[FloorPlan, int]], device: int = 0, rank: int = 0, world: int = 1,
               building_params: Optional[host_inputs.BuildingParams] = None, reward_function=None,
               building_materials: Optional[Sequence[Optional[host_inputs.BuildingMaterials]]] = None,
               initial_conditions: Optional[Sequence[Optional[host_inputs.InitialConditions]]] = None,
               episode_randomization=None, **env_kwargs):
    """``telemetry`` (among ``env_kwargs``): a list / tuple with one ``host_inputs.Telemetry`` or None per class (a
    recording has a floor plan's zones; its [B] arrays have one row per building of the class); one rank only.
    ``episode_randomization``: one ``host_inputs.EpisodeRandomization`` for every class, or a list / tuple with one or
    None per class (material slots are a floor plan's own); ``first_building`` moves to the class's first GLOBAL building
    on this rank, as for ``initial_conditions``.
    ``initial_conditions``: a list / tuple with one ``host_inputs.InitialConditions`` or None per class (a grid
    belongs to a floor plan); a class's [B] arrays have one row per building of the class over every rank
    (``class_totals[k]`` rows), this rank takes its share, and ``first_building`` moves to the share's first GLOBAL
    building of the mixed batch, as the generators' does.
    ``building_materials``: a list / tuple with one ``host_inputs.BuildingMaterials`` or None per class (material
    slots are a floor plan's own, so a table belongs to one class); a class's table has one row per building of the
    class over every rank (``class_totals[k]`` rows), and this rank takes its share (``class_ranges[k]``).
    ``building_params``: one row per GLOBAL building of the mixed batch (``sum(class_totals)`` rows, class-major);
    each class on this rank takes its buildings' rows (``distributed.class_global_rows``), whatever the sharding.
    ``reward_function``: one for every class (None: the default regret function), or a list / tuple with one per
    class (None entries: the default for that class)."""
    if not classes:
      raise ValueError("MixedBatchedEnvironment needs at least one (floor plan, number of buildings) class")
    if env_kwargs.get("per_building_episodes") or env_kwargs.get("episode_steps") is not None:
      raise ValueError("per_building_episodes is not implemented for MixedBatchedEnvironment (its classes step and end together)")
    if env_kwargs.get("calendars") is not None or env_kwargs.get("calendar_of") is not None:
      raise ValueError("calendars is not implemented for MixedBatchedEnvironment: calendar_of indexes the buildings of one "
                       "BatchedEnvironment, and the classes of a mixed batch are block-partitioned over classes and ranks")
    if env_kwargs.get("episode_starts") is not None:
      raise ValueError("episode_starts is not implemented for MixedBatchedEnvironment (its classes share one simulator clock)")
    if env_kwargs.get("telemetry") is not None:
      if not isinstance(env_kwargs["telemetry"], (list, tuple)) or len(env_kwargs["telemetry"]) != len(classes):
        raise ValueError(f"telemetry: a list with one host_inputs.Telemetry or None per class ({len(classes)})")
      if int(world) != 1:
        raise ValueError("telemetry is not implemented for a MixedBatchedEnvironment over several ranks")
    else:
      env_kwargs.pop("telemetry", None)
    if isinstance(env_kwargs.get("convection_simulator"), host_inputs.SeededStochasticConvectionSimulator):
      raise ValueError("SeededStochasticConvectionSimulator is not implemented for MixedBatchedEnvironment (its seeds belong "
                       "to the buildings of one BatchedEnvironment); use host_inputs.StochasticConvectionSimulator")
    from . import distributed as _sd
    self.device = int(device)
    self.tdev = torch.device("cuda", self.device)
    self.envs: List[BatchedEnvironment] = []
    self.streams: List[torch.cuda.Stream] = []
    self.slices: List[Tuple[int, int]] = []
    self.rank, self.world = int(rank), int(world)
    self.class_totals = [int(n) for _, n in classes]
    self.class_ranges = _sd.class_shard_ranges(self.class_totals, self.rank, self.world)
    # the same test on every rank (a rank that raised alone would leave the others in their first collective)
    if any(n < self.world for n in self.class_totals):
      raise ValueError(f"every class needs at least one building per rank: totals {self.class_totals}, {world} ranks")
    classes = [(plan, hi - lo_) for (plan, _), (lo_, hi) in zip(classes, self.class_ranges)]
    self.global_rows = _sd.class_global_rows(self.class_totals, self.rank, self.world)
    self._check_building_params(building_params)
    self._check_building_materials(building_materials)
    self._check_initial_conditions(initial_conditions, [plan for plan, _ in classes])
    rewards = self._per_class_rewards(reward_function, len(classes))
    if isinstance(episode_randomization, (list, tuple)):
      if len(episode_randomization) != len(classes):
        raise ValueError(f"episode_randomization: one per class ({len(classes)}), or one for all")
      randomizations = list(episode_randomization)
    else:
      randomizations = [episode_randomization] * len(classes)
    for k, er in enumerate(randomizations):
      if er is not None and not isinstance(er, host_inputs.EpisodeRandomization):
        raise ValueError(f"episode_randomization[{k}] must be a host_inputs.EpisodeRandomization or None")
    lo = 0
    for k, (plan, n) in enumerate(classes):
      # per-building generators (convection shuffle, randomized occupancy) draw from streams keyed by the GLOBAL
      # building index: class k's building i is building sum(totals[:k]) + i of the whole mixed batch, on whichever
      # rank it lives -- so the draws do not depend on the sharding, and no two buildings share a stream
      first = self.global_rows[k][0]
      kw = dict(env_kwargs)
      if isinstance(kw.get("solver"), (list, tuple)):   # one finite-difference solver per class
        if len(kw["solver"]) != len(classes):
          raise ValueError(f"solver: one per class ({len(classes)}), or one for all")
        kw["solver"] = kw["solver"][k]
      if "telemetry" in kw:   # one Telemetry (or None) per class: a recording has a floor plan's zones
        kw["telemetry"] = kw["telemetry"][k]
      if isinstance(kw.get("spatial"), (list, tuple)):   # one SpatialOutputs (or None) per class
        if len(kw["spatial"]) != len(classes):
          raise ValueError(f"spatial: one per class ({len(classes)}), or one for all")
        kw["spatial"] = kw["spatial"][k]
      for key in ("convection_simulator", "occupancy"):
        gen = kw.get(key)
        if gen is not None and hasattr(gen, "first_building"):
          gen = copy.copy(gen)
          gen.first_building = int(gen.first_building) + first
          kw[key] = gen
      stream = torch.cuda.Stream(device=self.tdev)
      if building_params is not None:
        kw["building_params"] = building_params.rows(*self.global_rows[k])
      kw["reward_function"] = rewards[k]
      if building_materials is not None and building_materials[k] is not None:
        kw["building_materials"] = building_materials[k].rows(*self.class_ranges[k])
      if initial_conditions is not None and initial_conditions[k] is not None:
        kw["initial_conditions"] = self._class_initial_conditions(initial_conditions[k], k)
      if randomizations[k] is not None:   # drawing as global building global_rows[k][0] + i
        kw["episode_randomization"] = randomizations[k].rows(first)
      with torch.cuda.stream(stream):
        env = BatchedEnvironment(plan, int(n), device=self.device, **kw)
      self.envs.append(env)
      self.streams.append(stream)
      self.slices.append((lo, lo + env.batch_size))
      lo += env.batch_size
    torch.cuda.synchronize(self.tdev)
    self.batch_size = lo
    specs = {tuple(e.action_spec().shape) for e in self.envs}
    if len(specs) != 1 or len({e.steps_per_episode for e in self.envs}) != 1:
      raise ValueError("the classes of a MixedBatchedEnvironment share the action set and the episode length")
    self.observation_widths = [e.sim.O for e in self.envs]
    O = max(self.observation_widths)
    self._action_spec = self.envs[0].action_spec()
    self._observation_spec = ArraySpec((O,), np.dtype(np.float32), "observation")
    self._obs = torch.zeros((self.batch_size, O), dtype=torch.float32, device=self.tdev)
    self._reward = torch.zeros((self.batch_size,), dtype=torch.float32, device=self.tdev)
    self._discount = torch.zeros((self.batch_size,), dtype=torch.float32, device=self.tdev)
    self._step_type = torch.zeros((self.batch_size,), dtype=torch.int32, device=self.tdev)
    cls = torch.zeros((self.batch_size,), dtype=torch.int32, device=self.tdev)
    for k, (a, b) in enumerate(self.slices):
      cls[a:b] = k
    self.class_of_building = cls
    self.profile = False          # True: every step records (start, end) HIP events per class on its stream
    self.class_events: List[List[Tuple[torch.cuda.Event, torch.cuda.Event]]] = [[] for _ in self.envs]

  def action_spec(self) -> ArraySpec:
    return self._action_spec

  def observation_spec(self) -> ArraySpec:
    return self._observation_spec

  @property
  def batched(self) -> bool:
    return True

  @property
  def steps_per_episode(self) -> int:
    return self.envs[0].steps_per_episode

  @property
  def current_simulation_timestamp(self) -> dt.datetime:
    return self.envs[0].current_simulation_timestamp

  @property
  def temperature_maps(self) -> List[Optional[torch.Tensor]]:
    """Every class's ``BatchedEnvironment.temperature_map`` ([B_k, map_h_k, map_w_k] float32, or None), computed on the
    class's stream by the last ``reset`` / ``step`` / ``restore`` / ``fork`` (``spatial``: one for all classes, or one per
    class)."""
    return [e.temperature_map for e in self.envs]

  @property
  def zone_temp_stats(self) -> List[Optional[torch.Tensor]]:
    """Every class's ``BatchedEnvironment.zone_temp_stats`` ([B_k, Z_k, 3] float64, or None)."""
    return [e.zone_temp_stats for e in self.envs]

  # ---- episode totals per building (episode_metrics=True goes to every class) ----
  EPISODE_METRIC_NAMES = _ffi.EPISODE_METRIC_NAMES

  @property
  def has_episode_metrics(self) -> bool:
    return all(e.has_episode_metrics for e in self.envs)

  def episode_metrics(self) -> torch.Tensor:
    """``BatchedEnvironment.episode_metrics`` of every class, read on the class streams: float64 [B_total, 20], the
    rows in class order."""
    return self._cat_rows(lambda k, env: env.episode_metrics())

  def completed_episodes(self) -> torch.Tensor:
    """``BatchedEnvironment.completed_episodes`` of every class: float64 [B_total, 20], the rows in class order."""
    return self._cat_rows(lambda k, env: env.completed_episodes())

  # ---- every building scored against recorded zone temperatures (telemetry=[one or None per class]) ----
  TELEMETRY_SCORE_NAMES = _ffi.TELEMETRY_SCORE_NAMES
  TELEMETRY_ZONE_SCORE_NAMES = _ffi.TELEMETRY_ZONE_SCORE_NAMES

  @property
  def has_telemetry(self) -> bool:
    return all(e.has_telemetry for e in self.envs)

  def telemetry_scores(self) -> torch.Tensor:
    """``BatchedEnvironment.telemetry_scores`` of every class: float64 [B_total, 13], the rows in class order."""
    return self._cat_rows(lambda k, env: env.telemetry_scores())

  def completed_telemetry_scores(self) -> torch.Tensor:
    """``BatchedEnvironment.completed_telemetry_scores`` of every class: float64 [B_total, 13], in class order."""
    return self._cat_rows(lambda k, env: env.completed_telemetry_scores())

  def telemetry_zone_scores(self) -> List[torch.Tensor]:
    """Every class's running per-zone rows, a list of float64 [B_k, Z_k, 4] (Z differs between classes)."""
    return self._list_rows(lambda k, env: env.telemetry_zone_scores())

  def completed_telemetry_zone_scores(self) -> List[torch.Tensor]:
    """Every class's completed per-zone rows, a list of float64 [B_k, Z_k, 4]."""
    return self._list_rows(lambda k, env: env.completed_telemetry_zone_scores())

  def telemetry_actions(self) -> torch.Tensor:
    """``BatchedEnvironment.telemetry_actions`` of every class: float32 [B_total, A], the rows in class order."""
    return self._cat_rows(lambda k, env: env.telemetry_actions())

  def _list_rows(self, fn) -> List[torch.Tensor]:
    cur = torch.cuda.current_stream(self.tdev)
    parts = self._on_streams(fn)
    for t in parts:   # allocated on a class stream, read on the caller's
      t.record_stream(cur)
    return parts

  def _cat_rows(self, fn) -> torch.Tensor:
    cur = torch.cuda.current_stream(self.tdev)
    parts = self._on_streams(fn)
    for t in parts:   # allocated on a class stream, read on the caller's
      t.record_stream(cur)
    return torch.cat(parts)

  def _check_building_params(self, params: Optional[host_inputs.BuildingParams]) -> None:
    total = sum(self.class_totals)
    if params is not None and params.n_buildings != total:
      raise ValueError(f"building_params has {params.n_buildings} rows; the mixed batch has {total} buildings "
                       "(rows are indexed by the global building number, over every rank)")

  def set_building_params(self, params: Optional[host_inputs.BuildingParams]) -> None:
    """Per-building parameters of the whole mixed batch (global rows, as the constructor's ``building_params``);
    None clears every class's table."""
    self._check_building_params(params)
    self._on_streams(lambda k, env: env.set_building_params(None if params is None else params.rows(*self.global_rows[k])))

  def _class_initial_conditions(self, ic: host_inputs.InitialConditions, k: int) -> host_inputs.InitialConditions:
    """Class k's conditions on this rank: its share of the rows, drawing as global building ``global_rows[k][0] + i``."""
    lo, hi = self.class_ranges[k]
    share = ic.rows(lo, hi)   # (first_building + lo: the position inside the class)
    share.first_building = ic.first_building + self.global_rows[k][0]
    return share

  def _check_initial_conditions(self, conditions, plans) -> None:
    if conditions is None:
      return
    if not isinstance(conditions, (list, tuple)) or len(conditions) != len(plans):
      raise ValueError(f"initial_conditions: a list with one host_inputs.InitialConditions or None per class ({len(plans)})")
    for k, (ic, plan) in enumerate(zip(conditions, plans)):
      if ic is None:
        continue
      if not isinstance(ic, host_inputs.InitialConditions):
        raise ValueError(f"initial_conditions[{k}] must be a host_inputs.InitialConditions or None")
      try:
        ic.check(self.class_totals[k], tuple(plan.shape))
      except ValueError as e:
        raise ValueError(f"initial_conditions[{k}]: {e}") from None

  def _check_building_materials(self, materials) -> None:
    if materials is None:
      return
    if not isinstance(materials, (list, tuple)) or len(materials) != len(self.class_totals):
      raise ValueError(f"building_materials: a list with one BuildingMaterials or None per class ({len(self.class_totals)})")
    for k, (bm, total) in enumerate(zip(materials, self.class_totals)):
      if bm is not None and (not isinstance(bm, host_inputs.BuildingMaterials) or bm.n_buildings != total):
        raise ValueError(f"building_materials[{k}] needs one row per building of class {k} over every rank ({total})")

  def set_building_materials(self, materials) -> None:
    """Per-building materials per class (as the constructor's ``building_materials``) from the next step on; a None
    entry returns that class to its plan's own values -- or leaves it alone if it was created without a table."""
    self._check_building_materials(materials)
    if materials is None:
      materials = [None] * len(self.envs)

    def apply(k, env):
      if env.sim._materials_handle:
        env.set_building_materials(None if materials[k] is None else materials[k].rows(*self.class_ranges[k]))
      elif materials[k] is not None:
        raise ValueError(f"class {k} was created without building_materials")
    self._on_streams(apply)

  @staticmethod
  def _per_class_rewards(reward_function, n_classes: int) -> list:
    if isinstance(reward_function, (list, tuple)):
      if len(reward_function) != n_classes:
        raise ValueError(f"reward_function: one per class ({n_classes}), or one for all")
      return list(reward_function)
    return [reward_function] * n_classes

  def set_reward_function(self, reward_function) -> None:
    """The reward function of every class (one ``host_inputs.SetpointEnergyCarbonReward`` or None), or a list / tuple
    with one per class, from the next step on."""
    rewards = self._per_class_rewards(reward_function, len(self.envs))
    for env, r in zip(self.envs, rewards):   # a host value of each handle: nothing to order on the streams
      env.set_reward_function(r)

  def _each(self, fn) -> TimeStep:
    """Runs fn(class index, env) -> TimeStep on every class's stream between two joins with the caller's stream."""
    cur = torch.cuda.current_stream(self.tdev)
    ready = torch.cuda.Event()
    ready.record(cur)
    for k, (env, stream, (a, b)) in enumerate(zip(self.envs, self.streams, self.slices)):
      stream.wait_event(ready)
      with torch.cuda.stream(stream):
        if self.profile:
          e0 = torch.cuda.Event(enable_timing=True)
          e0.record(stream)
        ts = fn(k, env)
        if self.profile:
          e1 = torch.cuda.Event(enable_timing=True)
          e1.record(stream)
          self.class_events[k].append((e0, e1))
        self._obs[a:b, : self.observation_widths[k]].copy_(ts.observation)
        self._reward[a:b].copy_(ts.reward)
        self._discount[a:b].copy_(ts.discount)
        self._step_type[a:b].copy_(ts.step_type)
        done = torch.cuda.Event()
        done.record(stream)
      cur.wait_event(done)
    return TimeStep(self._step_type, self._reward, self._discount, self._obs)

  def reset(self) -> TimeStep:
    return self._each(lambda k, env: env.reset())

  def step(self, action: torch.Tensor, rejected: Optional[torch.Tensor] = None) -> TimeStep:
    """``BatchedEnvironment.step`` for every class (actions / rejected flags of its slice of the batch).  The
    TimeStep's tensors are this environment's own buffers: the next ``step`` / ``reset`` overwrites them."""
    if tuple(action.shape) != (self.batch_size,) + tuple(self._action_spec.shape):
      raise ValueError(f"action must be [{self.batch_size}, {self._action_spec.shape[0]}]")
    action = action.contiguous()
    return self._each(lambda k, env: env.step(action[self.slices[k][0]:self.slices[k][1]],
                                              None if rejected is None else rejected[self.slices[k][0]:self.slices[k][1]]))


  def _on_streams(self, fn) -> list:
    """fn(class index, env) on every class's stream between two joins with the caller's stream (as _each)."""
    cur = torch.cuda.current_stream(self.tdev)
    ready = torch.cuda.Event()
    ready.record(cur)
    out = []
    for k, (env, stream) in enumerate(zip(self.envs, self.streams)):
      stream.wait_event(ready)
      with torch.cuda.stream(stream):
        out.append(fn(k, env))
        done = torch.cuda.Event()
        done.record(stream)
      cur.wait_event(done)
    return out

  def snapshot(self) -> List[EnvSnapshot]:
    """One ``EnvSnapshot`` per class (``BatchedEnvironment.snapshot``), taken on the class streams."""
    return self._on_streams(lambda k, env: env.snapshot())

  def restore(self, snaps: Sequence[EnvSnapshot]) -> TimeStep:
    if len(snaps) != len(self.envs):
      raise ValueError(f"restore needs one EnvSnapshot per class ({len(self.envs)})")
    return self._each(lambda k, env: env.restore(snaps[k]))

  def fork(self, src: torch.Tensor) -> None:
    """Building b takes building src[b]'s state (GLOBAL indices, int64 [B_total] on the device); a building takes
    state only from its own class (ValueError otherwise).  See ``BatchedEnvironment.fork``."""
    if not isinstance(src, torch.Tensor) or src.dtype != torch.int64 or tuple(src.shape) != (self.batch_size,):
      raise ValueError(f"src must be an int64 [{self.batch_size}] tensor")
    if src.device != self.tdev:
      raise ValueError(f"src must be on {self.tdev}")
    if int(src.min()) < 0 or int(src.max()) >= self.batch_size:
      raise ValueError(f"src out of range [0, {self.batch_size})")
    if not bool((self.class_of_building[src] == self.class_of_building).all()):
      raise ValueError("fork: a building can only take the state of a building of its own floor-plan class")
    self._on_streams(lambda k, env: env.fork(src[self.slices[k][0]:self.slices[k][1]] - self.slices[k][0]))
    for k, (a, b) in enumerate(self.slices):   # the mixed TimeStep buffers follow
      self._obs[a:b, : self.observation_widths[k]].copy_(self.envs[k]._obs)
      self._reward[a:b].copy_(self.envs[k]._reward)

  def close(self) -> None:
    for env in self.envs:
      env.close()


class GymVectorEnv:
  """gymnasium.vector-style view of a ``BatchedEnvironment`` (no gymnasium import needed):

      obs, info = venv.reset()
      obs, reward, terminated, truncated, info = venv.step(actions)      # all [B, ...] tensors in HBM

  Over an environment with ``per_building_episodes`` (same-step autoreset): ``truncated`` / ``terminated`` are per
  building, the observation of a building whose episode just ended is the first of its next episode,
  ``info["final_obs"]`` is ``env.final_observation`` (a building's row: the last observation of its episode that ended
  last) and ``info["autoreset_mode"]`` is ``"same_step"``.  Over any other environment:

  Every sub-environment shares the simulator clock, so they end together: the last step of an
  episode (``environment.py:1366-1368``: its time is up) returns ``truncated = True`` for all of
  them (``terminated`` with ``time_limit_is_truncation=False``), and -- gymnasium's "next-step" autoreset mode -- the following ``step`` ignores its
  actions and returns the first observation of the next episode with zero reward."""

  def __init__(self, env: BatchedEnvironment, time_limit_is_truncation: bool = True):
    self.env = env
    self.time_limit_is_truncation = bool(time_limit_is_truncation)
    self.num_envs = env.batch_size
    self.single_action_shape = tuple(env.action_spec().shape)
    self.single_observation_shape = tuple(env.observation_spec().shape)
    self.action_low, self.action_high = -1.0, 1.0

  def reset(self, seed=None, options=None):
    del seed, options   # the simulator is deterministic; inputs come from the host controllers
    ts = self.env.reset()
    return ts.observation, {"step_type": ts.step_type}

  def step(self, actions: torch.Tensor):
    ts = self.env.step(actions)
    # an episode ends only because its time is up: gymnasium's TRUNCATION (a learner keeps bootstrapping);
    # time_limit_is_truncation=False reports it as a termination, like the reference's discount 0
    last = ts.step_type == STEP_LAST
    terminated, truncated = (torch.zeros_like(last), last) if self.time_limit_is_truncation else (last, torch.zeros_like(last))
    info = {"step_type": ts.step_type, "discount": ts.discount}
    if getattr(self.env, "per_building_episodes", False):
      info.update(final_obs=self.env.final_observation, autoreset_mode="same_step")
    if getattr(self.env, "has_episode_metrics", False):
      # gymnasium's RecordEpisodeStatistics convention: info["episode"] counts where info["_episode"] is set.  Same-step
      # autoreset: the reset inside step() has closed the episodes that ended, so they are the completed rows; on a
      # shared clock the reset follows with the next step(), and the episode still is the running rows
      rows = self.env.completed_episodes() if getattr(self.env, "per_building_episodes", False) else self.env.episode_metrics()
      info["episode"] = {"r": rows[:, _ffi.EPISODE_METRIC_NAMES.index("return")],
                         "l": rows[:, _ffi.EPISODE_METRIC_NAMES.index("steps")].to(torch.int64)}
      info["_episode"] = last
    return ts.observation, ts.reward, terminated, truncated, info

  def close(self) -> None:
    self.env.close()
