"""Crossed batch features against per-building oracle twins (test utility, no GPU).

Every per-building feature of a batch -- start offsets, calendars, episodes, parameter and material rows, the second
reward function, damper commands, rejection, the device weather and occupancy forms, the histogram reducer, snapshots and
forks -- has tests of its own, in which the other features stay at their defaults and the oracle is mostly the library
itself.  Here the features meet: `CASES` is a pairwise covering array over `FACTORS`, `Scenario` turns a case into the
arguments of one `BatchedEnvironment` and a program of steps, and `Twin` is ONE building of that batch as plain Python on
the CPU oracle, which knows nothing about batches, clock tables or offsets.

A twin takes every input of a step from the public methods of its own host models at its own time stamp (the calls
`BatchedEnvironment.make_step_in` makes for a plain environment: `host_inputs.step_inputs`), its physics from
`oracle.OracleBuilding` on a plan with its own materials and an `OracleParams` of its own row, its device occupants from
`DeviceOccupancyOracle`, the dollars reward from `tests/reward_cases.restate` and its observation row from the
reference's chain (native value -> float32 -> (x - mean) / sigma in float64 -> float32; `oracle/hist_oracle.py` where a
reducer is configured).  It never reads a `CalendarTimeline` row, a `ClockView` offset or a tensor of the environment.

tests/test_crossed_batches_cpu.py checks the table and the conditions on the inputs on the twins alone,
tests/test_crossed_batches_gpu.py runs every case on the device against them."""
from __future__ import annotations

import copy
import dataclasses
import datetime as dt
import itertools
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import hist_oracle
from oracle import oracle as orc
from oracle.occupancy_oracle import DeviceOccupancyOracle
from sbsim_amd import host_inputs
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
from tests import calendar_cases as cc
from tests.materials_cases import substituted
from tests.params_cases import c_row, random_params
from tests.reward_cases import restate
from tests.twins import copy_twin, native_value, oracle_plan_of

UTC = dt.timezone.utc
DT = dt.timedelta(seconds=300)
B, T = 67, 12
N_EPISODE = 16                      # the batch's steps_per_episode: no batch episode ends inside a run
ROOMS, ROOM_SHAPE = (2, 3), (5, 7)  # 17 x 29 cells, six zones, 493 cells
START = dt.datetime(2023, 7, 6, 12, 0, tzinfo=UTC)   # Thursday 05:00 PDT: SB1's morning switch at position 12
STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2
WEATHER_CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_weather_test_data.csv")
H_CONV = 100.0
INITIAL_TEMP = 293.37
SEED = 97

# ---------------------------------------------------------------- factors, refusals, cases
FACTORS: Dict[str, Tuple[str, ...]] = {   # every factor's first level is "off"
    "time": ("shared", "start_offsets", "calendars"),
    "episodes": ("batch", "per_building"),
    "params": ("none", "building_params"),
    "materials": ("none", "building_materials"),
    "kernel": ("register", "lds"),          # SBSIM_FORCE_LDS_PATH=1; building_materials always runs on k_sweep_lds
    "reward": ("regret", "dollars"),
    "actions": ("pair", "dampers"),
    "rejection": ("none", "mask"),
    "weather": ("default", "sinusoid", "replay"),
    "occupancy": ("step", "device"),
    "observation": ("plain", "histogram"),
    "lifecycle": ("none", "snapshot_fork"),
}

_OCC_MESSAGE = "per_building_episodes: BatchedRandomizedArrivalDepartureOccupancy is not supported"
# What the library refuses (ValueError, before any step): the levels that meet and the message it raises.  The third is
# raised by snapshot() / fork() after reset(): the per-building episode positions are not in a snapshot.
REFUSED: Tuple[Tuple[Dict[str, str], str], ...] = (
    ({"occupancy": "device", "episodes": "per_building"}, _OCC_MESSAGE),
    ({"occupancy": "device", "episodes": "per_building", "time": "calendars"}, _OCC_MESSAGE),
    ({"lifecycle": "snapshot_fork", "episodes": "per_building"},
     r"is not supported with per_building_episodes: the per-building episode positions are not in the snapshot"),
)
# Not a refusal but a definition: a materials handle has no register kernel.
NOT_A_PAIR: Tuple[Dict[str, str], ...] = ({"materials": "building_materials", "kernel": "register"},)

NAMED = ("dollars-on-the-clock", "materials-on-calendars", "episodes-with-rejections", "histograms-per-building",
         "everything")


def _case(**levels) -> Dict[str, str]:
  out = {f: lv[0] for f, lv in FACTORS.items()}
  for f, lv in levels.items():
    assert lv in FACTORS[f], (f, lv)
    out[f] = lv
  if out["materials"] == "building_materials":
    out["kernel"] = "lds"
  return out


CASES: Dict[str, Dict[str, str]] = {
    # k_post<SB_REWARD_SETPOINT_ENERGY_CARBON, true>: no other test launches it
    "dollars-on-the-clock": _case(reward="dollars", time="start_offsets", params="building_params"),
    # k_pre<true, true> and k_sweep_lds<true> against an oracle that is not the library
    "materials-on-calendars": _case(materials="building_materials", time="calendars", params="building_params",
                                    weather="sinusoid"),
    # the three sources of comfort_prev, scal[18], scal[19], the rewind in reset_episode, the rejected branch's damper
    "episodes-with-rejections": _case(episodes="per_building", time="start_offsets", rejection="mask", actions="dampers"),
    # write_obs with a.bp, src_dest, num_occupants_dev and the clock together
    "histograms-per-building": _case(observation="histogram", params="building_params", time="start_offsets",
                                     occupancy="device"),
    "everything": _case(time="calendars", params="building_params", materials="building_materials", reward="dollars",
                        actions="dampers", rejection="mask", weather="replay", occupancy="device",
                        observation="histogram", lifecycle="snapshot_fork"),
    # ---- the rest of the covering array
    "episodes-on-calendars": _case(time="calendars", episodes="per_building", materials="building_materials",
                                   reward="dollars", weather="replay", observation="histogram"),
    "lds-forks": _case(kernel="lds", lifecycle="snapshot_fork", actions="dampers", weather="sinusoid",
                       occupancy="device", reward="dollars", rejection="mask"),
    "episodes-shared-clock": _case(episodes="per_building", params="building_params", kernel="lds", reward="dollars",
                                   observation="histogram"),
    "offsets-replay-forks": _case(time="start_offsets", weather="replay", lifecycle="snapshot_fork", kernel="lds",
                                  observation="histogram", actions="dampers", materials="none"),
    "calendars-register": _case(time="calendars", rejection="mask", occupancy="device", actions="dampers",
                                lifecycle="snapshot_fork", observation="histogram"),
    "materials-offsets": _case(time="start_offsets", materials="building_materials", rejection="mask",
                               lifecycle="snapshot_fork", occupancy="device", weather="sinusoid", reward="dollars",
                               actions="dampers"),
    "episodes-materials-dampers": _case(episodes="per_building", materials="building_materials", actions="dampers",
                                        params="building_params", rejection="mask"),
    "calendars-episodes-sinusoid": _case(time="calendars", episodes="per_building", actions="dampers", weather="sinusoid",
                                         params="building_params", observation="histogram"),
    "shared-replay-device": _case(weather="replay", occupancy="device", params="building_params", rejection="mask",
                                  lifecycle="snapshot_fork", reward="dollars"),
}


def _holds(levels: Dict[str, str], case: Dict[str, str]) -> bool:
  return all(case[f] == lv for f, lv in levels.items())


def forbidden_pairs() -> set:
  """The pairs ((factor, level), (factor, level)) no case may hold: the two-level refusals and NOT_A_PAIR."""
  out = set()
  for levels in [r[0] for r in REFUSED if len(r[0]) == 2] + list(NOT_A_PAIR):
    out.add(frozenset(levels.items()))
  return out


def all_pairs() -> set:
  out = set()
  for (fa, la), (fb, lb) in itertools.combinations(FACTORS.items(), 2):
    for a in la:
      for b in lb:
        out.add(frozenset(((fa, a), (fb, b))))
  return out


def covered_pairs() -> set:
  out = set()
  for case in CASES.values():
    for a, b in itertools.combinations(case.items(), 2):
      out.add(frozenset((a, b)))
  return out


# ---------------------------------------------------------------- the observation row, restated
_TEMPERATURE_FIELDS = ("zone_air_temperature_sensor", "supply_water_temperature_sensor", "outside_air_temperature_sensor")


class ObsLayout:
  """The observation row of one building: device fields in sorted (device, field) order, the reference's normalisation
  chain, the optional HistogramReducer, then the auxiliary features."""

  def __init__(self, zone_names: Sequence[str], normalization: Dict[str, Tuple[float, float]],
               hist_params: Optional[Sequence[Tuple[str, Sequence[float]]]], normalize_reduce: bool):
    from sbsim_amd.environment import observation_field_names   # (the layout only: pinned by tests/test_hist_reducer.py)
    names, _, _, _, n_src = observation_field_names(list(zone_names), True)
    self.sources, self.aux_names = names[:n_src], names[n_src:]
    self.hist_params = [(n, list(b)) for n, b in hist_params] if hist_params else None
    self.normalize_reduce = bool(normalize_reduce)
    self.mean, self.sigma = np.zeros(n_src), np.ones(n_src)
    for i, name in enumerate(self.sources):
      mu, var = normalization.get(name.split("/", 1)[1], (0.0, 1.0))
      mu, var = float(np.float32(mu)), float(np.float32(var))   # proto floats (smart_control_normalization.proto)
      self.mean[i], self.sigma[i] = mu, (np.sqrt(var) if var > 0.0 else 0.0)
    if self.hist_params:
      self.fields = hist_oracle.field_order(self.sources, self.hist_params)
    else:
      self.fields = [n.replace("/", "_", 1) for n in self.sources]
    self.n_dev = len(self.fields)
    self.O = self.n_dev + len(self.aux_names)
    # what a column is made of: "count" (a histogram bin), "temperature" (a pass-through of a temperature), "exact"
    self.kind = []
    src_of = {n.replace("/", "_", 1): i for i, n in enumerate(self.sources)}
    self.col_source = []
    for f in self.fields:
      if "_h_" in f and f not in src_of:
        self.kind.append("count")
        self.col_source.append(-1)
      else:
        i = src_of[f]
        self.kind.append("temperature" if self.sources[i].split("/", 1)[1] in _TEMPERATURE_FIELDS else "exact")
        self.col_source.append(i)
    self.kind += ["exact"] * len(self.aux_names)
    self.col_source += [-1] * len(self.aux_names)

  def normalised(self, native: Sequence[float]) -> np.ndarray:
    """observation_normalizer.py:68-91 on the proto's float32 values, float32 out."""
    x = np.asarray(native, dtype=np.float64).astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
      v = np.where(self.sigma > 0.0, (x - self.mean) / np.where(self.sigma > 0.0, self.sigma, 1.0), 0.0)
    return v.astype(np.float32)

  def row(self, native: Sequence[float], aux: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """(the float32 row, per column the float32 native value it came from or NaN)."""
    v = self.normalised(native)
    if self.hist_params:
      out = hist_oracle.reduce(self.sources, v, self.hist_params, self.normalize_reduce)
      dev = np.array([out[f] for f in self.fields], dtype=np.float32)
    else:
      dev = v
    nat = np.array([np.float32(native[i]) if i >= 0 else np.nan for i in self.col_source], dtype=np.float64)
    return np.concatenate([dev, np.asarray(aux, dtype=np.float32)]), nat

  def hist_inputs(self, native: Sequence[float]) -> Dict[str, np.ndarray]:
    """Per reduced measurement: the normalised values that are binned (for the margin checks)."""
    v = self.normalised(native).astype(np.float64)
    return {m: v[[i for i, n in enumerate(self.sources) if n.split("/", 1)[1] == m]] for m, _ in self.hist_params or ()}


# ---------------------------------------------------------------- one building
class _Replay:
  """One building's ReplayWeatherController: the trace read `offset_sec` ahead."""

  def __init__(self, offset_sec: float):
    self._ctrl = host_inputs.ReplayWeatherController(WEATHER_CSV, convection_coefficient=H_CONV)
    self._shift = dt.timedelta(seconds=float(offset_sec))

  def get_current_temp(self, ts) -> float:
    return self._ctrl.get_current_temp(ts + self._shift)


class Twin:
  """One building as plain Python: see the module's docstring."""

  def __init__(self, *, plan: FloorPlan, h_conv: float, params: orc.OracleParams, start: dt.datetime,
               models: host_inputs.StepModels, episode_steps: int, discount: float, reward_function, layout: ObsLayout,
               action_names: Sequence[str], action_zones: Sequence[int], action_ranges, init_grid: np.ndarray,
               initial_temp: float, occupants: Optional[DeviceOccupancyOracle]):
    self.oplan = oracle_plan_of(plan)
    self.params, self.h_conv, self.start, self.models = params, float(h_conv), start, models
    self.episode_steps, self.discount, self.reward_function, self.layout = int(episode_steps), float(discount), reward_function, layout
    self.action_names, self.action_zones, self.action_ranges = tuple(action_names), tuple(action_zones), tuple(action_ranges)
    self.ob = orc.OracleBuilding(self.oplan, params, float(initial_temp), reset_temps=np.ascontiguousarray(init_grid))
    self.occupants = occupants
    self.pos = 0                    # position in the own episode
    self.prev_update = None         # Thermostat._previous_timestamp: survives reset() (thermostat.py:66-69) ...
    self.prev_schedule = models.schedule   # ... and the schedule of the building that made that update (a fork moves both)
    self.first_episode = True
    self.trace = False

  # ---- time
  @property
  def now(self) -> dt.datetime:
    return self.start + self.pos * DT

  def _num_occupants(self, ts) -> Optional[float]:
    if self.occupants is None:
      return None
    hour, work = host_inputs.occupancy_clock(self.models.occupancy, ts - dt.timedelta(minutes=5))
    return float(self.occupants.peek(hour, bool(work)).sum())

  def _aux(self, aux: Sequence[float], n_occ: Optional[float]) -> List[np.float32]:
    aux = [np.float32(v) for v in aux]
    if n_occ is not None:   # environment.py:951-955 with the building's own int(num_occupants)
      k = self.models.occupancy_norm
      aux[-1] = np.float32((float(int(n_occ)) - k) / (k + 1.0))
    return aux

  def _native_obs(self, t_amb_obs: float) -> List[float]:
    """The native value of every source field, sorted (device, field): air_handler.py:66-95, boiler.py:69-79,
    vav.py:54-64 on the oracle's state."""
    s, p = self.ob.state, self.params
    flow = s.ahu_flow
    ahu = [float(s.ahu_count), p.ahu_dp, flow / p.ahu_max_flow, (1.0 - p.ahu_recirc) * flow, t_amb_obs, s.ahu_cool_sp, flow,
           s.ahu_heat_sp, flow / p.ahu_max_flow]
    blr = [float(s.blr_count), s.blr_setpoint, s.blr_tank_temp]
    by_dev = {"air_handler_id": ahu, "boiler_id": blr}
    for z, name in enumerate(self.models.zone_names):
      by_dev[f"vav_{name}"] = [float(self.ob.damper[z]), p.vav_max_air_flow, float(self.ob.zone_air_temp[z])]
    out, seen = [], {}
    for full in self.layout.sources:
      dev = full.split("/", 1)[0]
      k = seen.get(dev, 0)
      out.append(by_dev[dev][k])
      seen[dev] = k + 1
    return out

  # ---- the three methods
  def reset(self) -> dict:
    """Environment.reset() (environment.py:1165-1212): the simulator's reset, then the first observation, whose boiler
    read stamps the episode's first instant."""
    self.ob.reset()
    if self.first_episode:          # a later episode starts from the configuration's initial temperature
      self.first_episode = False
      self.ob.reset_temps = None
    self.pos = 0
    ts = self.now
    self.ob.observe_boiler(0.0)
    n_occ = self._num_occupants(ts)
    native = self._native_obs(self.models.weather.get_current_temp(ts))
    row, nat = self.layout.row(native, self._aux(host_inputs.aux_features(self.models, ts), n_occ))
    return dict(obs=row, obs_native=nat, native=native, step_type=STEP_FIRST, reward=0.0, discount=1.0,
                duration_now=float(self.ob.state.blr_last_duration))

  def step(self, action_row: np.ndarray, rejected: bool) -> dict:
    m, ts = self.models, self.now
    d = host_inputs.step_inputs(m, ts, self.prev_update)
    if self.prev_update is not None:   # thermostat.py:134-135 on the state a fork may have brought from another building
      d["comfort_prev"] = int(self.prev_schedule.is_comfort_mode(self.prev_update))
    nxt = ts + DT
    n_occ = self._num_occupants(nxt)           # the reference asks in this order (environment.py:1310-1330)
    if self.occupants is not None:
      hour, work = host_inputs.occupancy_clock(m.occupancy, nxt)
      occupancy = self.occupants.peek(hour, bool(work))[0]
    else:
      occupancy = np.full(self.oplan.Z, float(d["occupancy"]))
    kw, cmd = {}, np.full(self.oplan.Z, np.nan)
    for col, name in enumerate(self.action_names):
      v = native_value(action_row[col], *self.action_ranges[col])
      if name == "supply_water_setpoint":
        blr = v
      elif name == "supply_air_heating_temperature_setpoint":
        heat = v
      elif name == "supply_air_cooling_temperature_setpoint":
        kw["cool_sp"] = v
      else:
        cmd[self.action_zones[col]] = float(v)
    if "supply_air_damper_percentage_command" in self.action_names:
      kw["damper_cmd"] = cmd
    o = self.ob.step(now_ts=300.0 * self.pos, t_amb_now=d["t_amb_now"], h_conv=self.h_conv, t_amb_next=d["t_amb_next"],
                     comfort_now=bool(d["comfort_now"]), comfort_prev=d["comfort_prev"] == 1,
                     comfort_next=bool(d["comfort_next"]), occupancy=occupancy, e_price=d["e_price"],
                     e_carbon=d["e_carbon"], g_price=d["g_price"], g_carbon=d["g_carbon"], action=[blr, heat], observe=True,
                     reject=bool(rejected), trace=self.trace, **kw)
    if not rejected:
      self.prev_update, self.prev_schedule = ts, m.schedule
    out = dict(n_sweeps=o["n_sweeps"], converged=int(o["converged"]), zone_temp_pre=o["zone_temp_pre"],
               zone_temp_post=o["zone_temp_post"],
               rates=np.array([o["blower_rate"], o["ac_rate"], o["gas_rate"], o["pump_rate"]], dtype=np.float64),
               mode=o["mode"], damper=o["damper"], ahu_count=o["ahu_count"], blr_count=o["blr_count"],
               accepted=o["action_accepted"], comfort=(bool(d["comfort_now"]), bool(d["comfort_next"])),
               occupancy=np.array(occupancy, dtype=np.float64), max_delta=o.get("max_delta"))
    win = ("comfort" if d["comfort_next"] else "eco")
    lo, hi = getattr(self.params, win + "_lo"), getattr(self.params, win + "_hi")
    out["window_next"] = (lo, hi)
    out["window_now"] = ((self.params.comfort_lo, self.params.comfort_hi) if d["comfort_now"]
                         else (self.params.eco_lo, self.params.eco_hi))
    out["regret"] = float(o["reward"])
    if self.reward_function is None:
      reward, out["dollars"] = float(o["reward"]), None
    else:
      r, p = self.reward_function, self.params
      cfg = dict(max_productivity_personhour_usd=p.max_prod, productivity_midpoint_delta=p.prod_delta,
                 productivity_decay_stiffness=p.prod_stiff, energy_cost_weight=r.energy_cost_weight,
                 carbon_cost_weight=r.carbon_cost_weight, carbon_cost_factor=r.carbon_cost_factor,
                 reward_normalizer_shift=r.reward_normalizer_shift, reward_normalizer_scale=r.reward_normalizer_scale)
      want = restate(cfg, lo, hi, o["zone_temp_post"], occupancy, [(o["blower_rate"], o["ac_rate"])],
                     [(o["gas_rate"], o["pump_rate"])], (d["e_price"], d["e_carbon"], d["g_price"], d["g_carbon"]), p.dt)
      reward, out["dollars"] = float(np.float32(want["agent_reward_value"])), {k: float(v) for k, v in want.items()}
    out["reward"] = reward if o["action_accepted"] else float("-inf")   # environment.py:52,1301-1302
    native = self._native_obs(d["t_amb_next"])
    out["native"] = native
    out["obs"], out["obs_native"] = self.layout.row(native, self._aux(d["aux"], n_occ))
    out["n_occ"] = n_occ
    self.pos += 1
    ended = self.pos - 1 >= self.episode_steps          # environment.py:1366-1368: N transitions plus a terminal step
    out["step_type"], out["discount"] = (STEP_LAST, 0.0) if ended else (STEP_MID, self.discount)
    if ended:                                            # the feature's same-step autoreset
      out["final_obs"], out["final_obs_native"] = out["obs"], out["obs_native"]
      first = self.reset()
      out["obs"], out["obs_native"], out["first_native"] = first["obs"], first["obs_native"], first["native"]
    out["zone_now"] = orc.zone_means(self.oplan, self.ob.temp)
    out["mode_now"], out["damper_now"] = self.ob.mode.copy(), self.ob.damper.copy()
    out["counts_now"] = (int(self.ob.state.ahu_count), int(self.ob.state.blr_count))
    # boiler.py:158-168: the duration since the boiler's last action that the last observation stamped -- after an own
    # reset the clock has gone back under the action's time stamp, and it is negative
    out["duration_now"] = float(self.ob.state.blr_last_duration)
    return out

  def copy_from(self, other: "Twin") -> None:
    """fork / restore: the other building's state into this slot -- the thermostats' previous update among it, which is
    an instant of the other building's calendar; the slot's configuration (parameters, materials, calendar, start, random
    stream) stays."""
    copy_twin(self.ob, other.ob)
    self.ob.reset_temps, self.first_episode = None, False
    self.pos = other.pos
    self.prev_update, self.prev_schedule = other.prev_update, other.prev_schedule   # state: the other building's
    if self.occupants is not None:
      self.occupants.at_work[:] = other.occupants.at_work
      self.occupants.query = other.occupants.query

  def clone(self) -> "Twin":
    """A saved copy (what a snapshot holds)."""
    c = copy.copy(self)
    c.ob = orc.OracleBuilding(self.oplan, self.params, self.ob.initial_temp)
    c.occupants = copy.deepcopy(self.occupants)
    c.copy_from(self)
    return c


# ---------------------------------------------------------------- a case as a batch
# The reducer bins NORMALISED values: (T - 190) / sqrt(408.11) for the zone temperatures (5.10 is 293 K), the command itself
# for the dampers.  The edges sit in gaps of what the twins produce: no binned value of any case comes within 1e-5
# (relative) of one, so a last-bit difference in a temperature cannot move a count (tests/test_crossed_batches_cpu.py).
HIST_PARAMS = (("zone_air_temperature_sensor", (4.0, 4.52245, 4.90363, 5.10178, 5.13874, 5.21421, 5.48743, 6.08748)),
               ("supply_air_damper_percentage_command", (0.0, 0.27753, 0.62578, 0.89506)))
REWARD = host_inputs.SetpointEnergyCarbonReward(1.5, 0.75, 0.2, reward_normalizer_shift=-3.0, reward_normalizer_scale=50.0)
OCC_NORM = 20.0
_SWITCH_ROWS = (12, 168, 300)       # SB1's schedule from START: 06:00, 19:00 and the next 06:00 local
_CAL_SWITCH = (12, 12, 18)          # tests/calendar_cases.py: each calendar's comfort switch, in rows from its start
_CAL_SWITCH_COMMON = (12, 36)       # the calendars on START (replay weather): Pacific 06:00, Berlin 17:00; UTC's is out of reach
_OCC_HOURS = ((4, 7, 13, 20), (3, 8, 12, 21), (2, 9, 14, 22))


@dataclasses.dataclass
class Op:
  kind: str                              # "step", "reset_buildings", "snapshot", "restore", "fork"
  row: int = -1                          # step: the action row
  rejected: Optional[np.ndarray] = None  # step: bool [B] or None
  mask: Optional[np.ndarray] = None      # reset_buildings
  src: Optional[np.ndarray] = None       # fork


class Scenario:
  """Everything a case needs on either side: the BatchedEnvironment's arguments, the program, and the twins."""

  def __init__(self, name: str):
    from sbsim_amd.environment import SB1_OBSERVATION_NORMALIZATION, SimConfig
    self.name, self.case = name, CASES[name]
    c = self.case
    rs = np.random.RandomState(SEED + sorted(CASES).index(name))
    self.plan = FloorPlan.from_file_input(rectangular_floor_plan(ROOMS, ROOM_SHAPE), Materials.sb1(), 10.0, 300.0)
    Z = self.plan.n_zones
    self.switches = (("SBSIM_FORCE_LDS_PATH", "1"),) if c["kernel"] == "lds" and c["materials"] == "none" else ()
    # ---- actions
    names = ["supply_water_setpoint", "supply_air_heating_temperature_setpoint"]
    ranges, zones = [(310.0, 355.0), (285.0, 300.0)], [0, 0]
    if c["actions"] == "dampers":
      names += ["supply_air_cooling_temperature_setpoint"] + ["supply_air_damper_percentage_command"] * Z
      ranges += [(301.0, 306.0)] + [(0.0, 1.0)] * Z
      zones += [0] + list(range(Z))
    # (a reset grid of 294 K would sit on SB1's heating setpoint: the episodes after the first start a little below)
    self.config = dataclasses.replace(SimConfig.sb1(), action_names=tuple(names), action_ranges=tuple(ranges),
                                      action_zones=tuple(zones), initial_temp=INITIAL_TEMP)
    self.n_steps = T + (3 if c["lifecycle"] != "none" else 0)
    self.actions = rs.uniform(-1, 1, size=(self.n_steps, B, len(names))).astype(np.float32)
    self.actions[:, 1] = self.actions[:, 0]   # buildings 0 and 1: equal actions and (below) equal initial grids
    self.bad_command = None
    if c["actions"] == "dampers":       # one command outside [0, 1]: vav.py:125-129 raises, the reward is -inf
      self.bad_command = (7, 41, 3 + 4)   # (action row, building, column)
      self.actions[self.bad_command] = np.float32(1.5)
    # ---- time
    self.per_building = c["episodes"] == "per_building"
    j, g = np.arange(B) // 3, np.arange(B) % 3
    near = lambda s: np.where(j <= min(11, s - 1), s - 1 - np.minimum(j, s - 1), s + (j - min(11, s - 1)))
    self.calendar_of = self.offsets = None
    self.calendar_kw = None
    if c["time"] == "start_offsets":
      if c["weather"] == "replay":      # the trace holds ten hours: one comfort switch is all it can show
        self.offsets = np.arange(B)
      else:
        self.offsets = np.choose(g, [near(s) for s in _SWITCH_ROWS])
    elif c["time"] == "calendars":
      self.calendar_of = g.astype(np.int32)
      common = c["weather"] == "replay"
      if common:   # (calendar 2's switch is out of the trace's reach: its buildings live in the afternoon)
        self.offsets = np.choose(g, [near(s) for s in _CAL_SWITCH_COMMON] + [60 + j])
      else:
        self.offsets = np.choose(g, [near(s) for s in _CAL_SWITCH])
      self.calendar_kw = []
      for k in range(3):
        kw = cc.members(k)
        if c["weather"] != "default":   # the per-building weather is the environment's
          kw["weather"] = None
        if common:                      # ... and the replay trace holds one morning: every calendar on the batch's date
          kw["start_timestamp"] = None
        if c["occupancy"] == "device":
          kw["occupancy"] = self._device_occupancy(k)
        self.calendar_kw.append(kw)
    if self.offsets is not None:
      self.offsets = self.offsets.astype(np.int64)
    self.episode_steps = None
    if self.per_building:               # 3 .. 9; the buildings placed before a switch long enough to cross it
      self.episode_steps = np.where(j <= 9, np.maximum(3, j), 3 + (np.arange(B) * 5) % 7).astype(np.int64)
    # ---- rows
    self.bparams = random_params(B, seed=SEED + 1, keep_default=()) if c["params"] != "none" else None
    self.bmaterials = None
    if c["materials"] != "none":
      self.slot_ids, table = self.plan.material_slots()
      self.material_sets = table[None] * rs.uniform(0.5, 2.0, size=(B,) + table.shape)
      self.h_convs = rs.uniform(20.0, 150.0, size=B)
      self.bmaterials = host_inputs.BuildingMaterials(
          conductivity=self.material_sets[:, :, 0], heat_capacity=self.material_sets[:, :, 1],
          density=self.material_sets[:, :, 2], convection_coefficient=self.h_convs)
    # ---- weather
    self.weather_rows = None
    if c["weather"] == "sinusoid":
      low = 268.0 + 0.2 * np.arange(B)
      self.weather_rows = (low, low + 8.0 + 0.1 * np.arange(B))
    elif c["weather"] == "replay":      # whole seconds: ts + offset is exact on either side
      t0 = dt.datetime(2023, 7, 1, 0, 0, tzinfo=UTC)
      self.weather_rows = ((t0 - START).total_seconds() + 600.0 + 37.0 * np.arange(B),)
    # ---- the initial grids: a different offset per zone and building (tests/zone_ladder.py)
    from tests.zone_ladder import initial_grids
    self.init = initial_grids(self.plan, B, seed=SEED + 2)
    self.init[1] = self.init[0]
    # ---- observation
    self.hist = c["observation"] == "histogram"
    self.layout = ObsLayout(self.plan.zone_names, SB1_OBSERVATION_NORMALIZATION, HIST_PARAMS if self.hist else None,
                            self.hist)
    self.occ_norm = OCC_NORM if c["occupancy"] == "device" else 0.0
    self.reward_function = REWARD if c["reward"] == "dollars" else None
    # ---- the program
    self.program: List[Op] = []
    rej = {}
    if c["rejection"] == "mask":
      rej = {2: (np.arange(B) % 5 == 1), 5: (np.arange(B) % 4 == 2)}
    # (not the buildings whose episode would then no longer end inside the run, nor those still on their way to a switch)
    self.reset_mask = ((np.arange(B) % 3 != 1) & (self.episode_steps <= 6) & ~((j >= 5) & (j <= 9))) if self.per_building else None
    self.fork_src = (np.arange(B) * 7 + 3) % 23
    row = 0
    for t in range(T):
      if self.per_building and t == 5:
        self.program.append(Op("reset_buildings", mask=self.reset_mask))
      if c["lifecycle"] != "none" and t == 4:
        self.program.append(Op("snapshot"))
        for _ in range(3):
          self.program.append(Op("step", row=row))
          row += 1
        self.program.append(Op("restore"))
      if c["lifecycle"] != "none" and t == 9:
        self.program.append(Op("fork", src=self.fork_src))
      self.program.append(Op("step", row=row, rejected=rej.get(t)))
      row += 1
    assert row == self.n_steps

  # ---- models
  def _device_occupancy(self, k: int):
    zone = ("US/Pacific", "Europe/Berlin", "UTC")[k]
    return host_inputs.BatchedRandomizedArrivalDepartureOccupancy(10, *_OCC_HOURS[k], 300.0, seed=77, time_zone=zone,
                                                                  holiday_calendar=None)

  def _weather(self):
    c = self.case
    if c["weather"] == "sinusoid":
      return host_inputs.BatchedSinusoidWeather(*self.weather_rows, convection_coefficient=H_CONV)
    if c["weather"] == "replay":
      return host_inputs.BatchedReplayWeather(WEATHER_CSV, self.weather_rows[0], convection_coefficient=H_CONV)
    return host_inputs.WeatherController(273.0, 283.0, convection_coefficient=H_CONV)

  def env_kwargs(self) -> dict:
    """BatchedEnvironment(plan, B, **these): fresh model objects on every call."""
    c = self.case
    kw = dict(config=self.config, weather=self._weather(), start_timestamp=START, num_days_in_episode=(N_EPISODE + 0.5) / 288,
              collect_info=True, building_params=self.bparams, building_materials=self.bmaterials,
              reward_function=self.reward_function, occupancy_normalization_constant=self.occ_norm)
    from sbsim_amd.environment import SB1_OBSERVATION_NORMALIZATION
    kw["observation_normalization"] = SB1_OBSERVATION_NORMALIZATION
    if self.hist:
      kw.update(observation_histogram_parameters=[(n, list(b)) for n, b in HIST_PARAMS], normalize_reduce=True)
    if c["occupancy"] == "device" and self.calendar_kw is None:
      kw["occupancy"] = self._device_occupancy(0)
    if c["time"] == "start_offsets":
      kw["start_offsets"] = self.offsets
    if self.calendar_kw is not None:
      kw.update(calendars=[host_inputs.Calendar(**k) for k in self.calendar_kw], calendar_of=self.calendar_of,
                start_offsets=self.offsets)
    if self.per_building:
      kw["episode_steps"] = self.episode_steps
    return kw

  def twin(self, b: int) -> Twin:
    c, cfg = self.case, self.config
    # the building's own models: fresh objects, nothing shared with the environment under test
    weather = host_inputs.WeatherController(273.0, 283.0, convection_coefficient=H_CONV)
    sched = cfg.schedule()
    occ = host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1, holiday_calendar="us")
    elec, gas = host_inputs.ElectricityEnergyCost(holiday_calendar="us"), host_inputs.NaturalGasEnergyCost()
    start, k = START, 0
    if self.calendar_kw is not None:
      k = int(self.calendar_of[b])
      m = cc.members(k)
      sched, occ, elec, gas = m["schedule"], m["occupancy"], m["electricity_energy_cost"], m["natural_gas_energy_cost"]
      if self.calendar_kw[k]["weather"] is not None:
        weather = m["weather"]
      if self.calendar_kw[k]["start_timestamp"] is not None:
        start = m["start_timestamp"]
    occupants = None
    if c["occupancy"] == "device":
      occ = self._device_occupancy(k)
      occupants = DeviceOccupancyOracle(1, self.plan.n_zones, occ.zone_assignment, *occ.hours, occ.time_step_sec, seed=occ.seed,
                                        first_building=b)
    if c["weather"] == "sinusoid":
      weather = host_inputs.WeatherController(float(self.weather_rows[0][b]), float(self.weather_rows[1][b]))
    elif c["weather"] == "replay":
      weather = _Replay(float(self.weather_rows[0][b]))
    if self.offsets is not None:
      start = start + int(self.offsets[b]) * DT
    models = host_inputs.StepModels(weather, sched, occ, elec, gas, DT, tuple(self.plan.zone_names), self.occ_norm)
    row = c_row(self.bparams, b) if self.bparams is not None else {}
    base = dict(
        dt=cfg.time_step_sec, conv_threshold=cfg.convergence_threshold, iter_limit=cfg.iteration_limit,
        vav_max_air_flow=cfg.vav_max_air_flow_rate, vav_max_water_flow=cfg.vav_reheat_max_water_flow_rate,
        ahu_recirc=cfg.ahu_recirculation, ahu_heat_sp=cfg.ahu_heating_air_temp_setpoint,
        ahu_cool_sp=cfg.ahu_cooling_air_temp_setpoint, ahu_dp=cfg.ahu_fan_differential_pressure,
        ahu_eff=cfg.ahu_fan_efficiency, ahu_max_flow=cfg.ahu_max_air_flow_rate, blr_setpoint=cfg.boiler_reheat_water_setpoint,
        blr_head=cfg.boiler_water_pump_differential_head, blr_pump_eff=cfg.boiler_water_pump_efficiency,
        comfort_lo=cfg.comfort_temp_window[0], comfort_hi=cfg.comfort_temp_window[1], eco_lo=cfg.eco_temp_window[0],
        eco_hi=cfg.eco_temp_window[1], blr_heating_rate=cfg.boiler_heating_rate, blr_cooling_rate=cfg.boiler_cooling_rate,
        blr_conv=cfg.boiler_convection_coefficient, blr_len=cfg.boiler_tank_length, blr_radius=cfg.boiler_tank_radius,
        blr_capacity=cfg.boiler_water_capacity, blr_ins_k=cfg.boiler_insulation_conductivity,
        blr_ins_thick=cfg.boiler_insulation_thickness, max_prod=cfg.max_productivity_personhour_usd,
        min_prod=cfg.min_productivity_personhour_usd, max_elec=cfg.max_electricity_rate, max_gas=cfg.max_natural_gas_rate,
        prod_delta=cfg.productivity_midpoint_delta, prod_stiff=cfg.productivity_decay_stiffness,
        w_prod=cfg.productivity_weight, w_cost=cfg.energy_cost_weight, w_carbon=cfg.carbon_emission_weight, ahu_has_weather=1)
    base.update(row)
    plan, h = self.plan, H_CONV
    if self.bmaterials is not None:
      plan, h = substituted(self.plan, self.slot_ids, self.material_sets[b]), float(self.h_convs[b])
    return Twin(plan=plan, h_conv=h, params=orc.OracleParams(**base), start=start, models=models,
                episode_steps=int(self.episode_steps[b]) if self.per_building else N_EPISODE, discount=1.0,
                reward_function=self.reward_function, layout=self.layout, action_names=cfg.action_names,
                action_zones=cfg.action_zones, action_ranges=cfg.action_ranges, init_grid=self.init[b],
                initial_temp=cfg.initial_temp, occupants=occupants)

  def twins(self) -> List[Twin]:
    return [self.twin(b) for b in range(B)]


# ---------------------------------------------------------------- the twins' rollout of a case (computed once)
_SCENARIOS: Dict[str, Scenario] = {}
_EXPECTED: Dict[Tuple[str, bool], list] = {}


def scenario(name: str) -> Scenario:
  if name not in _SCENARIOS:
    _SCENARIOS[name] = Scenario(name)
  return _SCENARIOS[name]


def expected(name: str, trace: bool = False) -> list:
  """Per entry of the program (index 0: reset()): (op, [B] results of the twins, or None for an op without outputs), and
  at the end ("final", the twins' grids [B, H * W]).  trace: every step also holds its sweeps' max|delta|."""
  key = (name, trace)
  if key in _EXPECTED:
    return _EXPECTED[key]
  if not trace and (name, True) in _EXPECTED:
    return _EXPECTED[(name, True)]
  sc = scenario(name)
  twins = sc.twins()
  for tw in twins:
    tw.trace = trace
  out = [(Op("reset"), [tw.reset() for tw in twins])]
  saved = None
  for op in sc.program:
    if op.kind == "step":
      rej = op.rejected if op.rejected is not None else np.zeros(B, dtype=bool)
      out.append((op, [twins[b].step(sc.actions[op.row, b], bool(rej[b])) for b in range(B)]))
    elif op.kind == "reset_buildings":
      out.append((op, [twins[b].reset() if op.mask[b] else None for b in range(B)]))
    elif op.kind == "snapshot":
      saved = [tw.clone() for tw in twins]
      out.append((op, None))
    elif op.kind == "restore":
      for tw, s in zip(twins, saved):
        tw.copy_from(s)
      out.append((op, None))
    elif op.kind == "fork":
      copies = [tw.clone() for tw in twins]
      for b in range(B):
        twins[b].copy_from(copies[int(op.src[b])])
      out.append((op, None))
  out.append((Op("final"), np.stack([tw.ob.temp.copy() for tw in twins])))
  _EXPECTED[key] = out
  return out
