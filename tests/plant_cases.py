"""k_pre and k_post at the plant's edges, against oracle twins (test utility, no GPU).

A step is k_pre, the sweep kernel, k_post.  The plant algebra around the sweep (pre_building / post_building in
sbsim_amd/csrc/sb_device.h) is a chain of comparisons and float32 roundings; a rollout keeps every decision off its
edge and compares rates at 2e-6, so `<` for `<=` or one rounding fewer pass it.  Here every case puts an operand ON an
edge, one nextafter below it and one above it, and the device is held to the twin bit for bit through the C ABI's taps
(sb_tap_pre / sb_tap_post: prescribed doubles in, no sweep kernel).

A `Case` is one building's prescribed state and one sb_step_in; `expected(case)` is its twin: an `OracleBuilding` on the
same plan with its own `OracleParams` (the case's row of the per-building parameter table), its grid filled zone by
zone, stepped once -- the pre half before its own sweep, the post half after it.  The info row, whose columns the
oracle does not all expose, is `post_chain`: productivity -> reward and the boiler's gas rate in Python floats
(float64, one rounding per operation, the reference's order) and np.float32, which
tests/test_plant_cases_cpu.py holds EQUAL to sbo_reward / sbo_dev_boiler_gas_rate on every case.  exp and log are the
only operations in which the device's libm and the host's may differ: `excused(case)` says whether moving their
results by up to two double ulps changes any float32 output.

tests/test_plant_cases_cpu.py checks the conditions on the inputs (every edge hit from both sides), on the oracle
alone; tests/test_plant_differential_gpu.py runs the cases on the device."""
from __future__ import annotations

import collections
import dataclasses
import fractions
import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import oracle as orc
from sbsim_amd import _ffi
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
from sbsim_amd.host_inputs import BuildingParams, SetpointEnergyCarbonReward
from tests.params_cases import c_row, random_params
from tests.twins import oracle_plan_of

B = 70
TAPPED = (0, 15, 16, 63, 64, 69)    # bparam's k * B + b at rows far apart (a tap launches its one building alone)
ROOM = (8, 8)                       # 64 cells: zone_temp * 64 / 64 is exact
H_CONV = 12.0
SEED = 4711
KEEP = float(np.float32(_ffi.SB_ACTION_KEEP))
C_AIR, C_WATER, RHO_WATER, GRAVITY = 1006.0, 4180.0, 1000.0, 9.8   # utils/constants.py:21-22, 46-47
REWARD = SetpointEnergyCarbonReward(1.5, 0.75, 0.2, reward_normalizer_shift=-3.0, reward_normalizer_scale=50.0)
WATER, HEAT, COOL, DAMPER = ("supply_water_setpoint", "supply_air_heating_temperature_setpoint",
                             "supply_air_cooling_temperature_setpoint", "supply_air_damper_percentage_command")


def up(x: float, n: int = 1) -> float:
  for _ in range(n):
    x = math.nextafter(x, math.inf)
  return x


def dn(x: float, n: int = 1) -> float:
  for _ in range(n):
    x = math.nextafter(x, -math.inf)
  return x


def nudge(x: float, k: int) -> float:
  return up(x, k) if k >= 0 else dn(x, -k)


def trio(x: float) -> Tuple[float, float, float]:
  """One nextafter below the edge, the edge, one above."""
  return dn(x), x, up(x)


def f32(x) -> float:
  """A double through a proto float field."""
  with np.errstate(over="ignore"):
    return float(np.float32(x))


def up32(x: float) -> float:
  return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def dn32(x: float) -> float:
  return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


# ---------------------------------------------------------------- handles
@dataclasses.dataclass(frozen=True)
class Spec:
  """One device handle: what sb_create and the per-handle setters fix."""
  name: str
  rooms: Tuple[int, int]
  dampers: bool          # False: the default two-column action set; True: + cooling setpoint + a damper column per zone
  dollars: bool          # sb_set_reward_function(REWARD)
  dt: float
  params_seed: int       # of the handle's per-building parameter table


SPECS: Dict[str, Spec] = {s.name: s for s in (
    Spec("z2-pair-regret", (1, 2), False, False, 300.0, 1),
    Spec("z18-dampers-regret", (3, 6), True, False, 300.0, 2),
    Spec("z18-pair-dollars", (3, 6), False, True, 180.0, 3),
    Spec("z2-dampers-dollars", (1, 2), True, True, 180.0, 4),
)}


@functools.lru_cache(maxsize=None)
def plan_of(rooms: Tuple[int, int]) -> FloorPlan:
  return FloorPlan.from_file_input(rectangular_floor_plan(rooms, ROOM), Materials.sb1(), 10.0, 300.0)


@functools.lru_cache(maxsize=None)
def oracle_plan(rooms: Tuple[int, int]) -> orc.OraclePlan:
  return oracle_plan_of(plan_of(rooms))


def n_zones(spec: Spec) -> int:
  return spec.rooms[0] * spec.rooms[1]


def action_set(spec: Spec):
  """(names, zones, ranges): the damper columns in REVERSE zone order -- a column is not its zone's index."""
  Z = n_zones(spec)
  if not spec.dampers:
    return (WATER, HEAT), (0, 0), ((310.0, 355.0), (285.0, 300.0))
  return ((WATER, HEAT, COOL) + (DAMPER,) * Z, (0, 0, 0) + tuple(range(Z - 1, -1, -1)),
          ((310.0, 355.0), (285.0, 300.0), (296.0, 305.0)) + ((0.0, 1.0),) * Z)


def config_of(spec: Spec):
  from sbsim_amd.environment import SimConfig   # (here, not at the top: the module imports torch)
  names, zones, ranges = action_set(spec)
  return dataclasses.replace(SimConfig.sb1(), time_step_sec=spec.dt, action_names=names, action_zones=zones,
                             action_ranges=ranges)


def _seq_sum(x: float, k: int) -> float:
  s = 0.0
  for _ in range(k):
    s += x
  return s


@functools.lru_cache(maxsize=None)
def building_params(name: str):
  """The handle's per-building table: every field of every building drawn around SB1, then, for the tapped buildings,
  the fields an edge needs.  ahu_max_air_flow_rate sits on the running air flow of a building whose dampers are all
  open (k zones of 1.0 * vav_max_air_flow, added in zone order): reached exactly, or one nextafter under it so that the
  clamp binds at that zone -- 15 is the last zone of k_pre's first pass, 16 and 17 are its second."""
  spec = SPECS[name]
  Z = n_zones(spec)
  bp = random_params(B, seed=SEED + spec.params_seed, keep_default=())
  f = {k: v.copy() for k, v in bp.fields.items()}
  vav = f["vav_max_air_flow_rate"]
  if Z == 18:
    at = {0: _seq_sum(vav[0], 16), 15: dn(_seq_sum(vav[15], 16)), 16: dn(_seq_sum(vav[16], 17)),
          63: dn(_seq_sum(vav[63], 18)), 64: _seq_sum(vav[64], 18)}
  else:
    at = {0: _seq_sum(vav[0], 2), 15: dn(_seq_sum(vav[15], 2)), 16: dn(_seq_sum(vav[16], 1)), 63: _seq_sum(vav[63], 1)}
  for b, v in at.items():
    f["ahu_max_air_flow_rate"][b] = v
  f["ahu_recirculation"][64] = 1.0         # mixed == the grid's mean: an fp32 action can land on it
  f["boiler_heating_rate"][63] = 0.0       # one of the two rates 0: the tank follows the setpoint at once
  f["boiler_cooling_rate"][69] = 0.0
  f["max_electricity_rate"][63] = 2500.0   # the caps bind
  f["max_natural_gas_rate"][69] = 450.0
  f["max_natural_gas_rate"][15] = 20000.0
  # ... and ON the caps: the rates do not depend on them, so building 16's max_electricity_rate is the electricity rate
  # (blower + |air conditioning|) + pump of cap_case on the rows so far, building 64's max_natural_gas_rate its gas rate
  for b, field, rate in ((ELEC_CAP_BUILDING, "max_electricity_rate", lambda r: (r[0] + abs(r[1])) + r[3]),
                         (GAS_CAP_BUILDING, "max_natural_gas_rate", lambda r: r[2])):
    row = _row_of(name, f, b)
    case = cap_case(name, b, row, "probe")
    rates = [float(v) for v in post_chain(case, _twin_step(case, None, row=row), p=row)["info"][:4]]
    assert rate(rates) > 0.0, (name, b, rates)
    f[field][b] = rate(rates)
  return BuildingParams(f)


def cap_case(name: str, b: int, row: dict, label: str, occupancy=2.5, prices=None) -> "Case":
  """A fixed, quiet state of building b (row: its parameters): no request, every zone inside the comfort window, the
  tank on its setpoint.  Its energy rates depend on neither cap, occupancy nor prices; building_params puts a cap on them."""
  Z = n_zones(SPECS[name])
  lo, hi = row["comfort_lo"], row["comfort_hi"]
  sc = np.zeros(16)
  sc[0], sc[1], sc[4], sc[8], sc[10] = row["ahu_heat_sp"], row["ahu_cool_sp"], row["blr_setpoint"], row["blr_setpoint"], SPECS[name].dt
  sc[12:16] = (1.5e6, 2.5e6, 3.5e6, 4.5e6)
  c = Case("reward", label, name, b, zone_temps=lo + (hi - lo) * (0.35 + 0.05 * (np.arange(Z) % 7)),
           modes=np.zeros(Z, np.int32), valves=np.zeros(Z), scal=sc, occupancy=occupancy, tags=("reward:on-cap",))
  if prices is not None:
    c.prices = prices
  n_cells = oracle_plan(SPECS[name].rooms).n_cells
  for k in range(16):   # (the wall _Builder.add will settle on: the grid's mean must survive sb_tap_post's (mean * N) / N)
    c.wall = 291.25 + 0.0625 * k
    c.scal[11] = orc.np_mean(grid_of(c))
    if grid_mean_arg(c.scal[11], n_cells) is not None:
      return c
  raise AssertionError((name, b))


ELEC_CAP_BUILDING, GAS_CAP_BUILDING = 16, 64


@functools.lru_cache(maxsize=None)
def params_row(name: str, b: int) -> dict:
  """Building b's OracleParams arguments (tests/crossed_batches.py builds them the same way)."""
  return _row_of(name, building_params(name).fields, b)


def _row_of(name: str, fields: dict, b: int) -> dict:
  cfg = config_of(SPECS[name])
  base = dict(
      dt=cfg.time_step_sec, conv_threshold=0.0, iter_limit=0,
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
  base.update(c_row(BuildingParams(fields), b))
  return base


# ---------------------------------------------------------------- weather: the three device forms of ambient_temp
TRACES: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}


def _make_traces():
  rs = np.random.RandomState(SEED)
  for n in (2, 37):
    times = np.cumsum(rs.uniform(200.0, 900.0, size=n)) + 1000.0
    tempf = rs.uniform(20.0, 95.0, size=n)
    TRACES[f"trace{n}"] = (times, tempf)
  TRACES["offsets"] = (np.round(rs.uniform(-50.0, 50.0, size=B)), None)            # whole seconds per building
  lo = rs.uniform(265.0, 285.0, size=B)
  TRACES["lohi"] = (np.stack([lo, lo + rs.uniform(3.0, 17.0, size=B)], axis=1), None)   # the sinusoid's (low, high)
  TRACES["tamb"] = (rs.uniform(260.0, 310.0, size=(B, 2)), None)                   # t_amb_dev: (now, next) per building


_make_traces()


def replay_kelvin(trace: str, x: float) -> float:
  """np.interp, then conversion_utils.fahrenheit_to_kelvin (conversion_utils.py:155-171) as written there."""
  times, tempf = TRACES[trace]
  f = float(np.interp(x, times, tempf))
  return (f - 32.0) * 5.0 / 9.0 + 273.15


def ambient_of(weather: tuple, b: int) -> Tuple[float, float]:
  """(t_now, t_next) of building b under a case's weather: ("scalar", now, next), ("tamb",),
  ("sinusoid", f_now, f_next) or ("replay", trace, x_now, x_next, with per-building offsets)."""
  kind = weather[0]
  if kind == "scalar":
    return float(weather[1]), float(weather[2])
  if kind == "tamb":
    return float(TRACES["tamb"][0][b, 0]), float(TRACES["tamb"][0][b, 1])
  if kind == "sinusoid":   # weather_controller.py:119-121: two roundings, no fused multiply-add
    lo, hi = (float(v) for v in TRACES["lohi"][0][b])
    return tuple(float(f) * (hi - lo) + lo for f in weather[1:3])
  _, trace, x_now, x_next, shifted = weather
  off = float(TRACES["offsets"][0][b]) if shifted else 0.0
  return replay_kelvin(trace, x_now + off), replay_kelvin(trace, x_next + off)


# ---------------------------------------------------------------- a case
@dataclasses.dataclass
class Case:
  family: str
  label: str
  spec: str
  b: int
  zone_temps: np.ndarray                 # [Z] the zones' means before the step (their fill values are searched)
  modes: np.ndarray                      # [Z] stored thermostat modes 0..3
  valves: np.ndarray                     # [Z] stored reheat valves (read by a rejected building alone)
  scal: np.ndarray                       # [16] sb_get_scalars' order; [11] is set from the grid
  action: Optional[np.ndarray] = None    # float32 [n_actions] or None
  native: bool = False                   # sb_step_in.actions_native
  comfort: Tuple[int, int, int] = (1, 1, 1)   # now, prev (-1: none), next
  has_action: bool = False
  occupancy: object = 2.5                # one value for every zone, or [Z] (sb_step_in.occupancy_dev)
  prices: Tuple[float, float, float, float] = (3.1e-8, 1.3e-7, 9.7e-9, 4.9e-8)
  weather: tuple = ("scalar", 280.3, 281.1)
  reject: bool = False                   # sb_step_in.reject_dev[b]
  sweeps: int = 0                        # the twin's iteration limit: 0 leaves the grid as it is (post means == pre means)
  wall: float = 291.25                   # every cell outside the zones
  prime: Optional["Case"] = None         # tapped on the same building just before (a rejected building keeps ITS dampers)
  tags: Tuple[str, ...] = ()
  tie: object = None                     # called with the case once its grid is known (a setpoint tied to the grid's mean)
  twin: Optional[dict] = dataclasses.field(default=None, repr=False, compare=False)   # expected(case), computed once

  @property
  def id(self) -> str:
    return f"{self.family}/{self.label}"


_NROOM = ROOM[0] * ROOM[1]


@functools.lru_cache(maxsize=4096)
def _fill_for(target: float) -> Tuple[float, float]:
  hi = float((np.array([target]).view(np.int64) & ~np.int64(7)).view(np.float64)[0])
  first = hi + float(_NROOM) * (target - hi)
  cells = np.full(_NROOM, hi)
  cells[0] = first
  assert orc.np_mean(cells) == target, f"no fill gives a zone mean of {target!r}"
  return first, hi


def fill_for(target: float) -> np.ndarray:
  """64 cell values whose numpy mean is `target` exactly.  64 copies of the target will not do: numpy's pairwise sum
  rounds at 3x, 5x, 6x, 7x.  The target with its last three bits cleared adds up without a rounding, and the zone's
  first cell carries 64 times what was cleared (at most 448 ulps)."""
  first, hi = _fill_for(float(target))
  cells = np.full(_NROOM, hi)
  cells[0] = first
  return cells


def grid_of(case: Case) -> np.ndarray:
  op = oracle_plan(SPECS[case.spec].rooms)
  g = np.full(op.n_cells, float(case.wall))
  for z, cells in enumerate(op.zones):
    g[cells] = fill_for(float(case.zone_temps[z]))
  return g


def grid_mean_arg(m: float, n_cells: int) -> Optional[float]:
  """sb_tap_post takes the grid's mean and hands k_post its sum: the argument g with (g * N) / N == m."""
  for k in (0, 1, -1, 2, -2, 3, -3):
    g = nudge(m, k)
    if g * float(n_cells) / float(n_cells) == m:
      return g
  return None


def native_values(spec: Spec, action, native: bool) -> List[Optional[float]]:
  """Per column the native value as the device forms it (bounded_action_normalizer.py:73-98, then the proto's float
  field), or None for a column the request does not mention."""
  out = []
  _, _, ranges = action_set(spec)
  for a, (lo, hi) in zip(action, ranges):
    a = float(np.float32(a))
    if native:
      out.append(None if a <= KEEP else a)
    else:
      out.append(f32((a + 1.0) / 2.0 * (hi - lo) + lo))
  return out


# ---------------------------------------------------------------- the post half in Python floats
def gas_rate(p: dict, blr_sp, blr_flow, blr_return, t_next, tank_change, duration, lg=math.log) -> float:
  """boiler.py:233-320 (+ the tank term of :158-217): sbo_dev_boiler_gas_rate, operation by operation."""
  supply_w = blr_sp if blr_sp > blr_return else blr_return
  flow_heat = C_WATER * blr_flow * (supply_w - blr_return)
  num = p["blr_len"] * 2.0 * math.pi * (supply_w - t_next)
  r1 = p["blr_radius"]
  r2 = r1 + p["blr_ins_thick"]
  diss = num / (lg(r2 / r1) / p["blr_ins_k"] + 1.0 / p["blr_conv"] / r2)
  tank = 0.0
  if duration > 0:
    tank = C_WATER * p["blr_capacity"] * tank_change / duration
  return flow_heat + diss + tank


def productivity(p: dict, hsp32: float, csp32: float, zt32, occ32, dt: float, ex=math.exp) -> Tuple[float, float]:
  """base_setpoint_energy_carbon_reward.py:52-123 on proto floats: (cumulative productivity, total occupancy)."""
  cumulative = total = 0.0
  for t, occ in zip(zt32, occ32):
    total += occ
    if t < hsp32:
      prod = p["max_prod"] / (1.0 + ex(-p["prod_stiff"] * (t - (hsp32 - p["prod_delta"]))))
    elif t > csp32:
      prod = p["max_prod"] * (1.0 - 1.0 / (1.0 + ex(-p["prod_stiff"] * (t - (csp32 + p["prod_delta"])))))
    else:
      prod = p["max_prod"]
    cumulative += prod * occ * dt / 3600.0
  return cumulative, total


def regret(p: dict, hsp32, csp32, zt32, occ32, rates32, dt, prices, ex=math.exp) -> Tuple[float, Dict[int, float]]:
  """setpoint_energy_carbon_regret.py:142-291: (the reward, the RewardResponse fields by info column) in float64."""
  e_price, e_carbon, g_price, g_carbon = prices
  blower, ac, gas, pump = rates32
  cumulative, total = productivity(p, hsp32, csp32, zt32, occ32, dt, ex)
  max_p = p["max_prod"] * total * dt / 3600.0
  min_p = p["min_prod"] * total * dt / 3600.0
  actual = cumulative if cumulative > min_p else min_p
  npr = (actual - min_p) / (max_p - min_p) - 1.0 if total > 0.0 else 0.0
  elec = (blower + abs(ac)) + pump
  cap_e = elec if elec < p["max_elec"] else p["max_elec"]
  ce, ce_max = e_price * abs(cap_e) * dt, e_price * abs(p["max_elec"]) * dt
  ke, ke_max = e_carbon * abs(cap_e) * dt, e_carbon * abs(p["max_elec"]) * dt
  cap_g = gas if gas < p["max_gas"] else p["max_gas"]
  g_eff = 0.0 if cap_g < 0.0 else cap_g
  cg, cg_max = g_price * (g_eff * dt), g_price * (p["max_gas"] * dt)
  kg, kg_max = g_carbon * (g_eff * dt), g_carbon * (p["max_gas"] * dt)
  nec = (ce + cg) / (ce_max + cg_max)
  nce = (ke + kg) / (ke_max + kg_max)
  reward = (npr * p["w_prod"] - nec * p["w_cost"] - nce * p["w_carbon"]) / (p["w_prod"] + p["w_cost"] + p["w_carbon"])
  cols = {8: actual, 9: ce, 10: cg, 11: ke + kg, 12: 0.0, 13: p["w_prod"], 14: p["w_cost"], 15: p["w_carbon"],
          16: p["max_prod"], 17: total, 18: 1.0, 19: 0.0, 20: actual - max_p, 21: npr, 22: nec, 23: nce}
  return reward, cols


def dollars(p: dict, hsp32, csp32, zt32, occ32, rates32, dt, prices, ex=math.exp) -> Tuple[float, Dict[int, float]]:
  """setpoint_energy_carbon_reward.py:127-190 (tests/reward_cases.restate holds the same, with numpy's exp)."""
  e_price, e_carbon, g_price, g_carbon = prices
  blower, ac, gas, pump = rates32
  cumulative, _ = productivity(p, hsp32, csp32, zt32, occ32, dt, ex)
  elec = (blower + abs(ac)) + pump
  gas = 0.0 if gas < 0.0 else gas
  ce, ke = e_price * abs(elec) * dt, e_carbon * abs(elec) * dt
  cg, kg = g_price * (gas * dt), g_carbon * (gas * dt)
  carbon = ke + kg
  carbon_cost = f32(carbon * REWARD.carbon_cost_factor)
  raw = cumulative - REWARD.energy_cost_weight * (ce + cg) - REWARD.carbon_cost_weight * carbon_cost
  reward = (raw - REWARD.reward_normalizer_shift) / REWARD.reward_normalizer_scale
  cols = {8: cumulative, 9: ce, 10: cg, 11: carbon, 12: carbon_cost}
  cols.update({k: 0.0 for k in range(13, _ffi.SB_INFO_STRIDE)})
  return reward, cols


def post_chain(case: Case, e: dict, ex=math.exp, lg=math.log, p: Optional[dict] = None) -> dict:
  """Everything k_post writes for the case, from the twin's pre half `e`, its post-sweep zone means and grid mean:
  the float32 info row and reward, and the 16 scalars afterwards."""
  spec = SPECS[case.spec]
  p = p or params_row(case.spec, case.b)
  dt = spec.dt
  win = ("comfort" if case.comfort[2] else "eco")
  hsp32, csp32 = f32(p[win + "_lo"]), f32(p[win + "_hi"])
  zt32 = [f32(t) for t in e["zone_temp_post"]]
  occ32 = [f32(o) for o in e["occupancy"]]
  r = p["ahu_recirc"]
  intake = e["ahu_flow"] * p["ahu_dp"] / p["ahu_eff"]                                  # air_handler.py:287-320
  exhaust = (e["ahu_flow"] * (1.0 - r)) * p["ahu_dp"] / p["ahu_eff"]
  mixed2 = r * e["grid_mean"] + (1 - r) * e["t_next"]
  supply2 = e["cool_sp"] if mixed2 > e["cool_sp"] else e["heat_sp"] if mixed2 < e["heat_sp"] else mixed2
  rates = (f32(intake + exhaust), f32(e["ahu_flow"] * C_AIR * (supply2 - mixed2)),
           f32(gas_rate(p, e["blr_sp"], e["blr_flow"], e["blr_return"], e["t_next"], e["tank_change"], e["duration"], lg)),
           f32(e["blr_flow"] * RHO_WATER * GRAVITY * p["blr_head"] / p["blr_pump_eff"]))
  fn = dollars if spec.dollars else regret
  reward, cols = fn(p, hsp32, csp32, zt32, occ32, rates, dt, case.prices, ex)
  info = np.zeros(_ffi.SB_INFO_STRIDE, dtype=np.float32)
  info[:4] = rates
  info[4], info[5], info[6], info[7] = e["n_sweeps"], 1.0, f32(e["t_sa"]), f32(reward)   # (the tap says "converged")
  for k, v in cols.items():
    info[k] = f32(v)
  scal = np.array([e["heat_sp"], e["cool_sp"], e["ahu_flow"], e["ahu_count"], e["blr_sp"], e["blr_flow"], e["blr_count"],
                   e["blr_return"], e["tank"], e["tank_change"], e["duration"], e["grid_mean"]] +
                  [case.scal[12 + i] + rates[i] * dt for i in range(4)])
  return dict(info=info, reward=np.float32(reward) if e["accepted"] else np.float32(-np.inf), reward_f64=reward,
              scal_after=scal, cols=cols)


# ---------------------------------------------------------------- the twin
def _twin_step(case: Case, carry: Optional[dict], row: Optional[dict] = None) -> dict:
  """The case on an OracleBuilding of its own (row: the building's parameters, default params_row's)."""
  spec = SPECS[case.spec]
  Z, op = n_zones(spec), oracle_plan(spec.rooms)
  prm = orc.OracleParams(**dict(row or params_row(case.spec, case.b), iter_limit=int(case.sweeps)))
  ob = orc.OracleBuilding(op, prm, 0.0, reset_temps=grid_of(case))
  s = ob.state
  ob.mode[:] = case.modes
  ob.valve[:] = case.valves
  if carry is not None:
    ob.damper[:] = carry["damper"]
  sc = case.scal
  s.ahu_heat_sp, s.ahu_cool_sp, s.blr_setpoint = sc[0], sc[1], sc[4]
  s.blr_tank_temp, s.blr_tank_change, s.blr_last_duration = sc[8], sc[9], sc[10]
  now, prev, nxt = case.comfort
  s.thermostat_has_prev, s.thermostat_skipped = int(prev != -1), 0
  dt = spec.dt
  if case.has_action and not case.reject and carry is None:
    now_ts = 0.0                        # the action stamps the boiler: the duration it sees is dt
  elif case.has_action and carry is not None:
    now_ts = dt                         # the request after the prime's, rejected: the prime's stamp is two steps old
    s.blr_has_action_ts, s.blr_action_ts = 1, 0.0
  else:
    # no request at all: the observation at now + dt finds the stored duration
    now_ts = -dt
    s.blr_has_action_ts, s.blr_action_ts = 1, -float(sc[10])
  kw, action = {}, None
  if case.has_action:
    # a field the request leaves out: the setpoint in force, handed over as the double it is
    blr, heat, cmd = float(sc[4]), float(sc[0]), np.full(Z, np.nan)
    names, zones, _ = action_set(spec)
    for name, zone, v in zip(names, zones, native_values(spec, case.action, case.native)):
      if v is None:
        assert name != WATER, "every request carries the boiler's setpoint (the twin's interface stamps it)"
      elif name == WATER:
        blr = v
      elif name == HEAT:
        heat = v
      elif name == COOL:
        kw["cool_sp"] = v
      else:
        cmd[zone] = v
    if spec.dampers:
      kw["damper_cmd"] = cmd
    action = (blr, heat)
  t_now, t_next = ambient_of(case.weather, case.b)
  occ = np.ascontiguousarray(np.broadcast_to(np.asarray(case.occupancy, dtype=np.float64), (Z,)))
  e_price, e_carbon, g_price, g_carbon = case.prices
  o = ob.step(now_ts=now_ts, t_amb_now=t_now, h_conv=H_CONV, t_amb_next=t_next, comfort_now=bool(now),
              comfort_prev=prev == 1, comfort_next=bool(nxt), occupancy=occ, e_price=e_price, e_carbon=e_carbon,
              g_price=g_price, g_carbon=g_carbon, action=action, observe=True, reject=case.reject, round_action=False, **kw)
  return dict(
      zone_temp_pre=o["zone_temp_pre"], recirc_pre=o["recirc_pre"], t_now=t_now, t_next=t_next, t_sa=o["t_supply_air"],
      q_zone=o["q_zone"], damper=o["damper"], mode=o["mode"], valve=o["valve"], ahu_flow=o["ahu_flow"],
      ahu_count=o["ahu_count"], blr_flow=o["blr_flow"], blr_count=o["blr_count"], blr_return=o["blr_return_temp"],
      tank=o["blr_tank_temp"], tank_change=o["blr_tank_change"], duration=o["blr_last_duration"], heat_sp=o["ahu_heat_sp"],
      cool_sp=o["ahu_cool_sp"], blr_sp=o["blr_setpoint"], accepted=o["action_accepted"], zone_temp_post=o["zone_temp_post"],
      grid_mean=orc.np_mean(ob.temp), n_sweeps=int(o["n_sweeps"]), occupancy=occ, grid_finite=bool(np.isfinite(ob.temp).all()),
      oracle=dict(rates=np.array([o["blower_rate"], o["ac_rate"], o["gas_rate"], o["pump_rate"]], dtype=np.float32),
                  reward=np.float32(o["reward"]), reward_f64=o["reward_f64"],
                  diag=(o["productivity"], o["norm_prod_regret"], o["norm_energy_cost"], o["norm_carbon"])))


def expected(case: Case) -> dict:
  """The twin's step of the case (computed once): the pre half, the post half (`post`: post_chain's), and
  `grid_mean_arg`, what sb_tap_post is given for the grid's mean."""
  if case.twin is None:
    carry = None
    if case.prime is not None:
      carry = dict(damper=expected(case.prime)["damper"])
    e = _twin_step(case, carry)
    e["post"] = post_chain(case, e)
    e["grid_mean_arg"] = grid_mean_arg(e["grid_mean"], oracle_plan(SPECS[case.spec].rooms).n_cells)
    case.twin = e
  return case.twin


def excused(case: Case) -> bool:
  """Does any float32 output of k_post change when the results of exp (productivity) and log (the tank's dissipation)
  move by up to two double ulps -- both libraries' documented 1-ulp bound added together?"""
  e = expected(case)
  base = e["post"]
  for ke in (-2, -1, 0, 1, 2):
    for kl in (-2, -1, 0, 1, 2):
      if ke == 0 and kl == 0:
        continue
      alt = post_chain(case, e, ex=lambda x: nudge(math.exp(x), ke), lg=lambda x: nudge(math.log(x), kl))
      if alt["info"].tobytes() != base["info"].tobytes() or alt["reward"].tobytes() != base["reward"].tobytes():
        return True
  return False


# the info columns (and scalars) that descend from exp or log: gas, the productivity, costs and rewards computed from them
EXCUSABLE_INFO = (2, 7, 8, 10, 11, 12, 20, 21, 22, 23)
EXCUSABLE_SCAL = (14,)


# ---------------------------------------------------------------- the families
def _default_scal(name: str, b: int, rs) -> np.ndarray:
  p = params_row(name, b)
  s = np.zeros(16)
  s[0], s[1], s[4] = p["ahu_heat_sp"], p["ahu_cool_sp"], p["blr_setpoint"]
  s[8], s[9], s[10] = p["blr_setpoint"], 0.0, SPECS[name].dt
  s[12:16] = rs.uniform(0.0, 5e7, size=4)
  return s


class _Builder:
  def __init__(self):
    self.rs = np.random.RandomState(SEED)
    self.cases: List[Case] = []

  def quiet(self, family, label, name, b, **over) -> Case:
    """A case in which nothing sits on an edge: every zone inside the comfort window, no action."""
    p, Z = params_row(name, b), n_zones(SPECS[name])
    lo, hi = p["comfort_lo"], p["comfort_hi"]
    zt = lo + (hi - lo) * (0.55 + 0.3 * (np.arange(Z) % 5) / 5.0)
    c = Case(family, label, name, b, zone_temps=zt, modes=np.zeros(Z, np.int32), valves=np.zeros(Z),
             scal=_default_scal(name, b, self.rs))
    for k, v in over.items():
      setattr(c, k, v)
    return c

  def add(self, case: Case) -> Case:
    # the grid's mean must survive sb_tap_post's (mean * N) / N, and the stored scalar [11] is the twin's
    for wall in [case.wall + 0.0625 * k for k in range(16)]:
      case.wall = wall
      case.twin = None
      case.scal[11] = orc.np_mean(grid_of(case))
      if case.tie is not None:  # (a family that ties a setpoint to the grid's mean re-derives it for this wall)
        case.tie(case)
      if expected(case)["grid_mean_arg"] is not None:
        self.cases.append(case)
        return case
    raise AssertionError(f"{case.id}: no wall temperature gives a grid mean that sb_tap_post can be handed")

  def action(self, name: str, b: int, **cols) -> np.ndarray:
    """A normalised action row: random, the named columns (water, heat, cool, or an int zone) replaced."""
    spec = SPECS[name]
    names, zones, _ = action_set(spec)
    a = self.rs.uniform(-1.0, 1.0, size=len(names)).astype(np.float32)
    for k, v in cols.items():
      for i, (nm, z) in enumerate(zip(names, zones)):
        if (k == "water" and nm == WATER) or (k == "heat" and nm == HEAT) or (k == "cool" and nm == COOL):
          a[i] = v
    return a


def _damper_col(spec: Spec, zone: int) -> int:
  names, zones, _ = action_set(spec)
  return [i for i, (n, z) in enumerate(zip(names, zones)) if n == DAMPER and z == zone][0]


def _window(p: dict, comfort: int) -> Tuple[float, float]:
  return (p["comfort_lo"], p["comfort_hi"]) if comfort else (p["eco_lo"], p["eco_hi"])


def _thermostat(bd: _Builder):
  """tz on hsp, csp and mid (one below, on, one above, cycling over the zones) for each stored mode, under every
  (comfort_now, comfort_prev); the passive-cool exit is (0, 0 / -1) with stored mode 3 and tz on hsp."""
  combos = [(1, 1), (1, 0), (1, -1), (0, 1), (0, 0), (0, -1)]
  for name in ("z18-dampers-regret", "z2-pair-regret", "z18-pair-dollars"):
    Z = n_zones(SPECS[name])
    shifts = (0,) if Z == 18 else (0, 1, 2)
    for ci, (now, prev) in enumerate(combos):
      for ei, edge in enumerate(("hsp", "csp", "mid")):
        for m in range(4):
          for sh in shifts:
            b = TAPPED[(ci + ei + m + sh) % 6]
            p = params_row(name, b)
            hsp, csp = _window(p, now)
            x = dict(hsp=hsp, csp=csp, mid=0.5 * (csp - hsp) + hsp)[edge]
            zt = np.array([trio(x)[(z + sh) % 3] for z in range(Z)])
            modes = np.array([(z // 3 + m + sh) % 4 for z in range(Z)], np.int32)
            bd.add(bd.quiet("thermostat", f"{name}-b{b}-now{now}-prev{prev}-{edge}-m{m}-s{sh}", name, b, zone_temps=zt,
                            modes=modes, comfort=(now, prev, now), tags=("edge:" + edge,)))
  # a rejected building: modes, valves and dampers kept -- the dampers are those of the tap before it
  for name in ("z18-dampers-regret", "z2-dampers-dollars"):
    spec = SPECS[name]
    Z = n_zones(spec)
    for k, b in enumerate(TAPPED):
      p = params_row(name, b)
      act = bd.action(name, b)
      prime = bd.add(bd.quiet("thermostat", f"{name}-b{b}-prime", name, b, has_action=True, action=act,
                              zone_temps=np.array([trio(p["comfort_lo"])[z % 3] for z in range(Z)])))
      zt = np.array([trio(p["comfort_hi"])[z % 3] for z in range(Z)])
      modes = np.array([(z + k) % 4 for z in range(Z)], np.int32)
      bd.add(bd.quiet("thermostat", f"{name}-b{b}-rejected", name, b, zone_temps=zt, modes=modes,
                      valves=(np.arange(Z) + k) % 2.0, has_action=True, action=bd.action(name, b), reject=True,
                      prime=prime, tags=("rejected",)))


def _air_handler(bd: _Builder):
  """mixed on heat_sp and on cool_sp in k_pre; mixed2 (t_next != t_now) on them in k_post; an action that moves the
  heating or the cooling setpoint onto mixed (building 64 recirculates all its air: mixed is the grid's mean, and the
  whole grid holds the fp32 value the action carries)."""
  for name in ("z18-dampers-regret", "z2-pair-regret"):
    for b in TAPPED:
      p = params_row(name, b)
      r = p["ahu_recirc"]
      for which, slot in (("heat", 0), ("cool", 1)):
        for half in ("pre", "post"):
          for k in range(3):
            def tie(c, slot=slot, half=half, k=k, r=r):
              t = ambient_of(c.weather, c.b)[0 if half == "pre" else 1]
              c.scal[slot] = trio(r * c.scal[11] + (1 - r) * t)[k]
              # (the other setpoint far away, and the pair in the air handler's order)
              c.scal[1 - slot] = c.scal[slot] + (15.0 if slot == 0 else -15.0)
            bd.add(bd.quiet("air_handler", f"{name}-b{b}-{which}-{half}-{k}", name, b, weather=("scalar", 284.7, 279.9),
                            tags=(f"ahu:{which}:{half}",), tie=tie))
  name = "z18-dampers-regret"
  spec, b = SPECS[name], 64
  Z = n_zones(spec)
  for which in ("heat", "cool"):
    for j, k, native in [(j, k, n) for j in range(3) for k in range(3) for n in (False, True)]:
      a = bd.action(name, b)
      col = 1 if which == "heat" else 2
      lo, hi = action_set(spec)[2][col]
      target = f32(lo + 0.37 * (hi - lo) + 0.01 * k + 0.1 * j)
      if native:
        a = np.array([v if v is not None else KEEP for v in native_values(spec, a, False)], dtype=np.float32)
        a[col] = target
        a[3 + (k % Z)] = KEEP
      else:
        target = native_values(spec, a, False)[col]
      v = (dn32(target), target, up32(target))[k]       # the grid one fp32 below, on and above the setpoint
      other = {"heat": 1, "cool": 0}[which]
      sc = _default_scal(name, b, bd.rs)
      sc[other] = v + (15.0 if which == "heat" else -15.0)
      if native:
        a[2 if which == "heat" else 1] = KEEP             # the other setpoint stays where the state has it
      else:
        a[2 if which == "heat" else 1] = np.float32(1.0 if which == "heat" else -1.0)
      bd.add(bd.quiet("air_handler", f"{name}-b{b}-action-{which}-{j}{k}-{'native' if native else 'norm'}", name, b,
                      zone_temps=np.full(Z, v), wall=v, scal=sc, has_action=True, action=a, native=native,
                      tags=(f"ahu-action:{which}",)))


def _actions(bd: _Builder):
  """Normalised -1 and +1 (native 0 and 1 under the dampers' (0, 1)), native commands 0, -0.0, 1, one fp32 over 1 and
  one under 0, columns left out (SB_ACTION_KEEP), random normalised values (their native value is rounded to fp32)."""
  for name in ("z18-dampers-regret", "z2-dampers-dollars"):
    spec = SPECS[name]
    Z = n_zones(spec)
    for bi, b in enumerate(TAPPED):
      p = params_row(name, b)
      apart = np.array([(p["comfort_lo"] - 1.5) if z % 2 else (p["comfort_hi"] + 1.0) for z in range(Z)])   # HEAT / COOL
      for v in range(4):     # normalised: -1, +1 and random, cycling over the zones
        a = bd.action(name, b)
        for z in range(Z):
          pick = (z + v + bi) % 4
          if pick < 2:
            a[_damper_col(spec, z)] = np.float32(-1.0 if pick == 0 else 1.0)
        bd.add(bd.quiet("actions", f"{name}-b{b}-norm-{v}", name, b, zone_temps=apart,
                        has_action=True, action=a, tags=("damper:norm",)))
      accepted = [0.0, -0.0, 1.0, KEEP, f32(0.3), dn32(1.0), f32(2.0 ** -12)]
      for v in range(len(accepted)):
        a = np.array([x if x is not None else KEEP for x in native_values(spec, bd.action(name, b), False)], np.float32)
        for z in range(Z):
          a[_damper_col(spec, z)] = np.float32(accepted[(z + v + bi) % len(accepted)])
        if v % 2:
          a[1] = KEEP
        if v % 3 == 0:
          a[2] = KEEP
        bd.add(bd.quiet("actions", f"{name}-b{b}-native-{v}", name, b, zone_temps=apart, has_action=True, action=a,
                        native=True, tags=("damper:native",)))
      for v, bad in enumerate((up32(1.0), dn32(0.0), -0.25, 1.5)):   # outside [0, 1]: that action is rejected
        z = (0, 15, 16, 17)[(v + bi) % 4] % Z
        a = np.array([x if x is not None else KEEP for x in native_values(spec, bd.action(name, b), False)], np.float32)
        a[_damper_col(spec, z)] = np.float32(bad)
        bd.add(bd.quiet("actions", f"{name}-b{b}-outside-{v}", name, b, zone_temps=apart, has_action=True, action=a,
                        native=True, tags=("damper:outside",)))


def _demand(bd: _Builder):
  """The running air flow reaching ahu_max_flow exactly and one nextafter over it at zones 15, 16, 17 (the tapped
  buildings' rows, building_params); all valves shut (den = 0), one valve open, all open."""
  for name in ("z18-dampers-regret", "z2-pair-regret", "z18-pair-dollars"):
    Z = n_zones(SPECS[name])
    for b in TAPPED:
      p = params_row(name, b)
      cold, warm = p["comfort_lo"] - 2.0, p["comfort_hi"] + 2.0
      patterns = [("all-heat", np.full(Z, cold)), ("all-cool", np.full(Z, warm))]
      for k in sorted({0, Z - 3, Z - 2, Z - 1} & set(range(Z))):
        zt = np.full(Z, warm)
        zt[k] = cold - 0.25 * k
        patterns.append((f"heat-at-{k}", zt))
      zt = np.array([cold - 0.125 * z if z % 3 else warm + 0.125 * z for z in range(Z)])
      patterns.append(("mixed", zt))
      for label, zt in patterns:
        bd.add(bd.quiet("demand", f"{name}-b{b}-{label}", name, b, zone_temps=zt, tags=("demand",)))


def _boiler(bd: _Builder):
  """blr_sp equal to the tank; heating / cooling that lands exactly on the setpoint, one step short of it and one past
  it; a rate of 0 (buildings 63, 69); duration 0 and positive; requests (the action stamps the boiler: the duration is dt.  The age scal[19] is not
  among the scalars a tap writes: only a building's first tap after reset() goes none -> 1, and both branches give dt)."""
  for name in ("z18-pair-dollars", "z2-pair-regret"):
    dt = SPECS[name].dt
    for b in (TAPPED if name.startswith("z18") else (0, 63, 69)):
      p = params_row(name, b)
      for dur in (0.0, dt, 77.7):
        for direction in ("equal", "heat", "cool"):
          for k in range(3):
            sc = _default_scal(name, b, bd.rs)
            begin = sc[8] = p["blr_setpoint"] + (0.3 if direction == "cool" else -0.2)
            sc[9], sc[10] = 0.125, dur
            if direction == "equal":
              sc[4] = trio(begin)[k]
            elif direction == "heat":      # begin + rate * duration / 60 == the setpoint (or the setpoint one off it)
              sc[4] = trio(begin + p["blr_heating_rate"] * dur / 60.0)[k] if dur else up(begin, 1 + k)
            else:
              sc[4] = trio(begin - p["blr_cooling_rate"] * dur / 60.0)[k] if dur else dn(begin, 1 + k)
            bd.add(bd.quiet("boiler", f"{name}-b{b}-{direction}-d{dur:g}-{k}", name, b, scal=sc, tags=("boiler",)))
      for k in range(3):   # a request: the setpoint is the action's fp32 value, the duration dt
        a = bd.action(name, b)
        sp = native_values(SPECS[name], a, False)[0]
        for direction, begin in (("equal", sp), ("heat", sp - p["blr_heating_rate"] * dt / 60.0),
                                 ("cool", sp + p["blr_cooling_rate"] * dt / 60.0)):
          sc = _default_scal(name, b, bd.rs)
          sc[8], sc[9], sc[10] = trio(begin)[k], -0.5, 42.0
          bd.add(bd.quiet("boiler", f"{name}-b{b}-action-{direction}-{k}", name, b, scal=sc, has_action=True, action=a,
                          tags=("boiler", "request")))


def _reward(bd: _Builder):
  """The fp32 zone temperature on the fp32 setpoints (the windows are not fp32 numbers); occupancy all zero; cumulative
  below min_p; the caps (buildings 63, 69, 15); gas negative; both reward kinds."""
  for name in SPECS:
    Z = n_zones(SPECS[name])
    for b in (TAPPED if Z == 18 else (0, 15, 69)):
      p = params_row(name, b)
      for nxt in (1, 0):
        lo, hi = _window(p, nxt)
        for which, x in (("hsp2", lo), ("csp2", hi)):
          x32 = f32(x)
          # doubles that round to the setpoint's fp32 value, the fp32 neighbours, and the double setpoint's own neighbours
          pts = [x32, up(x32), dn(x32), dn32(x32), up32(x32), x, up(x), dn(x), x32 + (x32 - x), (x + x32) / 2.0]
          for sh in range(0, len(pts), 3 if Z == 18 else 2):
            zt = np.array([pts[(z + sh) % len(pts)] for z in range(Z)])
            occ = np.array([1.0 + 0.7 * ((z * 7 + sh) % 5) for z in range(Z)])
            # (the thermostat runs on the comfort window at t, far from these temperatures' last bits or not: either way)
            bd.add(bd.quiet("reward", f"{name}-b{b}-next{nxt}-{which}-{sh}", name, b, zone_temps=zt, occupancy=occ,
                            comfort=(1, 1, nxt), tags=("reward:" + which,)))
      lo, hi = p["comfort_lo"], p["comfort_hi"]
      freezing = np.array([lo - 6.0 - 0.5 * z for z in range(Z)])
      bd.add(bd.quiet("reward", f"{name}-b{b}-empty", name, b, occupancy=0.0, tags=("reward:empty",)))
      bd.add(bd.quiet("reward", f"{name}-b{b}-empty-cold", name, b, occupancy=np.zeros(Z), zone_temps=freezing,
                      tags=("reward:empty",)))
      bd.add(bd.quiet("reward", f"{name}-b{b}-below-min", name, b, zone_temps=freezing, occupancy=3.3,
                      tags=("reward:below-min",)))
      bd.add(bd.quiet("reward", f"{name}-b{b}-hot", name, b, zone_temps=np.array([hi + 0.3 + 0.2 * z for z in range(Z)]),
                      occupancy=np.array([0.1 + 1.3 * (z % 4) for z in range(Z)]), tags=("reward:hot",)))
      # gas: the outside warmer than the water (negative dissipation, no reheat flow), a heated tank, reheat flowing
      bd.add(bd.quiet("reward", f"{name}-b{b}-gas-negative", name, b, weather=("scalar", 283.0, 391.5),
                      tags=("reward:gas",)))
      sc = _default_scal(name, b, bd.rs)
      sc[8], sc[10] = sc[4] - 40.0, 600.0
      bd.add(bd.quiet("reward", f"{name}-b{b}-gas-tank", name, b, scal=sc, zone_temps=freezing, tags=("reward:gas",)))
      sc = _default_scal(name, b, bd.rs)
      sc[8], sc[10] = sc[4] + 25.0, 45.0
      bd.add(bd.quiet("reward", f"{name}-b{b}-gas-tank-cooling", name, b, scal=sc, tags=("reward:gas",)))
  _caps(bd)


def _caps(bd: _Builder):
  """The electricity rate ON max_electricity_rate (building 16) and the gas rate ON max_natural_gas_rate (64): the state
  building_params took the caps from, under occupancies and prices of its own (neither moves a rate)."""
  for name in SPECS:
    for b in (ELEC_CAP_BUILDING, GAS_CAP_BUILDING):
      for k, occ in enumerate((2.5, 0.0, 7.3, 11.9)):
        prices = tuple(float(v) * (1.0 + 0.37 * k) for v in (3.1e-8, 1.3e-7, 9.7e-9, 4.9e-8))
        bd.add(cap_case(name, b, params_row(name, b), f"{name}-b{b}-on-cap-{k}", occupancy=occ, prices=prices))


def _ambient(bd: _Builder):
  """ambient_temp's three device forms through bld.t_now / t_next: a replay trace of 2 and of 37 knots asked below the
  first knot, above the last, on the first, an interior and the last knot and between knots, with and without the
  per-building offset; the sinusoid's f * (hi - lo) + lo; the per-building pair."""
  for name in ("z18-dampers-regret", "z2-pair-regret"):
    for bi, b in enumerate(TAPPED if name.startswith("z18") else (0, 69)):
      off = float(TRACES["offsets"][0][b])
      for trace in ("trace2", "trace37"):
        times = TRACES[trace][0]
        n = len(times)
        knots = [0, n - 1] + ([n // 2, 1] if n > 2 else [])
        for shifted in (False, True):
          o = off if shifted else 0.0
          qs = [times[0] - 100.0 - o, times[-1] + 50.0 - o] + [float(times[k]) - o for k in knots]
          qs += [dn(float(times[k])) - o for k in knots] + [up(float(times[k])) - o for k in knots]
          qs += [float(times[0] + 0.37 * (times[-1] - times[0])) - o]
          for k in range(0, len(qs) - 1, 2 if shifted else 1):
            bd.add(bd.quiet("ambient", f"{name}-b{b}-{trace}-{'off' if shifted else 'raw'}-{k}", name, b,
                            weather=("replay", trace, qs[k], qs[(k + 1 + bi) % len(qs)], shifted), tags=("ambient:replay",)))
      for k, f in enumerate((0.0, 1.0, 0.5, 1.0 / 3.0, 0.7071067811865476, 0.1, 0.9999999999999999, 0.3, 0.123456789,
                            0.987654321, 2.0 / 3.0, 0.2, 0.8535533905932737)):
        bd.add(bd.quiet("ambient", f"{name}-b{b}-sinusoid-{k}", name, b, weather=("sinusoid", f, 1.0 - f * 0.5),
                        tags=("ambient:sinusoid",)))
      bd.add(bd.quiet("ambient", f"{name}-b{b}-tamb", name, b, weather=("tamb",), tags=("ambient:tamb",)))


def _random(bd: _Builder):
  """States drawn over the whole range: summer and winter, occupied and empty, with and without a request, two sweeps
  of the twin's own between the halves (the post means and the grid's mean then differ from the pre ones)."""
  rs = bd.rs
  names = list(SPECS)
  for i in range(240):
    name = names[i % len(names)]
    spec = SPECS[name]
    Z, b = n_zones(spec), TAPPED[(i // len(names)) % 6]
    p = params_row(name, b)
    summer = bool(i % 2)
    zt = rs.uniform(p["eco_lo"] - 4.0, p["eco_hi"] + 4.0, size=Z) + (2.0 if summer else -2.0)
    sc = _default_scal(name, b, rs)
    sc[0] = p["ahu_heat_sp"] + rs.uniform(-3, 3)
    sc[1] = sc[0] + rs.uniform(5.0, 15.0)
    sc[4] = p["blr_setpoint"] + rs.uniform(-20, 20)
    sc[8], sc[9], sc[10] = sc[4] + rs.uniform(-3, 3), rs.uniform(-1, 1), float(rs.choice([0.0, spec.dt, 2 * spec.dt, 91.3]))
    has_action = bool(rs.rand() < 0.6)
    native = bool(has_action and rs.rand() < 0.4)
    a = None
    if has_action:
      a = bd.action(name, b)
      if native:
        a = np.array([x for x in native_values(spec, a, False)], np.float32)
        keep = rs.rand(len(a)) < 0.25
        keep[0] = False
        a[keep] = KEEP
    occ = 0.0 if i % 7 == 0 else (rs.uniform(0.0, 12.0, size=Z) if i % 3 else float(rs.uniform(0.0, 12.0)))
    comfort = (int(rs.rand() < 0.6), int(rs.randint(-1, 2)), int(rs.rand() < 0.6))
    amb = rs.uniform(295.0, 312.0) if summer else rs.uniform(255.0, 285.0)
    bd.add(bd.quiet("random", f"{name}-b{b}-{i}", name, b, zone_temps=zt, modes=rs.randint(0, 4, size=Z).astype(np.int32),
                    scal=sc, has_action=has_action, action=a, native=native, occupancy=occ, comfort=comfort,
                    weather=("scalar", amb, amb + rs.uniform(-0.5, 0.5)), sweeps=2, wall=float(rs.uniform(286.0, 300.0)),
                    prices=tuple(float(v) for v in rs.uniform(1e-9, 3e-7, size=4)), tags=("random",)))


FAMILIES = (("thermostat", _thermostat), ("air_handler", _air_handler), ("actions", _actions), ("demand", _demand),
            ("boiler", _boiler), ("reward", _reward), ("ambient", _ambient), ("random", _random))
_CASES: Optional[List[Case]] = None


def cases() -> List[Case]:
  """Every case, in a fixed order (deterministic: one seeded generator), with its twin's step computed."""
  global _CASES
  if _CASES is None:
    bd = _Builder()
    for _, fn in FAMILIES:
      fn(bd)
    _CASES = bd.cases
  return _CASES


def family(name: str) -> List[Case]:
  return [c for c in cases() if c.family == name]


_EXCUSED: Optional[frozenset] = None


def excused_ids() -> frozenset:
  global _EXCUSED
  if _EXCUSED is None:
    _EXCUSED = frozenset(c.id for c in cases() if excused(c))
  return _EXCUSED


# ---------------------------------------------------------------- which side of which edge the cases take
def _side(x: float, edge: float) -> Optional[str]:
  """below / on / above for an operand within one nextafter of the edge, else None."""
  return "on" if x == edge else "below" if x == dn(edge) else "above" if x == up(edge) else None


def census() -> Dict[str, int]:
  """Counts, from the twins' outputs, of the cases (or zones of cases) on each side of every edge."""
  n: Dict[str, int] = collections.Counter()
  for c in cases():
    spec, e, p = SPECS[c.spec], expected(c), params_row(c.spec, c.b)
    Z = n_zones(spec)
    now, prev, nxt = c.comfort
    n[f"family:{c.family}"] += 1
    n[f"building:{c.b}"] += 1
    n[f"handle:{c.spec}"] += 1
    # ---- thermostat (thermostat.py:76-148)
    if c.reject:
      n["rejected"] += 1
      n["rejected:modes-kept"] += int(np.array_equal(e["mode"], c.modes))
    else:
      n[f"comfort:now{now}:prev{prev}"] += 1
      hsp, csp = _window(p, now)
      mid = 0.5 * (csp - hsp) + hsp
      for z in range(Z):
        tz, m0, m1 = float(e["zone_temp_pre"][z]), int(c.modes[z]), int(e["mode"][z])
        n[f"mode:{m0}->{m1}"] += 1
        eco_hold = not now and prev != 1 and m0 == 3
        for name, edge in (("hsp", hsp), ("csp", csp), ("mid", mid)):
          s = _side(tz, edge)
          if s and not (not now and prev == 1):
            n[f"tz:{name}:{s}"] += 1
            if name == "mid" and m0 in (1, 2):
              n[f"tz:mid:mode{m0}:{s}"] += 1
            if name == "hsp" and eco_hold:
              n[f"passive-cool:{s}:->{m1}"] += 1
    # ---- air handler (air_handler.py:204-233), both halves
    r = p["ahu_recirc"]
    for half, mixed in (("pre", r * e["recirc_pre"] + (1 - r) * e["t_now"]), ("post", r * e["grid_mean"] + (1 - r) * e["t_next"])):
      for name, sp in (("heat_sp", e["heat_sp"]), ("cool_sp", e["cool_sp"])):
        s = _side(mixed, sp)
        if s:
          n[f"mixed:{half}:{name}:{s}"] += 1
        if c.has_action and half == "pre" and sp != c.scal[0 if name == "heat_sp" else 1]:
          s32 = "on" if mixed == sp else "below" if mixed == dn32(sp) else "above" if mixed == up32(sp) else None
          if s32:   # (the action's value is an fp32 number, and so is the grid it meets)
            n[f"mixed:action-moved:{name}:{s32}"] += 1
    n["t_next!=t_now"] += int(e["t_next"] != e["t_now"])
    # ---- actions (bounded_action_normalizer.py:73-98, vav.py:125-129)
    if c.has_action and not c.reject:
      n["action:native" if c.native else "action:normalised"] += 1
      names, zones, ranges = action_set(spec)
      vals = native_values(spec, c.action, c.native)
      for a, nm, v, (lo, hi) in zip(c.action, names, vals, ranges):
        if v is None:
          n[f"action:keep:{nm == DAMPER and 'damper' or 'setpoint'}"] += 1
          continue
        if not c.native and (float(np.float32(a)) + 1.0) / 2.0 * (hi - lo) + lo != v:
          n["action:fp32-rounding-moves-the-native-value"] += 1
        if nm != DAMPER:
          continue
        if not c.native and float(a) in (-1.0, 1.0):
          n[f"damper:normalised:{float(a):+g}"] += 1
        key = ("-0" if math.copysign(1.0, v) < 0 else "+0") if v == 0.0 else "1" if v == 1.0 else \
              "over-1-by-one-fp32" if v == up32(1.0) else "under-0-by-one-fp32" if v == dn32(0.0) else \
              "under-1-by-one-fp32" if v == dn32(1.0) else \
              "outside" if (v < 0.0 or v > 1.0) else "inside"
        n[f"damper:{key}"] += 1
      n["action:accepted" if e["accepted"] else "action:not-accepted"] += 1
    # ---- demand sums (air_handler.py:254-268, boiler.py:219-231, simulator.py:373-381)
    flow, bound, reached = 0.0, None, None
    for z in range(Z):
      air = float(e["damper"][z]) * p["vav_max_air_flow"]
      if air > 0:
        flow += air
        if flow > p["ahu_max_flow"]:
          flow = p["ahu_max_flow"]
          bound = z if bound is None else bound
        elif flow == p["ahu_max_flow"] and reached is None:
          reached = z
    assert flow == e["ahu_flow"]
    if bound is not None:
      n["clamp:binds:first-pass" if bound < 16 else "clamp:binds:second-pass"] += 1
      n[f"clamp:binds:zone{bound}"] += 1
    else:
      n["clamp:free"] += 1
    if reached is not None and (bound is None or reached < bound):
      n["clamp:reached-exactly"] += 1
    den = float(np.sum(e["valve"]))
    n["valves:none" if den == 0 else "valves:one" if den == 1 else "valves:all" if den == Z else "valves:some"] += 1
    n["air:zero-flow-zone"] += int(np.any(e["damper"] == 0.0))
    # ---- boiler (boiler.py:158-217)
    sp, begin, dur = e["blr_sp"], float(c.scal[8]), e["duration"]
    hr, cr = p["blr_heating_rate"], p["blr_cooling_rate"]
    n["duration:zero" if dur == 0 else "duration:positive"] += 1
    if not (hr > 0.0 and cr > 0.0):
      n["tank:a-rate-is-zero"] += 1
    elif sp == begin:
      n["tank:equal"] += 1
    elif sp > begin:
      step = begin + hr * dur / 60.0
      n["tank:heats:" + ("lands-on-setpoint" if step == sp else "capped" if step > sp else "short")] += 1
      n["tank:blr_sp-above-by-one"] += int(sp == up(begin))
    else:
      step = begin - cr * dur / 60.0
      n["tank:cools:" + ("lands-on-setpoint" if step == sp else "capped" if step < sp else "short")] += 1
      n["tank:blr_sp-below-by-one"] += int(sp == dn(begin))
    # ---- reward (base_setpoint_energy_carbon_reward.py:52-172, setpoint_energy_carbon_regret.py:142-291)
    win = "comfort" if nxt else "eco"
    for name, x in (("hsp2", p[win + "_lo"]), ("csp2", p[win + "_hi"])):
      x32 = f32(x)
      n[f"{name}:not-an-fp32-number"] += int(x32 != x)
      for z in range(Z):
        t = float(e["zone_temp_post"][z])
        t32 = f32(t)
        s = "on" if t32 == x32 else "below" if t32 == dn32(x32) else "above" if t32 == up32(x32) else None
        if s:
          n[f"t32:{name}:{s}"] += 1
          # the roundings decide: the doubles compare otherwise than the fp32 values do
          n[f"t32:{name}:rounding-decides"] += int((t < x) != (t32 < x32) or (t > x) != (t32 > x32) or
                                                   (t < x32) != (t32 < x32) or (t > x32) != (t32 > x32) or
                                                   (t32 < x) != (t32 < x32) or (t32 > x) != (t32 > x32))
    occ32 = [f32(o) for o in e["occupancy"]]
    n["occupancy:rounds"] += int(any(o != float(v) for o, v in zip(occ32, e["occupancy"])))
    cum, total = productivity(p, f32(p[win + "_lo"]), f32(p[win + "_hi"]), [f32(t) for t in e["zone_temp_post"]], occ32, spec.dt)
    n["total_occ:zero" if total == 0.0 else "total_occ:positive"] += 1
    blower, ac, gas, pump = (float(v) for v in e["post"]["info"][:4])
    if not spec.dollars:
      if total > 0.0:
        n["cumulative:below-min_p" if cum < p["min_prod"] * total * spec.dt / 3600.0 else "cumulative:above-min_p"] += 1
      elec = (blower + abs(ac)) + pump
      n["elec:over-max" if elec > p["max_elec"] else "elec:on-max" if elec == p["max_elec"] else "elec:under-max"] += 1
      n["gas:negative" if gas < 0 else "gas:over-max" if gas > p["max_gas"] else "gas:on-max" if gas == p["max_gas"]
        else "gas:inside"] += 1
    else:
      n["dollars:gas-negative" if gas < 0 else "dollars:gas-positive"] += 1
      n["dollars:ac-negative" if ac < 0 else "dollars:ac-not-negative"] += 1
    n["tank_rate:duration-zero" if dur == 0 else "tank_rate:duration-positive"] += 1
    # ---- ambient (weather_controller.py:93-123, :166-218)
    kind = c.weather[0]
    if kind == "replay":
      _, trace, x_now, x_next, shifted = c.weather
      times = TRACES[trace][0]
      off = float(TRACES["offsets"][0][c.b]) if shifted else 0.0
      for x in (x_now + off, x_next + off):
        where = ("below-first" if x < times[0] else "above-last" if x > times[-1] else "on-first" if x == times[0] else
                 "on-last" if x == times[-1] else "on-interior" if x in times else "between")
        n[f"replay:{trace}:{where}"] += 1
      n["replay:offset" if shifted else "replay:no-offset"] += 1
    elif kind == "sinusoid":
      lo, hi = (float(v) for v in TRACES["lohi"][0][c.b])
      for f in c.weather[1:3]:
        F = fractions.Fraction
        fused = float(F(float(f)) * F(hi - lo) + F(lo))
        n["sinusoid:fma-would-differ" if fused != float(f) * (hi - lo) + lo else "sinusoid:fma-would-agree"] += 1
    elif kind == "tamb":
      n["tamb:per-building"] += 1
  return dict(n)
