"""The oracle side of the parity harness: one building of a batch as a CPU-oracle twin, the inputs of its step, and the
bars a device step is held to against it.  numpy, the oracle and the library's host-only modules: no torch, so the CPU
suite and the case tables import it.  tests/parity.py holds the device side.

The bars: Gauss-Seidel sweep counts and converged flags EQUAL; zone temperatures within T_TOL (the kernels compute in
float64 with reassociated sums, reciprocal multiplies and fma: 1e-8 K is the observed bound, 1e-4 K the contract);
the float32 energy rates at RATE_RTOL / RATE_ATOL; the float32 reward within REWARD_TOL."""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from oracle import oracle as orc
from sbsim_amd import _ffi
from sbsim_amd.floorplan import FloorPlan

T_TOL = 1e-8         # K
RATE_RTOL = 2e-6
RATE_ATOL = 1e-6     # W
REWARD_TOL = 2e-6


def plan_from_npz(p) -> FloorPlan:
  """The FloorPlan of a tests/golden/plan_*.npz file (or of a dict of its arrays)."""
  return FloorPlan(conductivity=p["conductivity"], heat_capacity=p["heat_capacity"], density=p["density"],
                   exterior_space=p["exterior_space"], zone_label=p["zone_label"], diffusers=p["diffusers"],
                   cv_size_cm=float(p["cv_size_cm"]), floor_height_cm=float(p["floor_height_cm"]),
                   zone_names=tuple(str(z) for z in p["zone_names"]) if "zone_names" in p else ())


def ringless_plan(g) -> FloorPlan:
  """The deprecated rectangular Building of tests/golden/rect_building_cold200.npz (building.py:394-605): no ring of
  exterior space, every in-bounds cell keeps its neighbours, rooms labelled as building.py:167-180 lays them out."""
  H, W = g["conductivity"].shape
  rs, bs = g["room_shape"], g["building_shape"]
  label = np.full((H, W), -1, dtype=np.int64)
  for zx in range(bs[0]):
    for zy in range(bs[1]):
      x0, y0 = zx * (rs[0] + 1) + 2, zy * (rs[1] + 1) + 2
      label[x0:x0 + rs[0], y0:y0 + rs[1]] = zx * bs[1] + zy
  return FloorPlan(conductivity=g["conductivity"], heat_capacity=g["heat_capacity"], density=g["density"],
                   exterior_space=np.zeros((H, W), bool), zone_label=label, diffusers=g["diffusers"],
                   cv_size_cm=float(g["cv_size_cm"]), floor_height_cm=float(g["floor_height_cm"]),
                   skip_exterior_neighbors=False)


def oracle_plan_of(fp, **kw) -> orc.OraclePlan:
  """FloorPlan -> OraclePlan: the oracle reads k, rho, c, the exterior mask, the zones and the diffusers, never the
  class tables of FloorPlan.compile()."""
  return orc.OraclePlan(fp.conductivity, fp.density, fp.heat_capacity, fp.exterior_space, fp.zone_cell_lists(),
                        fp.diffusers, fp.cv_size_cm, fp.floor_height_cm, **kw)


def oracle_params_of(cfg, **over) -> orc.OracleParams:
  """SimConfig (any object with its fields) -> OracleParams."""
  c = cfg
  d = dict(
      dt=c.time_step_sec, conv_threshold=c.convergence_threshold, iter_limit=c.iteration_limit,
      vav_max_air_flow=c.vav_max_air_flow_rate, vav_max_water_flow=c.vav_reheat_max_water_flow_rate,
      ahu_recirc=c.ahu_recirculation, ahu_heat_sp=c.ahu_heating_air_temp_setpoint,
      ahu_cool_sp=c.ahu_cooling_air_temp_setpoint, ahu_dp=c.ahu_fan_differential_pressure,
      ahu_eff=c.ahu_fan_efficiency, ahu_max_flow=c.ahu_max_air_flow_rate, blr_setpoint=c.boiler_reheat_water_setpoint,
      blr_head=c.boiler_water_pump_differential_head, blr_pump_eff=c.boiler_water_pump_efficiency,
      comfort_lo=c.comfort_temp_window[0], comfort_hi=c.comfort_temp_window[1],
      eco_lo=c.eco_temp_window[0], eco_hi=c.eco_temp_window[1],
      blr_heating_rate=c.boiler_heating_rate, blr_cooling_rate=c.boiler_cooling_rate, ahu_has_weather=1)
  d.update(over)
  return orc.OracleParams(**d)


def oracle_twin(fp, cfg, init_flat) -> orc.OracleBuilding:
  """The CPU oracle of one building of a BatchedSimulator(fp, cfg) reset to ``init_flat``."""
  return orc.OracleBuilding(oracle_plan_of(fp), oracle_params_of(cfg), 0.0, reset_temps=init_flat)


def copy_twin(dst, src):
  """dst becomes src: the grid, the per-zone state and the scalars of the oracle's state."""
  for k in ("temp", "input_q", "mode", "damper", "valve", "zone_air_temp"):
    getattr(dst, k)[:] = getattr(src, k)
  for name, ctype in orc._State._fields_:
    if not hasattr(ctype, "contents"):   # the scalars, not the array pointers
      setattr(dst.state, name, getattr(src.state, name))


def native_value(a, lo, hi) -> np.float32:
  """A normalised action as the native setpoint (bounded_action_normalizer.py:73-98), then the proto's float field."""
  return np.float32((float(a) + 1.0) / 2.0 * (hi - lo) + lo)


def native_action(cfg, a) -> List[np.float32]:
  return [native_value(x, lo, hi) for x, (lo, hi) in zip(a, cfg.action_ranges)]


def step_kwargs(g, tt: int, t: int, cfg, a, h_conv=None, step_sec: float = 300.0, observe: bool = True) -> dict:
  """OracleBuilding.step's arguments at step t of a run that feeds the device row tt of the golden's step inputs `g`
  (what step_in(g, tt) gives sb_step); `a` the building's normalised action; `h_conv` and `step_sec` replace the rows'
  convection coefficient and the 300 s between two steps."""
  return dict(now_ts=step_sec * t, t_amb_now=float(g["t_amb_now"][tt]),
              h_conv=float(g["h_conv"]) if h_conv is None else float(h_conv),
              t_amb_next=float(g["t_amb_next"][tt]), comfort_now=bool(g["comfort_now"][tt]),
              comfort_prev=g["comfort_prev"][tt] == 1, comfort_next=bool(g["comfort_next"][tt]),
              occupancy=float(g["occupancy"][tt]), e_price=float(g["e_price"][tt]), e_carbon=float(g["e_carbon"][tt]),
              g_price=float(g["g_price"][tt]), g_carbon=float(g["g_carbon"][tt]), action=native_action(cfg, a),
              observe=observe)


def step_in(g, t: int, has_action: bool = True, occupancy=None) -> _ffi.StepIn:
  """sb_step's inputs from row t of a golden's step inputs."""
  si = _ffi.StepIn()
  si.t_amb_now, si.t_amb_next = float(g["t_amb_now"][t]), float(g["t_amb_next"][t])
  si.comfort_now, si.comfort_prev, si.comfort_next = (int(g["comfort_now"][t]), int(g["comfort_prev"][t]),
                                                      int(g["comfort_next"][t]))
  si.has_action = int(has_action)
  si.occupancy = float(g["occupancy"][t]) if occupancy is None else occupancy
  si.e_price, si.e_carbon = float(g["e_price"][t]), float(g["e_carbon"][t])
  si.g_price, si.g_carbon = float(g["g_price"][t]), float(g["g_carbon"][t])
  return si


def oracle_rates(o) -> np.ndarray:
  """The four energy rates of an OracleBuilding.step result in the order of the device's info row."""
  return np.array([o["blower_rate"], o["ac_rate"], o["gas_rate"], o["pump_rate"]], np.float64)


def rates_match(got, ref) -> bool:
  return bool(np.allclose(got, ref, rtol=RATE_RTOL, atol=RATE_ATOL))


def assert_step_matches(info_row, zone_temps, reward, o, where):
  """One building's device step (its info row, zone temperatures and reward) against its twin's result `o` of
  OracleBuilding.step, at the bars of this module.  `where` names the step and the building in the messages."""
  n, conv = float(info_row[4]), float(info_row[5])
  assert n == o["n_sweeps"], f"{where}: {n:g} sweeps on the device, {o['n_sweeps']} on the oracle"
  assert conv == o["converged"], f"{where}: converged {conv:g} on the device, {o['converged']} on the oracle"
  dz = float(np.abs(np.asarray(zone_temps, np.float64) - o["zone_temp_post"]).max())
  assert dz < T_TOL, f"{where}: zone temperatures differ by {dz:.3e} K (bar {T_TOL:g})"
  got, ref = np.asarray(info_row[:4], np.float64), oracle_rates(o)
  assert rates_match(got, ref), f"{where}: rates {got} on the device, {ref} on the oracle"
  dr = abs(float(reward) - o["reward"])
  assert dr < REWARD_TOL, f"{where}: reward {float(reward)!r} on the device, {o['reward']!r} on the oracle"


def plan_info(fp, n_obs: int = 46, n_buildings: int = 1024):
  """sb_plan_info (host only): (return code, the launch geometry the planner gives the plan)."""
  cp = fp.compile(300.0, 12.0)
  keep = [np.ascontiguousarray(x) for x in (cp.cell_class, cp.class_coef, cp.class_zone, cp.zone_off, cp.zone_cells)]
  desc = _ffi.PlanDesc(cp.H, cp.W, cp.Z, cp.n_classes, keep[0].ctypes.data_as(C.POINTER(C.c_uint8)),
                       keep[1].ctypes.data_as(_ffi._dp), keep[2].ctypes.data_as(_ffi._ip),
                       keep[3].ctypes.data_as(_ffi._ip), keep[4].ctypes.data_as(_ffi._ip))
  info = _ffi.LaunchInfo()
  rc = _ffi.load().sb_plan_info(C.byref(desc), n_obs, n_buildings, C.byref(info))
  return rc, {f[0]: getattr(info, f[0]) for f in _ffi.LaunchInfo._fields_}
