"""Shared cases of the episode-randomisation tests (host_inputs.EpisodeRandomization, sb_randomization_attach): the plans,
the randomisations, and the tables a handle must hold after a given history of resets, restated in NumPy from
``EpisodeRandomization.values``.  No device needed.

The small two-room plan is ``rectangular_floor_plan((1, 2), (1, 1))``: the smallest two-room plan the generator makes,
7 x 9 cells with its exterior ring and walls (5 x 7 inside the ring) -- a few hundred bytes of state per building."""
import datetime as dt

import numpy as np

from sbsim_amd import _ffi
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
from sbsim_amd.host_inputs import (BUILDING_PARAM_NAMES, BuildingMaterials, BuildingParams, Choice, EpisodeRandomization,
                                   Uniform, effective_building_materials, effective_building_params)
from tests.golden_util import load
from tests.twins import plan_from_npz

KINDS = ("conductivity", "heat_capacity", "density")
PARAM_INDEX = {name: k for k, name in enumerate(_ffi.BUILDING_PARAM_FIELDS)}
START = dt.datetime(2023, 7, 6, 7, 0, 0)
H_CONV = 100.0   # BatchedEnvironment's default weather controller


def plan_small():
  return plan_from_npz(load("plan_small_test.npz"))


def plan_two_rooms():
  return FloorPlan.from_file_input(rectangular_floor_plan((1, 2), (1, 1)), Materials.sb1(), 10.0, 300.0)


def config():
  from sbsim_amd.environment import SimConfig   # (imports torch: this module must load without it)
  return SimConfig.sb1()


def building_params(B):
  """Rows that a reset must read per building (the AHU and boiler setpoints it restores) and one the steps read."""
  return BuildingParams(ahu_heating_air_temp_setpoint=np.linspace(283.0, 288.0, B),
                        boiler_reheat_water_setpoint=np.linspace(330.0, 360.0, B),
                        vav_max_air_flow_rate=np.linspace(0.03, 0.045, B))


def building_materials(plan, B):
  table = plan.material_slots()[1]
  sets = np.stack([table * (np.array([0.5, 2.0, 1.5]) if i % 2 == 0 else np.array([2.0, 0.5, 0.75])) for i in range(B)])
  return BuildingMaterials(conductivity=sets[:, :, 0], heat_capacity=sets[:, :, 1], density=sets[:, :, 2],
                           convection_coefficient=np.linspace(8.0, 60.0, B))


def param_fields():
  """Uniform, Choice and scale fields, among them the three a reset kernel reads from the building's row."""
  return {"ahu_fan_efficiency": Uniform(0.7, 0.95),
          "vav_max_air_flow_rate": Uniform(0.8, 1.2, scale=True),
          "comfort_temp_window": Uniform((293.0, 296.5), (295.0, 299.0)),
          "ahu_heating_air_temp_setpoint": Uniform(0.995, 1.005, scale=True),
          "ahu_cooling_air_temp_setpoint": Choice([297.0, 298.0, 299.5]),
          "boiler_reheat_water_setpoint": Choice([330.0, 340.0, 350.0, 360.0]),
          "energy_cost_weight": Uniform(0.5, 2.0, scale=True)}


def material_fields():
  return {"conductivity": {0: Choice([0.5, 1.0, 2.0, 4.0], scale=True)},
          "heat_capacity": {1: Uniform(0.8, 1.25, scale=True)},
          "density": {0: Uniform(0.9, 1.1, scale=True)},
          "convection_coefficient": Uniform(6.0, 25.0)}


def randomization(materials: bool, seed=7, first_building=0):
  return EpisodeRandomization(params=param_fields(), materials=material_fields() if materials else None, seed=seed,
                              first_building=first_building)


def every_field(n_slots):
  """Every parameter field and every material field of a plan of n_slots slots at once: each within 0.1 % of its base
  row (the setpoint pairs and windows of the SimConfig stay ordered at their worst)."""
  u = lambda: Uniform(0.999, 1.001, scale=True)
  params = {name: (u() if len(c) == 1 else (u(), u())) for name, c in BUILDING_PARAM_NAMES.items()}
  mats = {kind: {s: u() for s in range(n_slots)} for kind in KINDS}
  mats["convection_coefficient"] = u()
  return params, mats


def base_rows(B, bp=None, bm=None, plan=None, cfg=None, h_conv=H_CONV):
  """The rows in force without a randomisation, by name (what ``values`` takes as ``base``); the materials only with a plan."""
  base = effective_building_params(bp, cfg or config(), B)
  if plan is not None:
    base.update(effective_building_materials(bm, plan.material_slots()[1], h_conv, B))
  return base


def param_table(rows):
  """{SimConfig field: [B] or [B, 2]} as the device's [SB_NUM_BUILDING_PARAMS][B]."""
  B = len(next(iter(rows.values())))
  tab = np.zeros((_ffi.SB_NUM_BUILDING_PARAMS, B))
  for name, c_names in BUILDING_PARAM_NAMES.items():
    a = np.asarray(rows[name], dtype=np.float64)
    for j, c in enumerate(c_names):
      tab[PARAM_INDEX[c]] = a if a.ndim == 1 else a[:, j]
  return tab


def material_table(rows):
  """{kind: [B, M], convection_coefficient: [B]} as the device's [3 M + 1][B]."""
  M = rows["conductivity"].shape[1]
  return np.concatenate([np.asarray(rows[k], dtype=np.float64).T for k in KINDS] + [np.asarray(rows["convection_coefficient"])[None]]).reshape(3 * M + 1, -1)


def rows_in_force(er, base, episodes, buildings=None):
  """The rows by name after the given history: building b holds ``values(b, episodes[b], base)``, its base row where
  episodes[b] < 0 (never drawn).  ``buildings``: only these rows are computed (the others stay at their base)."""
  out = {k: np.array(v, dtype=np.float64) for k, v in base.items()}
  for b in (range(len(episodes)) if buildings is None else buildings):
    if episodes[b] < 0:
      continue
    for name, v in er.values(b, int(episodes[b]), base).items():
      out[name][b] = v
  return out


def split(rows):
  """(parameters, materials or None) of a by-name dict, as BuildingParams / BuildingMaterials arguments."""
  params = {k: v for k, v in rows.items() if k in BUILDING_PARAM_NAMES}
  mats = {k: v for k, v in rows.items() if k not in BUILDING_PARAM_NAMES}
  return params, (mats or None)


def same_bits(a, b):
  a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
  return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
