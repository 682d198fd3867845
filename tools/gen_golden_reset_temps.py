"""Generates tests/golden/reset_temp_values.npz from the reference's own ``FloorPlanBasedBuilding(reset_temp_values=grid)``
(simulator/building.py:650,680,784-792) under SimulatorFlexibleGeometries.  Run it where the reference tree exists
(``python tools/gen_golden_reset_temps.py``); tests never run it and never read the reference.

The building: the reference tests' small floor plan (23 x 12, two rooms) with SB1's materials and plant (oracle/gen_golden.py's
SB1 table, as its H2 fixtures), constructed with a seeded, smooth start grid as ``reset_temp_values``.  The run: oracle/gen_golden.py's
H2 harness (SimulatorBuilding.request_action -> wait_time -> request_observations -> reward_info) for 12 steps, then
SimulatorBuilding.reset() -- which copies the grid back -- and the same 12 actions again, on ONE simulator, as
oracle/gen_golden_episodes.py runs its pair.  Recorded per step and episode (prefixes e1_, e2_): everything the H2 harness
records -- zone temperatures, sweep counts, the four energy rates among it -- and the full grid after step 1; besides: the
start grid, the floor-plan arrays of the building (prefix plan_), the plant's parameters and the start time.

The grid and the actions are chosen so that no stopping decision sits on its edge: tests/test_initial_conditions_cpu.py
asserts a relative margin of 1e-9 between every sweep's max|delta| and the threshold on the oracle.  Should it fail after a
change here, change SEED, never the margin."""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402
from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 20261020
N_STEPS = 12


def start_grid(shape, seed: int = SEED) -> np.ndarray:
  """A smooth field around SB1's heating setpoint: two low-frequency waves with seeded phases and a slope across the
  rows, 291.6 .. 296.4 K, the exterior ring included (the first sweep of a step overwrites the ring's cells)."""
  H, W = shape
  rs = np.random.RandomState(seed)
  p = rs.uniform(0.0, 1.0, size=3)
  y, x = np.mgrid[0:H, 0:W].astype(np.float64)
  return (294.0 + 1.2 * np.sin(2.0 * np.pi * (y / H + p[0])) * np.cos(2.0 * np.pi * (x / W + p[1]))
          + 0.8 * np.cos(2.0 * np.pi * (0.5 * x / W + p[2])) + 0.4 * (y / H - 0.5))


def build(m, floor_plan, start, grid):
  """oracle/gen_golden.py's build_sb1 with the grid as the building's reset_temp_values."""
  S = gg.SB1
  bp = m["building"]
  mk = lambda t: bp.MaterialProperties(conductivity=t[0], heat_capacity=t[1], density=t[2])
  building = bp.FloorPlanBasedBuilding(
      cv_size_cm=S["cv_size_cm"], floor_height_cm=S["floor_height_cm"], initial_temp=S["initial_temp"],
      inside_air_properties=mk(S["air"]), inside_wall_properties=mk(S["wall"]), building_exterior_properties=mk(S["ext"]),
      floor_plan=floor_plan, zone_map=floor_plan.copy(), reset_temp_values=grid)
  weather = m["weather_controller"].WeatherController(**S["weather"])
  boiler = m["boiler"].Boiler(device_id="boiler_id", **S["boiler"])
  ahu = m["air_handler"].AirHandler(device_id="air_handler_id", sim_weather_controller=weather, **S["ahu"])
  schedule = m["setpoint_schedule"].SetpointSchedule(**S["schedule"])
  hvac = m["hvac_floorplan_based"].FloorPlanBasedHvac(
      air_handler=ahu, boiler=boiler, schedule=schedule, vav_max_air_flow_rate=S["vav_max_air_flow_rate"],
      vav_reheat_max_water_flow_rate=S["vav_reheat_max_water_flow_rate"])
  sim = m["simulator_flexible_floor_plan"].SimulatorFlexibleGeometries(
      building, hvac, weather, S["time_step_sec"], S["convergence_threshold"], S["iteration_limit"], S["iteration_warning"],
      start)
  return sim, building, hvac, weather, schedule


def main() -> None:
  if not refshim.available():
    print("reference tree not present; nothing to do")
    return
  m = gg._mods()
  floor_plan = np.asarray(np.load(os.path.join(OUT, "plan_small_test.npz"))["floor_plan"])
  start = pd.Timestamp("2023-07-06 07:00:00")
  grid = start_grid(floor_plan.shape)
  sim, building, hvac, weather, schedule = build(m, floor_plan, start, grid)
  assert building.temp.shape == grid.shape, (building.temp.shape, grid.shape)
  acts = np.random.RandomState(SEED + 1).uniform(-1.0, 1.0, size=(N_STEPS, 2)).astype(np.float32)
  e1 = gg.rollout_h2(m, sim, building, hvac, weather, schedule, N_STEPS, acts, (1,), "reset_temp_values episode 1")
  last_ts = start + pd.Timedelta(300 * (N_STEPS - 1), unit="s")
  e2 = gg.rollout_h2(m, sim, building, hvac, weather, schedule, N_STEPS, acts, (1,), "reset_temp_values episode 2",
                     prev_ts=last_ts)
  out = {}
  for tag, e in (("e1_", e1), ("e2_", e2)):
    for k, v in e.items():
      out[tag + k] = v
  for k, v in gg.dump_building(building, floor_plan).items():
    out["plan_" + k] = v
  prm = gg.hvac_params_of(hvac, sim, schedule)
  R = gg.SB1["reward"]
  prm.update({k: float(v) for k, v in dict(
      max_prod=R["max_productivity_personhour_usd"], min_prod=R["min_productivity_personhour_usd"],
      max_elec=R["max_electricity_rate"], max_gas=R["max_natural_gas_rate"],
      prod_delta=R["productivity_midpoint_delta"], prod_stiff=R["productivity_decay_stiffness"],
      w_prod=R["productivity_weight"], w_cost=R["energy_cost_weight"], w_carbon=R["carbon_emission_weight"]).items()})
  out["params_json"] = np.array(json.dumps(prm))
  out["h_conv"] = gg.SB1["weather"]["convection_coefficient"]
  out["initial_temp"] = gg.SB1["initial_temp"]
  out["start_timestamp"] = np.array(str(start))
  out["reset_temp_values"] = grid
  out["seed"] = SEED
  out["numpy"] = np.array(np.__version__)
  path = os.path.join(OUT, "reset_temp_values.npz")
  np.savez_compressed(path, **out)
  print("wrote", path, os.path.getsize(path), "bytes; sweeps", e1["n_sweeps"].tolist(), e2["n_sweeps"].tolist())


if __name__ == "__main__":
  main()
