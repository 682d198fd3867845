"""Generates tests/golden/regimes.npz by RUNNING THE REFERENCE ITSELF at every coefficient regime of tests/regimes.py.

TEST INFRASTRUCTURE -- runs only where the reference tree exists (``python -m oracle.gen_golden_regimes``); the
reference is imported through ``oracle.refshim`` as in oracle/gen_golden.py and none of its text is stored.  Per regime:
the reference's FloorPlanBasedBuilding on the 2 x 2 rooms of 5 x 9 CVs (15 x 23 inside the ring) with the regime's
materials and CV size, its SimulatorFlexibleGeometries at the regime's time step, threshold, limit and convection
coefficient, the SB1 devices with the regime's VAV flows; harness level H1 (bare step_sim(), which runs the thermostats
and the HVAC), six steps from a seeded rough grid.  Written: the inputs, and per step n_sweeps, the converged flag,
zone_temp_post, the modes and the boiler's return-water temperature, and the final grid.  tests/test_regimes_cpu.py runs
oracle/sb_oracle.c on the same inputs."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pandas as pd

from oracle import gen_golden as gg
from oracle import refshim

START = "2023-07-06 10:00:00"     # mid-morning: comfort mode throughout
T_AMB = 281.0


def _build(m, floor_plan, regime, cfg, start):
  """gen_golden.build_sb1 with the regime's materials, CV size, simulator constants, weather and VAV flows."""
  bp = m["building"]
  mk = lambda t: bp.MaterialProperties(conductivity=t.conductivity, heat_capacity=t.heat_capacity, density=t.density)
  mats = regime.materials
  building = bp.FloorPlanBasedBuilding(
      cv_size_cm=regime.cv_size_cm, floor_height_cm=gg.SB1["floor_height_cm"], initial_temp=gg.SB1["initial_temp"],
      inside_air_properties=mk(mats.air), inside_wall_properties=mk(mats.interior_wall),
      building_exterior_properties=mk(mats.exterior_wall), floor_plan=floor_plan, zone_map=floor_plan.copy())
  weather = m["weather_controller"].WeatherController(default_low_temp=T_AMB, default_high_temp=T_AMB,
                                                      convection_coefficient=regime.h_conv)
  boiler = m["boiler"].Boiler(device_id="boiler_id", **gg.SB1["boiler"])
  ahu = m["air_handler"].AirHandler(device_id="air_handler_id", sim_weather_controller=weather, **gg.SB1["ahu"])
  schedule = m["setpoint_schedule"].SetpointSchedule(**gg.SB1["schedule"])
  hvac = m["hvac_floorplan_based"].FloorPlanBasedHvac(
      air_handler=ahu, boiler=boiler, schedule=schedule, vav_max_air_flow_rate=cfg.vav_max_air_flow_rate,
      vav_reheat_max_water_flow_rate=cfg.vav_reheat_max_water_flow_rate)
  sim = m["simulator_flexible_floor_plan"].SimulatorFlexibleGeometries(
      building, hvac, weather, regime.time_step_sec, regime.convergence_threshold, cfg.iteration_limit,
      gg.SB1["iteration_warning"], start)
  return sim, building, hvac, schedule


def main() -> None:
  if not refshim.available():
    print("reference tree not present; nothing to do")
    return
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  from tests import regimes as rg
  m = gg._mods()
  file_plan = rectangular_floor_plan(*rg.GOLDEN_PLAN)
  out = {"regimes": np.array(list(rg.REGIMES)), "floor_plan": file_plan.astype(np.int8), "t_amb": T_AMB,
         "start_timestamp": np.array(START)}
  for name, regime in rg.REGIMES.items():
    cfg = rg.case_config(rg.CASES["reg32-15x23"], regime)
    start = pd.Timestamp(START)
    sim, building, hvac, schedule = _build(m, file_plan, regime, cfg, start)
    d = gg.dump_building(building)
    ours = rg.apply(FloorPlan.from_file_input(file_plan, Materials.sb1(), 10.0, 300.0), regime)
    for k in ("conductivity", "heat_capacity", "density", "exterior_space", "zone_label", "diffusers"):
      assert np.array_equal(d[k], getattr(ours, k)), (name, k)     # the plan the tests build is the reference's
    init = rg.golden_inputs(regime, building.temp.shape)
    building.temp = init.copy()
    counter = gg.SweepCounter(sim)
    conv_flags = []
    orig = sim.finite_differences_timestep

    def wrapped(*a, _orig=orig, **k):
      conv_flags.append(bool(_orig(*a, **k)))
      return conv_flags[-1]

    sim.finite_differences_timestep = wrapped
    zones = list(hvac.vavs.keys())
    rec = {k: [] for k in ("n_sweeps", "zone_temp_post", "zone_temp_pre", "mode", "blr_return_temp", "ahu_flow", "blr_flow")}
    for _ in range(rg.GOLDEN_STEPS):
      sim.step_sim()
      rec["n_sweeps"].append(counter.take())
      post = building.get_zone_average_temps()
      rec["zone_temp_post"].append([post[z] for z in zones])
      rec["zone_temp_pre"].append([hvac.vavs[z].zone_air_temperature for z in zones])
      rec["mode"].append([hvac.vavs[z].thermostat._current_mode.value for z in zones])
      rec["blr_return_temp"].append(hvac.boiler.return_water_temperature_sensor)
      rec["ahu_flow"].append(hvac.air_handler.air_flow_rate)
      rec["blr_flow"].append(hvac.boiler._total_flow_rate)
    assert len(conv_flags) == rg.GOLDEN_STEPS
    print(f"  {name}: sweeps {rec['n_sweeps']} converged {[int(c) for c in conv_flags]}")
    ts = [start + pd.Timedelta(regime.time_step_sec * i, unit="s") for i in range(rg.GOLDEN_STEPS + 1)]
    out[f"{name}/initial_grid"] = init
    out[f"{name}/converged"] = np.array(conv_flags, dtype=np.int64)
    out[f"{name}/comfort"] = np.array([schedule.is_comfort_mode(t) for t in ts], dtype=np.int64)
    out[f"{name}/final_grid"] = building.temp.copy()
    out[f"{name}/params_json"] = np.array(json.dumps(gg.hvac_params_of(hvac, sim, schedule)))
    out[f"{name}/h_conv"] = regime.h_conv
    for k, v in rec.items():
      out[f"{name}/{k}"] = np.asarray(v, dtype=np.int64 if k in ("n_sweeps", "mode") else np.float64)
  path = os.path.join(gg.OUT, rg.GOLDEN)
  np.savez_compressed(path, **out)
  print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
  sys.exit(main())
