"""New per-building parameters and materials at an episode start, three ways on one MI355X.

65,536 R9 buildings on a materials handle (k_sweep_lds), four parameter fields, one material field and the convection
coefficient.  Timed: ``reset_buildings(mask)`` with 1/64 of the buildings masked, and a full ``reset()``, each

  (a) without any redraw: a handle with no randomisation attached;
  (b) the host route: ``set_building_params`` + ``set_building_materials`` of the full tables (the objects built
      beforehand: only the two calls are timed), then the reset;
  (c) with an ``EpisodeRandomization`` attached: the reset redraws on the device.

HIP events around the call on the current stream (they bracket the host work of (b) too: the device waits for it);
the arms alternate within a repetition, ``--repeats`` repetitions after ``--warmup``, median / minimum / maximum per
arm.  (c) is left out when the library has no sb_randomization_attach (an older build).  One JSON line on stdout; no
GPU, no result.

    python tools/bench_randomization.py [--buildings 65536] [--warmup 3] [--repeats 15]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from sbsim_amd.host_inputs import BuildingMaterials, BuildingParams  # noqa: E402


def event_ms(fn) -> float:
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0.record()
  fn()
  t1.record()
  t1.synchronize()
  return t0.elapsed_time(t1)


def summary(ms):
  return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def main() -> None:
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--repeats", type=int, default=15)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_randomization needs a GPU: a reset's time is a device measurement")
  B = args.buildings
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)   # R9
  cfg = SimConfig.sb1()
  rng = np.random.RandomState(1234)
  table = plan.material_slots()[1]
  M = len(table)
  bm = BuildingMaterials(conductivity=table[:, 0] * rng.uniform(0.5, 2.0, size=(B, M)), convection_coefficient=rng.uniform(6.0, 25.0, size=B))
  bp = BuildingParams(ahu_fan_efficiency=rng.uniform(0.7, 0.95, size=B), vav_max_air_flow_rate=rng.uniform(0.03, 0.045, size=B),
                      boiler_reheat_water_setpoint=rng.uniform(330.0, 360.0, size=B),
                      ahu_heating_air_temp_setpoint=rng.uniform(283.0, 289.0, size=B))
  mask = np.zeros(B, dtype=bool)
  mask[::64] = True
  plain = BatchedSimulator(plan, cfg, B, 100.0, building_materials=bm)
  plain.set_building_params(bp)
  plain.reset()
  arms = {"a_no_redraw": (lambda: plain.reset_buildings(mask), lambda: plain.reset())}

  def host_route(reset):
    plain.set_building_params(bp)
    plain.set_building_materials(bm)
    reset()

  arms["b_host_tables"] = (lambda: host_route(lambda: plain.reset_buildings(mask)), lambda: host_route(plain.reset))
  has_randomization = all(hasattr(_ffi.load(), name) for name in getattr(_ffi, "RANDOMIZATION_ENTRIES", ("sb_randomization_attach",)))
  rand = None
  if has_randomization:
    U, Ch = host_inputs.Uniform, host_inputs.Choice
    er = host_inputs.EpisodeRandomization(
        params={"ahu_fan_efficiency": U(0.7, 0.95), "vav_max_air_flow_rate": U(0.8, 1.2, scale=True),
                "boiler_reheat_water_setpoint": U(330.0, 360.0), "ahu_heating_air_temp_setpoint": U(283.0, 289.0)},
        materials={"conductivity": {0: Ch([0.5, 0.75, 1.0, 1.5, 2.0], scale=True)}, "convection_coefficient": U(6.0, 25.0)}, seed=7)
    rand = BatchedSimulator(plan, cfg, B, 100.0, building_materials=bm)
    rand.set_building_params(bp)
    rand.randomization_attach(er)
    rand.reset()
    arms["c_randomization"] = (lambda: rand.reset_buildings(mask), lambda: rand.reset())
  out = dict(buildings=B, plan=list(plan.shape), masked=int(mask.sum()), kernel=plain.launch_info["kernel"],
             device=torch.cuda.get_device_name(0), randomization=has_randomization)
  for which, name in ((0, "reset_buildings"), (1, "reset")):
    ms = {arm: [] for arm in arms}
    for rep in range(args.warmup + args.repeats):
      for arm, fns in arms.items():   # the arms alternate inside a repetition
        t = event_ms(fns[which])
        if rep >= args.warmup:
          ms[arm].append(t)
    out[name] = {arm: summary(v) for arm, v in ms.items()}
  plain.close()
  if rand is not None:
    rand.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
