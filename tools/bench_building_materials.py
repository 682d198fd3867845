"""Developer aid: what per-building coefficient rows cost k_sweep_lds.  65,536 R9 buildings for 288 steps, twice: a
default handle forced onto k_sweep_lds (SBSIM_FORCE_LDS_PATH=1: one coefficient table per workgroup, loaded once) and a
materials handle (building_materials=...: a table per wavefront, reloaded for every building) whose rows all repeat the
plan's own values -- the same physics, the same sweep counts, bitwise the same results.  Prints the step time (three
launches, wall clock over the run) and the sweep kernel's time (HIP events around its launch) of both, and one JSON line.
Usage (GPU box): python tools/bench_building_materials.py        (B=..., STEPS=..., WARM=... to change the run)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sbsim_amd.environment import BatchedEnvironment  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from sbsim_amd.host_inputs import BuildingMaterials  # noqa: E402

dev = torch.device("cuda", 0)
B = int(os.environ.get("B", "65536"))
STEPS = int(os.environ.get("STEPS", "288"))
WARM = int(os.environ.get("WARM", "10"))
plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
table = plan.material_slots()[1]
own = BuildingMaterials(conductivity=np.tile(table[:, 0], (B, 1)), heat_capacity=np.tile(table[:, 1], (B, 1)),
                        density=np.tile(table[:, 2], (B, 1)), convection_coefficient=np.full(B, 100.0))
gen = torch.Generator(device=dev)
gen.manual_seed(1234)
acts = torch.rand((STEPS + WARM, B, 2), generator=gen, device=dev, dtype=torch.float32) * 2.0 - 1.0
rs = np.random.RandomState(7)
t_init = torch.tensor(np.clip(294.0 + rs.randn(B), 285.0, 305.0), dtype=torch.float64, device=dev)
H, W = plan.shape

result, finals = {}, {}
for label in ("default_on_k_sweep_lds", "materials"):
  if label == "materials":
    env = BatchedEnvironment(plan, B, collect_info=True, building_materials=own)
  else:
    before = os.environ.get("SBSIM_FORCE_LDS_PATH")
    os.environ["SBSIM_FORCE_LDS_PATH"] = "1"
    env = BatchedEnvironment(plan, B, collect_info=True)
    if before is None:
      del os.environ["SBSIM_FORCE_LDS_PATH"]
    else:
      os.environ["SBSIM_FORCE_LDS_PATH"] = before
  assert env.sim.launch_info["kernel"] == 0, env.sim.launch_info
  env.reset()
  env.sim.reset(temps=t_init[:, None].expand(B, H * W).contiguous())
  for t in range(WARM):
    env.step(acts[t])
  torch.cuda.synchronize()
  env.sim.sweep_events = []
  t0 = time.perf_counter()
  for t in range(WARM, WARM + STEPS):
    env.step(acts[t])
  torch.cuda.synchronize()
  wall = (time.perf_counter() - t0) / STEPS * 1e3
  sweep_ms = float(np.mean([a.elapsed_time(b) for a, b in env.sim.sweep_events]))
  env.sim.sweep_events = None
  li = env.sim.launch_info
  result[label] = {"step_ms": wall, "sweep_kernel_ms": sweep_ms, "workgroups": li["workgroups"],
                   "waves_per_workgroup": li["waves_per_workgroup"], "lds_bytes_per_workgroup": li["lds_bytes_per_workgroup"],
                   "mean_sweeps_last_step": float(env.info[:, 4].double().mean())}
  finals[label] = env.sim.zone_temps().clone()
  print(f"{label}: {wall:.3f} ms per step, sweep kernel {sweep_ms:.3f} ms; {li['workgroups']} workgroups x "
        f"{li['waves_per_workgroup']} wavefronts, {li['lds_bytes_per_workgroup']} B of LDS each")
  env.close()
result["bitwise_equal"] = bool(torch.equal(finals["default_on_k_sweep_lds"], finals["materials"]))
result["buildings"], result["steps"] = B, STEPS
print(json.dumps(result))
