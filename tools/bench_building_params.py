"""Times the R9 step of BASELINE.json configs[1] (65,536 buildings) with and without a full per-building parameter
table (sb_set_building_params, all 32 fields).  Two simulators in one process, one without a table and one with it,
step alternately, one step each in turn.  The table holds SB1's own values, so both compute the same numbers bit for bit
and take the same sweeps (checked): the difference is the table's reads in k_pre and k_post.  Each of the step's three
launches is bracketed with HIP events (sb_step_phases); the medians per launch and of the whole step are printed as
one JSON line.

  python tools/bench_building_params.py [--buildings 65536] [--steps 60] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from sbsim_amd.host_inputs import BUILDING_PARAM_NAMES, BuildingParams  # noqa: E402


def step_in(t: int) -> _ffi.StepIn:
  si = _ffi.StepIn()
  si.t_amb_now, si.t_amb_next = 278.0 + 0.01 * t, 278.0 + 0.01 * (t + 1)
  si.comfort_now = si.comfort_next = 1
  si.comfort_prev = 1 if t else -1
  si.has_action = 1
  si.occupancy = 10.0
  si.e_price, si.e_carbon, si.g_price, si.g_carbon = 3e-8, 1e-7, 1e-8, 5e-8
  return si


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=60, help="timed steps of each simulator")
  ap.add_argument("--warmup", type=int, default=10)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_building_params.py needs a GPU")
  B = args.buildings
  cfg = SimConfig.sb1()
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  table = BuildingParams({name: np.broadcast_to(np.asarray(getattr(cfg, name), dtype=np.float64),
                                                (B,) + np.asarray(getattr(cfg, name)).shape)
                          for name in BUILDING_PARAM_NAMES})
  assert int(table.c_table()[0].shape[0]) == _ffi.SB_NUM_BUILDING_PARAMS
  sims = {"no_table": BatchedSimulator(plan, cfg, B, 12.0), "table": BatchedSimulator(plan, cfg, B, 12.0)}
  sims["table"].set_building_params(table)
  dev = sims["table"].tdev
  gen = torch.Generator(device=dev)
  gen.manual_seed(3)
  acts = torch.rand((args.warmup + args.steps, B, 2), generator=gen, device=dev) * 2 - 1
  out = {mode: (torch.empty((B, sim.O), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                torch.empty((B, _ffi.SB_INFO_STRIDE), dtype=torch.float32, device=dev)) for mode, sim in sims.items()}
  ms = {mode: {"pre": [], "sweep": [], "post": [], "step": []} for mode in sims}
  for sim in sims.values():
    sim.reset()
  for t in range(args.warmup + args.steps):
    si = step_in(t)
    for mode, sim in sims.items():   # one step of each in turn: clock drift and the sweeps' transient hit both alike
      ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
      ev[0].record()
      for k, phase in enumerate((1, 2, 4)):
        sim.step(acts[t], si, *out[mode], phases=phase)
        ev[k + 1].record()
      ev[3].synchronize()
      if t >= args.warmup:
        for k, name in enumerate(("pre", "sweep", "post")):
          ms[mode][name].append(ev[k].elapsed_time(ev[k + 1]))
        ms[mode]["step"].append(ev[0].elapsed_time(ev[3]))
    for a, b in zip(out["no_table"], out["table"]):
      assert torch.equal(a, b), "a table of SB1's values must not change a bit"
  res = {"buildings": B, "kernel": _ffi.SWEEP_KERNELS.get(sims["table"].launch_info["kernel"], "?"),
         "timed_steps": args.steps, "table_bytes": 8 * _ffi.SB_NUM_BUILDING_PARAMS * B}
  for mode, d in ms.items():
    for name, v in d.items():
      res[f"{mode}_{name}_ms"] = round(float(np.median(v)), 4)
  for name in ("pre", "sweep", "post", "step"):
    res[f"delta_{name}_ms"] = round(res[f"table_{name}_ms"] - res[f"no_table_{name}_ms"], 4)
  res["delta_pre_post_percent_of_step"] = round(
      100.0 * (res["delta_pre_ms"] + res["delta_post_ms"]) / res["no_table_step_ms"], 3)
  res["delta_step_percent"] = round(100.0 * res["delta_step_ms"] / res["no_table_step_ms"], 3)
  print(json.dumps(res))
  for sim in sims.values():
    sim.close()


if __name__ == "__main__":
  main()
