"""Times k_post of the R9 step of BASELINE.json configs[1] (65,536 buildings) under the default reward function (the
regret, k_post<0>) and under SetpointEnergyCarbonReward (k_post<1>).  Two simulators in one process step alternately,
one step each in turn; the reward function changes nothing but the reward, so both hold the same state and take the
same sweeps (checked).  Each of the step's three launches is bracketed with HIP events (sb_step_phases); the medians
per launch are printed as one JSON line.  Under ``rocprofv3 --kernel-trace --stats`` the two kernels show up by name.

  python tools/bench_reward_function.py [--buildings 65536] [--steps 60] [--warmup 10] [--no-info]
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
from sbsim_amd.host_inputs import SetpointEnergyCarbonReward  # noqa: E402
from tools.bench_building_params import step_in  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=60, help="timed steps of each simulator")
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--no-info", action="store_true", help="without the info rows (what bench.py's step passes)")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_reward_function.py needs a GPU")
  B = args.buildings
  cfg = SimConfig.sb1()
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  sims = {"regret": BatchedSimulator(plan, cfg, B, 12.0), "setpoint_energy_carbon": BatchedSimulator(plan, cfg, B, 12.0)}
  sims["setpoint_energy_carbon"].set_reward_function(SetpointEnergyCarbonReward(1.0, 1.0, 0.2, 250.0, 5000.0))
  dev = sims["regret"].tdev
  gen = torch.Generator(device=dev)
  gen.manual_seed(3)
  acts = torch.rand((args.warmup + args.steps, B, 2), generator=gen, device=dev) * 2 - 1
  out = {mode: (torch.empty((B, sim.O), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                None if args.no_info else torch.empty((B, _ffi.SB_INFO_STRIDE), dtype=torch.float32, device=dev))
         for mode, sim in sims.items()}
  ms = {mode: {"pre": [], "sweep": [], "post": []} for mode in sims}
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
    a, b = out["regret"], out["setpoint_energy_carbon"]
    assert torch.equal(a[0], b[0]), "the reward function must not change the observation"
    assert a[2] is None or torch.equal(a[2][:, :7], b[2][:, :7]), "... nor info columns 0..6"
  res = {"buildings": B, "kernel": _ffi.SWEEP_KERNELS.get(sims["regret"].launch_info["kernel"], "?"),
         "timed_steps": args.steps, "info": not args.no_info}
  for mode, d in ms.items():
    for name, v in d.items():
      res[f"{mode}_{name}_ms"] = round(float(np.median(v)), 4)
  res["delta_post_ms"] = round(res["setpoint_energy_carbon_post_ms"] - res["regret_post_ms"], 4)
  print(json.dumps(res))
  for sim in sims.values():
    sim.close()


if __name__ == "__main__":
  main()
