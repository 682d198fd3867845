"""Times episodes per building (sb_reset_buildings) on the R9 step of BASELINE.json configs[1] (65,536 buildings) with
random start offsets.

(a) Steps on which no episode ends.  Two simulators on the same calendar and offsets step alternately, one step each in
turn (tools/bench_clock.py's scheme): "clock" is the plain calendar per building, "episodes" has had half of its
buildings restarted by sb_reset_buildings, so that its effective offsets differ from the attached ones and k_pre takes
the previous thermostat update from the building's scalars.  They launch the same kernels; the medians per launch and of
the whole step are printed.
(b) One reset_buildings() of 1 building, 1 %, 50 % and 100 % of the batch against reset(): host wall time of the call
up to the device's completion (the call uploads its mask and synchronises with the stream), median of --resets calls.

One JSON line.  python tools/bench_episodes.py [--buildings 65536] [--steps 60] [--warmup 10] [--resets 15]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from tools.bench_clock import rows  # noqa: E402

MAX_OFFSET = 2000
RESTART_AT = 3     # the batch position at which half of the "episodes" simulator restarts


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=60, help="timed steps of each simulator")
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--resets", type=int, default=15, help="timed calls per mask size")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_episodes.py needs a GPU")
  B = args.buildings
  cfg = SimConfig.sb1()
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  rs = np.random.RandomState(1)
  offsets = rs.randint(0, MAX_OFFSET, size=B).astype(np.int32)
  n = RESTART_AT + args.warmup + args.steps
  table = rows(MAX_OFFSET + n + 2)
  sims = {"clock": BatchedSimulator(plan, cfg, B, 12.0), "episodes": BatchedSimulator(plan, cfg, B, 12.0)}
  for sim in sims.values():
    sim.clock_attach(table, offsets)
  dev = sims["clock"].tdev
  gen = torch.Generator(device=dev)
  gen.manual_seed(3)
  acts = torch.rand((n, B, 2), generator=gen, device=dev) * 2 - 1
  out = {mode: (torch.empty((B, sim.O), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                torch.empty((B, _ffi.SB_INFO_STRIDE), dtype=torch.float32, device=dev)) for mode, sim in sims.items()}
  no_reject = torch.zeros((B,), dtype=torch.uint8, device=dev)
  si = _ffi.StepIn()
  si.has_action = 1
  si.reject_dev = no_reject.data_ptr()   # both read the previous thermostat update from the scalars: the same k_pre path
  ms = {mode: {"pre": [], "sweep": [], "post": [], "step": []} for mode in sims}
  for sim in sims.values():
    sim.reset()
  half = rs.rand(B) < 0.5
  for t in range(n):
    if t == RESTART_AT:
      sims["episodes"].reset_buildings(half, restart_pos=t)
    for mode, sim in sims.items():
      sim.clock_seek(t, t - 1)
      ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
      ev[0].record()
      for k, phase in enumerate((1, 2, 4)):
        sim.step(acts[t], si, *out[mode], phases=phase)
        ev[k + 1].record()
      ev[3].synchronize()
      if t >= RESTART_AT + args.warmup:
        for k, name in enumerate(("pre", "sweep", "post")):
          ms[mode][name].append(ev[k].elapsed_time(ev[k + 1]))
        ms[mode]["step"].append(ev[0].elapsed_time(ev[3]))
  res = {"buildings": B, "kernel": _ffi.SWEEP_KERNELS.get(sims["clock"].launch_info["kernel"], "?"), "timed_steps": args.steps}
  for mode, d in ms.items():
    for name, v in d.items():
      res[f"{mode}_{name}_ms"] = round(float(np.median(v)), 4)
      if name == "step":
        res[f"{mode}_step_ms_p10_p90"] = [round(float(np.percentile(v, q)), 4) for q in (10, 90)]
  for name in ("pre", "sweep", "post", "step"):
    res[f"delta_{name}_ms"] = round(res[f"episodes_{name}_ms"] - res[f"clock_{name}_ms"], 4)

  # (b) the reset calls, on the "episodes" simulator
  sim = sims["episodes"]
  masks = {"1_building": np.arange(B) == B // 2, "1_percent": rs.rand(B) < 0.01, "50_percent": rs.rand(B) < 0.5,
           "100_percent": np.ones(B, dtype=bool)}

  def timed(call):
    v = []
    for _ in range(args.resets + 3):
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      call()
      torch.cuda.synchronize(dev)
      v.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(v[3:])), 4)

  res["reset_ms"] = timed(sim.reset)
  for name, m in masks.items():
    m8 = np.ascontiguousarray(m, dtype=np.uint8)
    res[f"reset_buildings_{name}_ms"] = timed(lambda: sim.reset_buildings(m8, restart_pos=0))
  print(json.dumps(res))
  for sim in sims.values():
    sim.close()


if __name__ == "__main__":
  main()
