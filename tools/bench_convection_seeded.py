"""Times one launch of the seeded convection shuffle (k_convect_seeded, sb_convection_attach_seeded) on 65,536 R9
buildings at p = 1, distance = 5 with HIP events, next to the counter-based shuffle (k_convect) on the same handle in the
same run.  Both permute the grid in place, so every repetition does the same amount of work.  Prints one JSON line.

  python tools/bench_convection_seeded.py [--buildings 65536] [--reps 7]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402


def timed(fn, reps):
  fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  ms = []
  for _ in range(reps):
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
  ms.sort()
  return ms[len(ms) // 2], ms[0], ms[-1]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--reps", type=int, default=7)
  ap.add_argument("--p", type=float, default=1.0)
  ap.add_argument("--distance", type=int, default=5)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_convection_seeded.py needs a GPU")
  B = args.buildings
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  sim = BatchedSimulator(plan, SimConfig.sb1(), B, 12.0)
  gen = torch.Generator(device="cuda")
  gen.manual_seed(1)
  sim.reset(temps=(294.0 + torch.randn((B, sim.H * sim.W), generator=gen, device="cuda", dtype=torch.float64)))
  res = {"buildings": B, "p": args.p, "distance": args.distance, "reps": args.reps}
  sim.convection_attach(args.p, args.distance, seed=5)
  res["counter_ms"], res["counter_min_ms"], res["counter_max_ms"] = (round(v, 4) for v in timed(sim.convection_apply, args.reps))
  sim.convection_attach_seeded(args.p, args.distance, 5)
  res["seeded_ms"], res["seeded_min_ms"], res["seeded_max_ms"] = (round(v, 4) for v in timed(sim.convection_apply, args.reps))
  res["seeded_vs_counter"] = round(res["seeded_ms"] / res["counter_ms"], 2)
  res["seeded_us_per_building_per_workgroup"] = round(res["seeded_ms"] * 1e3 / max(1, -(-B // 4096)), 2)
  print(json.dumps(res))
  sim.close()


if __name__ == "__main__":
  main()
