"""Times the state snapshots of BASELINE.json configs[1] (65,536 R9 buildings): BatchedSimulator.save_state (every
building), load_state (identity), and a fork (save of one building + load with a pick of it everywhere), with HIP
events, next to torch.Tensor.copy_ of the snapshot's byte count in the same run as the yardstick.  Prints one JSON line.

  python tools/bench_state.py [--buildings 65536] [--reps 10]
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
  return ms[len(ms) // 2]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--reps", type=int, default=10)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_state.py needs a GPU")
  B = args.buildings
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  sim = BatchedSimulator(plan, SimConfig.sb1(), B, 12.0)
  gen = torch.Generator(device="cuda")
  gen.manual_seed(1)
  sim.reset(temps=(294.0 + torch.randn((B, sim.H * sim.W), generator=gen, device="cuda", dtype=torch.float64)))
  snap = sim.save_state()
  nbytes = sum(t.numel() * t.element_size() for t in snap.tensors().values() if t is not None)
  src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
  dst = torch.empty_like(src)
  one = torch.zeros((1,), dtype=torch.int32, device="cuda")
  pick = torch.zeros((B,), dtype=torch.int32, device="cuda")

  def save():
    sim.save_state()

  def load():
    sim.load_state(snap)

  def fork():   # BatchedEnvironment.fork(full(B, 0)) without the host-side checks
    sim.load_state(sim.save_state(rows=one), pick=pick, clock=False)

  res = {"buildings": B, "snapshot_bytes": nbytes, "launch": sim.launch_info["kernel"]}
  for name, fn in (("copy_", lambda: dst.copy_(src)), ("save", save), ("load", load), ("fork", fork),
                   ("copy_again", lambda: dst.copy_(src))):
    res[name + "_ms"] = round(timed(fn, args.reps), 4)
  yard = min(res["copy__ms"], res["copy_again_ms"])
  for name in ("save", "load"):
    res[name + "_vs_copy"] = round(res[name + "_ms"] / yard, 3)
    res[name + "_TBps"] = round(2 * nbytes / res[name + "_ms"] / 1e9, 3)   # read + write
  res["copy_TBps"] = round(2 * nbytes / yard / 1e9, 3)
  print(json.dumps(res))
  sim.close()


if __name__ == "__main__":
  main()
