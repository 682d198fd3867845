"""Per-building start temperatures two ways on one MI355X: the staging array against attached initial conditions.

  (a) the staging path: ``t_init[:, None].expand(B, H * W).contiguous()`` and ``sim.reset(temps=...)`` -- what bench.py
      does for its headline run: a float64 [B, H*W] array (3.5 GB at 65,536 R9 buildings) to carry B numbers;
  (b) ``InitialConditions(initial_temp=t_init)`` attached once, then ``sim.reset()``.

Start temperatures as bench.py draws them: clip(294 + N(0, 1), 285, 305).  Reported per way: milliseconds per reset (HIP
events around the call on the current stream; median, minimum and maximum of ``--repeats`` timed resets after
``--warmup``; (a) is timed with the array already built and, separately, with the expand().contiguous() inside the timed
window, which is what a caller pays at every episode start), ``torch.cuda.max_memory_allocated`` of the way's own
allocations (the simulator's state is the library's own hipMalloc and is not in that figure either way), and whether
both leave bitwise equal state (temps, zone temperatures, scalars).  One JSON line on stdout; no GPU, no result.

    python tools/bench_initial_conditions.py [--buildings 65536] [--warmup 3] [--repeats 20]"""
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

from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from sbsim_amd.host_inputs import InitialConditions  # noqa: E402


def timed(fn, warmup: int, repeats: int):
  """Milliseconds of fn() on the current stream: HIP events, one pair per call."""
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(repeats):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    ms.append(t0.elapsed_time(t1))
  return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def main() -> None:
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--repeats", type=int, default=20)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_initial_conditions needs a GPU: a reset's time is a device measurement")
  if args.repeats < 10:
    raise SystemExit("--repeats must be at least 10 (the median of fewer says little)")
  B = args.buildings
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)   # R9
  H, W = plan.shape
  dev = torch.device("cuda", 0)
  t_init = np.clip(294.0 + np.random.RandomState(1234).randn(B), 285.0, 305.0)
  sim = BatchedSimulator(plan, SimConfig.sb1(), B, 100.0)
  out = dict(buildings=B, plan=[H, W], kernel=sim.launch_info["kernel"], staging_bytes=8 * B * H * W,
             device=torch.cuda.get_device_name(0))

  # (a) the staging array
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  t_dev = torch.tensor(t_init, dtype=torch.float64, device=dev)
  staged = t_dev[:, None].expand(B, H * W).contiguous()
  reset_only = timed(lambda: sim.reset(temps=staged), args.warmup, args.repeats)
  del staged

  def stage_and_reset():
    sim.reset(temps=t_dev[:, None].expand(B, H * W).contiguous())

  with_staging = timed(stage_and_reset, args.warmup, args.repeats)
  torch.cuda.synchronize()
  out["staging"] = dict(reset=reset_only, stage_and_reset=with_staging,
                        max_memory_allocated=torch.cuda.max_memory_allocated() - base)
  state_a = [sim.temps(), sim.zone_temps(), sim.scalars()]   # (kept on the device: 3.5 GB more than (b) needs, inside its base)
  del t_dev
  torch.cuda.empty_cache()

  # (b) the conditions in the handle
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  sim.initial_conditions_attach(InitialConditions(initial_temp=t_init))
  attached = timed(lambda: sim.reset(), args.warmup, args.repeats)
  torch.cuda.synchronize()
  out["initial_conditions"] = dict(reset=attached, max_memory_allocated=torch.cuda.max_memory_allocated() - base)
  state_b = [sim.temps(), sim.zone_temps(), sim.scalars()]
  out["bitwise_equal_state"] = all(torch.equal(x, y) for x, y in zip(state_a, state_b))
  sim.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
