"""Times sb_spatial on BASELINE.json configs[1] (65,536 R9 buildings, the default kernel): zone statistics plus the
(4, 4) pooled map in ONE launch, next to today's route on the same handle in the same run --

  (a) sim.temps() alone: k_copy_temps writes [B, H * W] float64 (the yardstick: sb_spatial reads the same state and
      writes under a tenth as much, so it must not take longer);
  (b) temps() followed by torch: avg_pool2d (ceil_mode, summed, divided by the tiles' own cell counts) and amin / amax /
      mean over each zone's cells.

HIP events around each call after a warm-up; the three routes alternate inside every repetition and the median of the
repetitions is reported (tools/bench_state.py's scheme).  Prints one JSON line; state bytes per second of sb_spatial is
B * H * W * 8 bytes (the float64 grid the kernel reads once) over its median time.

  python tools/bench_spatial.py [--buildings 65536] [--reps 15] [--pool 4 4]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402


def median(xs):
  xs = sorted(xs)
  return xs[len(xs) // 2]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--reps", type=int, default=15)
  ap.add_argument("--pool", type=int, nargs=2, default=(4, 4))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_spatial.py needs a GPU")
  B, pool = args.buildings, tuple(args.pool)
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  sim = BatchedSimulator(plan, SimConfig.sb1(), B, 12.0)
  H, W = sim.H, sim.W
  gen = torch.Generator(device="cuda")
  gen.manual_seed(1)
  sim.reset(temps=(294.0 + torch.randn((B, H * W), generator=gen, device="cuda", dtype=torch.float64)))
  sim.spatial_attach(pool)
  stats = torch.empty((B, sim.Z, 3), dtype=torch.float64, device="cuda")
  tmap = torch.empty((B,) + sim.map_shape, dtype=torch.float32, device="cuda")
  zones = [torch.as_tensor(c, dtype=torch.int64, device="cuda") for c in plan.zone_cell_lists()]
  count = torch.nn.functional.avg_pool2d(torch.ones((1, 1, H, W), dtype=torch.float64, device="cuda"), pool, ceil_mode=True,
                                         divisor_override=1)

  def new():
    sim.spatial(None, stats_out=stats, map_out=tmap)

  def route_a():
    return sim.temps()

  def route_b():
    t = sim.temps()
    m = (torch.nn.functional.avg_pool2d(t[:, None], pool, ceil_mode=True, divisor_override=1) / count)[:, 0].float()
    flat = t.reshape(B, -1)
    out = torch.empty((B, len(zones), 3), dtype=torch.float64, device="cuda")
    for z, cells in enumerate(zones):
      x = flat[:, cells]
      out[:, z, 0], out[:, z, 1], out[:, z, 2] = x.amin(dim=1), x.amax(dim=1), x.mean(dim=1)
    return m, out

  routes = (("sb_spatial", new), ("temps", route_a), ("temps_torch", route_b))
  for _, fn in routes:      # warm-up: code objects, the caching allocator's blocks
    fn()
    fn()
  torch.cuda.synchronize()
  m, out = route_b()        # the two routes agree (reordered float64 sums: last bits)
  new()
  torch.cuda.synchronize()
  agree = dict(map_max_abs=float((m - tmap).abs().max()), mean_max_abs=float((out[:, :, 2] - stats[:, :, 2]).abs().max()),
               minmax_equal=bool(torch.equal(out[:, :, :2], stats[:, :, :2])))
  del m, out
  ms = {name: [] for name, _ in routes}
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for _ in range(args.reps):
    for name, fn in routes:
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      ms[name].append(e0.elapsed_time(e1))
  med = {name: median(v) for name, v in ms.items()}
  state_bytes = B * H * W * 8
  res = {"buildings": B, "plan": [H, W], "pool": list(pool), "kernel": sim.launch_info["kernel"], "reps": args.reps,
         "sb_spatial_ms": round(med["sb_spatial"], 4), "temps_ms": round(med["temps"], 4),
         "temps_torch_ms": round(med["temps_torch"], 4),
         "sb_spatial_min_max_ms": [round(min(ms["sb_spatial"]), 4), round(max(ms["sb_spatial"]), 4)],
         "temps_min_max_ms": [round(min(ms["temps"]), 4), round(max(ms["temps"]), 4)],
         "sb_spatial_over_temps": round(med["sb_spatial"] / med["temps"], 3),
         "temps_torch_over_sb_spatial": round(med["temps_torch"] / med["sb_spatial"], 2),
         "state_bytes": state_bytes, "sb_spatial_state_TBps": round(state_bytes / med["sb_spatial"] / 1e9, 3),
         "output_bytes": stats.numel() * 8 + tmap.numel() * 4, "agreement_with_torch": agree,
         "bar_met": bool(med["sb_spatial"] <= med["temps"])}
  print(json.dumps(res))
  sim.close()


if __name__ == "__main__":
  main()
