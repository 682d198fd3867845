"""Measures the Jacobi solver (BatchedEnvironment(solver="jacobi_fp32"): k_sweep_jacobi, or k_sweep_jacobi_g on plans
beyond one CU's LDS) on 65,536 SB1 R9 buildings (or --rooms / --room-shape: another rectangular plan) under random
actions: in the driver-like window (the first steps after reset) and in the steady state after 100 steps.
Prints one JSON line per window: ms per step, the sweep kernel's ms (HIP events around sb_step_phases' sweep launch),
Jacobi iterations per step, CV-iterations per second, and `frac` of 8 TB/s against the algorithmic bytes.  For
k_sweep_jacobi_g (launch path 2) also the kernel's own traffic: per CV 13 bytes an iteration (T and (M*Tprev)/dt read,
the class byte read, T' written; the four neighbours are in lines the workgroup reads for T) and 12 a step (Tprev
read, (M*Tprev)/dt and the final grid written), over the sweep kernel's time.

  python tools/bench_jacobi.py [--buildings 65536] [--steps 20] [--warmup 5] [--steady-after 100]
  python tools/bench_jacobi.py --rooms 14 9 --room-shape 20 43 --buildings 1536      # the 299 x 401 SB1 stand-in"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sbsim_amd.environment import BatchedEnvironment  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def window(env, steps, rs, label):
  B = env.batch_size
  env.sim.sweep_events = []
  iters = []
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  acts = [torch.tensor(rs.uniform(-1, 1, (B, 2)), dtype=torch.float32, device="cuda") for _ in range(steps)]
  torch.cuda.synchronize()
  t0.record()
  for a in acts:
    env.step(a)
    iters.append(env.info[:, 4].mean())
  t1.record()
  torch.cuda.synchronize()
  ev = env.sim.sweep_events
  env.sim.sweep_events = None
  ms = t0.elapsed_time(t1) / steps
  sweep_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
  it = float(torch.stack(iters).mean())
  li = env.sim.launch_info
  N = env.sim.H * env.sim.W
  extra = {}
  if li["path"] == 2:
    extra["sweep_kernel_traffic_GBps"] = B * N * (13.0 * it + 12.0) / (sweep_ms * 1e-3) / 1e9
  return {**extra, "window": label, "buildings": B, "steps": steps, "ms_per_step": ms, "sweep_kernel_ms": sweep_ms,
          "iterations_per_step": it, "cv_iterations_per_s": B * N * it / (sweep_ms * 1e-3),
          "frac_step": li["algorithmic_bytes_per_env_step"] * B / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
          "frac_sweep_kernel": li["algorithmic_bytes_per_env_step"] * B / (sweep_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
          "launch": li}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--steady-after", type=int, default=100)
  ap.add_argument("--rooms", type=int, nargs=2, default=(3, 3), help="rooms down and across (default: SB1 R9)")
  ap.add_argument("--room-shape", type=int, nargs=2, default=(20, 30), help="air CVs of a room, down and across")
  a = ap.parse_args()
  plan = FloorPlan.from_file_input(rectangular_floor_plan(tuple(a.rooms), tuple(a.room_shape)), Materials.sb1(), 10.0, 300.0)
  env = BatchedEnvironment(plan, a.buildings, holiday_calendar=None, collect_info=True, solver="jacobi_fp32")
  rs = np.random.RandomState(0)
  env.reset()
  for _ in range(a.warmup):
    env.step(torch.tensor(rs.uniform(-1, 1, (a.buildings, 2)), dtype=torch.float32, device="cuda"))
  print(json.dumps(window(env, a.steps, rs, "driver")), flush=True)
  done = a.warmup + a.steps
  while done < a.steady_after:
    env.step(torch.tensor(rs.uniform(-1, 1, (a.buildings, 2)), dtype=torch.float32, device="cuda"))
    done += 1
  print(json.dumps(window(env, a.steps, rs, f"steady (after {done} steps)")), flush=True)
  env.close()


if __name__ == "__main__":
  main()
