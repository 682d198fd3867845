"""What the episode totals cost per step, on one MI355X at the headline configuration (65,536 R9 buildings, random actions).

Arms, each an environment of its own that is reset like ``bench.py``'s and fed the same actions, so every arm's
buildings need the same sweeps in the same window:

  plain     sb_step on a handle without the attachment;
  attached  sb_step on a handle with ``episode_metrics_attach()``: k_episode_metrics behind k_post;
  torch     the plain step followed by a torch restatement of the same accumulation on a field-major [20, B] float64
            table (about thirty small launches and a ``zone_temps()`` copy), with the latch as ``torch.where`` once per
            window.

A window is ``--steps`` steps between two device synchronisations on the host clock; the arms alternate within a round,
``--rounds`` rounds after ``--warmup`` steps.  One JSON line on stdout: per arm the windows' ms per step, their median,
minimum and maximum.  The parent commit's step is this tool's ``plain`` arm on the parent's library:

    SBSIM_LIB=<parent checkout>/sbsim_amd/libsbsim_amd.so python tools/bench_episode_metrics.py --arms plain

(alternate the two commands to see the spread between processes).  No GPU, no result.

    python tools/bench_episode_metrics.py [--buildings 65536] [--steps 100] [--rounds 5] [--warmup 24] [--arms plain,attached,torch]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402

ARMS = ("plain", "attached", "torch")


def r9_plan() -> FloorPlan:
  return FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)


class TorchTotals:
  """The table of include/sbsim_amd.h (sb_episode_metrics_attach) in torch, field-major so every update is contiguous."""

  def __init__(self, B: int, dt: float, dev):
    self.dt, self.K = dt, 1.0 / 3600.0 / 1000.0
    self.run = torch.zeros((_ffi.SB_EM_FIELDS, B), dtype=torch.float64, device=dev)
    self.done = torch.zeros_like(self.run)
    self.run[18], self.run[19] = float("inf"), float("-inf")

  def step(self, reward: torch.Tensor, info: torch.Tensor, zone_means: torch.Tensor) -> None:
    R, dt, K = self.run, self.dt, self.K
    r = reward.double()
    rejected = reward == float("-inf")
    I = info.double().t()
    R[1] += 1.0
    R[2] += rejected
    R[3] += r
    R[4] += torch.where(rejected, 0.0, r)
    R[5] += (I[0] * dt * K + I[1] * dt * K) + I[3] * dt * K
    R[6] += I[2] * dt * K
    for col, src in ((7, 9), (8, 10), (9, 11), (10, 17), (11, 20), (12, 21), (13, 22), (14, 23), (15, 8), (16, 4)):
      R[col] += I[src]
    R[17] += info[:, 5] == 0
    R[18] = torch.minimum(R[18], zone_means.amin(dim=1))
    R[19] = torch.maximum(R[19], zone_means.amax(dim=1))

  def close(self, mask: torch.Tensor) -> None:
    closing = mask & (self.run[1] > 0)
    self.done = torch.where(closing[None, :], self.run, self.done)
    fresh = torch.zeros_like(self.run)
    fresh[0] = self.run[0] + 1.0
    fresh[18], fresh[19] = float("inf"), float("-inf")
    self.run = torch.where(closing[None, :], fresh, self.run)


def main() -> None:
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=100)
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=24)
  ap.add_argument("--arms", default=",".join(ARMS))
  args = ap.parse_args()
  arms = [a for a in args.arms.split(",") if a]
  if not arms or any(a not in ARMS for a in arms):
    ap.error(f"--arms: a comma-separated subset of {ARMS}")
  if not torch.cuda.is_available():
    raise SystemExit("bench_episode_metrics.py needs a GPU: no result")
  dev = torch.device("cuda", 0)
  B, K, W = args.buildings, args.steps, args.warmup
  plan = r9_plan()
  H, Wd = plan.shape
  rs = np.random.RandomState(7)
  t_init = np.clip(294.0 + rs.randn(B), 285.0, 305.0)
  init = torch.tensor(t_init, dtype=torch.float64, device=dev)[:, None].expand(B, H * Wd).contiguous()
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  total = W + K * args.rounds
  actions = torch.rand((total, B, 2), generator=gen, device=dev, dtype=torch.float32) * 2.0 - 1.0

  envs, totals = {}, None
  for arm in arms:
    env = BatchedEnvironment(plan, B, holiday_calendar="us", collect_info=True, num_days_in_episode=3, config=SimConfig(),
                             episode_metrics=arm == "attached")
    env.reset()
    env.sim.reset(temps=init)
    envs[arm] = env
    if arm == "torch":
      totals = TorchTotals(B, env.config.time_step_sec, dev)
  everyone = torch.ones((B,), dtype=torch.bool, device=dev)

  def one_step(arm: str, t: int) -> None:
    env = envs[arm]
    si = env.make_step_in(env.current_simulation_timestamp)
    env.sim.step(actions[t], si, env._obs, env._reward, env._info)
    env._prev_thermostat_ts = env._now
    env._now = env._now + env._step_interval
    if arm == "torch":
      totals.step(env._reward, env._info, env.sim.zone_temps())

  for arm in arms:
    for t in range(W):
      one_step(arm, t)
  torch.cuda.synchronize(dev)
  ms = {arm: [] for arm in arms}
  for r in range(args.rounds):
    for arm in arms[r % len(arms):] + arms[:r % len(arms)]:   # the order rotates from round to round
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      for t in range(W + r * K, W + (r + 1) * K):
        one_step(arm, t)
      if arm == "torch":
        totals.close(everyone)
      torch.cuda.synchronize(dev)
      ms[arm].append((time.perf_counter() - t0) / K * 1e3)
  out = dict(tool="bench_episode_metrics", device=torch.cuda.get_device_name(0), library=_ffi.LIB_PATH, buildings=B,
             steps_per_window=K, rounds=args.rounds, warmup=W,
             arms={arm: dict(ms_per_step=v, median=statistics.median(v), min=min(v), max=max(v)) for arm, v in ms.items()})
  if "attached" in arms:   # the totals are real: every building has stepped through every window
    steps = envs["attached"].episode_metrics()[:, 1]
    out["attached_steps_counted"] = [float(steps.min()), float(steps.max())]
  if "torch" in arms:   # ... and the restatement's latch closed the last window's
    out["torch_last_window_steps"] = [float(totals.done[1].min()), float(totals.done[1].max())]
  print(json.dumps(out))
  for env in envs.values():
    env.close()


if __name__ == "__main__":
  main()
