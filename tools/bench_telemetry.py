"""What scoring every building against recorded zone temperatures costs per step, on one MI355X at the headline
configuration (65,536 R9 buildings, random actions).

Arms, each an environment of its own that is reset like ``bench.py``'s and fed the same actions, so every arm's
buildings need the same sweeps in the same window:

  plain              sb_step on a handle without the attachment;
  attached           sb_step on a handle with ``telemetry_attach(Telemetry(...))``: k_telemetry behind k_post, scalar tables;
  attached_per_zone  the same with ``per_zone=True``: also the [4][Z][B] per-zone tables;
  torch              the plain step followed by a torch restatement of the same accumulation on field-major [13, B] and
                     [4, Z, B] float64 tables: a ``zone_temps()`` copy, a gather of every building's own row of the
                     recording, some forty small launches, and the latch as ``torch.where`` once per window.

The recording holds ``--traces`` traces of ``--rows`` rows (NaN in one value of a hundred); the buildings are spread over
the traces and start at staggered first rows, so a wavefront's buildings read scattered rows.  Every window walks the
recording from the buildings' first rows: the torch arm latches at the end of its window (inside the clock, as in
tools/bench_episode_metrics.py), the attached arms' tables are read and re-initialised between windows, outside the clock.

A window is ``--steps`` steps between two device synchronisations on the host clock; the arms alternate within a round,
``--rounds`` rounds after ``--warmup`` steps.  One JSON line on stdout: per arm the windows' ms per step, their median,
minimum and maximum, and for every other arm the difference of its median to ``plain``'s of the same process.  The parent
commit's step is this tool's ``plain`` arm on the parent's library:

    SBSIM_LIB=<parent checkout>/sbsim_amd/libsbsim_amd.so python tools/bench_telemetry.py --arms plain

(alternate the two commands to see the spread between processes).  No GPU, no result.

    python tools/bench_telemetry.py [--buildings 65536] [--steps 100] [--rounds 5] [--warmup 24] [--traces 8] [--rows 288]
                                    [--arms plain,attached,attached_per_zone,torch]"""
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

ARMS = ("plain", "attached", "attached_per_zone", "torch")


def r9_plan() -> FloorPlan:
  return FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)


class TorchScores:
  """The tables of include/sbsim_amd.h (sb_telemetry_attach) in torch, field-major so every update is contiguous."""

  def __init__(self, traces, trace_of, first_row, weights, dev):
    self.traces = torch.tensor(traces, dtype=torch.float64, device=dev)           # [n_traces, n_rows, Z]
    self.trace_of = torch.tensor(trace_of, dtype=torch.int64, device=dev)
    self.first_row = torch.tensor(first_row, dtype=torch.float64, device=dev)
    self.w = torch.tensor(weights, dtype=torch.float64, device=dev)[:, None]      # [Z, 1]
    self.n_rows, Z, B = traces.shape[1], traces.shape[2], len(trace_of)
    self.zone_index = torch.arange(Z, dtype=torch.float64, device=dev)[:, None]
    self.run = self._fresh(B, dev)
    self.done = self._fresh(B, dev)
    self.zrun = torch.zeros((4, Z, B), dtype=torch.float64, device=dev)
    self.zdone = torch.zeros_like(self.zrun)

  @staticmethod
  def _fresh(B, dev):
    rows = torch.zeros((13, B), dtype=torch.float64, device=dev)
    rows[7:10] = -1.0
    return rows

  def step(self, zone_means: torch.Tensor) -> None:
    R, Z = self.run, self.zone_index.shape[0]
    r = self.first_row + R[1]
    R[1] += 1.0
    inside = r < self.n_rows
    row = torch.clamp(r, max=self.n_rows - 1).to(torch.int64)
    obs = self.traces[self.trace_of, row].t()                                     # [Z, B]: every building's own row
    have = inside[None, :] & ~torch.isnan(obs)
    e = torch.where(have, zone_means.t() - obs, 0.0)
    a, q = e.abs(), e * e
    n = have.to(torch.float64)
    R[2] += n.sum(dim=0)
    R[3] += Z - n.sum(dim=0)
    R[4] += e.sum(dim=0)
    R[5] += a.sum(dim=0)
    R[6] += q.sum(dim=0)
    amax, zmax = torch.where(have, a, -1.0).max(dim=0)
    better = amax > R[7]
    R[7] = torch.where(better, amax, R[7])
    R[8] = torch.where(better, r, R[8])
    R[9] = torch.where(better, zmax.to(torch.float64), R[9])
    R[10] += (self.w * a).sum(dim=0)
    R[11] += (self.w * q).sum(dim=0)
    R[12] += (self.w * n).sum(dim=0)
    self.zrun[0] += n
    self.zrun[1] += e
    self.zrun[2] += a
    self.zrun[3] += q

  def close(self, mask: torch.Tensor) -> None:
    closing = mask & (self.run[1] > 0)
    self.done = torch.where(closing[None, :], self.run, self.done)
    fresh = self._fresh(self.run.shape[1], self.run.device)
    fresh[0] = self.run[0] + 1.0
    self.run = torch.where(closing[None, :], fresh, self.run)
    self.zdone = torch.where(closing[None, None, :], self.zrun, self.zdone)
    self.zrun = torch.where(closing[None, None, :], 0.0, self.zrun)


def main() -> None:
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=100)
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=24)
  ap.add_argument("--traces", type=int, default=8)
  ap.add_argument("--rows", type=int, default=288)
  ap.add_argument("--arms", default=",".join(ARMS))
  args = ap.parse_args()
  arms = [a for a in args.arms.split(",") if a]
  if not arms or any(a not in ARMS for a in arms):
    ap.error(f"--arms: a comma-separated subset of {ARMS}")
  if not torch.cuda.is_available():
    raise SystemExit("bench_telemetry.py needs a GPU: no result")
  dev = torch.device("cuda", 0)
  B, K, W = args.buildings, args.steps, args.warmup
  plan = r9_plan()
  H, Wd = plan.shape
  Z = plan.n_zones
  rs = np.random.RandomState(7)
  t_init = np.clip(294.0 + rs.randn(B), 285.0, 305.0)
  init = torch.tensor(t_init, dtype=torch.float64, device=dev)[:, None].expand(B, H * Wd).contiguous()
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  total = W + K * args.rounds
  actions = torch.rand((total, B, 2), generator=gen, device=dev, dtype=torch.float32) * 2.0 - 1.0
  traces = rs.uniform(290.0, 298.0, size=(args.traces, args.rows, Z))
  traces[rs.rand(*traces.shape) < 0.01] = np.nan
  trace_of = rs.randint(0, args.traces, size=B).astype(np.int32)
  first_row = rs.randint(0, max(1, args.rows - K), size=B).astype(np.int32)      # staggered; a window stays inside the recording
  weights = rs.uniform(0.5, 2.0, size=Z)

  envs, scores = {}, None
  for arm in arms:
    tel = None
    if arm.startswith("attached"):
      from sbsim_amd.host_inputs import Telemetry   # (the parent's package has none: its plain arm never gets here)
      tel = dict(telemetry=Telemetry(traces, trace_of=trace_of, first_row=first_row, zone_weights=weights,
                                     per_zone=arm == "attached_per_zone"))
    env = BatchedEnvironment(plan, B, holiday_calendar="us", collect_info=True, num_days_in_episode=3, config=SimConfig(),
                             **(tel or {}))
    env.reset()
    env.sim.reset(temps=init)
    envs[arm] = env
    if arm == "torch":
      scores = TorchScores(traces, trace_of, first_row, weights, dev)
  everyone = torch.ones((B,), dtype=torch.bool, device=dev)

  def one_step(arm: str, t: int) -> None:
    env = envs[arm]
    si = env.make_step_in(env.current_simulation_timestamp)
    env.sim.step(actions[t], si, env._obs, env._reward, env._info)
    env._prev_thermostat_ts = env._now
    env._now = env._now + env._step_interval
    if arm == "torch":
      scores.step(env.sim.zone_temps())

  for arm in arms:
    for t in range(W):
      one_step(arm, t)
    if arm.startswith("attached"):
      envs[arm].sim.telemetry_attach(envs[arm].sim.telemetry)   # the warm-up does not count: fresh tables, step count 0
  if scores is not None:
    scores.close(everyone)
  torch.cuda.synchronize(dev)
  ms = {arm: [] for arm in arms}
  sums = {}
  for r in range(args.rounds):
    for arm in arms[r % len(arms):] + arms[:r % len(arms)]:   # the order rotates from round to round
      env = envs[arm]
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      for t in range(W + r * K, W + (r + 1) * K):
        one_step(arm, t)
      if arm == "torch":
        scores.close(everyone)
      torch.cuda.synchronize(dev)
      ms[arm].append((time.perf_counter() - t0) / K * 1e3)
      if arm.startswith("attached"):   # outside the clock: the window's scores are read, and the next window starts at step 0 again
        run = env.sim.telemetry_scores()
        sums[arm] = [float(run[:, 1].min()), float(run[:, 1].max()), float(run[:, 2].sum()), float(run[:, 3].sum()), float(run[:, 5].sum())]
        env.sim.telemetry_attach(env.sim.telemetry)
  med = {arm: statistics.median(v) for arm, v in ms.items()}
  out = dict(tool="bench_telemetry", device=torch.cuda.get_device_name(0), library=_ffi.LIB_PATH, buildings=B, zones=Z,
             steps_per_window=K, rounds=args.rounds, warmup=W, traces=args.traces, rows=args.rows,
             arms={arm: dict(ms_per_step=v, median=med[arm], min=min(v), max=max(v)) for arm, v in ms.items()})
  if "plain" in arms:
    out["added_ms_per_step_to_plain"] = {arm: med[arm] - med["plain"] for arm in arms if arm != "plain"}
  for arm, s in sums.items():   # the scores are real: every building stepped through the last window
    out[arm + "_last_window"] = dict(steps_min=s[0], steps_max=s[1], samples=s[2], missing=s[3], sum_abs_err=s[4])
  if "torch" in arms:
    d = scores.done
    out["torch_last_window"] = dict(steps_min=float(d[1].min()), steps_max=float(d[1].max()), samples=float(d[2].sum()),
                                    missing=float(d[3].sum()), sum_abs_err=float(d[5].sum()))
  print(json.dumps(out))
  for env in envs.values():
    env.close()


if __name__ == "__main__":
  main()
