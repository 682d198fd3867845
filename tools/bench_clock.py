"""Times the R9 step of BASELINE.json configs[1] (65,536 buildings) with and without a calendar per building
(sb_clock_attach).  Two simulators in one process, one on sb_step_in's scalars and one on a clock whose offsets are all 0
and whose rows hold the same values, step alternately, one step each in turn: both compute the same numbers bit for bit
(checked), and the difference is the row gather in k_pre and k_post -- the sweep kernel is the same kernel with the same
arguments.  Each of the step's three launches is bracketed with HIP events (sb_step_phases); the medians per launch and of
the whole step are printed as one JSON line, with the time the host takes to build a timeline of --timeline-days days.

  python tools/bench_clock.py [--buildings 65536] [--steps 60] [--warmup 10] [--timeline-days 365]
"""
import argparse
import datetime as dt
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402

RATES = (3e-8, 1e-7, 1e-8, 5e-8)


def step_in(t: int) -> _ffi.StepIn:
  si = _ffi.StepIn()
  si.t_amb_now, si.t_amb_next = 278.0 + 0.01 * t, 278.0 + 0.01 * (t + 1)
  si.comfort_now = si.comfort_next = 1
  si.comfort_prev = 1 if t else -1
  si.has_action = 1
  si.occupancy = 10.0
  si.e_price, si.e_carbon, si.g_price, si.g_carbon = RATES
  return si


def rows(n: int) -> np.ndarray:
  """The table whose row r holds what step_in(r) says about instant r."""
  f = {name: i for i, name in enumerate(_ffi.CLOCK_FIELDS)}
  tab = np.zeros((n, _ffi.SB_CLOCK_FIELDS))
  tab[:, f["t_amb"]] = [278.0 + 0.01 * r for r in range(n)]
  tab[:, f["comfort"]] = 1.0
  tab[:, f["occupancy"]] = 10.0
  tab[:, f["e_price"]:f["g_carbon"] + 1] = RATES
  return tab


def timeline_seconds(days: int) -> float:
  """The host's time to build a Timeline of `days` days of SB1's 5-minute steps with the environment's default models."""
  cfg = SimConfig.sb1()
  step = dt.timedelta(seconds=cfg.time_step_sec)
  m = host_inputs.StepModels(host_inputs.WeatherController(273.0, 283.0, convection_coefficient=100.0), cfg.schedule(),
                             host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1),
                             host_inputs.ElectricityEnergyCost(), host_inputs.NaturalGasEnergyCost(), step, ("room_1",), 0.0)
  t0 = time.perf_counter()
  host_inputs.Timeline(m, dt.datetime(2023, 1, 1, tzinfo=dt.timezone.utc), [0], int(dt.timedelta(days=days) / step) - 2)
  return time.perf_counter() - t0


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=60, help="timed steps of each simulator")
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--timeline-days", type=int, default=365, help="0: do not time the host's timeline")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_clock.py needs a GPU")
  B = args.buildings
  cfg = SimConfig.sb1()
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  sims = {"no_clock": BatchedSimulator(plan, cfg, B, 12.0), "clock": BatchedSimulator(plan, cfg, B, 12.0)}
  n = args.warmup + args.steps
  sims["clock"].clock_attach(rows(n + 1), np.zeros(B, np.int32))
  dev = sims["clock"].tdev
  gen = torch.Generator(device=dev)
  gen.manual_seed(3)
  acts = torch.rand((n, B, 2), generator=gen, device=dev) * 2 - 1
  out = {mode: (torch.empty((B, sim.O), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                torch.empty((B, _ffi.SB_INFO_STRIDE), dtype=torch.float32, device=dev)) for mode, sim in sims.items()}
  ms = {mode: {"pre": [], "sweep": [], "post": [], "step": []} for mode in sims}
  for sim in sims.values():
    sim.reset()
  blank = _ffi.StepIn()
  blank.has_action = 1
  for t in range(n):
    sims["clock"].clock_seek(t, t - 1)
    for mode, sim in sims.items():   # one step of each in turn: clock drift and the sweeps' transient hit both alike
      si = blank if mode == "clock" else step_in(t)
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
    for a, b in zip(out["no_clock"], out["clock"]):
      assert torch.equal(a, b), "a clock whose rows hold the step's own scalars must not change a bit"
  res = {"buildings": B, "kernel": _ffi.SWEEP_KERNELS.get(sims["clock"].launch_info["kernel"], "?"),
         "timed_steps": args.steps, "table_bytes": 8 * _ffi.SB_CLOCK_FIELDS * (n + 1) + 4 * B}
  for mode, d in ms.items():
    for name, v in d.items():
      res[f"{mode}_{name}_ms"] = round(float(np.median(v)), 4)
  for name in ("pre", "sweep", "post", "step"):
    res[f"delta_{name}_ms"] = round(res[f"clock_{name}_ms"] - res[f"no_clock_{name}_ms"], 4)
  if args.timeline_days > 0:
    res["timeline_days"] = args.timeline_days
    res["timeline_host_seconds"] = round(timeline_seconds(args.timeline_days), 2)
  print(json.dumps(res))
  for sim in sims.values():
    sim.close()


if __name__ == "__main__":
  main()
