"""A new start time and new weather at an episode start, three ways on one MI355X.

65,536 R9 buildings on a clock table of one year of 5-minute rows, sinusoid weather per building.  Timed:
``reset_buildings(mask)`` with 1/64 of the buildings masked, and a full ``reset()``, each

  (a) without the attachment: the offsets and the weather stay what they are;
  (b) the host route in front: ``clock_set_offsets`` of a full [B] array and a host-to-device copy of the [B, 2] weather
      array (what ``BatchedEnvironment.set_start_offsets`` + ``set_weather`` do; the arrays built beforehand), then the
      reset;
  (c) with an ``EpisodeStarts`` attached (offset, low and high drawn): the reset draws on the device.

HIP events around the call on the current stream (they bracket the host work of (b) too: the device waits for it);
the arms alternate within a repetition, ``--repeats`` repetitions after ``--warmup``, median / minimum / maximum per
arm.  ``--timeline`` also times, on the host, the build of the year-long ``host_inputs.Timeline`` an environment would
attach (the benchmark itself uses a table of zeros: a reset reads no row).  One JSON line on stdout; no GPU, no result.

    python tools/bench_episode_starts.py [--buildings 65536] [--warmup 3] [--repeats 15] [--timeline]"""
from __future__ import annotations

import argparse
import datetime as dt
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402

YEAR_ROWS = 364 * 288


def event_ms(fn) -> float:
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0.record()
  fn()
  t1.record()
  t1.synchronize()
  return t0.elapsed_time(t1)


def summary(ms):
  return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def timeline_build_seconds(es) -> float:
  cfg = SimConfig.sb1()
  m = host_inputs.StepModels(host_inputs.BatchedSinusoidWeather([270.0], [290.0], 100.0), cfg.schedule(),
                             host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1),
                             host_inputs.ElectricityEnergyCost(), host_inputs.NaturalGasEnergyCost(),
                             dt.timedelta(seconds=cfg.time_step_sec), ("z",), 0.0)
  t0 = time.perf_counter()
  tl = host_inputs.Timeline(m, dt.datetime(2023, 1, 1), [0], 864, episode_starts=es)
  assert tl.n_rows == YEAR_ROWS + 864 + 2
  return time.perf_counter() - t0


def main() -> None:
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=65536)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--timeline", action="store_true")
  args = ap.parse_args()
  es = host_inputs.EpisodeStarts(offsets=host_inputs.UniformInt(0, YEAR_ROWS, step=288), weather_low=host_inputs.Uniform(268.0, 285.0),
                                 weather_high=host_inputs.Uniform(286.0, 305.0), seed=11)
  out = {}
  if args.timeline:
    out["timeline_build_s"] = timeline_build_seconds(es)
    out["timeline_rows"] = YEAR_ROWS + 864 + 2
  if not torch.cuda.is_available():
    if args.timeline:
      print(json.dumps(out))
      return
    raise SystemExit("bench_episode_starts needs a GPU: a reset's time is a device measurement")
  if not all(hasattr(_ffi.load(), name) for name in _ffi.EPISODE_STARTS_ENTRIES):
    raise SystemExit("the library has no sb_episode_starts_attach: rebuild it")
  B = args.buildings
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)   # R9
  cfg = SimConfig.sb1()
  rng = np.random.RandomState(1234)
  rows = np.zeros((YEAR_ROWS + 864 + 2, _ffi.SB_CLOCK_FIELDS))
  mask = np.zeros(B, dtype=bool)
  mask[::64] = True
  new_offsets = (rng.randint(0, 365, size=B) * 288).astype(np.int32)
  new_lohi = np.stack([rng.uniform(268.0, 285.0, size=B), rng.uniform(286.0, 305.0, size=B)], axis=1)

  def make():
    sim = BatchedSimulator(plan, cfg, B, 100.0)
    sim.clock_attach(rows, np.zeros(B, dtype=np.int32))
    lohi = torch.tensor(np.stack([np.full(B, 273.0), np.full(B, 283.0)], axis=1), dtype=torch.float64, device=sim.tdev).contiguous()
    return sim, lohi

  plain, plain_lohi = make()
  plain.reset()
  arms = {"a_no_starts": (lambda: plain.reset_buildings(mask), lambda: plain.reset())}

  def host_route(reset):
    plain.clock_set_offsets(new_offsets)
    plain_lohi.copy_(torch.from_numpy(new_lohi))
    reset()

  arms["b_host_route"] = (lambda: host_route(lambda: plain.reset_buildings(mask)), lambda: host_route(plain.reset))
  drawn, drawn_lohi = make()
  drawn.episode_starts_attach(es, weather_lohi=drawn_lohi)
  drawn.reset()
  arms["c_episode_starts"] = (lambda: drawn.reset_buildings(mask), lambda: drawn.reset())
  out.update(buildings=B, plan=list(plan.shape), masked=int(mask.sum()), kernel=plain.launch_info["kernel"],
             device=torch.cuda.get_device_name(0))
  for which, name in ((0, "reset_buildings"), (1, "reset")):
    ms = {arm: [] for arm in arms}
    for rep in range(args.warmup + args.repeats):
      for arm, fns in arms.items():   # the arms alternate inside a repetition
        t = event_ms(fns[which])
        if rep >= args.warmup:
          ms[arm].append(t)
    out[name] = {arm: summary(v) for arm, v in ms.items()}
  plain.close()
  drawn.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
