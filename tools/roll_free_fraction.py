"""roll_free_fraction.py -- how many of k_sweep_roll's periods could run "free" on the bench workload (CPU only).

A period of k_sweep_roll finishes sweep k of a building's step and starts sweep k+1.  Its window copies and its
max|delta| exist only for the case that sweep k is the step's last one.  At the period's top sweep k has already
finished its upper-left triangle {(l, c): c <= 62 - l} (rows and columns counted inside the exterior ring), and the
travelling accumulators hold those columns' partial max|delta|.  If that partial maximum is above the convergence
threshold (high 32 bits strictly greater), the whole sweep's is, so sweep k is not the last one (unless the iteration
limit ends the step) and the period needs neither copies nor a measurement.  For a step's first sweep the ring's
|delta| (every exterior cell outside the trim box becomes t_amb) proves the same.

This script replays bench.py's headline workload (R9, seed-7 initial temperatures, seeded U[-1,1]^2 actions, sinusoid
weather, step-function occupancy) on the CPU oracle, sweep by sweep, and counts the periods that such a test would let
run free: per step, for the timed window (steps 12..35) and for the warm-up.  NumPy + oracle/sb_oracle.c, no GPU.

  python tools/roll_free_fraction.py [--buildings 256] [--steps 36] [--out profiles/roll_free_fraction.txt]
"""
from __future__ import annotations

import argparse
import datetime as dt
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402
from sbsim_amd import host_inputs  # noqa: E402
from sbsim_amd.environment import SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402

K_WIN = 63   # step_roll.hip kWin: lanes 0..62 have started the next sweep when a period ends


def hi32(x: float) -> int:
  """High word of a non-negative double: what the kernel's 32-bit decisions compare."""
  return int(np.float64(x).view(np.uint64) >> np.uint64(32))


def oracle_params(c: SimConfig) -> "orc.OracleParams":
  return orc.OracleParams(
      dt=c.time_step_sec, conv_threshold=c.convergence_threshold, iter_limit=c.iteration_limit,
      vav_max_air_flow=c.vav_max_air_flow_rate, vav_max_water_flow=c.vav_reheat_max_water_flow_rate,
      ahu_recirc=c.ahu_recirculation, ahu_heat_sp=c.ahu_heating_air_temp_setpoint,
      ahu_cool_sp=c.ahu_cooling_air_temp_setpoint, ahu_dp=c.ahu_fan_differential_pressure,
      ahu_eff=c.ahu_fan_efficiency, blr_setpoint=c.boiler_reheat_water_setpoint,
      blr_head=c.boiler_water_pump_differential_head, blr_pump_eff=c.boiler_water_pump_efficiency,
      comfort_lo=c.comfort_temp_window[0], comfort_hi=c.comfort_temp_window[1],
      eco_lo=c.eco_temp_window[0], eco_hi=c.eco_temp_window[1],
      blr_heating_rate=c.boiler_heating_rate, blr_cooling_rate=c.boiler_cooling_rate, ahu_has_weather=1)


def trim_box(plan: FloorPlan):
  """Bounding box of the cells that are not exterior space: what the sweep kernels keep in registers."""
  inside = ~np.asarray(plan.exterior_space, dtype=bool).reshape(plan.shape)
  xs, ys = np.nonzero(inside.any(axis=1))[0], np.nonzero(inside.any(axis=0))[0]
  return xs[0], xs[-1] + 1, ys[0], ys[-1] + 1


def step_sweeps(oplan, prev, q, t_amb, h, dt_, n_sweeps, box, tri):
  """Replays the n_sweeps sweeps of one building-step; per sweep: (proof value at the period's top, max|delta|)."""
  x0, x1, y0, y1 = box
  H, W = oplan.H, oplan.W
  est = prev.copy()
  ring = np.ones((H, W), bool)
  ring[x0:x1, y0:y1] = False
  out = []
  for k in range(n_sweeps):
    old = est.copy()
    md = orc.sweep(oplan, prev, est, q, t_amb, h, dt_)
    d = np.abs(est - old).reshape(H, W)
    inner = d[x0:x1, y0:y1]
    proof = float(inner[:tri.shape[0], :tri.shape[1]][tri].max())
    if k == 0 and ring.any():
      proof = max(proof, float(d[ring].max()))
    out.append((proof, md))
  return out, est


def main() -> None:
  ap = argparse.ArgumentParser()
  ap.add_argument("--buildings", type=int, default=256)
  ap.add_argument("--steps", type=int, default=36)
  ap.add_argument("--warmup", type=int, default=12)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roll_free_fraction.txt"))
  args = ap.parse_args()
  B, K, W0 = args.buildings, args.steps, args.warmup

  cfg = SimConfig.sb1()
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  oplan = orc.OraclePlan(plan.conductivity, plan.density, plan.heat_capacity, plan.exterior_space,
                         plan.zone_cell_lists(), plan.diffusers, plan.cv_size_cm, plan.floor_height_cm)
  oprm = oracle_params(cfg)
  H, W = plan.shape
  box = trim_box(plan)
  rows, cols = box[1] - box[0], box[3] - box[2]
  ll, cc = np.meshgrid(np.arange(min(rows, K_WIN)), np.arange(min(cols, K_WIN)), indexing="ij")
  tri = cc <= K_WIN - 1 - ll   # lane l has finished columns 0 .. 62 - l at the period's top
  thr_hi = hi32(cfg.convergence_threshold)

  rs = np.random.RandomState(7)
  t_init = np.clip(294.0 + rs.randn(max(B, 1)), 285.0, 305.0)[:B]
  acts = np.random.RandomState(1234).uniform(-1.0, 1.0, size=(K, B, 2)).astype(np.float32)
  twins = [orc.OracleBuilding(oplan, oprm, 0.0, reset_temps=np.full(H * W, float(t_init[b]))) for b in range(B)]
  for tw in twins:
    tw.observe_boiler(0.0)

  weather = host_inputs.WeatherController(273.0, 283.0, convection_coefficient=100.0)
  occupancy = host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1,
                                                holiday_calendar="us")
  schedule = cfg.schedule()
  elec, gas = host_inputs.ElectricityEnergyCost(holiday_calendar="us"), host_inputs.NaturalGasEnergyCost()
  step_iv = dt.timedelta(seconds=cfg.time_step_sec)
  lo, hi = cfg.action_ranges
  ts, prev_ts = dt.datetime(2023, 7, 6, 7, 0, 0), None

  periods = np.zeros(K, dtype=np.int64)   # all periods (= sweeps) of the step, over the buildings
  free = np.zeros(K, dtype=np.int64)      # those that the top test proves unfinished
  mism = 0
  for t in range(K):
    nxt = ts + step_iv
    t_now, t_next = weather.get_current_temp(ts), weather.get_current_temp(nxt)
    start_utc = host_inputs.reward_start_time_utc(nxt)
    e_price, e_carbon = elec.rates(start_utc)
    g_price, g_carbon = gas.rates(start_utc)
    occ = occupancy.average_zone_occupancy("", nxt, nxt + step_iv)
    for b, tw in enumerate(twins):
      a = acts[t, b]
      native = [np.float32((float(a[0]) + 1.0) / 2.0 * (lo[1] - lo[0]) + lo[0]),
                np.float32((float(a[1]) + 1.0) / 2.0 * (hi[1] - hi[0]) + hi[0])]
      prev, q = tw.temp.copy(), tw.input_q.copy()   # the sweeps run on the heat the PREVIOUS step's VAVs set
      o = tw.step(now_ts=300.0 * t, t_amb_now=t_now, h_conv=100.0, t_amb_next=t_next,
                  comfort_now=bool(schedule.is_comfort_mode(ts)),
                  comfort_prev=prev_ts is not None and bool(schedule.is_comfort_mode(prev_ts)),
                  comfort_next=bool(schedule.is_comfort_mode(nxt)), occupancy=occ, e_price=e_price,
                  e_carbon=e_carbon, g_price=g_price, g_carbon=g_carbon, action=native)
      n = o["n_sweeps"]
      sw, est = step_sweeps(oplan, prev, q, t_now, 100.0, cfg.time_step_sec, n, box, tri)
      mism += int(not np.array_equal(est, tw.temp))
      for k, (proof, md) in enumerate(sw):
        is_free = hi32(proof) > thr_hi and k + 1 < cfg.iteration_limit
        assert not is_free or k + 1 < n, "a proven sweep must not be the step's last one"
        free[t] += int(is_free)
      periods[t] += n
    prev_ts, ts = ts, nxt
    print(f"step {t:2d}: {periods[t] / B:6.2f} sweeps/building, free {free[t] / periods[t]:.3f}", flush=True)

  timed = slice(W0, K)
  lines = [
      "k_sweep_roll: share of periods that the top-of-period test proves unfinished (CPU oracle replay)",
      f"command: python tools/roll_free_fraction.py --buildings {B} --steps {K} --warmup {W0}",
      f"workload: bench.py's headline (R9 {H}x{W}, seed-7 initial temperatures, seeded U[-1,1]^2 actions), {B} buildings",
      f"test: max|delta| over the triangle c <= 62 - l inside the ring (first sweep: also the ring's) with high word > "
      f"the threshold's (0x{thr_hi:08x}, {cfg.convergence_threshold} K), and sweep + 1 < iteration limit",
      f"replayed grids that differ from the oracle's own step: {mism}",
      "",
      "step  sweeps/building  free periods  share",
  ]
  for t in range(K):
    lines.append(f"{t:4d}  {periods[t] / B:15.2f}  {free[t]:12d}  {free[t] / periods[t]:.3f}")
  lines += ["",
            f"warm-up (steps 0..{W0 - 1}): {periods[:W0].sum() / (B * max(W0, 1)):.2f} sweeps/building-step, "
            f"free share {free[:W0].sum() / max(periods[:W0].sum(), 1):.3f}",
            f"timed window (steps {W0}..{K - 1}): {periods[timed].sum() / (B * (K - W0)):.2f} sweeps/building-step, "
            f"free share {free[timed].sum() / periods[timed].sum():.3f}",
            f"overall: free share {free.sum() / periods.sum():.3f}",
            "go / no-go: a share of the timed window below 1/3 means a saving under 3 % of the kernel's time"]
  text = "\n".join(lines) + "\n"
  with open(args.out, "w") as fh:
    fh.write(text)
  print(text)


if __name__ == "__main__":
  main()
