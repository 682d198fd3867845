"""GPU: k_sweep_roll's free periods (step_roll.hip: a period whose finishing sweep is proven unfinished at its top keeps no
window copies and measures nothing) against the same kernel with every period measuring (SBSIM_ROLL_FREE=0), against the
float64 instantiation alone (SBSIM_ROLL_EXACT=1: today's schedule, the independent check) and against CPU-oracle twins.

The switches are read once in sb_create, so every configuration runs in a fresh child process (this file with
--worker), under a time limit; a child that fails ends the test.  Free and measuring periods share the update's
arithmetic and its order: temperature grids, zone sums and sweep counts must be EQUAL bit for bit, not close."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

# case: (plan, buildings, steps, start, iteration limit, oracle twins)
#   plan: (rooms, room shape) of rectangular_floor_plan, or "ringless" (tests/golden/rect_building_cold200.npz: no exterior ring)
#   start: "bench" = bench.py's seed-7 per-building temperatures; "cold" = 280..300 K per building (tens of sweeps in step 0)
CASES = {
    "bench": (((3, 3), (20, 30)), 4096, 40, "bench", 100, 4),
    "limit-1": (((3, 3), (20, 30)), 256, 3, "cold", 1, 3),
    "limit-2": (((3, 3), (20, 30)), 256, 3, "cold", 2, 3),
    "limit-3": (((3, 3), (20, 30)), 256, 3, "cold", 3, 3),
    "limit-100": (((3, 3), (20, 30)), 256, 3, "cold", 100, 3),
    "redo": (((3, 3), (20, 30)), 258, 6, "cold", 100, 3),
    "nr64-pad-lanes": (((2, 2), (20, 29)), 130, 5, "cold", 100, 3),    # 43 x 61 inside the ring: 64 slots, 21 pad lanes
    "nr80-pad-lanes": (((2, 3), (20, 25)), 130, 5, "cold", 100, 3),    # 43 x 79: 80 slots
    "ringless": ("ringless", 66, 4, "cold", 100, 0),
}
SB_KERNEL_ROLL = 3
TIMEOUT_S = 600


def _plan(spec):
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  if spec == "ringless":
    from tests.golden_util import load
    from tests.twins import ringless_plan
    return ringless_plan(load("rect_building_cold200.npz"))
  return FloorPlan.from_file_input(rectangular_floor_plan(*spec), Materials.sb1(), 10.0, 300.0)


def worker(case: str, out: str) -> None:
  """One configuration (the environment says which) of one case: sweep counts and converged flags of every step, the
  last grids and zone sums, and the twins' sweep counts, into `out`."""
  import dataclasses
  import torch
  from sbsim_amd.environment import BatchedEnvironment, SimConfig
  from tests.twins import native_action, oracle_twin
  spec, B, T, start, limit, n_twins = CASES[case]
  plan = _plan(spec)
  cfg = dataclasses.replace(SimConfig.sb1(), iteration_limit=limit)
  env = BatchedEnvironment(plan, B, config=cfg, device=0, holiday_calendar="us", collect_info=True, num_days_in_episode=3)
  H, W = plan.shape
  rs = np.random.RandomState(7)
  t_init = np.clip(294.0 + rs.randn(B), 285.0, 305.0) if start == "bench" else rs.uniform(280.0, 300.0, B)
  env.reset()
  env.sim.reset(temps=torch.tensor(t_init, dtype=torch.float64, device="cuda")[:, None].expand(B, H * W).contiguous())
  acts = np.random.RandomState(1234).uniform(-1.0, 1.0, size=(T, B, 2)).astype(np.float32)
  twins = [oracle_twin(plan, cfg, np.full(H * W, float(t_init[b]))) for b in range(n_twins)]
  for tw in twins:
    tw.observe_boiler(0.0)
  nsw, conv, tw_nsw = [], [], []
  for t in range(T):
    si = env.make_step_in(env.current_simulation_timestamp)
    env.step(torch.tensor(acts[t], device="cuda"))
    info = env.info.cpu().numpy()
    nsw.append(info[:, 4].astype(np.int64))
    conv.append(info[:, 5].astype(np.int64))
    tw_nsw.append([tw.step(now_ts=300.0 * t, t_amb_now=si.t_amb_now, h_conv=100.0, t_amb_next=si.t_amb_next,
                           comfort_now=bool(si.comfort_now), comfort_prev=si.comfort_prev == 1,
                           comfort_next=bool(si.comfort_next), occupancy=si.occupancy, e_price=si.e_price,
                           e_carbon=si.e_carbon, g_price=si.g_price, g_carbon=si.g_carbon,
                           action=native_action(cfg, acts[t, b]))["n_sweeps"] for b, tw in enumerate(twins)])
  li = env.sim.launch_info
  np.savez(out, nsw=np.array(nsw), conv=np.array(conv), twins=np.array(tw_nsw, dtype=np.int64).reshape(T, n_twins),
           temps=env.sim.temps().cpu().numpy(), zones=env.sim.zone_temps().cpu().numpy(), kernel=int(li["kernel"]))
  env.close()


def _run(case, tmp_path, tag, **switches):
  out = str(tmp_path / f"{case}-{tag}.npz")
  env = {k: v for k, v in os.environ.items() if k not in ("SBSIM_ROLL_FREE", "SBSIM_ROLL_EXACT", "SBSIM_DEBUG_FORCE_REDO")}
  env.update(switches)
  r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", case, out], env=env, cwd=ROOT,
                     timeout=TIMEOUT_S, capture_output=True, text=True)
  if r.returncode != 0:   # nothing more is started on the GPU after a failed child
    pytest.fail(f"{case} / {tag}: child ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", pytrace=False)
  d = dict(np.load(out))
  assert int(d["kernel"]) == SB_KERNEL_ROLL, (case, tag, d["kernel"])
  return d


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _compare(case, tmp_path, free_switches=None):
  """SBSIM_ROLL_FREE=1 (+ free_switches) against =0 against the float64 instantiation; -> the free run."""
  pytest.importorskip("torch")
  import torch
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  free = _run(case, tmp_path, "free", SBSIM_ROLL_FREE="1", **(free_switches or {}))
  meas = _run(case, tmp_path, "measuring", SBSIM_ROLL_FREE="0")
  exact = _run(case, tmp_path, "exact", SBSIM_ROLL_EXACT="1")
  assert np.array_equal(free["nsw"], meas["nsw"]) and np.array_equal(free["conv"], meas["conv"])
  assert _same_bits(free["temps"], meas["temps"]), float(np.abs(free["temps"] - meas["temps"]).max())
  assert _same_bits(free["zones"], meas["zones"])
  assert np.array_equal(free["nsw"], exact["nsw"]) and np.array_equal(free["conv"], exact["conv"])
  assert _same_bits(free["temps"], exact["temps"])   # EXACT changes only how max|delta| is kept
  n_twins = free["twins"].shape[1]
  assert np.array_equal(free["nsw"][:, :n_twins], free["twins"]), (free["nsw"][:, :n_twins], free["twins"])
  print(f"\n[{case}] sweeps per building-step: mean {free['nsw'].mean():.2f}, max {free['nsw'].max()}; "
        f"{json.dumps({k: list(v.shape) for k, v in free.items() if v.ndim})}")
  return free


@pytest.mark.gpu
def test_bench_like_batch_is_bit_identical_with_and_without_free_periods(tmp_path):
  """4,096 R9 buildings, 40 steps from bench.py's seed-7 start with seeded random actions."""
  free = _compare("bench", tmp_path)
  assert free["nsw"][0].mean() > 20 and free["nsw"][-1].mean() > 2   # steps with many free periods and the steady regime


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [1, 2, 3, 100])
def test_iteration_limit_ends_a_step_that_is_still_proven_above(limit, tmp_path):
  """A cold start needs tens of sweeps: limits 1..3 end step 0 while the top test still proves every sweep unfinished --
  the sweep that reaches the limit must run as a measuring period (its copies undo the started sweep)."""
  free = _compare(f"limit-{limit}", tmp_path)
  if limit < 100:
    assert (free["nsw"][0] == limit).all() and (free["conv"][0] == 0).all()
  else:
    # (a building that starts near the outside temperature needs few sweeps: the batch's mean is what shows the cold start)
    assert free["nsw"][0].min() > 3 and free["nsw"][0].mean() > 20 and (free["nsw"] < 100).all()


@pytest.mark.gpu
def test_forced_redo_list_together_with_free_periods(tmp_path):
  """SBSIM_DEBUG_FORCE_REDO=3: every third building leaves the fast kernel at its stopping sweep, behind free periods, and is
  redone by the float64 instantiation from its untouched state."""
  _compare("redo", tmp_path, {"SBSIM_DEBUG_FORCE_REDO": "3"})


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nr64-pad-lanes", "nr80-pad-lanes", "ringless"])
def test_other_instantiations_pad_lanes_and_no_exterior_ring(case, tmp_path):
  """NR = 64 and NR = 80 with fewer than 64 rows (pad lanes feed zeros to the accumulators), and a plan without an exterior
  ring (no ring |delta| in the first sweep's proof)."""
  _compare(case, tmp_path)


if __name__ == "__main__":
  if len(sys.argv) == 4 and sys.argv[1] == "--worker":
    worker(sys.argv[2], sys.argv[3])
  else:
    raise SystemExit("usage: test_roll_free_gpu.py --worker CASE OUT.npz")
