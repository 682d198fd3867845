"""GPU: the ramp-up of a building's first sweep in k_sweep_roll (step_roll.hip: step_ramp and the A pass folded into it)
against the float64 instantiation alone (SBSIM_ROLL_EXACT=1) and against CPU-oracle twins.

The ramp-up is the first 63 steps of every building-step: lanes > s have not started at step s, A = ap * Tprev + g of a
slot is formed a few slots ahead of the step that reads it, and lane 63 collects no max |delta| yet.  A wrong A slot, a
wrong select or a dropped accumulator shows in the first sweep, so the cases are the smallest at which that sweep decides
something: a cold start (280 .. 300 K per building: tens of sweeps needed), three steps, 258 buildings (every resident
wavefront takes its first building through the ramp-up) -- and one batch of 2,048, where ramp-ups follow a hand-over.

  * iteration limit 1: the step IS the ramp-up plus one period -- nothing dilutes it;
  * iteration limit 2: the first period's top test reads the accumulators the ramp-up fed;
  * iteration limit 100: the step runs to convergence behind it;
  * one plan per slot count of the kernel (launch_info["sweep_steps"] = slots + 4 per tail row), and the ringless fixture;
  * SBSIM_DEBUG_FORCE_REDO=3: the float64 instantiation's ramp-up runs behind the fast kernel's, on the redo list.

Both instantiations share the update's arithmetic and its order: temperature grids, zone sums, sweep counts and converged
flags must be EQUAL bit for bit.  Sweep counts must be EQUAL to the twins', zone temperatures within 1e-8 K of theirs
(tests/twins.py's T_TOL) at every step.

The switches are read once in sb_create, so every configuration (default / exact / forced redo) is ONE child process (this
file with --worker) that runs its cases one after the other, under a time limit; a child that fails ends every test that
needs it and no further child is started."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

T_TOL = 1e-8   # K, zone temperatures against the oracle twins
N_TWINS = 3
STEPS = 3
SB_KERNEL_ROLL = 3
TIMEOUT_S = 300

# plan: (rooms, room shape) of rectangular_floor_plan, or "ringless"; launch_info["sweep_steps"]; whether the cold start
# keeps step 0 of EVERY building going for tens of sweeps.  It does on the plans with an exterior ring (observed on all five:
# every building of the batch reaches limits 1 and 2, the mean at limit 100 is above 10); the ringless plan's 280 .. 300 K
# buildings settle within two sweeps, most of them converged -- there the twins alone say what a step must do.
PLANS = {
    "r9": (((3, 3), (20, 30)), 96 + 8, True),       # 66 x 96 inside the ring: 96 slots, two tail rows
    "w81": (((2, 3), (20, 25)), 88, True),        # 45 x 81: 88 slots, pad lanes
    "w78": (((2, 3), (20, 24)), 80, True),        # 45 x 78: 80 slots, pad lanes
    "w63": (((2, 2), (20, 29)), 64, True),        # 45 x 63: 64 slots (all of A in LDS), pad lanes
    "h65": (((2, 2), (30, 33)), 72 + 4, True),        # 65 x 71: 72 slots, ONE tail row
    "ringless": ("ringless", 96 + 8, False),       # tests/golden/rect_building_cold200.npz: 66 x 96, no exterior ring
}
LIMITS = (1, 2, 100)
# case: (plan, buildings, iteration limit)
CASES = {f"{p}-limit{l}": (p, 258, l) for p in PLANS for l in LIMITS}
CASES["r9-2048"] = ("r9", 2048, 100)
REDO_CASE = "r9-limit100"


def _plan(spec):
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  if spec == "ringless":
    from tests.golden_util import load
    from tests.twins import ringless_plan
    return ringless_plan(load("rect_building_cold200.npz"))
  return FloorPlan.from_file_input(rectangular_floor_plan(*spec), Materials.sb1(), 10.0, 300.0)


def worker(names, out_dir: str, with_twins: bool) -> None:
  """The cases `names` under the switches of the environment: per case the sweep counts, converged flags and the first
  N_TWINS buildings' zone temperatures of every step, the last grids and zone temperatures, and the twins' sweep counts,
  converged flags and zone temperatures, into out_dir/<case>.npz."""
  import dataclasses
  import torch
  from sbsim_amd.environment import BatchedEnvironment, SimConfig
  from tests.twins import native_action, oracle_twin
  for case in names:
    pname, B, limit = CASES[case]
    plan = _plan(PLANS[pname][0])
    cfg = dataclasses.replace(SimConfig.sb1(), iteration_limit=limit)
    env = BatchedEnvironment(plan, B, config=cfg, device=0, holiday_calendar="us", collect_info=True, num_days_in_episode=3)
    H, W = plan.shape
    t_init = np.random.RandomState(7).uniform(280.0, 300.0, B)
    env.reset()
    env.sim.reset(temps=torch.tensor(t_init, dtype=torch.float64, device="cuda")[:, None].expand(B, H * W).contiguous())
    acts = np.random.RandomState(1234).uniform(-1.0, 1.0, size=(STEPS, B, 2)).astype(np.float32)
    n_twins = N_TWINS if with_twins else 0
    twins = [oracle_twin(plan, cfg, np.full(H * W, float(t_init[b]))) for b in range(n_twins)]
    for tw in twins:
      tw.observe_boiler(0.0)
    nsw, conv, zt, tw_nsw, tw_conv, tw_zt = [], [], [], [], [], []
    for t in range(STEPS):
      si = env.make_step_in(env.current_simulation_timestamp)
      env.step(torch.tensor(acts[t], device="cuda"))
      info = env.info.cpu().numpy()
      nsw.append(info[:, 4].astype(np.int64))
      conv.append(info[:, 5].astype(np.int64))
      zt.append(env.sim.zone_temps().cpu().numpy()[:N_TWINS])
      for b, tw in enumerate(twins):
        o = tw.step(now_ts=300.0 * t, t_amb_now=si.t_amb_now, h_conv=100.0, t_amb_next=si.t_amb_next,
                    comfort_now=bool(si.comfort_now), comfort_prev=si.comfort_prev == 1, comfort_next=bool(si.comfort_next),
                    occupancy=si.occupancy, e_price=si.e_price, e_carbon=si.e_carbon, g_price=si.g_price,
                    g_carbon=si.g_carbon, action=native_action(cfg, acts[t, b]))
        tw_nsw.append(o["n_sweeps"])
        tw_conv.append(int(o["converged"]))
        tw_zt.append(np.asarray(o["zone_temp_post"], dtype=np.float64))
    li = env.sim.launch_info
    np.savez(os.path.join(out_dir, case + ".npz"), nsw=np.array(nsw), conv=np.array(conv), zt=np.array(zt),
             twins=np.array(tw_nsw, dtype=np.int64).reshape(STEPS, n_twins),
             twins_conv=np.array(tw_conv, dtype=np.int64).reshape(STEPS, n_twins),
             twins_zt=np.array(tw_zt, dtype=np.float64).reshape(STEPS, n_twins, plan.n_zones),
             temps=env.sim.temps().cpu().numpy(), zones=env.sim.zone_temps().cpu().numpy(),
             kernel=int(li["kernel"]), sweep_steps=int(li["sweep_steps"]))
    env.close()


_CONFIGS = {   # tag -> (cases, switches, oracle twins)
    "default": (list(CASES), {}, True),
    "exact": (list(CASES), {"SBSIM_ROLL_EXACT": "1"}, False),
    "redo": ([REDO_CASE], {"SBSIM_DEBUG_FORCE_REDO": "3"}, False),
}
_children = {}   # tag -> directory of the child's results, or the failure's text


def _child(tag, tmp_path_factory):
  """The results of configuration `tag` (its child runs once per session)."""
  failed = [v for v in _children.values() if not os.path.isdir(v)]
  if tag not in _children and failed:   # nothing more is started on the GPU after a failed child
    pytest.fail("an earlier child failed:\n" + failed[0], pytrace=False)
  if tag not in _children:
    names, switches, with_twins = _CONFIGS[tag]
    out = str(tmp_path_factory.mktemp("ramp-" + tag))
    env = {k: v for k, v in os.environ.items() if k not in ("SBSIM_ROLL_FREE", "SBSIM_ROLL_EXACT", "SBSIM_DEBUG_FORCE_REDO")}
    env.update(switches)
    try:
      r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", ",".join(names), out, str(int(with_twins))],
                         env=env, cwd=ROOT, timeout=TIMEOUT_S, capture_output=True, text=True)
      _children[tag] = out if r.returncode == 0 else f"{tag}: child ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    except subprocess.TimeoutExpired:
      _children[tag] = f"{tag}: child ran into its time limit ({TIMEOUT_S} s)"
  if not os.path.isdir(_children[tag]):
    pytest.fail(_children[tag], pytrace=False)
  return _children[tag]


def _result(tag, case, tmp_path_factory):
  d = dict(np.load(os.path.join(_child(tag, tmp_path_factory), case + ".npz")))
  assert int(d["kernel"]) == SB_KERNEL_ROLL, (case, tag, d["kernel"])
  want = PLANS[CASES[case][0]][1]
  assert int(d["sweep_steps"]) == want, (case, tag, d["sweep_steps"], want)   # the instantiation meant
  return d


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _compare(fast, exact, case):
  """`fast` (the library's kernel, with its twins) against `exact` (the float64 instantiation alone)."""
  limit, cold_keeps_going = CASES[case][2], PLANS[CASES[case][0]][2]
  print(f"\n[{case}] sweeps per building-step: mean {fast['nsw'].mean():.2f}, max {fast['nsw'].max()}; worst zone temperature "
        f"against the twins {np.abs(fast['zt'] - fast['twins_zt']).max():.3e} K")
  assert np.array_equal(fast["nsw"], exact["nsw"]) and np.array_equal(fast["conv"], exact["conv"])
  assert _same_bits(fast["temps"], exact["temps"]), float(np.abs(fast["temps"] - exact["temps"]).max())
  assert _same_bits(fast["zones"], exact["zones"])
  assert fast["twins"].shape == (STEPS, N_TWINS)
  assert np.array_equal(fast["nsw"][:, :N_TWINS], fast["twins"]), (fast["nsw"][:, :N_TWINS], fast["twins"])
  assert np.array_equal(fast["conv"][:, :N_TWINS], fast["twins_conv"]), (fast["conv"][:, :N_TWINS], fast["twins_conv"])
  assert fast["zt"].shape == fast["twins_zt"].shape and np.abs(fast["zt"] - fast["twins_zt"]).max() < T_TOL
  # a step ends at the limit or by converging, never otherwise
  assert (fast["nsw"] >= 1).all() and (fast["nsw"] <= limit).all() and (fast["conv"][fast["nsw"] < limit] == 1).all()
  if cold_keeps_going and limit < 100:   # the limit ends step 0 of every building
    assert (fast["nsw"][0] == limit).all() and (fast["conv"][0] == 0).all()
  elif cold_keeps_going:
    assert fast["nsw"][0].mean() > 10 and (fast["nsw"] < 100).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_ramp_up_is_bit_identical_to_the_float64_instantiation_and_matches_the_twins(case, tmp_path_factory):
  pytest.importorskip("torch")
  from tests.parity import need_gpu
  need_gpu()
  _compare(_result("default", case, tmp_path_factory), _result("exact", case, tmp_path_factory), case)


@pytest.mark.gpu
def test_float64_ramp_up_behind_the_fast_one_on_the_redo_list(tmp_path_factory):
  """SBSIM_DEBUG_FORCE_REDO=3: every third building leaves the fast kernel at its stopping sweep and is redone by the
  float64 instantiation -- in the same step, from its untouched state.  Nothing may differ from the run without the switch."""
  pytest.importorskip("torch")
  from tests.parity import need_gpu
  need_gpu()
  fast, exact = _result("default", REDO_CASE, tmp_path_factory), _result("exact", REDO_CASE, tmp_path_factory)
  redo = _result("redo", REDO_CASE, tmp_path_factory)
  redo["twins"], redo["twins_conv"], redo["twins_zt"] = fast["twins"], fast["twins_conv"], fast["twins_zt"]   # (the same batch: the twins are the default child's)
  _compare(redo, exact, REDO_CASE)
  assert _same_bits(redo["temps"], fast["temps"]) and _same_bits(redo["zones"], fast["zones"])


if __name__ == "__main__":
  if len(sys.argv) == 5 and sys.argv[1] == "--worker":
    worker(sys.argv[2].split(","), sys.argv[3], sys.argv[4] == "1")
  else:
    raise SystemExit("usage: test_roll_ramp_gpu.py --worker CASE[,CASE...] OUT_DIR 0|1")
