"""CPU checks of tests/crossed_batches.py: the case table is a pairwise covering array, the plan and the planner's choices
are what the cases were sized for, every crossed feature changes what the twins compute, the inputs keep every exact
comparison of tests/test_crossed_batches_gpu.py away from a decision's edge, and the twin with every factor off is the
reference's own recorded rollout.  Oracle and host code only."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

from sbsim_amd import _ffi, host_inputs
from sbsim_amd.environment import BatchedSimulator, SimConfig
from tests import crossed_batches as cb
from tests.golden_util import load, oracle_params
from tests.threshold_cases import floor_plan
from tests.twins import native_value, plan_info

SB_KERNEL_LDS = 0
REGISTER_KERNELS = (1, 2, 3, 4, 5)   # sb_sweep_kernel: k_sweep_reg (one / two wavefronts), roll, two, band
ALL = list(cb.CASES)


def _steps(name, trace=False):
  """[(op, [B] results)] of the case's step operations, in order."""
  return [(op, res) for op, res in cb.expected(name, trace) if op.kind == "step"]


# ---------------------------------------------------------------- the table
def test_every_allowed_pair_of_levels_is_in_some_case():
  missing = cb.all_pairs() - cb.forbidden_pairs() - cb.covered_pairs()
  assert not missing, sorted(sorted(m) for m in missing)
  assert 10 <= len(cb.CASES) <= 14
  for name, case in cb.CASES.items():
    assert set(case) == set(cb.FACTORS) and all(case[f] in cb.FACTORS[f] for f in case), name


def test_the_named_cases_are_there_and_cross_what_they_say():
  want = {
      "dollars-on-the-clock": dict(reward="dollars", time="start_offsets", params="building_params"),
      "materials-on-calendars": dict(materials="building_materials", time="calendars", params="building_params",
                                     weather="sinusoid"),
      "episodes-with-rejections": dict(episodes="per_building", time="start_offsets", rejection="mask", actions="dampers"),
      "histograms-per-building": dict(observation="histogram", params="building_params", time="start_offsets",
                                      occupancy="device"),
  }
  assert set(cb.NAMED) <= set(cb.CASES)
  for name, levels in want.items():
    assert cb._holds(levels, cb.CASES[name]), name
  # everything: every factor off its first level, but for what the refusals take away (episodes) and the kernel factor,
  # which a materials handle does not have
  e = cb.CASES["everything"]
  off = [f for f in cb.FACTORS if e[f] == cb.FACTORS[f][0]]
  assert off == ["episodes"] and e["lifecycle"] == "snapshot_fork" and e["kernel"] == "lds"


def test_the_refused_pairs_are_exactly_the_modules_list():
  covered = cb.covered_pairs()
  assert cb.all_pairs() - covered == cb.forbidden_pairs()           # nothing else is left out, nothing refused is run
  for name, case in cb.CASES.items():
    for levels, _ in cb.REFUSED:
      assert not cb._holds(levels, case), (name, levels)
    for levels in cb.NOT_A_PAIR:
      assert not cb._holds(levels, case), (name, levels)
  assert [sorted(r[0]) for r in cb.REFUSED] == [["episodes", "occupancy"], ["episodes", "occupancy", "time"],
                                                ["episodes", "lifecycle"]]
  # the messages are the library's own (environment.py raises them; the GPU test asserts that it does)
  import inspect
  from sbsim_amd import environment
  src = inspect.getsource(environment)
  assert "per_building_episodes: BatchedRandomizedArrivalDepartureOccupancy is not supported" in src
  assert "is not supported with per_building_episodes: the per-building episode positions are not in " in src


# ---------------------------------------------------------------- the plan and the planner
def test_the_plan_is_17_by_29_with_six_zones_and_an_odd_cell_count():
  sc = cb.scenario("dollars-on-the-clock")
  plan = sc.plan
  assert plan.shape == (17, 29) and plan.n_zones == 6 and plan.shape[0] * plan.shape[1] == 493
  assert cb.B == 67 and cb.T == 12 and cb.B % 64 == 3 and cb.B % 16 == 3
  cp = plan.compile(300.0, cb.H_CONV)
  assert (cp.H, cp.W, cp.Z) == (17, 29, 6) or (cp.H, cp.W, cp.Z) == (15, 27, 6)   # (with or without the exterior ring)
  rc, info = plan_info(plan, n_obs=sc.layout.O, n_buildings=cb.B)
  assert rc == 0 and info["kernel"] in REGISTER_KERNELS and info["path"] == 1, info


@pytest.mark.parametrize("name", ALL)
def test_the_planner_picks_the_kernel_the_case_names(name, monkeypatch):
  sc = cb.scenario(name)
  monkeypatch.delenv("SBSIM_FORCE_LDS_PATH", raising=False)
  for k, v in sc.switches:
    monkeypatch.setenv(k, v)
  if sc.bmaterials is None:
    kinds = []
    for plan in (sc.plan, sc.plan.transposed()):
      rc, info = plan_info(plan, n_obs=sc.layout.O, n_buildings=cb.B)
      assert rc == 0, _ffi.load().sb_last_error()
      kinds.append(info["kernel"])
    if sc.case["kernel"] == "lds":
      assert sc.switches and kinds == [SB_KERNEL_LDS] * 2, kinds
    else:
      assert not sc.switches and all(k in REGISTER_KERNELS for k in kinds), kinds
  else:   # sb_plan_info_materials: a materials handle runs on k_sweep_lds or not at all
    assert not sc.switches and sc.case["kernel"] == "lds"
    slot_ids, table = sc.plan.material_slots()
    assert sc.material_sets.shape == (cb.B, len(table), 3)
    _, keep, pd_, sd_ = BatchedSimulator._describe_structural(sc.plan, 300.0, cb.H_CONV, (slot_ids, table))
    info = _ffi.LaunchInfo()
    rc = _ffi.materials_entry("sb_plan_info_materials")(C.byref(pd_), sc.layout.O, cb.B, C.byref(info))
    assert rc == 0 and info.kernel == SB_KERNEL_LDS, (rc, _ffi.load().sb_last_error())


# ---------------------------------------------------------------- every feature bites
@pytest.mark.parametrize("name", ALL)
def test_every_feature_of_the_case_bites(name):
  sc, case = cb.scenario(name), cb.CASES[name]
  steps = _steps(name)
  assert len(steps) == sc.n_steps and len(steps[0][1]) == cb.B
  # thermostats: at least two modes among the buildings' zones on at least two steps
  assert sum(len({int(m) for r in res for m in r["mode"]}) >= 2 for _, res in steps) >= 2
  # a rejected (building, step): -inf, modes and dampers as they were
  prev = [None] * cb.B
  n_rejected = 0
  for op, res in cb.expected(name):
    if op.kind == "step":
      for b, r in enumerate(res):
        rej = op.rejected is not None and bool(op.rejected[b])
        if rej:
          n_rejected += 1
          assert r["reward"] == float("-inf") and not r["accepted"], (op.row, b)
          if prev[b] is not None and r["step_type"] != cb.STEP_LAST:
            assert np.array_equal(r["mode_now"], prev[b][0]) and np.array_equal(r["damper_now"], prev[b][1]), (op.row, b)
        elif sc.bad_command is not None and (op.row, b) == sc.bad_command[:2]:   # the command outside [0, 1]
          assert r["reward"] == float("-inf") and not r["accepted"], (op.row, b)
        else:
          assert np.isfinite(r["reward"]) and r["accepted"], (op.row, b)
        prev[b] = (r["mode_now"], r["damper_now"])
    elif op.kind in ("reset_buildings", "restore", "fork"):
      prev = [None] * cb.B   # (the state moved between two steps)
  if case["rejection"] == "mask":
    assert n_rejected >= 20
    masks = [op.rejected for op, _ in steps if op.rejected is not None]
    assert len(masks) == 2
    if sc.per_building:   # one of the two steps is the step after some buildings' own reset
      assert (masks[1] & sc.reset_mask).any() and (masks[1] & ~sc.reset_mask).any()
  else:
    assert n_rejected == 0
  if case["actions"] == "dampers":
    row, b, col = sc.bad_command
    assert not 0.0 <= float(native_value(sc.actions[row, b, col], 0.0, 1.0)) <= 1.0
    others = np.delete(sc.actions[:, :, 3:].reshape(-1), np.ravel_multi_index((row, b, col - 3), sc.actions[:, :, 3:].shape))
    assert (np.abs(others) <= 1.0).all()
    bad = [r for op, res in steps if op.row == row for r in [res[b]]]
    assert bad and bad[0]["reward"] == float("-inf")
    # the commands are what the dampers show
    assert any(0.1 < d < 1.0 for _, res in steps for r in res for d in r["damper"])
  # time per building: the comfort flags differ between buildings on some step, and enough buildings cross a switch
  if case["time"] != "shared":
    assert any(len({r["comfort"][0] for r in res}) == 2 for _, res in steps)
    crossing = sum(len({f for _, res in steps for f in res[b]["comfort"]}) == 2 for b in range(cb.B))
    # the replay trace holds ten hours, i.e. one switch of one schedule: the twelve positions before it are all that can
    # cross (ten with episodes of at most nine steps); otherwise a third of the batch
    assert crossing >= (10 if case["weather"] == "replay" else (cb.B + 2) // 3), crossing
    assert len({tw.start for tw in sc.twins()}) == cb.B
  # rewards of two buildings with equal actions and initial grids differ once their rows do
  if case["params"] != "none" or case["materials"] != "none":
    assert any(res[0]["reward"] != res[1]["reward"] for _, res in steps)
  if case["reward"] == "dollars":
    assert all(r["reward"] != r["regret"] for _, res in steps for r in res if np.isfinite(r["reward"]))
    assert all(r["dollars"] is not None for _, res in steps for r in res)
  # histograms: fractions of the six zones; in each of them at least a tenth of the run's rows (80 of 804) spread over two bins or
  # more, on two steps of three at least (buildings whose six zones all call for heat have one damper bin whatever the
  # edges, and on a cold morning that is every building of some steps: "every row" is not a property of the physics)
  if sc.hist:
    lay = sc.layout
    for meas, bins in cb.HIST_PARAMS:
      cols = [i for i, f in enumerate(lay.fields) if f.startswith(meas + "_h_")]
      assert len(cols) == len(bins)
      spread = []
      for op, res in steps:
        rows = np.stack([r.get("final_obs", r["obs"])[cols] for r in res])
        assert np.abs(rows.sum(axis=1) - 1.0).max() < 1e-6 and set(np.round(rows * 6).reshape(-1)) <= set(range(7))
        spread.append(((rows > 0).sum(axis=1) >= 2).mean())
      assert np.mean(spread) >= 0.1 and np.mean(np.array(spread) > 0) >= 2 / 3, (meas, spread)
  # device occupants: the counts differ between buildings
  if case["occupancy"] == "device":
    assert any(len({r["n_occ"] for r in res}) >= 2 for _, res in steps)
    assert any(r["occupancy"].max() > 0 for _, res in steps for r in res)
  # episodes per building: everybody ends an episode of its own
  if sc.per_building:
    assert 3 <= sc.episode_steps.min() and sc.episode_steps.max() <= 9 and len(set(sc.episode_steps.tolist())) == 7
    for b in range(cb.B):
      assert any(res[b]["step_type"] == cb.STEP_LAST for _, res in steps), b
  else:
    assert all(r["step_type"] == cb.STEP_MID for _, res in steps for r in res)
  if case["lifecycle"] != "none":
    assert len(set(sc.fork_src.tolist())) < cb.B and [op.kind for op in sc.program].count("fork") == 1


# ---------------------------------------------------------------- margins: what makes exact comparison legitimate
@pytest.mark.parametrize("name", ALL)
def test_no_decision_of_the_case_sits_on_its_edge(name):
  """Conditions on the inputs: should one fail, change the seeds or the offsets, never the margin."""
  sc = cb.scenario(name)
  thr = sc.config.convergence_threshold
  lay = sc.layout
  for op, res in cb.expected(name, trace=True):
    if op.kind not in ("step", "reset", "reset_buildings"):
      continue
    for b, r in enumerate(res):
      if r is None:
        continue
      if op.kind == "step":
        rejected = op.rejected is not None and bool(op.rejected[b])
        if not rejected:   # the thermostat's three thresholds (thermostat.py:76-112) on the pre-update zone means
          lo, hi = r["window_now"]
          for edge in (lo, hi, 0.5 * (hi - lo) + lo):
            assert np.abs(r["zone_temp_pre"] - edge).min() >= 1e-6, (op.row, b, edge)
        md = r["max_delta"]
        assert len(md) == r["n_sweeps"] and (np.abs(md - thr) > 1e-9 * thr).all(), (op.row, b)
        lo, hi = r["window_next"]   # the productivity's branches, on the float32 values the reward sees
        t32 = r["zone_temp_post"].astype(np.float32).astype(np.float64)
        for edge in (float(np.float32(lo)), float(np.float32(hi))):
          assert np.abs(t32 - edge).min() >= 1e-4, (op.row, b, edge)
      if sc.hist:
        for meas, bins in cb.HIST_PARAMS:   # (a step's row before an own reset and the row after it: both are binned)
          for native in [r["native"]] + ([r["first_native"]] if "first_native" in r else []):
            v = lay.hist_inputs(native)[meas]
            for edge in bins:   # (relative to the edge; the dampers' lowest edge is 0: absolute there)
              assert (np.abs(v - edge) > 1e-5 * (abs(edge) if edge else 1.0)).all(), (op.kind, op.row, b, meas, edge)


# ---------------------------------------------------------------- the twin against the reference's recorded rollout
def _ulp32(a, b):
  a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
  b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
  return np.abs(a - b)


def test_the_twin_with_every_factor_off_is_the_reference_rollout():
  """h2_sb1_r9_random.npz, its first 12 steps: sweep counts equal, rewards within 2 float32 steps and rates within 1
  (the bounds of tests/test_oracle_golden.py::test_h2_one_day_rollout), the observation's device columns -- the golden
  holds the proto's float32 native values -- within one float32 step (np.log / np.exp in the boiler's fields)."""
  g = load("h2_sb1_r9_random.npz")
  plan = floor_plan("R9")
  cfg = SimConfig.sb1()
  zone_names = [str(z) for z in g["zone_names"]]
  layout = cb.ObsLayout(zone_names, {}, None, False)
  assert [n for n in layout.sources] == [str(n) for n in g["obs_names"]]
  start = dt.datetime.fromtimestamp(int(g["ts_seconds"][0]), tz=dt.timezone.utc).replace(tzinfo=None)
  models = host_inputs.StepModels(
      host_inputs.WeatherController(273.0, 283.0, convection_coefficient=100.0),
      host_inputs.SetpointSchedule(6, 19, (294, 297), (289, 298)),
      host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1, None),
      host_inputs.ElectricityEnergyCost(holiday_calendar=None), host_inputs.NaturalGasEnergyCost(), cb.DT,
      tuple(zone_names), 0.0)
  t0 = float(g["initial_temp"])
  tw = cb.Twin(plan=plan, h_conv=float(g["h_conv"]), params=oracle_params(g["params_json"]), start=start, models=models,
               episode_steps=288, discount=1.0, reward_function=None, layout=layout, action_names=cfg.action_names,
               action_zones=cfg.action_zones, action_ranges=cfg.action_ranges,
               init_grid=np.full(plan.shape[0] * plan.shape[1], t0), initial_temp=t0, occupants=None)
  first = tw.reset()
  assert first["step_type"] == cb.STEP_FIRST and first["obs"].shape == (layout.O,)
  for t in range(cb.T):
    r = tw.step(g["actions_norm"][t], False)
    assert r["n_sweeps"] == int(g["n_sweeps"][t]) and r["converged"] == 1, t
    assert np.array_equal(r["zone_temp_post"], g["zone_temp_post"][t]), t
    assert _ulp32(r["rates"], g["rates"][t]).max() <= 1, (t, r["rates"], g["rates"][t])
    assert _ulp32(r["reward"], g["reward"][t]) <= 2, (t, r["reward"], g["reward"][t])
    assert _ulp32(r["obs"][:layout.n_dev], g["obs"][t]).max() <= 1, (t, np.argmax(_ulp32(r["obs"][:layout.n_dev], g["obs"][t])))
    assert np.array_equal(r["mode"], g["mode"][t]) and r["step_type"] == cb.STEP_MID, t
    # the auxiliary features: the comfort flags and the head count of the reference's own run
    assert r["obs"][layout.n_dev + 4] == float(g["comfort_next"][t]) and r["obs"][layout.n_dev + 5] == float(g["comfort_soon"][t])
    assert r["obs"][layout.n_dev + 6] == np.float32(int(g["num_occupants"][t])), t
