"""Start temperatures per building on the GPU (sb_initial_conditions_attach; host_inputs.InitialConditions through
BatchedSimulator, BatchedEnvironment, MixedBatchedEnvironment and HipSimulatorBuilding).

The yardstick of the reset kernels is the staging path they replace: a start through the attached conditions must be
bit for bit what reset(temps = the array materialised from start_temps) leaves, in every state layout.  The values
themselves are held to the reference (tests/golden/reset_temp_values.npz) and to per-building oracle twins.

67 buildings of 493 cells (tests/initial_conditions_cases.py); a few steps per case.

k_sweep_stream adds a building's zone sums with LDS atomics in the order they arrive: two handles in
equal states need not step to equal bits on it.  Its reset state is compared bit for bit like every layout's; its steps
at tests/parity.py's assert_close bar, as the snapshot and episode tests do for that kernel."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd import building_adapter as ba  # noqa: E402
from sbsim_amd.environment import (STEP_FIRST, STEP_LAST, BatchedEnvironment, BatchedSimulator,  # noqa: E402
                                   MixedBatchedEnvironment, SimConfig)
from sbsim_amd.host_inputs import InitialConditions  # noqa: E402
from tests import crossed_batches as cb  # noqa: E402
from tests import initial_conditions_cases as icc  # noqa: E402
from tests import test_crossed_batches_gpu as cbg  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import assert_close, need_gpu, step_buffers  # noqa: E402
from tests.twins import T_TOL, assert_step_matches, plan_from_npz, rates_match, step_in  # noqa: E402

B = icc.B
LDS, STREAM, JACOBI = 0, 6, 7   # sb_sweep_kernel
# name -> (environment switches, BatchedSimulator arguments, what the launch must report, steps bitwise)
LAYOUTS = {
    "register": ((), {}, lambda s: s.launch_info["path"] == 1 and not s.transposed, True),
    "lds": ((("SBSIM_FORCE_LDS_PATH", "1"),), {}, lambda s: s.launch_info["kernel"] == LDS, True),
    "stream": ((("SBSIM_FORCE_STREAM_PATH", "1"),), {}, lambda s: s.launch_info["kernel"] == STREAM, False),
    "jacobi": ((), dict(solver="jacobi_fp32"), lambda s: s.launch_info["kernel"] == JACOBI, True),
    "columns": ((), dict(orientation="columns"), lambda s: s.transposed and s.launch_info["kernel"] != JACOBI, True),
}
MASK = np.zeros(B, dtype=bool)
MASK[[0, 3, 4, 17, 31, 32, 33, 47, 63, 64, 66]] = True


def _sims(layout, monkeypatch, n=2):
  switches, kw, reports, _ = LAYOUTS[layout]
  for k, v in switches:
    monkeypatch.setenv(k, v)
  g = load("h2_sb1_r9_random.npz")
  fp, cfg = icc.plan(), icc.twin_config()
  sims = [BatchedSimulator(fp, cfg, B, float(g["h_conv"]), **kw) for _ in range(n)]
  for s in sims:
    assert reports(s), (layout, s.launch_info, s.transposed)
  return fp, g, sims


def _dev(a, dtype=torch.float64):
  return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _state(sim):
  return dict(temps=sim.temps(), zone_temps=sim.zone_temps(), scalars=sim.scalars(), modes=sim.modes())


def _assert_same_state(a, b, what, rows=None):
  sa, sb = _state(a), _state(b)
  for k in sa:
    x, y = (sa[k], sb[k]) if rows is None else (sa[k][rows], sb[k][rows])
    assert torch.equal(x, y), f"{what}: {k} differs by {(x.double() - y.double()).abs().max().item()}"


def _steps(sim, g, acts, n):
  """n steps on the golden's rows: [step][obs, rew, info, temps, scalars, modes, zone temps] (clones)."""
  obs, rew, info = step_buffers(sim)
  out = []
  for t in range(n):
    sim.step(_dev(acts[t], torch.float32), step_in(g, icc.ROW0 + t), obs, rew, info)
    out.append([x.clone() for x in (obs, rew, info, sim.temps(), sim.scalars(), sim.modes(), sim.zone_temps())])
  return out


# ---------------------------------------------------------------- 1. equal to the staging path
@pytest.mark.parametrize("variant", icc.VARIANTS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_start_through_the_conditions_is_the_staging_path_bit_for_bit(layout, variant, monkeypatch):
  need_gpu()
  fp, g, (a, b) = _sims(layout, monkeypatch)
  ic = icc.conditions(variant, fp.shape)
  a.initial_conditions_attach(ic)
  a.reset()
  want = icc.materialised(ic, np.zeros(B, int), fp.shape)
  b.reset(temps=_dev(want))
  _assert_same_state(a, b, f"{layout}/{variant}: reset")
  got = a.temps().cpu().numpy().reshape(B, -1)
  if layout == "jacobi":   # the stored grid is the float32 rounding of the float64 value, rounded once
    assert np.array_equal(got, want.astype(np.float32).astype(np.float64))
    assert not np.array_equal(got, want)
  else:
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
  assert a.initial_condition_episodes().tolist() == [1] * B
  acts = icc.actions(4, seed=8)
  ra, rb = _steps(a, g, acts, 4), _steps(b, g, acts, 4)
  if LAYOUTS[layout][3]:
    for t, (x, y) in enumerate(zip(ra, rb)):
      for k, (u, v) in enumerate(zip(x, y)):
        assert torch.equal(u, v), (layout, variant, t, k, float((u.double() - v.double()).abs().max()))
  else:
    assert_close(ra, rb)
  for s in (a, b):
    s.close()


def test_an_explicit_initial_temp_beside_a_base_is_refused():
  need_gpu()
  fp, cfg = icc.plan(), icc.twin_config()
  sim = BatchedSimulator(fp, cfg, B, 100.0)
  sim.initial_conditions_attach(icc.conditions("initial_temp", fp.shape))
  with pytest.raises(ValueError, match="two bases"):
    sim.reset(initial_temp=290.0)
  sim.reset()
  with pytest.raises(ValueError, match="two bases"):
    sim.reset_buildings(MASK, initial_temp=290.0)
  ic = icc.conditions("jitter", fp.shape)
  sim.initial_conditions_attach(ic)   # replaces: the counters start again
  assert sim.initial_condition_episodes().tolist() == [0] * B
  sim.reset(initial_temp=290.0)       # the jitter rides on the call's scalar
  want = icc.materialised(ic, np.zeros(B, int), fp.shape, initial_temp=290.0)
  assert np.array_equal(sim.temps().cpu().numpy().reshape(B, -1), want)
  with pytest.raises(ValueError, match=r"grids of shape \(17, 29\), the floor plan is \(29, 17\)"):
    BatchedSimulator(fp.transposed(), cfg, B, 100.0).initial_conditions_attach(icc.conditions("grids", fp.shape))
  with pytest.raises(ValueError, match="offset has 5 rows, the batch 67"):
    sim.initial_conditions_attach(InitialConditions(offset=np.zeros(5)))
  sim.close()


# ---------------------------------------------------------------- 2. episodes advance the draw
def test_every_reset_advances_the_buildings_episode():
  need_gpu()
  fp, cfg = icc.plan(), icc.twin_config()
  sim = BatchedSimulator(fp, cfg, B, 100.0)
  ic = icc.conditions("grids", fp.shape)
  sim.initial_conditions_attach(ic)
  grid = lambda: sim.temps().cpu().numpy().reshape(B, -1)
  sim.reset()
  first = grid()
  sim.reset()
  assert np.array_equal(grid(), icc.materialised(ic, np.ones(B, int), fp.shape))
  assert not np.array_equal(grid()[5], first[5])
  assert sim.initial_condition_episodes().tolist() == [2] * B
  # an explicit array wins, and the counters advance all the same
  own = np.full((B, fp.shape[0] * fp.shape[1]), 291.25)
  sim.reset(temps=_dev(own))
  assert np.array_equal(grid(), own) and sim.initial_condition_episodes().tolist() == [3] * B
  # the pair a checkpoint keeps the counters with: rewinding replays the first episode
  e = torch.arange(B, dtype=torch.int32, device="cuda") % 3
  sim.set_initial_condition_episodes(e)
  sim.reset()
  assert np.array_equal(grid(), icc.materialised(ic, np.arange(B) % 3, fp.shape))
  assert torch.equal(sim.initial_condition_episodes(), e + 1)
  sim.set_initial_condition_episodes(torch.zeros(B, dtype=torch.int32, device="cuda"))
  sim.reset()
  assert np.array_equal(grid(), first)
  with pytest.raises(ValueError, match=r"contiguous int32 \[67\]"):
    sim.set_initial_condition_episodes(torch.zeros(B, dtype=torch.int64, device="cuda"))
  # snapshots carry neither the conditions nor the counters
  st = sim.save_state()
  sim.reset()
  sim.reset()
  assert sim.initial_condition_episodes().tolist() == [3] * B
  sim.load_state(st)
  assert np.array_equal(grid(), first) and sim.initial_condition_episodes().tolist() == [3] * B
  sim.reset()
  assert np.array_equal(grid(), icc.materialised(ic, np.full(B, 3), fp.shape))
  sim.close()


def test_environment_snapshot_and_restore_leave_the_counters():
  need_gpu()
  fp = icc.plan()
  ic = icc.conditions("grids", fp.shape)
  env = BatchedEnvironment(fp, B, config=icc.twin_config(), holiday_calendar=None, initial_conditions=ic)
  assert env.initial_conditions is ic
  env.reset()
  snap = env.snapshot()
  acts = _dev(icc.actions(2)[0], torch.float32)
  env.step(acts)
  env.reset()
  assert env.sim.initial_condition_episodes().tolist() == [2] * B
  env.restore(snap)
  assert env.sim.initial_condition_episodes().tolist() == [2] * B
  assert np.array_equal(env.sim.temps().cpu().numpy().reshape(B, -1), icc.materialised(ic, np.zeros(B, int), fp.shape))
  env.fork(torch.arange(B, device="cuda").flip(0))
  assert env.sim.initial_condition_episodes().tolist() == [2] * B
  # a snapshot belongs to the conditions it was taken under
  env.set_initial_conditions(None)
  with pytest.raises(ValueError, match="another floor plan, configuration or generator set"):
    env.restore(snap)
  env.close()


# ---------------------------------------------------------------- 3. masked resets
@pytest.mark.parametrize("layout", ["register", "lds", "jacobi", "columns"])
def test_a_masked_reset_starts_the_masked_buildings_and_touches_nothing_else(layout, monkeypatch):
  need_gpu()
  fp, g, (a, b) = _sims(layout, monkeypatch)
  ic = icc.conditions("grids", fp.shape)
  acts = icc.actions(3, seed=9)
  for s in (a, b):
    s.initial_conditions_attach(ic)
    s.reset()
    _steps(s, g, acts, 3)
  e = torch.ones(B, dtype=torch.int32, device="cuda")
  e[torch.as_tensor(MASK.nonzero()[0][::2], device="cuda")] = 4   # some of the masked buildings are further on
  for s in (a, b):
    s.set_initial_condition_episodes(e)
  before = _state(a)
  keep = torch.as_tensor(np.nonzero(~MASK)[0], device="cuda")
  hit = torch.as_tensor(np.nonzero(MASK)[0], device="cuda")
  a.reset_buildings(np.zeros(B, dtype=bool))   # an all-zero mask: nothing, the counters included
  assert torch.equal(a.initial_condition_episodes(), e)
  for k, v in _state(a).items():
    assert torch.equal(v, before[k]), k
  a.reset_buildings(MASK)
  want = icc.materialised(ic, e.cpu().numpy(), fp.shape)
  b.reset_buildings(MASK, temps=_dev(want))   # the staging path: the full array, of which the masked rows are read
  _assert_same_state(a, b, f"{layout}: masked reset")
  after = _state(a)
  for k in after:
    assert torch.equal(after[k][keep], before[k][keep]), f"{layout}: an unmasked building's {k} changed"
  got = after["temps"].cpu().numpy().reshape(B, -1)[MASK]
  ref = want[MASK].astype(np.float32).astype(np.float64) if layout == "jacobi" else want[MASK]
  assert np.array_equal(got, ref)
  for s in (a, b):   # their own e, used and then incremented -- the masked ones alone, whichever source the values had
    assert torch.equal(s.initial_condition_episodes(), e + torch.as_tensor(MASK, device="cuda").to(torch.int32))
  assert after["temps"][hit].shape[0] == int(MASK.sum()) and MASK[0] and MASK[66]
  ra, rb = _steps(a, g, acts, 2), _steps(b, g, acts, 2)
  for t, (x, y) in enumerate(zip(ra, rb)):
    for k, (u, v) in enumerate(zip(x, y)):
      assert torch.equal(u, v), (layout, t, k)
  for s in (a, b):
    s.close()


def _episode_env(fp, ic, lengths, **kw):
  return BatchedEnvironment(fp, B, config=icc.twin_config(), holiday_calendar=None, collect_info=True,
                            num_days_in_episode=12 / 288, episode_steps=lengths, initial_conditions=ic, **kw)


def test_autoreset_starts_every_episode_from_the_buildings_own_grid():
  """A: the conditions attached; S: its twin whose restarts go through the staging path (reset_buildings with the
  materialised array -- an explicit array wins, the counters advance all the same): equal bit for bit at every step.  A
  restarted building's zone temperatures in its first observation are those of a FRESH environment reset to the same
  grid (the rest of that row carries the building's history: request counts, the boiler's action age)."""
  need_gpu()
  fp = icc.plan()
  ic = icc.conditions("grids", fp.shape)
  lengths = 2 + (np.arange(B) * 5) % 4   # 2 .. 5 steps
  a, s = _episode_env(fp, ic, lengths), _episode_env(fp, ic, lengths)
  e_host = np.zeros(B, int)

  def staged_restart(ended):
    temps = _dev(icc.materialised(ic, e_host, fp.shape))
    s.sim.reset_buildings(ended, restart_pos=s._cursor.pos, temps=temps)
    s._cursor.restart(ended)
    s.sim.clock_seek(*s._cursor.seek_args())
    si = _ffi.StepIn()
    s._device_inputs(si)
    s.sim.observe_buildings(ended, si, s._obs)

  s._restart = staged_restart
  ta, ts = a.reset(), s.reset()
  assert torch.equal(ta.observation, ts.observation)
  first_obs = ta.observation.clone()
  e_host += 1
  zone_cols = [i for i, n in enumerate(a.field_names) if n.endswith("zone_air_temperature_sensor")]
  assert len(zone_cols) == fp.n_zones
  acts = _dev(icc.actions(11, seed=12), torch.float32)
  restarts, last = np.zeros(B, int), None
  for t in range(11):
    ta, ts = a.step(acts[t]), s.step(acts[t])
    for x, y in ((ta.observation, ts.observation), (ta.reward, ts.reward), (ta.step_type, ts.step_type),
                 (a.final_observation, s.final_observation), (a.info, s.info), (a.sim.temps(), s.sim.temps())):
      assert torch.equal(x, y), t
    ended = (ta.step_type == STEP_LAST).cpu().numpy()
    if ended.any():
      last = (ended.copy(), e_host.copy(), ta.observation.clone())
    restarts += ended
    e_host += ended
    assert a.sim.initial_condition_episodes().cpu().numpy().tolist() == e_host.tolist(), t
  # an episode of n steps ends with its step n + 1 (n transitions and a terminal step): 3, 2, 2, 1 restarts in 11 steps
  assert restarts.tolist() == (11 // (lengths + 1)).tolist() and restarts.min() >= 1 and restarts.max() == 3
  assert a.sim.initial_condition_episodes().cpu().numpy().tolist() == (1 + restarts).tolist()
  # fresh environments reset to the same grids: K = B grids, building b on grid b
  ended, e_then, obs_then = last
  for episodes, rows, obs, cols in ((np.zeros(B, int), np.ones(B, bool), first_obs, slice(None)), (e_then, ended, obs_then, zone_cols)):
    grids = icc.materialised(ic, episodes, fp.shape).reshape(B, *fp.shape)
    fresh = BatchedEnvironment(fp, B, config=icc.twin_config(), holiday_calendar=None,
                               initial_conditions=InitialConditions(reset_temp_values=grids, grid_of=np.arange(B)))
    tf = fresh.reset()
    idx = torch.as_tensor(np.nonzero(rows)[0], device="cuda")
    assert torch.equal(tf.observation[idx][:, cols], obs[idx][:, cols])
    assert tf.step_type.tolist() == [STEP_FIRST] * B
    fresh.close()
  a.close()
  s.close()


def test_reset_buildings_of_the_environment_returns_the_first_observation_of_the_new_grid():
  need_gpu()
  fp = icc.plan()
  ic = icc.conditions("grids", fp.shape)
  env = _episode_env(fp, ic, np.full(B, 9), spatial=host_inputs.SpatialOutputs(pool=(4, 4), zone_stats=True))
  env.reset()
  env.step(_dev(icc.actions(1)[0], torch.float32))
  ts = env.reset_buildings(MASK)
  e = 1 + MASK.astype(int)
  want = icc.materialised(ic, e - 1, fp.shape)   # the unmasked buildings' row is not what they hold: only MASK is compared
  got = env.sim.temps().cpu().numpy().reshape(B, -1)
  assert np.array_equal(got[MASK], want[MASK]) and not np.array_equal(got[~MASK], want[~MASK])
  assert ts.step_type[torch.as_tensor(MASK, device="cuda")].tolist() == [STEP_FIRST] * int(MASK.sum())
  # the spatial outputs describe the state the observation describes: the zone means of the new grid
  stats = env.zone_temp_stats.cpu().numpy()
  zt = env.sim.zone_temps().cpu().numpy()
  # (k_spatial sums a zone in its own fixed order, the reset kernel in its lane order: two float64 sums of n values near
  # 300 K differ by less than n units in the last place of 300 K -- 5.7e-14 K each)
  n_max = max(int((fp.zone_label == z).sum()) for z in range(fp.n_zones))
  assert np.abs(stats[MASK][:, :, 2] - zt[MASK]).max() <= n_max * np.spacing(300.0)
  zlab = fp.zone_label.reshape(-1)
  for b in np.nonzero(MASK)[0][:4]:
    for z in range(fp.n_zones):
      cells = want[b][zlab == z]
      assert stats[b, z, 0] == cells.min() and stats[b, z, 1] == cells.max()
  env.close()


# ---------------------------------------------------------------- 4. the reference and the twins
def _fixture():
  g = load("reset_temp_values.npz")
  return g, icc.fixture_plan(g), dt.datetime.fromisoformat(str(g["start_timestamp"]))


def test_the_reference_rollout_through_the_environment():
  """tests/golden/reset_temp_values.npz, both episodes, at the bars of tests/test_gpu_parity.py's golden rollouts: sweep
  counts EQUAL, zone temperatures and grids within 1e-8 K, the rates at tests/twins.py's bounds, rewards within 1e-6."""
  need_gpu()
  g, fp, start = _fixture()
  n = 3
  env = BatchedEnvironment(fp, n, config=SimConfig.sb1(), start_timestamp=start, holiday_calendar=None, collect_info=True,
                           initial_conditions=InitialConditions(reset_temp_values=g["reset_temp_values"]))
  for ep in ("e1_", "e2_"):
    ts = env.reset()
    assert np.array_equal(env.sim.temps().cpu().numpy()[0], g["reset_temp_values"])
    k = len(g[ep + "obs_reset"])
    assert np.allclose(ts.observation.cpu().numpy()[:, :k], g[ep + "obs_reset"], rtol=1e-6, atol=1e-6), ep
    for t in range(len(g[ep + "n_sweeps"])):
      act = torch.tensor(np.tile(g[ep + "actions_norm"][t], (n, 1)), dtype=torch.float32, device="cuda")
      ts = env.step(act)
      i = env.info.cpu().numpy().astype(np.float64)
      assert (i[:, 4] == g[ep + "n_sweeps"][t]).all(), (ep, t, i[:, 4], g[ep + "n_sweeps"][t])
      assert np.abs(env.sim.zone_temps().cpu().numpy() - g[ep + "zone_temp_post"][t]).max() < T_TOL, (ep, t)
      assert rates_match(i[:, :4], g[ep + "rates"][t].astype(np.float64)), (ep, t, i[0, :4], g[ep + "rates"][t])
      assert np.abs(ts.reward.cpu().numpy().astype(np.float64) - float(g[ep + "reward"][t])).max() < 1e-6, (ep, t)
      assert np.allclose(ts.observation.cpu().numpy()[:, :k], g[ep + "obs"][t], rtol=1e-6, atol=1e-6), (ep, t)
      if t == 0:
        assert np.abs(env.sim.temps().cpu().numpy() - g[ep + "grid_1"]).max() < T_TOL, ep
    assert np.abs(env.sim.temps().cpu().numpy() - g[ep + "final_grid"]).max() < T_TOL, ep
  assert env.sim.initial_condition_episodes().tolist() == [2] * n
  env.close()


def test_the_reference_rollout_through_the_single_building_adapter():
  """HipSimulatorBuilding(reset_temp_values=grid), the reference's own argument, driven like the harness that made the
  fixture drove SimulatorBuilding: request_action -> wait_time -> request_observations -> reward_info, reset() between."""
  need_gpu()
  g, fp, start = _fixture()
  b = ba.HipSimulatorBuilding(fp, start_timestamp=start, holiday_calendar=None, reset_temp_values=g["reset_temp_values"])
  req = b.observation_request_for_all_fields()
  for ep in ("e1_", "e2_"):
    if ep == "e2_":
      b.reset()
    first = b.request_observations(req)
    assert np.allclose([r.continuous_value for r in first.single_observation_responses], g[ep + "obs_reset"], rtol=1e-6, atol=1e-6)
    for t in range(len(g[ep + "n_sweeps"])):
      areq = ba.ActionRequest(timestamp=b.current_timestamp, single_action_requests=[
          ba.SingleActionRequest("boiler_id", "supply_water_setpoint", float(g[ep + "action_native"][t][0])),
          ba.SingleActionRequest("air_handler_id", "supply_air_heating_temperature_setpoint", float(g[ep + "action_native"][t][1]))])
      resp = b.request_action(areq)
      assert all(r.response_type == ba.ActionResponseType.ACCEPTED for r in resp.single_action_responses)
      b.wait_time()
      i = b.env.info.cpu().numpy().astype(np.float64)
      assert (i[:, 4] == g[ep + "n_sweeps"][t]).all(), (ep, t, i[:, 4], g[ep + "n_sweeps"][t])
      assert np.abs(b.env.sim.zone_temps().cpu().numpy() - g[ep + "zone_temp_post"][t]).max() < T_TOL, (ep, t)
      ri = b.reward_info
      ah, bl = ri.air_handler_reward_infos["air_handler_id"], ri.boiler_reward_infos["boiler_id"]
      rates = [ah.blower_electrical_energy_rate, ah.air_conditioning_electrical_energy_rate,
               bl.natural_gas_heating_energy_rate, bl.pump_electrical_energy_rate]
      assert rates_match(rates, g[ep + "rates"][t].astype(np.float64)), (ep, t)
      obs = b.request_observations(req)
      assert np.allclose([r.continuous_value for r in obs.single_observation_responses], g[ep + "obs"][t], rtol=1e-6, atol=1e-6), (ep, t)
    assert np.abs(b.env.sim.temps().cpu().numpy() - g[ep + "final_grid"]).max() < T_TOL, ep
  with pytest.raises(ValueError, match=r"one \[H, W\] grid"):
    ba.HipSimulatorBuilding(fp, holiday_calendar=None, reset_temp_values=np.zeros((2, 23, 12)))
  b.close()


@pytest.mark.parametrize("layout", ["register", "lds"])
def test_every_building_started_from_its_conditions_is_its_twin(layout, monkeypatch):
  need_gpu()
  fp, g, (sim,) = _sims(layout, monkeypatch, n=1)
  want = icc.twin_rollout()
  sim.initial_conditions_attach(icc.conditions("grids", fp.shape))
  sim.reset()
  acts = icc.actions(icc.T_TWINS)
  obs, rew, info = step_buffers(sim)
  for t in range(icc.T_TWINS):
    sim.step(_dev(acts[t], torch.float32), step_in(g, icc.ROW0 + t), obs, rew, info)
    i, zt, r = info.cpu().numpy().astype(np.float64), sim.zone_temps().cpu().numpy(), rew.cpu().numpy()
    for b in range(B):
      assert_step_matches(i[b], zt[b], r[b], want[t][b], (layout, t, b))
  d = np.abs(sim.temps().cpu().numpy().reshape(B, -1) - icc.twin_final_grids().reshape(B, -1)).max()
  assert d < T_TOL, d
  sim.close()


# ---------------------------------------------------------------- 5. crossing
def test_conditions_cross_materials_calendars_and_episodes_against_twins():
  """building_materials, calendars and per_building_episodes in one batch with the conditions attached: reset(), twelve
  steps with their autoresets and a reset_buildings in between, every building held to its own twin, whose every reset
  starts from start_temps(b, its own e) -- at the bars of tests/test_crossed_batches_gpu.py.  Unlike there, nothing is
  staged after reset(): the first observation already describes the right state."""
  need_gpu()
  sc, ic, want, episodes = icc.crossing()
  env = BatchedEnvironment(sc.plan, B, initial_conditions=ic, **sc.env_kwargs())
  assert env.sim.launch_info["kernel"] == LDS and env.steps_per_episode == cb.N_EPISODE
  worst = cbg.Worst()
  acts = torch.tensor(sc.actions, device="cuda")
  ts = env.reset()
  first = want[0][1]
  assert ts.step_type.tolist() == [cb.STEP_FIRST] * B
  cbg._check_rows(sc.layout, ts.observation.cpu().numpy(), [r["obs"] for r in first], [r["obs_native"] for r in first],
                  range(B), "reset()", worst)
  for i, (op, res) in enumerate(want[1:-1]):
    what = f"call {i} ({op.kind}{'' if op.row < 0 else ' ' + str(op.row)})"
    if op.kind == "step":
      rejected = None if op.rejected is None else torch.tensor(op.rejected, device="cuda")
      ts = env.step(acts[op.row], rejected=rejected)
      cbg._check_step(env, sc, ts, res, what, worst)
    else:
      ts = env.reset_buildings(op.mask)
      rows = [b for b in range(B) if op.mask[b]]
      cbg._check_rows(sc.layout, ts.observation.cpu().numpy(), {b: res[b]["obs"] for b in rows},
                      {b: res[b]["obs_native"] for b in rows}, rows, what, worst)
  d = np.abs(env.sim.temps().cpu().numpy().reshape(B, -1) - want[-1][1]).max(axis=1)
  assert (d < T_TOL).all(), (int(np.argmax(d)), d.max())
  assert env.sim.initial_condition_episodes().cpu().numpy().tolist() == episodes.tolist()
  env.close()
  print(f"\n[initial conditions, crossed] {worst}")


def test_mixed_environment_takes_conditions_per_class():
  need_gpu()
  big, small = icc.plan(), plan_from_npz(load("plan_small_test.npz"))
  n_big, n_small = 5, 4
  t0 = np.linspace(290.0, 296.0, n_small)
  ic = InitialConditions(initial_temp=t0, jitter=icc.JITTER)
  env = MixedBatchedEnvironment([(big, n_big), (small, n_small)], holiday_calendar=None, initial_conditions=[None, ic])
  env.reset()
  assert env.envs[0].initial_conditions is None
  assert np.array_equal(env.envs[0].sim.temps().cpu().numpy(), np.full((n_big, *big.shape), SimConfig.sb1().initial_temp))
  share = env.envs[1].initial_conditions
  assert share.first_building == n_big    # class 1's building 0 is building 5 of the mixed batch: it draws as such
  whole = InitialConditions(initial_temp=np.concatenate([np.zeros(n_big), t0]), jitter=icc.JITTER)
  got = env.envs[1].sim.temps().cpu().numpy()
  for i in range(n_small):
    assert np.array_equal(got[i], whole.start_temps(n_big + i, 0, shape=small.shape)), i
  env.close()
  with pytest.raises(ValueError, match=r"initial_conditions\[1\]: initial_temp has 4 rows, the batch 3"):
    MixedBatchedEnvironment([(big, n_big), (small, 3)], holiday_calendar=None, initial_conditions=[None, ic])
  with pytest.raises(ValueError, match="one host_inputs.InitialConditions or None per class"):
    MixedBatchedEnvironment([(big, n_big), (small, n_small)], holiday_calendar=None, initial_conditions=[ic])
  # two ranks: a class's rows are cut over the ranks, the draws stay the global building's
  for rank in (0, 1):
    env = MixedBatchedEnvironment([(big, n_big), (small, n_small)], holiday_calendar=None, initial_conditions=[None, ic],
                                  rank=rank, world=2)
    env.reset()
    lo, hi = env.class_ranges[1]
    got = env.envs[1].sim.temps().cpu().numpy()
    for i in range(hi - lo):
      assert np.array_equal(got[i], whole.start_temps(n_big + lo + i, 0, shape=small.shape)), (rank, i)
    env.close()


# ---------------------------------------------------------------- 6. the untouched default
def test_attach_and_detach_leave_no_trace():
  need_gpu()
  fp = icc.plan()
  mk = lambda: BatchedEnvironment(fp, B, config=icc.twin_config(), holiday_calendar=None, collect_info=True)
  plain, used = mk(), mk()
  fingerprint = plain.sim.state_fingerprint()
  ic = icc.conditions("grids", fp.shape)
  used.set_initial_conditions(ic)
  attached = used.sim.state_fingerprint()
  assert attached[:-1] == fingerprint and attached[-1] == ("initial_conditions", ic.digest())
  assert icc.conditions("grids", fp.shape).digest() == ic.digest() != icc.conditions("grids", fp.shape, first_building=1).digest()
  used.reset()
  used.set_initial_conditions(None)
  assert used.sim.state_fingerprint() == fingerprint and used.initial_conditions is None
  acts = _dev(icc.actions(4, seed=4), torch.float32)
  tp, tu = plain.reset(), used.reset()
  assert torch.equal(tp.observation, tu.observation)
  for t in range(4):
    tp, tu = plain.step(acts[t]), used.step(acts[t])
    for x, y in ((tp.observation, tu.observation), (tp.reward, tu.reward), (plain.info, used.info),
                 (plain.sim.temps(), used.sim.temps()), (plain.sim.scalars(), used.sim.scalars())):
      assert torch.equal(x, y), t
  # the counters' pair on a handle without conditions: SB_ERR_UNSUPPORTED
  out = torch.zeros(B, dtype=torch.int32, device="cuda")
  for name in ("sb_initial_conditions_episodes_get", "sb_initial_conditions_episodes_set"):
    rc = _ffi.initial_conditions_entry(name)(plain.sim._h, C.c_void_p(out.data_ptr()), plain.sim._stream())
    assert rc == -5 and b"no initial conditions" in _ffi.load().sb_last_error(), name
  with pytest.raises(ValueError, match="no initial conditions"):
    plain.sim.initial_condition_episodes()
  plain.sim.initial_conditions_detach()   # nothing attached: nothing to do
  for e in (plain, used):
    e.close()


def test_the_library_refuses_what_the_host_class_would():
  """sb_initial_conditions_attach's own checks (a caller of the C ABI has no InitialConditions in front of it)."""
  need_gpu()
  fp = icc.plan()
  sim = BatchedSimulator(fp, icc.twin_config(), B, 100.0)
  fn = _ffi.initial_conditions_entry("sb_initial_conditions_attach")
  N = fp.shape[0] * fp.shape[1]
  grids = np.full((2, N), 294.0)
  per, which = np.full(B, 294.0), np.zeros(B, np.int32)
  dp, ip = lambda a: a.ctypes.data_as(_ffi._dp), lambda a: a.ctypes.data_as(_ffi._ip)

  def rc_of(**kw):
    d = _ffi.InitialConditionsDesc()
    for k, v in kw.items():
      setattr(d, k, v)
    return fn(sim._h, C.byref(d)), (_ffi.load().sb_last_error() or b"").decode()

  bad_which = which.copy()
  bad_which[9] = 2
  nan_per = per.copy()
  nan_per[7] = np.nan
  inf_grid = grids.copy()
  inf_grid[1, 5] = np.inf
  for kw, msg in ((dict(), "no field given"),
                  (dict(grids=dp(grids), n_grids=0), "grids and n_grids >= 1 go together"),
                  (dict(n_grids=2), "grids and n_grids >= 1 go together"),
                  (dict(grids=dp(grids), n_grids=2), "grid_of: needed with more than one grid"),
                  (dict(grids=dp(grids), n_grids=2, grid_of=ip(bad_which)), "building 9: grid_of 2 is outside the 2 grids"),
                  (dict(grid_of=ip(which), offset=dp(per)), "grid_of: given without grids"),
                  (dict(grids=dp(grids), n_grids=1, initial_temp=dp(per)), "initial_temp: not together with grids"),
                  (dict(grids=dp(inf_grid), n_grids=2, grid_of=ip(which)), "grid 1 cell 5 is not finite"),
                  (dict(initial_temp=dp(nan_per)), "building 7: initial_temp is not finite"),
                  (dict(offset=dp(nan_per)), "building 7: offset is not finite"),
                  (dict(has_jitter=1, jitter_lo=1.0, jitter_hi=0.0), "jitter: needs finite lo <= hi"),
                  (dict(has_jitter=1, jitter_lo=0.0, jitter_hi=float("nan")), "jitter: needs finite lo <= hi"),
                  (dict(offset=dp(per), first_building=-1), "first_building must be >= 0")):
    rc, err = rc_of(**kw)
    assert rc == -1 and msg in err, (kw.keys(), rc, err)
  assert sim.initial_conditions is None
  rc, err = rc_of(offset=dp(per))
  assert rc == 0, err
  sim.close()
