"""Episode totals per building on the GPU (sb_episode_metrics_attach; BatchedEnvironment(episode_metrics=True)).

The running and completed rows are held EQUAL, bit for bit, to ``host_inputs.EpisodeMetricsTwin`` fed with the step's own
outputs (reward, info rows, zone means): the kernel and the twin do the same IEEE double operations in the same order.
Against the reference: the recorded two episodes of tests/golden/h2_sb1_r9_episodes.npz, at the bars the existing parity
tests use.  Plans of a few hundred cells, at most 30 steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import (STEP_LAST, BatchedEnvironment, BatchedSimulator, GymVectorEnv,  # noqa: E402
                                   MixedBatchedEnvironment, SimConfig)
from sbsim_amd.host_inputs import BuildingMaterials, EpisodeMetricsTwin  # noqa: E402
from tests import convection_cases as cc  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import need_gpu, step_buffers  # noqa: E402
from tests.twins import T_TOL, plan_from_npz, step_in  # noqa: E402

NAMES = _ffi.EPISODE_METRIC_NAMES
COL = {n: i for i, n in enumerate(NAMES)}
F = _ffi.SB_EM_FIELDS
LDS, REG, JACOBI = 0, 1, 7   # sb_sweep_kernel


def _tiny():
  return cc._plan(cc.TINY)


def _bits(x):
  x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
  return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(got, want):
  return np.array_equal(_bits(got), _bits(want))


def _inputs(T, B, seed, p_reject=0.25):
  rs = np.random.RandomState(seed)
  acts = torch.tensor(rs.uniform(-1, 1, size=(T, B, 2)).astype(np.float32), device="cuda")
  rej = torch.tensor(rs.rand(T, B) < p_reject, device="cuda")
  return acts, rej


def _materials(plan, B):
  table = plan.material_slots()[1]
  sets = np.stack([table * (np.array([0.2, 3.0, 2.0]) if i % 2 == 0 else np.array([4.0, 0.3, 0.5])) for i in range(B)])
  return BuildingMaterials(conductivity=sets[:, :, 0], heat_capacity=sets[:, :, 1], density=sets[:, :, 2],
                           convection_coefficient=np.linspace(5.0, 150.0, B))


def _env(B, plan=None, steps=24, **kw):
  args = dict(num_days_in_episode=steps / 288, holiday_calendar=None, collect_info=True, episode_metrics=True)
  args.update(kw)
  return BatchedEnvironment(plan if plan is not None else _tiny(), B, **args)


def _twin(env):
  return EpisodeMetricsTwin(env.batch_size, env.config.time_step_sec)


def _feed(twin, env, ts, zone_means=None):
  zm = env.sim.zone_temps() if zone_means is None else zone_means
  twin.step(ts.reward.cpu().numpy(), env.info.cpu().numpy(), zm.cpu().numpy())


# ---------------------------------------------------------------- 1. the running rows
LAYOUTS = {"reg": ({}, (), REG), "lds": ({}, (("SBSIM_FORCE_LDS_PATH", "1"),), LDS), "jacobi": (dict(solver="jacobi_fp32"), (), JACOBI),
           "materials": (dict(building_materials=True), (), LDS)}


@pytest.mark.parametrize("B,layout", [(1, "reg"), (63, "reg"), (64, "reg"), (65, "reg"), (257, "reg"),
                                      (65, "lds"), (65, "jacobi"), (65, "materials")])
def test_running_rows_equal_the_twin_after_every_step(B, layout, monkeypatch):
  need_gpu()
  kw, switches, kernel = LAYOUTS[layout]
  for k, v in switches:
    monkeypatch.setenv(k, v)
  kw = dict(kw)
  if kw.get("building_materials"):
    kw["building_materials"] = _materials(_tiny(), B)
  env = _env(B, **kw)
  assert env.sim.launch_info["kernel"] == kernel, env.sim.launch_info
  twin = _twin(env)
  T = 12
  acts, rej = _inputs(T, B, seed=100 + B)
  env.reset()                                          # the first reset: steps == 0, nothing closes
  assert _same(env.episode_metrics(), twin.running) and _same(env.completed_episodes(), twin.completed)
  for t in range(T):
    ts = env.step(acts[t], rej[t])
    _feed(twin, env, ts)
    assert _same(env.episode_metrics(), twin.running), (t, layout)
  run = env.episode_metrics().cpu().numpy()
  r = rej.cpu().numpy()
  assert (run[:, COL["steps"]] == T).all() and (run[:, COL["rejected_steps"]] >= r.sum(axis=0)).all()
  assert (np.isneginf(run[:, COL["return"]]) == (run[:, COL["rejected_steps"]] > 0)).all() and np.isfinite(run[:, COL["accepted_return"]]).all()
  assert (run[:, COL["zone_temp_min"]] <= run[:, COL["zone_temp_max"]]).all() and (run[:, COL["sweeps"]] >= T).all()
  assert _same(env.completed_episodes(), twin.completed)   # no reset since: untouched
  env.close()


# ---------------------------------------------------------------- 2. the latch
def test_the_latch_with_episodes_per_building(monkeypatch):
  need_gpu()
  B, T = 65, 30
  rs = np.random.RandomState(7)
  steps = rs.randint(3, 10, size=B)
  assert set(steps) == set(range(3, 10))
  env = _env(B, steps=12, episode_steps=steps)
  twin = _twin(env)
  seen = {}
  reset_buildings = env.sim.reset_buildings

  def spy(mask, **kw):                                 # the zone means of the step, before the masked reset overwrites them
    seen["zm"] = env.sim.zone_temps().clone()
    return reset_buildings(mask, **kw)

  monkeypatch.setattr(env.sim, "reset_buildings", spy)
  acts, rej = _inputs(T, B, seed=8)
  env.reset()
  closed_total = np.zeros(B, dtype=int)
  for t in range(T):
    before = env.completed_episodes().cpu().numpy()
    seen.clear()
    ts = env.step(acts[t], rej[t])
    last = (ts.step_type == STEP_LAST).cpu().numpy()
    assert last.any() == ("zm" in seen)
    _feed(twin, env, ts, seen.get("zm"))
    episode = twin.running[:, 0].copy()
    assert np.array_equal(twin.close(last), last)      # every building that ended had stepped
    closed_total += last
    done, run = env.completed_episodes().cpu().numpy(), env.episode_metrics().cpu().numpy()
    assert _same(done[last], twin.completed[last]), t
    assert _same(done[~last], before[~last]), t        # every other building: not a bit
    assert _same(run, twin.running), t
    assert (run[last, 0] == episode[last] + 1).all() and (run[last, 1:18] == 0).all()
    assert np.isposinf(run[last, 18]).all() and np.isneginf(run[last, 19]).all()
  assert (closed_total >= 3).all() and _same(env.episode_metrics()[:, 0], closed_total)
  # reset_buildings mid-episode; a second one right behind it holds buildings with no step since their reset
  m1 = np.zeros(B, dtype=bool)
  m1[[0, 5, 63, 64]] = True
  m2 = np.zeros(B, dtype=bool)
  m2[[5, 6, 64]] = True
  stepped = twin.running[:, 1] > 0
  for mask in (m1, m2):
    before_done, before_run = env.completed_episodes().cpu().numpy(), env.episode_metrics().cpu().numpy()
    env.reset_buildings(mask)
    closing = twin.close(mask)
    assert np.array_equal(closing, mask & stepped)
    done, run = env.completed_episodes().cpu().numpy(), env.episode_metrics().cpu().numpy()
    assert _same(done, twin.completed) and _same(run, twin.running)
    assert _same(done[~closing], before_done[~closing]) and _same(run[~closing], before_run[~closing])
    stepped = twin.running[:, 1] > 0
  assert not stepped[5] and not stepped[64]            # (they were in both masks: the second closed nothing for them)
  # a full reset closes every building that has stepped since
  before_done = env.completed_episodes().cpu().numpy()
  env.reset()
  closing = twin.close()
  assert closing.any() and not closing.all()
  done, run = env.completed_episodes().cpu().numpy(), env.episode_metrics().cpu().numpy()
  assert _same(done, twin.completed) and _same(run, twin.running) and _same(done[~closing], before_done[~closing])
  env.reset()                                          # two resets in a row: nothing closes
  assert _same(env.completed_episodes(), twin.completed) and _same(env.episode_metrics(), twin.running)
  env.close()


# ---------------------------------------------------------------- 3. against the reference
class _Episode:   # step_in reads g[key][t]
  def __init__(self, g, ep):
    self.g, self.ep = g, ep

  def __getitem__(self, k):
    return self.g[self.ep + k]


def test_totals_against_the_reference_episodes():
  """tests/test_episode_reset.py's replay with the metrics attached.  Measured figures are printed before they are
  asserted."""
  need_gpu()
  g = load("h2_sb1_r9_episodes.npz")
  B = 5
  sim = BatchedSimulator(plan_from_npz(load("plan_r9_sb1.npz")), SimConfig.sb1(), B, float(g["h_conv"]))
  sim.episode_metrics_attach()
  obs, rew, info = step_buffers(sim)
  aux = [0.0] * _ffi.SB_NUM_AUX
  K = 1.0 / 3600.0 / 1000.0
  sim.reset()
  for n, ep in enumerate(("e1_", "e2_")):
    e = _Episode(g, ep)
    sim.observe(aux, float(e["t_amb_now"][0]), obs)
    T = len(e["n_sweeps"])
    for t in range(T):
      act = torch.tensor(np.tile(e["actions_norm"][t], (B, 1)), dtype=torch.float32, device="cuda")
      rej = torch.full((B,), int(e["rejected"][t]), dtype=torch.uint8, device="cuda")
      si = step_in(e, t)
      si.reject_dev = rej.data_ptr()
      sim.step(act, si, obs, rew, info)
    sim.reset()                                        # closes episode n, opens the next
    done = sim.completed_episodes().cpu().numpy()
    rejected = e["rejected"].astype(bool)
    rates = e["rates"].astype(np.float64)
    want = {
        "electrical_energy": (rates[:, 0] + rates[:, 1] + rates[:, 3]).sum() * 300.0 * K,
        "natural_gas_energy": rates[:, 2].sum() * 300.0 * K,
        "electricity_energy_cost": e["rr_elec_cost"].astype(np.float64).sum(),
        "natural_gas_energy_cost": e["rr_gas_cost"].astype(np.float64).sum(),
        "carbon_emitted": e["rr_carbon"].astype(np.float64).sum(),
        "productivity_reward": e["rr_productivity"].astype(np.float64).sum(),
        "normalized_productivity_regret": e["rr_norm_prod_regret"].astype(np.float64).sum(),
        "normalized_energy_cost": e["rr_norm_energy_cost"].astype(np.float64).sum(),
        "normalized_carbon_emission": e["rr_norm_carbon"].astype(np.float64).sum(),
    }
    accepted = e["reward"][~rejected].astype(np.float64).sum()
    print(f"[{ep}] steps {done[:, COL['steps']]} rejected {done[:, COL['rejected_steps']]} return {done[:, COL['return']]}")
    print(f"[{ep}] accepted_return {done[:, COL['accepted_return']]} golden {accepted!r} "
          f"max |d| {np.abs(done[:, COL['accepted_return']] - accepted).max():.3e} bar {(~rejected).sum() * 1e-6:.1e}")
    for name, ref in want.items():
      print(f"[{ep}] {name} {done[0, COL[name]]!r} golden {ref!r} max rel {np.abs(done[:, COL[name]] / ref - 1.0).max():.3e}")
    zmin, zmax = e["zone_temp_post"].min(), e["zone_temp_post"].max()
    print(f"[{ep}] zone extremes |d| {np.abs(done[:, COL['zone_temp_min']] - zmin).max():.3e} {np.abs(done[:, COL['zone_temp_max']] - zmax).max():.3e}")
    assert (done[:, COL["episode"]] == n).all() and (done[:, COL["steps"]] == T).all() and T == (14, 16)[n]
    assert (done[:, COL["rejected_steps"]] == rejected.sum()).all()
    assert (np.isneginf(done[:, COL["return"]]) == bool(rejected.any())).all() and (np.isfinite(done[:, COL["return"]]) != bool(rejected.any())).all()
    assert np.abs(done[:, COL["accepted_return"]] - accepted).max() <= (~rejected).sum() * 1e-6
    for name, ref in want.items():
      assert np.allclose(done[:, COL[name]], ref, rtol=1e-6), (ep, name, done[:, COL[name]], ref)
    assert (done[:, COL["sweeps"]] == e["n_sweeps"].sum()).all() and (done[:, COL["unconverged_steps"]] == 0).all()
    assert np.abs(done[:, COL["zone_temp_min"]] - zmin).max() < T_TOL and np.abs(done[:, COL["zone_temp_max"]] - zmax).max() < T_TOL
    run = sim.episode_metrics().cpu().numpy()
    assert (run[:, 0] == n + 1).all() and (run[:, 1] == 0).all()
  sim.close()


# ---------------------------------------------------------------- 4. nothing else moves
def test_an_attached_handle_computes_what_a_plain_one_does():
  need_gpu()
  B, T = 5, 6
  with_m, plain, no_info = _env(B), _env(B, episode_metrics=False), _env(B, collect_info=False)
  assert plain.sim.episode_metrics_attached is False and with_m.sim.episode_metrics_attached and no_info.info is None
  with pytest.raises(ValueError, match="episode_metrics=True"):
    plain.episode_metrics()
  acts, rej = _inputs(T, B, seed=21)
  for env in (with_m, plain, no_info):
    env.reset()
  for t in range(T):
    a, p, n = with_m.step(acts[t], rej[t]), plain.step(acts[t], rej[t]), no_info.step(acts[t], rej[t])
    for x, y in ((a.observation, p.observation), (a.reward, p.reward), (with_m.info, plain.info), (with_m.sim.temps(), plain.sim.temps()),
                 (a.observation, n.observation), (a.reward, n.reward)):
      assert torch.equal(x, y), t
    # without a caller's info buffer the library sums its own: the same totals
    assert torch.equal(with_m.episode_metrics(), no_info.episode_metrics()), t
  assert plain.sim.state_fingerprint() == with_m.sim.state_fingerprint()
  assert (with_m.episode_metrics()[:, COL["steps"]] == T).all()
  for env in (with_m, plain, no_info):
    env.close()


def test_an_info_buffer_that_is_not_16_byte_aligned_gives_the_same_totals():
  """k_episode_metrics reads the info row in 16-byte pieces only from a buffer that allows it."""
  need_gpu()
  B, T = 65, 4
  sims = [BatchedSimulator(_tiny(), SimConfig.sb1(), B, 12.0) for _ in range(2)]
  obs, rew, aligned = step_buffers(sims[0])
  skewed = torch.zeros((B * _ffi.SB_INFO_STRIDE + 1,), dtype=torch.float32, device="cuda")[1:].view(B, _ffi.SB_INFO_STRIDE)
  assert aligned.data_ptr() % 16 == 0 and skewed.data_ptr() % 16 == 4 and skewed.is_contiguous()
  acts, rej = _inputs(T, B, seed=27)
  si = _ffi.StepIn()
  si.t_amb_now = si.t_amb_next = 285.0
  si.comfort_now = si.comfort_next = si.comfort_prev = 1
  si.has_action, si.occupancy, si.e_price, si.e_carbon, si.g_price, si.g_carbon = 1, 2.0, 0.1, 0.2, 0.3, 0.4
  for sim in sims:
    sim.episode_metrics_attach()
    sim.reset()
  for t in range(T):
    r8 = rej[t].to(torch.uint8)
    si.reject_dev = r8.data_ptr()
    for sim, info in zip(sims, (aligned, skewed)):
      sim.step(acts[t], si, obs, rew, info)
    assert torch.equal(aligned, skewed) and torch.equal(sims[0].episode_metrics(), sims[1].episode_metrics()), t
    torch.cuda.synchronize()                           # (r8 is read by the kernels queued above)
  assert (sims[0].episode_metrics()[:, COL["steps"]] == T).all()
  for sim in sims:
    sim.close()


# ---------------------------------------------------------------- 5. capture and checkpoint
def test_a_captured_step_replays_and_a_checkpoint_continues():
  need_gpu()
  B = 5
  sim = BatchedSimulator(_tiny(), SimConfig.sb1(), B, 12.0)
  get = _ffi.episode_metrics_entry("sb_episode_metrics_get")
  out = torch.zeros((B, F), dtype=torch.float64, device="cuda")
  assert get(sim._h, C.c_void_p(out.data_ptr()), None, None) == -5 and b"sb_episode_metrics_attach" in _ffi.load().sb_last_error()
  assert get(sim._h, None, None, None) == -1
  with pytest.raises(ValueError, match="no episode metrics"):
    sim.episode_metrics()
  sim.episode_metrics_attach()
  twin = EpisodeMetricsTwin(B, SimConfig.sb1().time_step_sec)
  obs, rew, info = step_buffers(sim)
  acts, _ = _inputs(1, B, seed=33)
  si = _ffi.StepIn()
  si.t_amb_now = si.t_amb_next = 290.0
  si.comfort_now = si.comfort_next = si.comfort_prev = 1
  si.has_action, si.occupancy, si.e_price, si.e_carbon, si.g_price, si.g_carbon = 1, 2.0, 0.1, 0.2, 0.3, 0.4
  sim.reset()

  def fed():
    twin.step(rew.cpu().numpy(), info.cpu().numpy(), sim.zone_temps().cpu().numpy())
    assert _same(sim.episode_metrics(), twin.running)

  sim.step(acts[0], si, obs, rew, info)                # (an ordinary step first: everything is loaded before the capture)
  fed()
  s = torch.cuda.Stream()
  graph = torch.cuda.CUDAGraph()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    graph.capture_begin()
    try:
      sim.step(acts[0], si, obs, rew, info)
    finally:
      graph.capture_end()
  torch.cuda.synchronize()
  assert _same(sim.episode_metrics(), twin.running)    # capturing ran nothing
  for _ in range(3):
    graph.replay()
    torch.cuda.synchronize()
    fed()
  assert (sim.episode_metrics()[:, COL["steps"]] == 4).all()
  # the checkpoint pair: get -> attach (re-initialises) -> set puts back every bit, and the handle continues
  sim.reset()
  twin.close()
  sim.step(acts[0], si, obs, rew, info)
  fed()
  run, done = sim.episode_metrics(), sim.completed_episodes()
  assert (done[:, COL["steps"]] == 4).all()
  sim.episode_metrics_attach()
  fresh = EpisodeMetricsTwin(B, 300.0)
  assert _same(sim.episode_metrics(), fresh.running) and _same(sim.completed_episodes(), fresh.completed)
  sim.episode_metrics_set(run, done)
  assert torch.equal(sim.episode_metrics(), run) and torch.equal(sim.completed_episodes(), done)
  with pytest.raises(ValueError):
    sim.episode_metrics_set(run[:, :5], None)
  with pytest.raises(ValueError):
    sim.episode_metrics_set(None, None)
  sim.step(acts[0], si, obs, rew, info)
  fed()
  sim.reset()
  twin.close()
  assert _same(sim.completed_episodes(), twin.completed) and (sim.completed_episodes()[:, 0] == 1).all()
  sim.episode_metrics_detach()
  assert get(sim._h, C.c_void_p(out.data_ptr()), None, None) == -5
  sim.step(acts[0], si, obs, rew, info)                # detached: a plain step
  sim.close()


# ---------------------------------------------------------------- 6. adapters
def test_gym_view_carries_the_episode_statistics_only_when_enabled():
  need_gpu()
  B = 5
  on, off = GymVectorEnv(_env(B, steps=3)), GymVectorEnv(_env(B, steps=3, episode_metrics=False))
  acts, _ = _inputs(6, B, seed=41)
  on.reset(), off.reset()
  ended = 0
  for t in range(6):
    _, reward, _, truncated, info = on.step(acts[t])
    assert set(off.step(acts[t])[4]) == {"step_type", "discount"}      # what it was
    assert set(info) == {"step_type", "discount", "episode", "_episode"} and torch.equal(info["_episode"], truncated)
    if truncated.any():                                # the shared clock: the episode still is the running rows
      ended += 1
      run = on.env.episode_metrics()
      assert truncated.all() and torch.equal(info["episode"]["r"], run[:, COL["return"]])
      assert torch.equal(info["episode"]["l"], run[:, COL["steps"]].to(torch.int64)) and (info["episode"]["l"] == 4).all()
      on.step(acts[t])                                 # next-step autoreset: the reset closes it
      assert torch.equal(on.env.completed_episodes(), run)
      break
  assert ended == 1
  on.close(), off.close()
  # same-step autoreset: the completed rows
  steps = np.array([2, 3, 5, 2, 4])
  venv = GymVectorEnv(_env(B, steps=12, episode_steps=steps))
  venv.reset()
  seen = np.zeros(B, dtype=bool)
  for t in range(6):
    _, _, _, truncated, info = venv.step(acts[t])
    assert torch.equal(info["_episode"], truncated) and info["autoreset_mode"] == "same_step"
    done = venv.env.completed_episodes()
    m = truncated
    assert torch.equal(info["episode"]["r"][m], done[m][:, COL["return"]])
    assert torch.equal(info["episode"]["l"][m], done[m][:, COL["steps"]].to(torch.int64))
    assert (venv.env.episode_metrics()[m][:, COL["steps"]] == 0).all()
    seen |= m.cpu().numpy()
  assert seen.any()
  venv.close()


def test_mixed_batch_concatenates_its_classes():
  need_gpu()
  plans = [_tiny(), plan_from_npz(load("plan_small_test.npz"))]
  counts = [3, 4]
  kw = dict(num_days_in_episode=3 / 288, collect_info=True, episode_metrics=True)
  mixed = MixedBatchedEnvironment(list(zip(plans, counts)), **kw)
  singles = [BatchedEnvironment(p, n, **kw) for p, n in zip(plans, counts)]
  assert mixed.has_episode_metrics
  acts, _ = _inputs(6, sum(counts), seed=51)
  mixed.reset()
  for s in singles:
    s.reset()
  for t in range(6):                                   # 4 steps, the shared reset, one more step
    mixed.step(acts[t])
    for s, (a, b) in zip(singles, mixed.slices):
      s.step(acts[t, a:b].contiguous())
    assert torch.equal(mixed.episode_metrics(), torch.cat([s.episode_metrics() for s in singles])), t
    assert torch.equal(mixed.completed_episodes(), torch.cat([s.completed_episodes() for s in singles])), t
  assert (mixed.completed_episodes()[:, COL["steps"]] == 4).all() and (mixed.episode_metrics()[:, COL["steps"]] == 1).all()
  plain = MixedBatchedEnvironment(list(zip(plans, counts)), num_days_in_episode=3 / 288)
  assert not plain.has_episode_metrics
  mixed.close(), plain.close()
  for s in singles:
    s.close()
