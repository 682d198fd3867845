"""GPU: snapshots of the complete per-building state (sb_state_save / sb_state_load; BatchedSimulator.save_state /
load_state, BatchedEnvironment.snapshot / restore / fork).  A restored batch replays bit for bit on every sweep kernel;
a snapshot moves between state layouts and orientations; forked buildings follow their CPU-oracle twins."""
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402  (checker only)
from sbsim_amd import host_inputs  # noqa: E402
from sbsim_amd.environment import (BatchedEnvironment, BatchedSimulator, EnvSnapshot,  # noqa: E402
                                   MixedBatchedEnvironment, SimConfig)
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from tests.golden_util import load, oracle_params, oracle_plan  # noqa: E402
from tests.parity import assert_close, assert_same, need_gpu, step_buffers  # noqa: E402
from tests.twins import T_TOL, copy_twin, plan_from_npz, step_in, step_kwargs  # noqa: E402

# the six wavefront schedules of test_one_day_rollout_against_reference_golden, plus the streaming kernel
SCHEDULES = {
    "reg": ("auto", {}, 3),
    "reg-pair": ("columns", {"SBSIM_NO_TWO_ROW_PATH": "1", "SBSIM_NO_BAND_PATH": "1"}, 2),
    "lds": ("rows", {"SBSIM_FORCE_LDS_PATH": "1"}, 0),
    "lds-columns": ("columns", {"SBSIM_FORCE_LDS_PATH": "1"}, 0),
    "reg-two": ("columns", {}, 4),
    "reg-band": ("columns", {"SBSIM_BAND_PATH": "1"}, 5),
    "stream": ("auto", {"SBSIM_FORCE_STREAM_PATH": "1"}, 6),
}


def _r9_sim(schedule, B, monkeypatch):
  orientation, env, kernel = SCHEDULES[schedule]
  for k in ("SBSIM_FORCE_LDS_PATH", "SBSIM_NO_TWO_ROW_PATH", "SBSIM_NO_BAND_PATH", "SBSIM_BAND_PATH",
            "SBSIM_FORCE_STREAM_PATH"):
    monkeypatch.delenv(k, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  g = load("h2_sb1_r9_random.npz")
  sim = BatchedSimulator(plan_from_npz(load("plan_r9_sb1.npz")), SimConfig.sb1(), B, float(g["h_conv"]), orientation=orientation)
  assert sim.launch_info["kernel"] == kernel, (schedule, sim.launch_info)
  for k in env:
    monkeypatch.delenv(k)
  return sim, g


def _seeded(B, T, seed):
  rs = np.random.RandomState(seed)
  init = np.clip(294.0 + rs.randn(B, 1, 1) + 0.3 * rs.randn(B, 68, 98), 285.0, 305.0)
  acts = rs.uniform(-1, 1, size=(T, B, 2)).astype(np.float32)
  return torch.tensor(init.reshape(B, -1), dtype=torch.float64, device="cuda"), torch.tensor(acts, device="cuda")


def _run(sim, g, acts, t0, steps, bufs, record=False):
  obs, rew, info = bufs
  out = []
  for t in range(t0, t0 + steps):
    sim.step(acts[t], step_in(g, 100 + t), obs, rew, info)
    if record:
      out.append([obs.clone(), rew.clone(), info.clone(), sim.temps(), sim.scalars(), sim.modes(), sim.zone_temps()])
  return out


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_restore_replays_bitwise_on_every_schedule(schedule, monkeypatch):
  need_gpu()
  B = 64
  sim, g = _r9_sim(schedule, B, monkeypatch)
  init, acts = _seeded(B, 50, 11)
  sim.reset(temps=init)
  bufs = step_buffers(sim)
  _run(sim, g, acts, 0, 20, bufs)
  snap = sim.save_state()
  first = _run(sim, g, acts, 20, 30, bufs, record=True)
  sim.load_state(snap)
  again = _run(sim, g, acts, 20, 30, bufs, record=True)
  if schedule == "stream":
    assert_close(first, again)
  else:
    assert_same(first, again)
  assert float(first[-1][2][:, 4].sum()) > 0   # (the sweeps ran)
  sim.close()


def _stochastic_env(B, conv_seed=3, occ_seed=5):
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  rs = np.random.RandomState(2)
  low = 270.0 + 5.0 * rs.rand(B)
  weather = host_inputs.BatchedSinusoidWeather(low, low + 10.0 + 5.0 * rs.rand(B))
  occ = host_inputs.BatchedRandomizedArrivalDepartureOccupancy(10, 5, 10, 15, 19, 300.0, seed=occ_seed)
  conv = host_inputs.StochasticConvectionSimulator(1.0, 5, conv_seed)
  return BatchedEnvironment(plan, B, weather=weather, occupancy=occ, convection_simulator=conv, collect_info=True,
                            start_timestamp=dt.datetime(2023, 7, 6, 6, 0, 0))


def _env_run(env, acts, steps, record=True):
  out = []
  for t in range(steps):
    ts = env.step(acts[t])
    if record:
      out.append([ts.step_type.clone(), ts.reward.clone(), ts.discount.clone(), ts.observation.clone(), env.info.clone(),
                  env.sim.temps(), env.sim.scalars(), env.sim.modes()])
  return out


def test_restore_replays_bitwise_with_device_occupancy_convection_and_weather():
  need_gpu()
  B = 64
  env = _stochastic_env(B)
  gen = torch.Generator(device="cuda")
  gen.manual_seed(4)
  acts = torch.rand((50, B, 2), generator=gen, device="cuda") * 2 - 1
  env.reset()
  _env_run(env, acts, 20, record=False)
  now = env.current_simulation_timestamp
  snap = env.snapshot()
  first = _env_run(env, acts[20:], 30)
  ts = env.restore(snap)
  assert env.current_simulation_timestamp == now
  assert torch.equal(ts.observation, snap.observation) and bool((ts.step_type == 1).all())
  again = _env_run(env, acts[20:], 30)
  assert_same(first, again)
  env.close()


def _check_golden_from(sim, g, t0, bufs):
  obs, rew, info = bufs
  B = sim.B
  for t in range(t0, len(g["n_sweeps"])):
    act = torch.tensor(np.tile(g["actions_norm"][t], (B, 1)), dtype=torch.float32, device="cuda")
    sim.step(act, step_in(g, t), obs, rew, info)
    i = info.cpu().numpy()
    assert (i[:, 4] == g["n_sweeps"][t]).all(), t
    assert np.abs(sim.zone_temps().cpu().numpy() - g["zone_temp_post"][t]).max() < T_TOL, t
    assert np.abs(rew.cpu().numpy().astype(np.float64) - float(g["reward"][t])).max() < 1e-6, t
  assert np.abs(sim.temps().cpu().numpy() - g["final_grid"]).max() < T_TOL
  ref_cum = g["rates"].astype(np.float64).sum(axis=0) * 300.0
  assert np.allclose(sim.scalars().cpu().numpy()[:, 12:16], ref_cum, rtol=1e-6)


def test_restored_day_matches_the_reference_golden_twice(monkeypatch):
  need_gpu()
  sim, g = _r9_sim("reg", 5, monkeypatch)
  sim.reset()
  bufs = step_buffers(sim)
  obs, rew, info = bufs
  for t in range(144):
    act = torch.tensor(np.tile(g["actions_norm"][t], (5, 1)), dtype=torch.float32, device="cuda")
    sim.step(act, step_in(g, t), obs, rew, info)
  assert np.abs(sim.temps().cpu().numpy() - g["grid_144"]).max() < T_TOL
  snap = sim.save_state()
  _check_golden_from(sim, g, 144, bufs)
  sim.load_state(snap)
  assert np.abs(sim.temps().cpu().numpy() - g["grid_144"]).max() < T_TOL
  _check_golden_from(sim, g, 144, bufs)
  sim.close()


def _twin_step(twin, g, tt, t, a):
  return twin.step(**step_kwargs(g, tt, t, SimConfig.sb1(), a))


def test_fork_against_the_oracle(monkeypatch):
  need_gpu()
  B = 16
  sim, g = _r9_sim("reg", B, monkeypatch)
  init, acts = _seeded(B, 30, 13)
  acts_np = acts.cpu().numpy()
  sim.reset(temps=init)
  p = load("plan_r9_sb1.npz")
  plan, prm = oracle_plan(p), oracle_params(g["params_json"])
  init_np = init.cpu().numpy()
  twins = [orc.OracleBuilding(plan, prm, 0.0, reset_temps=init_np[b]) for b in range(B)]
  bufs = step_buffers(sim)
  obs, rew, info = bufs
  for t in range(10):
    sim.step(acts[t], step_in(g, 100 + t), obs, rew, info)
    for b in range(B):
      _twin_step(twins[b], g, 100 + t, t, acts_np[t, b])
  src = [3, 3, 0, 7, 7, 7, 15, 2, 9, 9, 1, 4, 4, 12, 3, 0]
  uniq, inv = torch.unique(torch.tensor(src, device="cuda"), return_inverse=True)   # (what BatchedEnvironment.fork does)
  sim.load_state(sim.save_state(rows=uniq), pick=inv, clock=False)
  copies = [orc.OracleBuilding(plan, prm, 0.0, reset_temps=init_np[b]) for b in range(B)]
  for b in range(B):
    copy_twin(copies[b], twins[src[b]])
  twins = copies
  for t in range(10, 30):
    sim.step(acts[t], step_in(g, 100 + t), obs, rew, info)
    i = info.cpu().numpy()
    zt = sim.zone_temps().cpu().numpy()
    for b in range(B):
      o = _twin_step(twins[b], g, 100 + t, t, acts_np[t, b])
      assert i[b, 4] == o["n_sweeps"], (t, b)
      assert np.abs(zt[b] - o["zone_temp_post"]).max() < 1e-9, (t, b)
  grid = sim.temps().cpu().numpy()
  for b in range(B):
    assert np.abs(grid[b] - twins[b].grid()).max() < 1e-9, b
  sim.close()


def test_environment_fork_identity_and_broadcast():
  need_gpu()
  B, k = 16, 5
  plan = FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)
  envs = [BatchedEnvironment(plan, B, collect_info=True) for _ in range(2)]
  gen = torch.Generator(device="cuda")
  gen.manual_seed(8)
  acts = torch.rand((20, B, 2), generator=gen, device="cuda") * 2 - 1
  for e in envs:
    e.reset()
    _env_run(e, acts, 8, record=False)
  before = [envs[0].sim.temps(), envs[0].sim.scalars(), envs[0].sim.modes(), envs[0].sim.zone_temps()]
  envs[0].fork(torch.arange(B, device="cuda"))
  after = [envs[0].sim.temps(), envs[0].sim.scalars(), envs[0].sim.modes(), envs[0].sim.zone_temps()]
  assert_same([before], [after])
  envs[0].fork(torch.full((B,), k, dtype=torch.int64, device="cuda"))
  same = acts[8:, k:k + 1].expand(-1, B, -1).contiguous()   # building k's actions in every row
  forked = _env_run(envs[0], same, 10)
  control = _env_run(envs[1], acts[8:], 10)
  for t, (x, y) in enumerate(zip(forked, control)):
    for j, (u, v) in enumerate(zip(x, y)):   # every row of the forked env is the control's row k
      assert torch.equal(u, v[k:k + 1].expand_as(u)), (t, j)
  with pytest.raises(ValueError):
    envs[0].fork(torch.full((B,), B, dtype=torch.int64, device="cuda"))
  with pytest.raises(ValueError):
    envs[0].fork(torch.zeros((B,), dtype=torch.int32, device="cuda"))
  for e in envs:
    e.close()


@pytest.mark.parametrize("src,dst", [("reg", "lds-columns"), ("lds-columns", "reg")])
def test_snapshot_moves_between_layouts_and_orientations(src, dst, monkeypatch):
  need_gpu()
  B = 64
  a, g = _r9_sim(src, B, monkeypatch)
  b, _ = _r9_sim(dst, B, monkeypatch)
  assert a.transposed != b.transposed and (a.launch_info["path"] == 0) != (b.launch_info["path"] == 0)
  init, acts = _seeded(B, 40, 17)
  a.reset(temps=init)
  b.reset(temps=init)   # (b's own clock: reset once, like a's)
  ba, bb = step_buffers(a), step_buffers(b)
  _run(a, g, acts, 0, 20, ba)
  b.load_state(a.save_state())
  assert torch.equal(a.temps(), b.temps()) and torch.equal(a.scalars(), b.scalars())
  assert torch.equal(a.modes(), b.modes()) and torch.equal(a.zone_temps(), b.zone_temps())
  for t in range(20, 40):
    _run(a, g, acts, t, 1, ba)
    _run(b, g, acts, t, 1, bb)
    assert torch.equal(ba[2][:, 4], bb[2][:, 4]), t
    assert float((a.zone_temps() - b.zone_temps()).abs().max()) < 1e-9, t
  assert float((a.temps() - b.temps()).abs().max()) < 1e-9
  a.close()
  b.close()


def test_disk_checkpoint_restores_in_a_new_environment(tmp_path):
  need_gpu()
  B = 32
  env = _stochastic_env(B)
  gen = torch.Generator(device="cuda")
  gen.manual_seed(6)
  acts = torch.rand((25, B, 2), generator=gen, device="cuda") * 2 - 1
  env.reset()
  _env_run(env, acts, 15, record=False)
  path = tmp_path / "ckpt.pt"
  torch.save(env.snapshot().state_dict(), path)
  first = _env_run(env, acts[15:], 10)
  env.close()
  fresh = _stochastic_env(B)
  ts = fresh.restore(EnvSnapshot.from_state_dict(torch.load(path), "cuda"))
  assert bool((ts.step_type == 1).all())
  again = _env_run(fresh, acts[15:], 10)
  assert_same(first, again)
  fresh.close()


def test_mixed_environment_restore_and_cross_class_fork():
  need_gpu()
  plans = [FloorPlan.from_file_input(rectangular_floor_plan(r, s), Materials.sb1(), 10.0, 300.0)
           for r, s in (((3, 3), (20, 30)), ((2, 3), (9, 10)), ((2, 2), (5, 9)))]
  env = MixedBatchedEnvironment([(plans[0], 8), (plans[1], 6), (plans[2], 4)], collect_info=True)
  B = env.batch_size
  gen = torch.Generator(device="cuda")
  gen.manual_seed(9)
  acts = torch.rand((20, B, 2), generator=gen, device="cuda") * 2 - 1

  def run(t0, n):
    out = []
    for t in range(t0, t0 + n):
      ts = env.step(acts[t])
      out.append([ts.step_type.clone(), ts.reward.clone(), ts.observation.clone()] + [e.sim.temps() for e in env.envs])
    return out

  env.reset()
  run(0, 8)
  snaps = env.snapshot()
  first = run(8, 10)
  env.restore(snaps)
  again = run(8, 10)
  assert_same(first, again)
  src = torch.arange(B, device="cuda")
  src[0] = 9   # building 9 is in the second class
  with pytest.raises(ValueError):
    env.fork(src)
  src = torch.arange(B, device="cuda")
  src[1], src[9] = 0, 8   # within the classes
  env.fork(src)
  assert torch.equal(env.envs[0].sim.temps()[1], env.envs[0].sim.temps()[0])
  env.close()


def test_full_size_round_trip_is_bitwise():
  need_gpu()
  B = 65536
  g = load("h2_sb1_r9_random.npz")
  sim = BatchedSimulator(plan_from_npz(load("plan_r9_sb1.npz")), SimConfig.sb1(), B, float(g["h_conv"]))
  gen = torch.Generator(device="cuda")
  gen.manual_seed(5)
  t0 = (294.0 + torch.randn((B, 1), generator=gen, device="cuda", dtype=torch.float64)).clamp(285.0, 305.0)
  init = (t0 + 0.05 * torch.randn((B, 68 * 98), generator=gen, device="cuda", dtype=torch.float64)).contiguous()
  acts = torch.rand((3, B, 2), generator=gen, device="cuda") * 2 - 1
  sim.reset(temps=init)
  _run(sim, g, acts, 0, 3, step_buffers(sim))
  want = [sim.temps(), sim.scalars(), sim.modes(), sim.zone_temps()]
  snap = sim.save_state()
  sim.reset(temps=init)   # everything else
  sim.load_state(snap)
  got = [sim.temps(), sim.scalars(), sim.modes(), sim.zone_temps()]
  assert_same([want], [got])
  sim.close()


def test_refusals_before_any_launch(monkeypatch):
  need_gpu()
  sim, g = _r9_sim("reg", 8, monkeypatch)
  snap = sim.save_state()
  other_plan = FloorPlan.from_file_input(rectangular_floor_plan((2, 3), (9, 10)), Materials.sb1(), 10.0, 300.0)
  other = BatchedSimulator(other_plan, SimConfig.sb1(), 8, float(g["h_conv"]))
  with pytest.raises(ValueError):
    other.load_state(snap)
  cfg = SimConfig.sb1()
  cfg.boiler_heating_rate = 0.6
  other_cfg = BatchedSimulator(plan_from_npz(load("plan_r9_sb1.npz")), cfg, 8, float(g["h_conv"]))
  with pytest.raises(ValueError):
    other_cfg.load_state(snap)
  occ = BatchedSimulator(plan_from_npz(load("plan_r9_sb1.npz")), SimConfig.sb1(), 8, float(g["h_conv"]))
  occ.occupancy_attach(10, (5, 10, 15, 19), 300.0, 1)
  with pytest.raises(ValueError):
    occ.load_state(snap)
  with pytest.raises(ValueError):
    sim.load_state(occ.save_state())
  before = sim.temps()
  for bad in (torch.full((8,), 8, dtype=torch.int64, device="cuda"), torch.zeros((7,), dtype=torch.int64, device="cuda"),
              torch.zeros((8,), dtype=torch.float32, device="cuda"), torch.zeros((8,), dtype=torch.int64)):
    with pytest.raises(ValueError):
      sim.load_state(snap, pick=bad)
  with pytest.raises(ValueError):
    sim.save_state(rows=torch.tensor([0, 8], device="cuda"))
  assert torch.equal(before, sim.temps())
  for s in (sim, other, other_cfg, occ):
    s.close()
