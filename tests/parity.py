"""The device side of the parity harness: a batch on the GPU against the oracle twins of tests/twins.py, and the checks
several GPU test modules share.  Imports torch: the GPU test modules use it, the CPU suite never does."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from sbsim_amd import _ffi
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, SimConfig, observation_field_names
from sbsim_amd.floorplan import FloorPlan, Materials
from tests import jacobi_restatement as jr
from tests.golden_util import load
from tests.twins import RATE_RTOL, T_TOL, assert_step_matches, oracle_twin, step_in, step_kwargs

C_AIR = 1006.0            # J / (kg K), vav.py:197-217
JACOBI_ZONE_TOL = 1e-11   # K: device zone means against float64 means of the float32 grid
JACOBI_H_CONV = 100.0     # BatchedEnvironment's default weather: WeatherController(273, 283, convection_coefficient=100)


def need_gpu():
  if not torch.cuda.is_available():
    pytest.skip("no GPU")


def need_experimental_kernels(variant, monkeypatch):
  """The multi-sweep / overlapped streaming kernels are exact but slower than k_sweep_stream: since round 6 they are in the
  library only when it is built with SBSIM_BUILD_EXPERIMENTAL=1 (sbsim_amd/build.py); the default library ignores the flags.
  __graft_entry__.build() builds that library too (sbsim_amd/libsbsim_amd_exp.so): a test of those kernels loads it in
  place of the default one for its duration."""
  if variant and not _ffi.load().sb_has_experimental_kernels():
    monkeypatch.setattr(_ffi, "LIB_PATH", os.path.join(os.path.dirname(_ffi.__file__), "libsbsim_amd_exp.so"))
    monkeypatch.setattr(_ffi, "_lib", None)
    assert _ffi.load().sb_has_experimental_kernels()


def step_buffers(sim):
  """(obs, rew, info): the output buffers of sb_step for the simulator's batch."""
  B = sim.B
  return (torch.zeros((B, sim.O), dtype=torch.float32, device="cuda"), torch.zeros((B,), dtype=torch.float32, device="cuda"),
          torch.zeros((B, _ffi.SB_INFO_STRIDE), dtype=torch.float32, device="cuda"))


def check_plan_against_oracle(file_plan, n_zones, orientation, path, monkeypatch, expect_steps=None,
                              iteration_limit=None, expect_kernel=None, B=6, T=14, expect_waves=None,
                              init=None, acts=None, cfg=None, env=None, buildings=None, on_launch=None,
                              golden=None, on_step=None, force_path=True, h_conv=None, step_sec=300.0,
                              on_end=None):
  """Every building against its oracle twin at every step.  `file_plan` may be a FloorPlan; `init` [B, H*W], `acts`
  [T, B, 2] and `cfg` replace the seeded initial grids, actions and SimConfig.sb1(); `env` sets developer switches;
  `buildings` names the buildings that get a twin (default: every one); `on_launch` is called with the launch_info;
  `golden` replaces the step-input rows of h2_sb1_r9_random.npz; `on_step(sim, t, obs, outs)` is called after every
  step's own checks with the observation rows (numpy) and the twins' results of the step ({building: dict});
  `force_path=False` leaves the choice between the LDS-grid and the streaming kernel to the library (`path` is then
  only what the launch must report); `h_conv` replaces the rows' convection coefficient and `step_sec` the 300 s between
  the twins' timestamps (a cfg of another time_step_sec); `on_end(grid, twins)` is called with the final grids
  [B, H, W] and the twins ({building: OracleBuilding}) before the final grids are compared.
  Returns the info rows and the grids after every step."""
  need_gpu()
  for k, v in dict(env or {}).items():
    monkeypatch.setenv(k, v)
  g = load("h2_sb1_r9_random.npz") if golden is None else golden
  plan = file_plan if isinstance(file_plan, FloorPlan) else FloorPlan.from_file_input(file_plan, Materials.sb1(), 10.0, 300.0)
  H, W = plan.shape
  rs = np.random.RandomState(11)
  init_r = np.clip(294.0 + 2.0 * rs.randn(B, 1) + 0.2 * rs.randn(B, H * W), 285.0, 305.0)
  acts_r = rs.uniform(-1, 1, size=(T, B, 2)).astype(np.float32)
  init = init_r if init is None else init
  acts = acts_r if acts is None else acts
  cfg = SimConfig.sb1() if cfg is None else cfg
  if iteration_limit is not None:
    cfg = dataclasses.replace(cfg, iteration_limit=iteration_limit)
  if orientation == "generic":
    monkeypatch.setenv("SBSIM_FORCE_GENERIC_SWEEP", "1")
    orientation = "rows"
  if path == 0 and force_path:
    monkeypatch.setenv("SBSIM_FORCE_LDS_PATH", "1")
  if path == 2 and H * W < 100000 and force_path:
    monkeypatch.setenv("SBSIM_FORCE_STREAM_PATH", "1")   # small plans reach the streaming kernel only when told to
  h_conv = float(g["h_conv"]) if h_conv is None else float(h_conv)
  sim = BatchedSimulator(plan, cfg, B, h_conv, orientation=orientation)
  assert sim.Z == n_zones and sim.launch_info["path"] == path
  if expect_steps is not None:
    assert sim.launch_info["sweep_steps"] == expect_steps   # the two-rows kernel with two tail rows
  if expect_kernel is not None:
    assert sim.launch_info["kernel"] == expect_kernel
  if expect_waves is not None:
    assert sim.launch_info["waves_per_building"] == expect_waves
  if on_launch is not None:
    on_launch(sim.launch_info)
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  checked = list(range(B)) if buildings is None else [int(b) for b in buildings]
  twins = {b: oracle_twin(plan, cfg, init[b]) for b in checked}
  obs, rew, info = step_buffers(sim)
  infos, grids = [], []
  for t in range(T):
    tt = 96 + t   # mid-morning: occupied, comfort mode
    sim.step(torch.tensor(acts[t], device="cuda"), step_in(g, tt), obs, rew, info)
    i = info.cpu().numpy().astype(np.float64)
    zt = sim.zone_temps().cpu().numpy()
    r = rew.cpu().numpy()
    infos.append(i)
    grids.append(sim.temps().cpu().numpy())
    outs = {}
    for b in checked:
      o = twins[b].step(**step_kwargs(g, tt, t, cfg, acts[t, b], h_conv=h_conv, step_sec=step_sec))
      assert_step_matches(i[b], zt[b], r[b], o, (t, b))
      outs[b] = o
    if on_step is not None:
      on_step(sim, t, obs.cpu().numpy(), outs)
  grid = sim.temps().cpu().numpy()
  if on_end is not None:
    on_end(grid, twins)
  for b in checked:
    assert np.abs(grid[b] - twins[b].grid()).max() < T_TOL, b
  sim.close()
  return infos, grids


def zone_checks(cfg):
  """An on_step hook of check_plan_against_oracle: the per-zone state of every building against its twin's."""
  q_tol = cfg.vav_max_air_flow_rate * C_AIR * 2.0 * T_TOL    # air * c_air * (tzs - tz) with both off by T_TOL

  def on_step(sim, t, obs, outs):
    modes = sim.modes().cpu().numpy()
    power = sim.zone_power().cpu().numpy()
    scal = sim.scalars().cpu().numpy()
    damper = sim.save_state().zone[:, 2, :].cpu().numpy()
    col = np.asarray(observation_field_names(sim.zone_names, cfg.ahu_has_weather_sensor)[3])
    flow32 = np.float32(cfg.vav_max_air_flow_rate)
    for b, o in outs.items():
      assert np.array_equal(modes[b], o["mode"]), (t, b, np.flatnonzero(modes[b] != o["mode"]))
      assert np.array_equal(damper[b], o["damper"]), (t, b, np.flatnonzero(damper[b] != o["damper"]))
      dq = np.abs(power[b] - o["q_zone"])
      assert (dq <= q_tol + 1e-12 * np.abs(o["q_zone"])).all(), (t, b, int(dq.argmax()), dq.max())
      assert (scal[b, 3], scal[b, 6]) == (o["ahu_count"], o["blr_count"]), (t, b, scal[b, 3], scal[b, 6])
      got = np.array([scal[b, 2], scal[b, 5], scal[b, 7]])
      ref = np.array([o["ahu_flow"], o["blr_flow"], o["blr_return_temp"]])
      assert np.allclose(got, ref, rtol=RATE_RTOL, atol=0.0), (t, b, got, ref)
      assert np.array_equal(obs[b, col], o["damper"].astype(np.float32)), (t, b)
      assert (obs[b, col + 1] == flow32).all(), (t, b)
      want = o["zone_air_temp"].astype(np.float32)
      assert np.array_equal(obs[b, col + 2], want), (t, b, np.flatnonzero(obs[b, col + 2] != want))

  return on_step


def assert_same(a, b):
  """Two recordings [step][tensor] of a run are equal bit for bit."""
  for t, (x, y) in enumerate(zip(a, b)):
    for k, (u, v) in enumerate(zip(x, y)):
      assert torch.equal(u, v), (t, k, float((u.double() - v.double()).abs().max()))


def assert_close(a, b):
  """k_sweep_stream adds a building's zone sums with LDS atomics from several wavefronts, in the order they arrive: its
  zone means and grid sum are not bitwise repeatable from run to run, snapshot or not.  A replay on it meets the bar of
  the layout test instead: equal sweep counts and modes, grids within 1e-9 K."""
  for t, (x, y) in enumerate(zip(a, b)):
    obs, rew, info, temps, scal, modes, zt = zip(x, y)
    assert torch.equal(*modes) and torch.equal(info[0][:, 4], info[1][:, 4]), t
    assert float((temps[0] - temps[1]).abs().max()) < 1e-9 and float((zt[0] - zt[1]).abs().max()) < 1e-9, t
    assert float((rew[0] - rew[1]).abs().max()) < 1e-6 and torch.allclose(obs[0], obs[1], rtol=1e-5, atol=1e-5), t
    assert torch.allclose(scal[0], scal[1], rtol=1e-12, atol=1e-9), t


# ---- solver="jacobi_fp32" (k_sweep_jacobi) against tests/jacobi_restatement.py ----

def bits_equal(a, b):
  return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def jacobi_env(fp, B, **kw):
  env = BatchedEnvironment(fp, B, holiday_calendar=None, collect_info=True, solver="jacobi_fp32", **kw)
  env._plan_for_tests = fp
  return env


def rollout_against_restatement(env, steps, sample, seed):
  """Every step: the device grid after it equals the restatement of the step from the grid before it, the device's
  own q (the zone power of the previous step) and the step's ambient temperature."""
  sim, fp = env.sim, env._plan_for_tests
  tt = jr.tensors(fp, env.config.time_step_sec, JACOBI_H_CONV)
  rs = np.random.RandomState(seed)
  B = env.batch_size
  iters_seen = []
  for t in range(steps):
    picks = rs.choice(B, size=min(sample, B), replace=False)
    pk = torch.as_tensor(picks, device=sim.tdev)
    before = sim.temps()[pk].cpu().numpy().astype(np.float32)
    qz = sim.zone_power()[pk].cpu().numpy()
    tinf = env.make_step_in(env.current_simulation_timestamp).t_amb_now
    act = torch.tensor(rs.uniform(-1, 1, (B, env.action_spec().shape[0])), dtype=torch.float32, device="cuda")
    env.step(act)
    after = sim.temps()[pk].cpu().numpy()
    info = env.info[pk].cpu().numpy()
    for k, b in enumerate(picks):
      want, wi, wc = jr.fd_timestep(tt, before[k], jr.input_q(fp, qz[k]), tinf, env.config.time_step_sec,
                                    env.config.convergence_threshold, env.config.iteration_limit)
      assert int(info[k, 4]) == wi and bool(info[k, 5]) == wc, (t, b, info[k, 4], wi)
      assert np.array_equal(after[k], want.astype(np.float64)), (t, b, np.abs(after[k] - want).max())
      iters_seen.append(wi)
  return iters_seen


def jacobi_tap_bitwise(sim, fp, cfg, h_conv, seed, limit=None):
  """sb_tap_jacobi on seeded float32 grids, zone powers and ambient temperatures, one draw per building of the batch:
  grids bitwise, iteration counts and converged flags EQUAL to the restatement's.  Returns (iterations, converged)."""
  limit = cfg.iteration_limit if limit is None else limit
  n = sim.B
  tt = jr.tensors(fp, cfg.time_step_sec, h_conv)
  rs = np.random.RandomState(seed)
  tprev = (288.0 + 8.0 * rs.rand(n, *fp.shape)).astype(np.float32)
  q = np.stack([jr.input_q(fp, rs.uniform(-3000.0, 3000.0, fp.n_zones)) for _ in range(n)])
  tinf = rs.uniform(265.0, 305.0, n)
  grid, iters, conv = sim.tap_jacobi(tprev, q, tinf)
  for b in range(n):
    want, wi, wc = jr.fd_timestep(tt, tprev[b], q[b], tinf[b], cfg.time_step_sec, cfg.convergence_threshold, limit)
    assert (iters[b], bool(conv[b])) == (wi, wc), (b, iters[b], wi)
    assert bits_equal(grid[b], want), (b, np.abs(grid[b] - want).max())
  return iters, conv


def jacobi_zone_means_follow_grid(sim, fp, g, init, acts):
  """len(acts) real steps from `init` on rows 96 + t of `g`: the grid stays a float32 grid, widened, and the device's
  zone means are the float64 means of it."""
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  obs, rew, info = step_buffers(sim)
  zlab = fp.zone_label.reshape(-1)
  for t in range(len(acts)):
    sim.step(torch.tensor(acts[t], device="cuda"), step_in(g, 96 + t), obs, rew, info)
    flat = sim.temps().cpu().numpy().reshape(sim.B, -1)
    assert np.array_equal(flat, flat.astype(np.float32).astype(np.float64))       # a float32 grid, widened
    means = np.stack([flat[:, zlab == z].mean(axis=1) for z in range(fp.n_zones)], axis=1)
    zt = sim.zone_temps().cpu().numpy()
    assert np.abs(zt - means).max() <= JACOBI_ZONE_TOL, (t, np.abs(zt - means).max())
