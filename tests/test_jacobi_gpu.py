"""GPU: TFSimulator's float32 Jacobi solver on k_sweep_jacobi (sb_create_jacobi, BatchedEnvironment(solver=
"jacobi_fp32")), held bitwise to the NumPy float32 restatement of the reference's update (tests/jacobi_restatement.py):
the known-answer tap, every step of random-action rollouts, a full-size batch, a mixed batch, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan  # noqa: E402
from tests import jacobi_restatement as jr  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.jacobi_cases import GOLDEN_PLANS, golden_plan  # noqa: E402
from tests.parity import (JACOBI_H_CONV as H_CONV, bits_equal, jacobi_env, jacobi_tap_bitwise, need_gpu,  # noqa: E402
                          rollout_against_restatement, step_buffers)
from tests.twins import RATE_ATOL, RATE_RTOL, plan_from_npz, step_in  # noqa: E402

f32 = np.float32
PLANS = ("plan_r9_sb1.npz", "plan_r9_test.npz", "plan_small_test.npz", "plan_weird_test.npz")


@pytest.mark.parametrize("name", PLANS)
@pytest.mark.parametrize("limit", [100, 2])
def test_tap_equals_the_restatement_bitwise(name, limit):
  need_gpu()
  fp = plan_from_npz(load(name))
  cfg = SimConfig.sb1()
  cfg.iteration_limit = limit
  n = 4
  sim = BatchedSimulator(fp, cfg, n, H_CONV, solver="jacobi_fp32")
  assert sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI
  assert sim.launch_info["state_bytes_per_env_step"] == 8 * fp.shape[0] * fp.shape[1]
  jacobi_tap_bitwise(sim, fp, cfg, H_CONV, seed=11, limit=limit)
  sim.close()


def test_random_action_rollout_every_step_bitwise():
  """288 steps (one day of 5-minute steps) of 256 SB1 R9 buildings under random actions, 8 buildings a step checked."""
  need_gpu()
  fp = plan_from_npz(load("plan_r9_sb1.npz"))
  env = jacobi_env(fp, 256)
  env.reset()
  seen = rollout_against_restatement(env, 288, 8, seed=3)
  assert min(seen) >= 1 and max(seen) < env.config.iteration_limit
  env.close()


def test_full_size_batch_sampled_bitwise():
  """65,536 R9 buildings: the persistent grid's draw counter and the resident workgroups at scale."""
  need_gpu()
  fp = plan_from_npz(load("plan_r9_sb1.npz"))
  env = jacobi_env(fp, 65536)
  env.reset()
  g = torch.Generator(device="cuda").manual_seed(5)
  init = (290.0 + 6.0 * torch.rand((65536, fp.shape[0] * fp.shape[1]), generator=g, device="cuda")).double()
  env.sim.reset(temps=init)   # (float32-representable)
  del init
  rollout_against_restatement(env, 5, 64, seed=9)
  env.close()


def test_mixed_batch_equals_the_single_class_environments():
  need_gpu()
  plans = [plan_from_npz(load(n)) for n in ("plan_r9_sb1.npz", "plan_r9_test.npz", "plan_small_test.npz")]
  counts = [24, 16, 8]
  mixed = MixedBatchedEnvironment(list(zip(plans, counts)), holiday_calendar=None, collect_info=True,
                                  solver="jacobi_fp32")
  singles = [BatchedEnvironment(p, n, holiday_calendar=None, collect_info=True, solver="jacobi_fp32")
             for p, n in zip(plans, counts)]
  mixed.reset()
  for e in singles:
    e.reset()
  rs = np.random.RandomState(2)
  for t in range(12):
    act = torch.tensor(rs.uniform(-1, 1, (sum(counts), 2)), dtype=torch.float32, device="cuda")
    ts = mixed.step(act)
    for k, e in enumerate(singles):
      a, b = mixed.slices[k]
      tk = e.step(act[a:b].contiguous())
      assert torch.equal(ts.reward[a:b], tk.reward), (t, k)
      assert torch.equal(ts.observation[a:b, :e.sim.O], tk.observation), (t, k)
      assert torch.equal(mixed.envs[k].sim.temps(), e.sim.temps()), (t, k)
  mixed.close()
  for e in singles:
    e.close()


def test_mixed_batch_takes_one_solver_per_class():
  need_gpu()
  plans = [plan_from_npz(load(n)) for n in ("plan_r9_sb1.npz", "plan_small_test.npz")]
  mixed = MixedBatchedEnvironment([(plans[0], 4), (plans[1], 4)], holiday_calendar=None,
                                  solver=["jacobi_fp32", "gauss_seidel"])
  assert mixed.envs[0].sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI
  assert mixed.envs[1].sim.launch_info["kernel"] != _ffi.SB_KERNEL_JACOBI
  mixed.reset()
  mixed.step(torch.zeros((8, 2), dtype=torch.float32, device="cuda"))
  mixed.close()


def test_jacobi_refusals():
  need_gpu()
  fp = plan_from_npz(load("plan_small_test.npz"))
  with pytest.raises(ValueError, match="orientation"):
    BatchedSimulator(fp, SimConfig.sb1(), 2, H_CONV, solver="jacobi_fp32", orientation="columns")

  class Conv:
    p, distance, seed = 1.0, 5, 0
  with pytest.raises(ValueError, match="jacobi_fp32"):
    BatchedEnvironment(fp, 2, holiday_calendar=None, solver="jacobi_fp32", convection_simulator=Conv())
  env = BatchedEnvironment(fp, 2, holiday_calendar=None, solver="jacobi_fp32")
  env.reset()
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.snapshot()
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.restore(None)
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.fork(torch.zeros(2, dtype=torch.int64, device="cuda"))
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.sim.convection_attach(1.0, 5, 0)
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.sim.set_temps(env.sim.temps())
  # the C entries answer SB_ERR_UNSUPPORTED themselves
  L = _ffi.load()
  assert L.sb_convection_attach(env.sim._h, 1.0, 5, 0, 0, 0) == -5
  view = _ffi.StateView()
  view.n = 2
  assert L.sb_state_save(env.sim._h, None, 2, C_byref(view), None, 0, None) == -5
  assert L.sb_state_load(env.sim._h, None, C_byref(view), None, 0, None) == -5
  env.close()


def C_byref(x):
  import ctypes
  return ctypes.byref(x)


def test_reset_rounds_the_grid_to_float32_and_keeps_float64_zone_means():
  need_gpu()
  fp = plan_from_npz(load("plan_r9_sb1.npz"))
  sim = BatchedSimulator(fp, SimConfig.sb1(), 2, H_CONV, solver="jacobi_fp32")
  N = fp.shape[0] * fp.shape[1]
  rs = np.random.RandomState(4)
  init = 290.0 + rs.rand(2, N)
  sim.reset(temps=torch.tensor(init, device="cuda"))
  got = sim.temps().reshape(2, N).cpu().numpy()
  assert np.array_equal(got, init.astype(f32).astype(np.float64))
  zl = fp.zone_label.reshape(-1)
  zt = sim.zone_temps().cpu().numpy()
  for z in range(fp.n_zones):
    np.testing.assert_allclose(zt[:, z], init[:, zl == z].mean(axis=1), rtol=0, atol=1e-11)
  sim.close()


# ---- against the reference's own TFSimulator (tests/golden/jacobi_*.npz, tools/gen_golden_jacobi.py) ----


@pytest.mark.parametrize("name", sorted(GOLDEN_PLANS))
@pytest.mark.parametrize("limit", [100, 2])
def test_tap_equals_the_reference_fd_timestep_bitwise(name, limit):
  """(b): k_sweep_jacobi on the reference's finite_differences_timestep cases: grid, iterations, converged flag."""
  need_gpu()
  g = load("jacobi_fd.npz")
  fp = golden_plan(name)
  cfg = SimConfig.sb1()
  cfg.iteration_limit, cfg.convergence_threshold, cfg.time_step_sec = limit, float(g["thr"]), float(g["dt"])
  sim = BatchedSimulator(fp, cfg, 2, float(g["h"]), solver="jacobi_fp32")
  keys = [f"{name}_{case}_{limit}" for case in range(2)]
  tprev = np.stack([g[k + "_prev"] for k in keys]).astype(f32)
  q = np.stack([g[k + "_input_q"] for k in keys]).astype(f32)
  tinf = np.array([float(g[k + "_t_amb"]) for k in keys])
  grid, iters, conv = sim.tap_jacobi(tprev, q, tinf)
  for b, k in enumerate(keys):
    assert (int(iters[b]), bool(conv[b])) == (int(g[k + "_iterations"]), bool(g[k + "_converged"])), k
    assert bits_equal(grid[b], g[k + "_grid"]), (k, np.abs(grid[b] - g[k + "_grid"]).max())
  sim.close()


def test_plan_beyond_8192_cvs_equals_the_restatement_bitwise():
  """The 1,024-thread instantiation (plans of 8,193 .. 20,480 CVs): 83 x 129 = 10,707 CVs."""
  need_gpu()
  from sbsim_amd.floorplan import Materials, rectangular_floor_plan
  fp = FloorPlan.from_file_input(rectangular_floor_plan((3, 4), (25, 30)), Materials.sb1(), 10.0, 300.0)
  assert 8192 < fp.shape[0] * fp.shape[1] <= 20480
  cfg = SimConfig.sb1()
  sim = BatchedSimulator(fp, cfg, 3, H_CONV, solver="jacobi_fp32")
  assert sim.launch_info["waves_per_building"] == 16
  tt = jr.tensors(fp, cfg.time_step_sec, H_CONV)
  rs = np.random.RandomState(17)
  tprev = (286.0 + 10.0 * rs.rand(3, *fp.shape)).astype(f32)
  q = np.stack([jr.input_q(fp, rs.uniform(-3000.0, 3000.0, fp.n_zones)) for _ in range(3)])
  tinf = rs.uniform(265.0, 305.0, 3)
  grid, iters, conv = sim.tap_jacobi(tprev, q, tinf)
  for b in range(3):
    want, wi, wc = jr.fd_timestep(tt, tprev[b], q[b], tinf[b], cfg.time_step_sec, cfg.convergence_threshold, 100)
    assert (iters[b], bool(conv[b])) == (wi, wc)
    assert bits_equal(grid[b], want), (b, np.abs(grid[b] - want).max())
  sim.close()


ZONE_TOL = 1e-4   # K: the device algebra is float64 around the float32 grid; the reference carries float32 zone means


def test_thermostat_only_rollout_against_the_reference():
  """(c) 288 thermostat-only steps of TFSimulator on r9_test: iteration counts equal at every step, zone temperatures
  within ZONE_TOL."""
  need_gpu()
  import json
  g = load("jacobi_h1_r9_test.npz")
  prm = json.loads(str(g["params_json"]))
  cfg = SimConfig(
      time_step_sec=prm["dt"], convergence_threshold=prm["conv_threshold"], iteration_limit=prm["iter_limit"],
      comfort_temp_window=(prm["comfort_lo"], prm["comfort_hi"]), eco_temp_window=(prm["eco_lo"], prm["eco_hi"]),
      vav_max_air_flow_rate=prm["vav_max_air_flow"], vav_reheat_max_water_flow_rate=prm["vav_max_water_flow"],
      ahu_recirculation=prm["ahu_recirc"], ahu_heating_air_temp_setpoint=prm["ahu_heat_sp"],
      ahu_cooling_air_temp_setpoint=prm["ahu_cool_sp"], ahu_fan_differential_pressure=prm["ahu_dp"],
      ahu_fan_efficiency=prm["ahu_eff"], ahu_max_air_flow_rate=prm["ahu_max_flow"], ahu_has_weather_sensor=False,
      boiler_reheat_water_setpoint=prm["blr_setpoint"], boiler_water_pump_differential_head=prm["blr_head"],
      boiler_water_pump_efficiency=prm["blr_pump_eff"], boiler_heating_rate=prm["blr_heating_rate"],
      boiler_cooling_rate=prm["blr_cooling_rate"], initial_temp=float(g["initial_temp"]))
  B = 3
  sim = BatchedSimulator(plan_from_npz(load("plan_r9_test.npz")), cfg, B, float(g["h_conv"]), solver="jacobi_fp32")
  sim.reset()
  _, rew, info = step_buffers(sim)
  comfort = g["comfort"]
  worst = 0.0
  for t in range(len(g["n_sweeps"])):
    si = _ffi.StepIn()
    si.t_amb_now = si.t_amb_next = float(g["t_amb"])
    si.comfort_now, si.comfort_next = int(comfort[t]), int(comfort[t + 1])
    si.comfort_prev = int(comfort[t - 1]) if t else -1
    si.has_action = 0
    si.occupancy, si.e_price, si.e_carbon, si.g_price, si.g_carbon = 1.0, 1e-8, 1e-8, 1e-8, 1e-8
    sim.step(None, si, None, rew, info)
    i = info.cpu().numpy()
    assert (i[:, 4] == g["n_sweeps"][t]).all(), (t, i[:, 4], g["n_sweeps"][t])
    d = np.abs(sim.zone_temps().cpu().numpy() - g["zone_temp_post"][t]).max()
    worst = max(worst, d)
    assert d < ZONE_TOL, (t, d)
  assert np.abs(sim.temps().cpu().numpy() - g["final_grid"]).max() < ZONE_TOL
  print(f"[jacobi r9_test thermostat-only] max |dT_zone| vs reference = {worst:.3e} K")
  sim.close()


def test_random_action_rollout_against_the_reference():
  """(c) 288 random-action SB1 steps of TFSimulator on R9: iteration counts equal at every step, zone temperatures
  within ZONE_TOL, rewards and the blower, gas and pump rates within the library's rtol 2e-6 / abs 1e-6.  The
  air-conditioning rate is flow * c_air * (supply - mixed), and the mixed-air temperature takes the grid mean: a float32
  mean (NumPy's pairwise float32 sum) in the reference, a float64 one here.  It is held to flow * c_air * ZONE_TOL."""
  need_gpu()
  g = load("jacobi_h2_sb1_r9_random.npz")
  B = 4
  sim = BatchedSimulator(plan_from_npz(load("plan_r9_sb1.npz")), SimConfig.sb1(), B, float(g["h_conv"]), solver="jacobi_fp32")
  sim.reset()
  obs, rew, info = step_buffers(sim)
  worst_t = worst_r = worst_rate = 0.0
  for t in range(len(g["n_sweeps"])):
    act = torch.tensor(np.tile(g["actions_norm"][t], (B, 1)), dtype=torch.float32, device="cuda")
    sim.step(act, step_in(g, t), obs, rew, info)
    i = info.cpu().numpy().astype(np.float64)
    assert (i[:, 4] == g["n_sweeps"][t]).all(), (t, i[:, 4], g["n_sweeps"][t])
    d = np.abs(sim.zone_temps().cpu().numpy() - g["zone_temp_post"][t]).max()
    worst_t = max(worst_t, d)
    assert d < ZONE_TOL, (t, d)
    ref_rates = g["rates"][t].astype(np.float64)
    keep = [0, 2, 3]   # blower, gas, pump: as on the Gauss-Seidel path
    assert np.allclose(i[:, keep], ref_rates[keep], rtol=RATE_RTOL, atol=RATE_ATOL), (t, i[0, :4], ref_rates)
    ac_tol = float(g["ahu_flow"][t]) * 1006.0 * ZONE_TOL + 1e-3   # flow * c_air * (the mean's gap, < ZONE_TOL)
    worst_rate = max(worst_rate, float(np.abs(i[:, 1] - ref_rates[1]).max()))
    assert np.abs(i[:, 1] - ref_rates[1]).max() <= ac_tol, (t, i[0, 1], ref_rates[1], ac_tol)
    r = rew.cpu().numpy().astype(np.float64)
    worst_r = max(worst_r, np.abs(r - float(g["reward"][t])).max())
    assert np.allclose(r, float(g["reward"][t]), rtol=RATE_RTOL, atol=RATE_ATOL), (t, r, g["reward"][t])
  print(f"[jacobi sb1 r9 random] max |dT_zone| vs reference = {worst_t:.3e} K, max |d reward| = {worst_r:.3e}, "
        f"max |d air-conditioning W| = {worst_rate:.3e}")
  sim.close()
