"""GPU: solver="jacobi_fp32" on floor plans beyond one CU's LDS -- k_sweep_jacobi_g (step_jacobi_global.hip,
launch_info["path"] == 2), held bitwise to the NumPy restatement (tests/jacobi_restatement.py), to the reference's
recorded finite_differences_timestep outputs, and to k_sweep_jacobi on the plans both kernels take."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, MixedBatchedEnvironment, SimConfig  # noqa: E402
from tests import jacobi_restatement as jr  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.jacobi_cases import GOLDEN_PLANS, PLAN_155, PLAN_SB1, golden_plan, large_case, large_plan  # noqa: E402
from tests.parity import JACOBI_H_CONV as H_CONV, bits_equal, jacobi_env, need_gpu  # noqa: E402
from tests.twins import plan_from_npz  # noqa: E402

f32 = np.float32
FORCE = "SBSIM_FORCE_JACOBI_GLOBAL"


def _is_global(sim):
  return sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI and sim.launch_info["path"] == 2


@pytest.mark.parametrize("plan", [PLAN_155, PLAN_SB1], ids=["155x155", "299x401"])
@pytest.mark.parametrize("limit", [100, 2])
def test_tap_on_large_plans_equals_the_restatement_bitwise(plan, limit):
  """Three buildings with different seeded Tprev, q and T_inf; on 155 x 155 two of them are the reference's cases."""
  need_gpu()
  fp = large_plan(*plan)
  g = load("jacobi_fd_large.npz")
  golden = [int(s) for s in g["seeds"]] if plan == PLAN_155 else []
  seeds = golden + [31, 32, 33][len(golden):]
  cfg = SimConfig.sb1()
  cfg.iteration_limit = limit
  sim = BatchedSimulator(fp, cfg, 3, H_CONV, solver="jacobi_fp32")
  assert _is_global(sim), sim.launch_info
  assert sim.launch_info["state_bytes_per_env_step"] == 8 * fp.shape[0] * fp.shape[1]
  tt = jr.tensors(fp, cfg.time_step_sec, H_CONV)
  cases = [large_case(s, fp.shape, fp.n_zones) for s in seeds]
  tprev = np.stack([c[0] for c in cases])
  q = np.stack([jr.input_q(fp, c[1]) for c in cases])
  tinf = np.array([c[2] for c in cases])
  grid, iters, conv = sim.tap_jacobi(tprev, q, tinf)
  for b, seed in enumerate(seeds):
    want, wi, wc = jr.fd_timestep(tt, tprev[b], q[b], tinf[b], cfg.time_step_sec, cfg.convergence_threshold, limit)
    print(f"[tap {fp.shape} limit {limit} seed {seed}] {wi} iterations, converged={wc}; device {iters[b]}, {conv[b]}")
    assert (iters[b], bool(conv[b])) == (wi, wc), (b, iters[b], wi)
    assert bits_equal(grid[b], want), (b, np.abs(grid[b] - want).max())
    if seed in golden:
      key = f"{seed}_{limit}"
      assert (int(iters[b]), bool(conv[b])) == (int(g[key + "_iterations"]), bool(g[key + "_converged"])), key
      assert bits_equal(grid[b], g[key + "_grid"]), key
  sim.close()


@pytest.mark.parametrize("name", sorted(GOLDEN_PLANS))
@pytest.mark.parametrize("limit", [100, 2])
def test_forced_global_tap_equals_the_reference_fd_timestep_bitwise(name, limit, monkeypatch):
  """test_tap_equals_the_reference_fd_timestep_bitwise's cases on k_sweep_jacobi_g."""
  need_gpu()
  monkeypatch.setenv(FORCE, "1")
  g = load("jacobi_fd.npz")
  fp = golden_plan(name)
  cfg = SimConfig.sb1()
  cfg.iteration_limit, cfg.convergence_threshold, cfg.time_step_sec = limit, float(g["thr"]), float(g["dt"])
  sim = BatchedSimulator(fp, cfg, 2, float(g["h"]), solver="jacobi_fp32")
  assert _is_global(sim), sim.launch_info
  keys = [f"{name}_{case}_{limit}" for case in range(2)]
  tprev = np.stack([g[k + "_prev"] for k in keys]).astype(f32)
  q = np.stack([g[k + "_input_q"] for k in keys]).astype(f32)
  tinf = np.array([float(g[k + "_t_amb"]) for k in keys])
  grid, iters, conv = sim.tap_jacobi(tprev, q, tinf)
  for b, k in enumerate(keys):
    assert (int(iters[b]), bool(conv[b])) == (int(g[k + "_iterations"]), bool(g[k + "_converged"])), k
    assert bits_equal(grid[b], g[k + "_grid"]), (k, np.abs(grid[b] - g[k + "_grid"]).max())
  sim.close()


def _rollout(env, steps, sample, seed, zone_tol=None):
  """tests/test_jacobi_gpu.py's _rollout_against_restatement, and with zone_tol the zone temperatures after each step
  against the float64 mean of the widened grid over the zone's cells."""
  sim, fp = env.sim, env._plan_for_tests
  tt = jr.tensors(fp, env.config.time_step_sec, H_CONV)
  zl = fp.zone_label.reshape(-1)
  rs = np.random.RandomState(seed)
  B = env.batch_size
  seen = []
  for t in range(steps):
    picks = rs.choice(B, size=min(sample, B), replace=False)
    pk = torch.as_tensor(picks, device=sim.tdev)
    before = sim.temps()[pk].cpu().numpy().astype(f32)
    qz = sim.zone_power()[pk].cpu().numpy()
    tinf = env.make_step_in(env.current_simulation_timestamp).t_amb_now
    act = torch.tensor(rs.uniform(-1, 1, (B, env.action_spec().shape[0])), dtype=torch.float32, device="cuda")
    env.step(act)
    after = sim.temps()[pk].cpu().numpy()
    info = env.info[pk].cpu().numpy()
    zt = sim.zone_temps()[pk].cpu().numpy()
    for k, b in enumerate(picks):
      want, wi, wc = jr.fd_timestep(tt, before[k], jr.input_q(fp, qz[k]), tinf, env.config.time_step_sec,
                                    env.config.convergence_threshold, env.config.iteration_limit)
      assert int(info[k, 4]) == wi and bool(info[k, 5]) == wc, (t, b, info[k, 4], wi)
      assert np.array_equal(after[k], want.astype(np.float64)), (t, b, np.abs(after[k] - want).max())
      seen.append(wi)
      if zone_tol is not None:
        flat = after[k].reshape(-1)
        means = np.array([flat[zl == z].mean() for z in range(fp.n_zones)])
        assert np.abs(zt[k] - means).max() <= zone_tol, (t, b, np.abs(zt[k] - means).max())
  return seen


def test_random_action_rollout_on_the_155_plan_every_step_bitwise():
  need_gpu()
  fp = large_plan(*PLAN_155)
  env = jacobi_env(fp, 64)
  assert _is_global(env.sim), env.sim.launch_info
  env.reset()
  seen = _rollout(env, 24, 4, seed=6, zone_tol=1e-11)
  print(f"[rollout 155 x 155] iterations per step {min(seen)} .. {max(seen)}")
  assert min(seen) >= 1
  env.close()


def test_more_buildings_than_resident_workgroups_on_the_sb1_sized_plan():
  """1,536 buildings of 299 x 401: the draw counter, and a workgroup's scratch area reused by its next building."""
  need_gpu()
  fp = large_plan(*PLAN_SB1)
  env = jacobi_env(fp, 1536)
  assert _is_global(env.sim) and env.sim.launch_info["workgroups"] < 1536, env.sim.launch_info
  env.reset()
  g = torch.Generator(device="cuda").manual_seed(8)
  N = fp.shape[0] * fp.shape[1]
  init = (290.0 + 6.0 * torch.rand((1536, N), generator=g, device="cuda")).double()   # (float32-representable)
  env.sim.reset(temps=init)
  del init
  seen = _rollout(env, 3, 8, seed=12)
  print(f"[1536 x 299 x 401] iterations per step {min(seen)} .. {max(seen)}")
  env.close()


def test_r9_batch_is_the_same_on_both_kernels(monkeypatch):
  """256 R9 buildings, 20 random-action steps on k_sweep_jacobi and on k_sweep_jacobi_g: grids, info, rewards and
  observations bit for bit (both kernels add the float64 zone and grid sums in the same order)."""
  need_gpu()
  fp = plan_from_npz(load("plan_r9_sb1.npz"))

  def run(path):
    env = jacobi_env(fp, 256)
    assert env.sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI and env.sim.launch_info["path"] == path
    env.reset()
    rs = np.random.RandomState(21)
    out = []
    for _ in range(20):
      act = torch.tensor(rs.uniform(-1, 1, (256, env.action_spec().shape[0])), dtype=torch.float32, device="cuda")
      ts = env.step(act)
      out.append((env.sim.temps().clone(), env.info.clone(), ts.reward.clone(), ts.observation.clone()))
    env.close()
    return out

  lds = run(0)
  monkeypatch.setenv(FORCE, "1")
  glb = run(2)
  for t, (a, b) in enumerate(zip(lds, glb)):
    for what, x, y in zip(("grid", "info", "reward", "observation"), a, b):
      assert torch.equal(x, y), (t, what)


def test_mixed_batch_with_a_small_and_a_large_class():
  """Resets and steps; every building of the large class equals the restatement of each step bit for bit."""
  need_gpu()
  r9, p155 = plan_from_npz(load("plan_r9_sb1.npz")), large_plan(*PLAN_155)
  mixed = MixedBatchedEnvironment([(r9, 4), (p155, 4)], holiday_calendar=None, collect_info=True, solver="jacobi_fp32")
  infos = [e.sim.launch_info for e in mixed.envs]
  assert [i["kernel"] for i in infos] == [_ffi.SB_KERNEL_JACOBI] * 2
  assert [i["path"] for i in infos] == [0, 2]
  mixed.reset()
  big = mixed.envs[1]
  tt = jr.tensors(p155, big.config.time_step_sec, H_CONV)
  rs = np.random.RandomState(14)
  for t in range(3):
    before = big.sim.temps().cpu().numpy().astype(f32)
    qz = big.sim.zone_power().cpu().numpy()
    tinf = big.make_step_in(big.current_simulation_timestamp).t_amb_now
    ts = mixed.step(torch.tensor(rs.uniform(-1, 1, (8, 2)), dtype=torch.float32, device="cuda"))
    assert torch.isfinite(ts.reward).all()
    after = big.sim.temps().cpu().numpy()
    info = big.info.cpu().numpy()
    for b in range(4):
      want, wi, wc = jr.fd_timestep(tt, before[b], jr.input_q(p155, qz[b]), tinf, big.config.time_step_sec,
                                    big.config.convergence_threshold, big.config.iteration_limit)
      assert int(info[b, 4]) == wi and bool(info[b, 5]) == wc, (t, b, info[b, 4], wi)
      assert np.array_equal(after[b], want.astype(np.float64)), (t, b, np.abs(after[b] - want).max())
  mixed.close()


def test_refusals_are_unchanged_on_a_large_plan():
  need_gpu()
  fp = large_plan(*PLAN_155)
  with pytest.raises(ValueError, match="orientation"):
    BatchedSimulator(fp, SimConfig.sb1(), 2, H_CONV, solver="jacobi_fp32", orientation="columns")
  env = jacobi_env(fp, 2)
  env.reset()
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.snapshot()
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.sim.set_temps(env.sim.temps())
  with pytest.raises(ValueError, match="jacobi_fp32"):
    env.sim.convection_attach(1.0, 5, 0)
  env.close()
