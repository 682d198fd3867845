"""GPU: the hand-over between buildings in every persistent sweep kernel (tests/handover_cases.py).

The other oracle-checked tests run fewer buildings than there are resident workgroups, so every workgroup runs ONE
building and nothing a kernel keeps from one building to the next is ever read.  Here:

  * SBSIM_DEBUG_CUS=1 shrinks the launch to one CU's workgroups, and the divergent batches are large enough for every
    workgroup (wavefront, on k_sweep_roll and k_sweep_lds) to run at least four buildings: every building against its
    own oracle twin at every step, at the bars of tests/twins.py (tests/parity.py's check_plan_against_oracle, unchanged);
    k_sweep_jacobi bitwise against tests/jacobi_restatement.py;
  * the device's own geometry, no switch: just more buildings than are handed out by index, the drawn ones and a fixed
    sample of the others against their twins;
  * the same batch with SBSIM_DEBUG_CUS=1, =3 and unset: who runs a building must not change a bit of the result
    (k_sweep_stream: tests/parity.py's assert_close -- its zone sums are LDS atomics in arrival order).

Every case asserts its kernel, its wavefront count and its hand-over depth from launch_info.

Wall time of this file, oracle twins included: 17.6 s on an MI355X host (the C oracle is about 10 s of it); its CPU
companion tests/test_handover_cases_cpu.py: 37 .. 50 s on a slower CPU-only host (it runs 63 twins per plan of the five
device-geometry batches where this file runs 15)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd.environment import BatchedSimulator  # noqa: E402
from tests import handover_cases as hc  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import (assert_close, assert_same, check_plan_against_oracle, jacobi_env, need_gpu,  # noqa: E402
                          rollout_against_restatement, step_buffers)
from tests.twins import step_in  # noqa: E402


def _depth_check(case, B, cus):
  """launch_info of the case's simulator: the pinned kernel, wavefront count and sweep steps (together: the
  instantiation), and the hand-over depth -- with the launch capped at `cus` CUs, B buildings make every workgroup /
  wavefront run at least hc.DEPTH of them when cus == 1."""
  def check(info):
    assert (info["kernel"], info["waves_per_building"], info["path"]) == (case.kernel, case.waves, case.path), info
    assert info["sweep_steps"] == case.steps, info
    static = hc.static_count(info)
    if cus == 1:
      assert B >= hc.DEPTH * static + 3, (case.name, B, static, info)
  return check


@pytest.mark.parametrize("name", list(hc.CASES))
def test_every_building_against_its_twin_four_handovers_deep(name, monkeypatch):
  case = hc.CASES[name]
  fp = hc.floor_plan(case)
  init, acts, _ = hc.case_batch(case)
  env = dict(case.env)
  env[hc.SWITCH] = "1"
  infos, _ = check_plan_against_oracle(fp, fp.n_zones, case.orientation, case.path, monkeypatch, expect_kernel=case.kernel,
                                       expect_waves=case.waves, B=case.B, T=case.T, init=init, acts=acts,
                                       cfg=hc.config(case), env=env, on_launch=_depth_check(case, case.B, 1))
  n, conv = np.stack([i[:, 4] for i in infos]), np.stack([i[:, 5] for i in infos])
  assert hc.spread(n, conv, case.limit) is not None   # (equal to the oracle's, which the CPU test holds to the spread)


@pytest.mark.parametrize("name", list(hc.NATURAL))
def test_drawn_buildings_on_the_devices_own_geometry(name, monkeypatch):
  """No switch: B = the buildings handed out by index + 7, so buildings static .. static + 6 are exactly the drawn ones.
  All of them, and a fixed sample of 8 of the others, against their twins at every step."""
  need_gpu()
  case = hc.natural_case(name)
  monkeypatch.delenv(hc.SWITCH, raising=False)
  static = hc.natural_static(case)
  B = static + hc.NATURAL_EXTRA
  fp = hc.floor_plan(case)
  init, acts, _ = hc.case_batch(case, B)

  def check(info):
    _depth_check(case, B, None)(info)
    assert hc.static_count(info) == static, (info, static)   # the device is the one the probe assumed

  check_plan_against_oracle(fp, fp.n_zones, case.orientation, case.path, monkeypatch, expect_kernel=case.kernel,
                            expect_waves=case.waves, B=B, T=case.T, init=init, acts=acts, cfg=hc.config(case),
                            env=dict(case.env), buildings=hc.natural_checked(static), on_launch=check)


@pytest.mark.parametrize("name", list(hc.JACOBI_CASES))
def test_jacobi_every_building_bitwise_four_handovers_deep(name, monkeypatch):
  """k_sweep_jacobi's `next` broadcast: every building of a divergent batch, every step, bitwise against the restatement
  (tests/test_jacobi_gpu.py's rollout check with the whole batch sampled)."""
  need_gpu()
  case = hc.JACOBI_CASES[name]
  fp = hc.floor_plan(case)
  monkeypatch.setenv(hc.SWITCH, "1")
  env = jacobi_env(fp, case.B, config=hc.config(case))
  _depth_check(case, case.B, 1)(env.sim.launch_info)   # (one building per workgroup at a time)
  env.reset()
  init, _, _ = hc.case_batch(case)
  env.sim.reset(temps=torch.tensor(init.astype(np.float32).astype(np.float64), dtype=torch.float64, device="cuda"))
  seen = rollout_against_restatement(env, case.T, case.B, seed=7)
  print(f"{name}: iteration counts {sorted(set(seen))}")
  # the restatement's own iteration counts: some buildings end at the limit, others well before it
  assert max(seen) == case.limit and min(seen) < case.limit // 2 and len(set(seen)) >= 5, sorted(set(seen))
  env.close()


def _record(case, fp, init, acts, cus, monkeypatch):
  """The case's rollout with SBSIM_DEBUG_CUS=cus (None: unset): every output of every step."""
  g = load("h2_sb1_r9_random.npz")
  for k, v in hc.case_env(case).items():
    monkeypatch.setenv(k, v)
  if cus is None:
    monkeypatch.delenv(hc.SWITCH, raising=False)
  else:
    monkeypatch.setenv(hc.SWITCH, str(cus))
  sim = BatchedSimulator(fp, hc.config(case), case.B, float(g["h_conv"]), solver=case.solver,
                         orientation="rows" if case.orientation == "generic" else case.orientation)
  info = dict(sim.launch_info)
  _depth_check(case, case.B, cus)(info)
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  obs, rew, inf = step_buffers(sim)
  out = []
  for t in range(case.T):
    sim.step(torch.tensor(acts[t], device="cuda"), step_in(g, hc.tc.TT0 + t), obs, rew, inf)
    out.append([obs.clone(), rew.clone(), inf.clone(), sim.temps(), sim.scalars(), sim.modes(), sim.zone_temps()])
  sim.close()
  return info, out


@pytest.mark.parametrize("name", list(hc.CASES) + list(hc.JACOBI_CASES))
def test_result_does_not_depend_on_who_runs_a_building(name, monkeypatch):
  """SBSIM_DEBUG_CUS=1, =3 and unset: the planner's choice (kernel, path, wavefronts, LDS bytes, sweep steps) is the
  same, only the workgroup count follows the switch; obs, reward, info, grids, scalars, modes and zone temperatures are
  torch.equal (k_sweep_stream: assert_close)."""
  need_gpu()
  case = hc.CASES.get(name) or hc.JACOBI_CASES[name]
  fp = hc.floor_plan(case)
  init, acts, _ = hc.case_batch(case)
  if case.solver == "jacobi_fp32":
    init = init.astype(np.float32).astype(np.float64)
  runs = {cus: _record(case, fp, init, acts, cus, monkeypatch) for cus in (1, 3, None)}
  base = runs[None][0]
  for cus in (1, 3):
    info = runs[cus][0]
    assert all(info[k] == base[k] for k in hc.PINNED), (cus, info, base)
    assert hc.static_count(info) <= hc.static_count(base)
    # the capped geometry: as many workgroups as `cus` CUs hold, i.e. cus times what one CU holds
    assert info["workgroups"] == min(cus * runs[1][0]["workgroups"], base["workgroups"]), (cus, info, base)
    (assert_close if case.kernel == hc.STREAM else assert_same)(runs[cus][1], runs[None][1])
  assert float(runs[None][1][-1][2][:, 4].sum()) > 0   # (the sweeps ran)
