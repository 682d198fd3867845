"""GPU parity outside SB1's one coefficient regime (tests/regimes.py): every sweep kernel's smallest pinned plan at every
regime, every building against its CPU-oracle twin at every step.

Through tests/parity.py's check_plan_against_oracle at the bars of tests/twins.py -- sweep counts and converged flags EQUAL,
zone means and the final grid within T_TOL = 1e-8 K, rates at rtol 2e-6 / atol 1e-6, reward within 2e-6 -- with
tests/parity.py's per-zone hook on top (modes, dampers, zone powers, request counts, flows, observation
columns).  tests/test_regimes_cpu.py pins the oracle to the reference at these regimes and checks on the oracle alone
that the inputs make "EQUAL" a fair demand: no sweep's max|delta| within a relative 1e-9 of the threshold, no zone mean
within 1e-6 K of a thermostat threshold.

Further: k_sweep_roll's exact kernel, forced redo list and measuring periods and k_sweep_two with every step overrunning,
at every regime; the float32 Jacobi solver bitwise against tests/jacobi_restatement.py per regime on both of its kernels;
one batch on the per-building-materials handle whose buildings carry four regimes' materials at once.

Every case prints its worst |dT| (zone means over all steps, then the final grid); LABNOTES.md holds the table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator  # noqa: E402
from sbsim_amd.host_inputs import BuildingMaterials  # noqa: E402
from tests import regimes as rg  # noqa: E402
from tests import zone_ladder as zl  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import (check_plan_against_oracle, jacobi_tap_bitwise, jacobi_zone_means_follow_grid, need_gpu,  # noqa: E402
                          step_buffers, zone_checks)
from tests.twins import T_TOL, assert_step_matches, step_in, step_kwargs  # noqa: E402

REGIMES = list(rg.REGIMES)


def _run(case_name, regime_name, monkeypatch):
  c, regime = rg.case(case_name), rg.REGIMES[regime_name]
  fp, cfg = rg.plan(c, regime), rg.case_config(c, regime)
  init, acts = rg.batch(fp.shape[0] * fp.shape[1], regime)
  kernel, waves, steps, path = rg.pin(c, regime)
  env = dict(c.env)
  orientation = c.orientation
  if (kernel, path) != (c.kernel, c.path):      # rg.ROLL_CAPACITY: the planner's own choice, no switch of the case's path
    assert path == 0 and not env
  zone_hook = zone_checks(cfg)
  worst = [0.0, 0.0]

  def on_step(sim, t, obs, outs):
    zt = sim.zone_temps().cpu().numpy()
    worst[0] = max([worst[0]] + [float(np.abs(zt[b] - o["zone_temp_post"]).max()) for b, o in outs.items()])
    zone_hook(sim, t, obs, outs)

  def on_end(grid, twins):
    worst[1] = max(float(np.abs(grid[b] - tw.grid()).max()) for b, tw in twins.items())
    print(f"REGIME-DT {case_name} {regime_name} zone {worst[0]:.3e} grid {worst[1]:.3e}")

  infos, _ = check_plan_against_oracle(fp, fp.n_zones, orientation, path, monkeypatch, expect_steps=steps,
                                       expect_kernel=kernel, expect_waves=waves, B=rg.B, T=rg.T, init=init, acts=acts,
                                       cfg=cfg, env=env, on_step=on_step, on_end=on_end, h_conv=regime.h_conv,
                                       step_sec=regime.time_step_sec, force_path=(kernel, path) == (c.kernel, c.path))
  assert len(infos) == rg.T


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", list(rg.CASES))
def test_every_kernel_at_every_regime(case, regime, monkeypatch):
  _run(case, regime, monkeypatch)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", list(rg.VARIANTS))
def test_roll_and_two_rows_switches_at_every_regime(case, regime, monkeypatch):
  """roll-R9 on k_sweep_roll's exact (float64-compare) kernel, with every third building through the redo list, and with
  every period measuring; two-SB1 with the prediction switched off (every step overruns and is run again)."""
  _run(case, regime, monkeypatch)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kind", list(zl.JACOBI))
def test_jacobi_float32_class_tensors_at_every_regime(kind, regime, monkeypatch):
  """solver="jacobi_fp32" at Z = NW on the LDS-resident plan and on the global-memory variant: sb_tap_jacobi bitwise
  against the restatement with iteration counts and flags EQUAL (the float32 roundings of the class tensors differ at
  every regime), then three real steps whose zone means are the float64 means of the float32 grid."""
  need_gpu()
  env, nw = zl.JACOBI[kind]
  for k, v in env:
    monkeypatch.setenv(k, v)
  r = rg.REGIMES[regime]
  Z = nw
  fp = rg.apply(zl.jacobi_plan(Z), r)
  cfg = rg.config(r, fp)
  g = zl.step_rows()
  Bn = 4
  sim = BatchedSimulator(fp, cfg, Bn, r.h_conv, solver="jacobi_fp32")
  assert sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI and sim.launch_info["path"] == (2 if env else 0)
  assert sim.launch_info["waves_per_building"] == nw and sim.Z == Z
  iters, conv = jacobi_tap_bitwise(sim, fp, cfg, r.h_conv, seed=13)
  print(f"REGIME-JACOBI {kind} {regime} iterations {[int(i) for i in iters]} converged {[int(x) for x in conv]}")
  jacobi_zone_means_follow_grid(sim, fp, g, zl.initial_grids(fp, Bn), zl.actions(3, Bn))
  sim.close()


def test_one_batch_carries_four_regimes_on_the_materials_handle():
  """sb_create_materials / k_sweep_lds<true>: building b with the materials and h_conv of regime rg.MIXED[b % 4]
  (tests/test_building_materials_gpu.py spans factors of 0.2 .. 4; this spans six decades), every building against an
  oracle twin on the plan with its materials substituted."""
  need_gpu()
  g = load("h2_sb1_r9_random.npz")
  fp, cfg, ids, mats, hs, init, acts = rg.mixed_batch()
  B, T = rg.MIXED_B, rg.MIXED_T
  bm = BuildingMaterials(conductivity=mats[:, :, 0], heat_capacity=mats[:, :, 1], density=mats[:, :, 2],
                         convection_coefficient=hs)
  sim = BatchedSimulator(fp, cfg, B, 12.0, building_materials=bm)
  assert sim.launch_info["kernel"] == rg.hc.LDS
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  twins = rg.mixed_twins(fp, cfg, ids, mats, init)
  obs, rew, info = step_buffers(sim)
  worst, counts = 0.0, set()
  for t in range(T):
    sim.step(torch.tensor(acts[t], device="cuda"), step_in(g, rg.tc.TT0 + t), obs, rew, info)
    i = info.cpu().numpy().astype(np.float64)
    zt, r = sim.zone_temps().cpu().numpy(), rew.cpu().numpy()
    for b in range(B):
      o = twins[b].step(**step_kwargs(g, rg.tc.TT0 + t, t, cfg, acts[t, b], h_conv=hs[b]))
      worst = max(worst, float(np.abs(zt[b] - o["zone_temp_post"]).max()))
      assert_step_matches(i[b], zt[b], r[b], o, (t, b))
      counts.add(o["n_sweeps"])
  grid = sim.temps().cpu().numpy()
  gw = max(float(np.abs(grid[b] - twins[b].grid()).max()) for b in range(B))
  print(f"REGIME-DT materials-handle mixed zone {worst:.3e} grid {gw:.3e}")
  assert gw < T_TOL
  assert len(counts) >= 4          # (the rows do make the buildings differ)
  sim.close()
