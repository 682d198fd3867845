"""GPU parity on the zone ladder (tests/zone_ladder.py): every kernel's zone reduce and the per-zone passes of k_pre,
k_post and the observation writer on both sides of their grouping and capacity edges, against the CPU oracle, one twin
per building.  Every zone starts at a temperature of its own, so a reduce that drops its last pass, mixes two zones or
misplaces the dump zone moves a thermostat, a damper and a zone power, not just one mean among equals.

On top of tests/parity.py's check_plan_against_oracle (sweep counts and converged flags EQUAL, zone means and
the final grid within T_TOL, rates at rtol 2e-6 / atol 1e-6, reward within 2e-6), per step, building and zone:
thermostat modes and dampers EQUAL, zone powers within what a T_TOL difference of a zone mean allows, the air
handler's and the boiler's request counts EQUAL and flows at the rates' relative tolerance, and the observation row's
three columns per zone EQUAL to float32 of the oracle's values.  tests/test_zone_ladder_cpu.py checks on the oracle that
no zone mean of these runs comes within 1e-6 K of a thermostat threshold."""
import dataclasses

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from tests import zone_ladder as zl  # noqa: E402
from tests.parity import (check_plan_against_oracle, jacobi_tap_bitwise, jacobi_zone_means_follow_grid, need_gpu,  # noqa: E402
                          zone_checks)


def _run(name, monkeypatch, cfg=None):
  """The case on the kernel the planner picks under the case's own switches and no others (force_path=False): the two
  cases that fall off a register kernel reach the LDS-grid kernel by the library's choice."""
  c = zl.CASES[name]
  cfg = SimConfig.sb1() if cfg is None else cfg
  fp = zl.plan(name)
  path = {zl.LDS: 0, zl.STREAM: 2}.get(c.kernel, 1)
  return check_plan_against_oracle(fp, c.n_zones, c.orientation, path, monkeypatch, expect_steps=c.steps,
                                   expect_kernel=c.kernel, expect_waves=c.waves, B=zl.B, T=zl.T,
                                   init=zl.initial_grids(fp), acts=zl.actions(), cfg=cfg, env=dict(c.env),
                                   golden=zl.step_rows(), on_step=zone_checks(cfg), force_path=False)


@pytest.mark.parametrize("name", list(zl.CASES))
def test_case_against_oracle(name, monkeypatch):
  _run(name, monkeypatch)


@pytest.mark.parametrize("name", zl.CAP_CASES)
def test_ahu_flow_cap_binds_inside_the_second_pass_of_k_pre(name, monkeypatch):
  """33 zones with ahu_max_air_flow_rate = 0.5 m3/s: the running sum of the zones' air flows reaches the cap at a zone
  of k_pre's second 16-zone pass (tests/test_zone_ladder_cpu.py checks where on the oracle), so the clamp inside the
  sum, the carry of the clamped sum into the third pass and the request count past it are all in play."""
  cfg = dataclasses.replace(SimConfig.sb1(), ahu_max_air_flow_rate=zl.AHU_CAP)
  infos, _ = _run(name, monkeypatch, cfg=cfg)
  assert len(infos) == zl.T


@pytest.mark.parametrize("kind", list(zl.JACOBI))
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["Z=1", "Z=NW-1", "Z=NW", "Z=NW+1"])
def test_jacobi_zone_per_wavefront_edges(kind, which, monkeypatch):
  """solver="jacobi_fp32": a zone per wavefront, z += NW.  The tap bitwise against the restatement, then three real
  steps whose zone means must be the float64 means of the float32 grid."""
  need_gpu()
  env, nw = zl.JACOBI[kind]
  for k, v in env:
    monkeypatch.setenv(k, v)
  Z = zl.jacobi_zone_counts(nw)[which]
  fp = zl.jacobi_plan(Z)
  cfg = SimConfig.sb1()
  g = zl.step_rows()
  h = float(g["h_conv"])
  Bn = 4
  sim = BatchedSimulator(fp, cfg, Bn, h, solver="jacobi_fp32")
  assert sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI and sim.launch_info["path"] == (2 if env else 0)
  assert sim.launch_info["waves_per_building"] == nw and sim.Z == Z
  jacobi_tap_bitwise(sim, fp, cfg, h, seed=13)
  jacobi_zone_means_follow_grid(sim, fp, g, zl.initial_grids(fp, Bn), zl.actions(3, Bn))
  sim.close()
