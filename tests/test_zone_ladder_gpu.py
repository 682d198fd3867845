"""GPU parity on the zone ladder (tests/zone_ladder.py): every kernel's zone reduce and the per-zone passes of k_pre,
k_post and the observation writer on both sides of their grouping and capacity edges, against the CPU oracle, one twin
per building.  Every zone starts at a temperature of its own, so a reduce that drops its last pass, mixes two zones or
misplaces the dump zone moves a thermostat, a damper and a zone power, not just one mean among equals.

On top of tests/test_gpu_parity.py's _check_plan_against_oracle (sweep counts and converged flags EQUAL, zone means and
the final grid within T_TOL, rates at rtol 2e-6 / atol 1e-6, reward within 2e-6), per step, building and zone:
thermostat modes and dampers EQUAL, zone powers within what a T_TOL difference of a zone mean allows, the air
handler's and the boiler's request counts EQUAL and flows at the rates' relative tolerance, and the observation row's
three columns per zone EQUAL to float32 of the oracle's values.  tests/test_zone_ladder_cpu.py checks on the oracle that
no zone mean of these runs comes within 1e-6 K of a thermostat threshold."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig, observation_field_names  # noqa: E402
from tests import jacobi_restatement as jr  # noqa: E402
from tests import zone_ladder as zl  # noqa: E402
from tests.test_gpu_parity import T_TOL, _check_plan_against_oracle, _need_gpu, _step_in  # noqa: E402

C_AIR = 1006.0       # J / (kg K), vav.py:197-217
RATE_RTOL = 2e-6     # the rates' relative tolerance (tests/test_gpu_parity.py)
JACOBI_ZONE_TOL = 1e-11   # tests/test_jacobi_large_gpu.py: device zone means against float64 means of the float32 grid


def _zone_checks(cfg):
  """The on_step hook: the per-zone state of every building against its twin's."""
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


def _run(name, monkeypatch, cfg=None):
  """The case on the kernel the planner picks under the case's own switches and no others (force_path=False): the two
  cases that fall off a register kernel reach the LDS-grid kernel by the library's choice."""
  c = zl.CASES[name]
  cfg = SimConfig.sb1() if cfg is None else cfg
  fp = zl.plan(name)
  path = {zl.LDS: 0, zl.STREAM: 2}.get(c.kernel, 1)
  return _check_plan_against_oracle(fp, c.n_zones, c.orientation, path, monkeypatch, expect_steps=c.steps,
                                    expect_kernel=c.kernel, expect_waves=c.waves, B=zl.B, T=zl.T,
                                    init=zl.initial_grids(fp), acts=zl.actions(), cfg=cfg, env=dict(c.env),
                                    golden=zl.step_rows(), on_step=_zone_checks(cfg), force_path=False)


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
  _need_gpu()
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
  tt = jr.tensors(fp, cfg.time_step_sec, h)
  rs = np.random.RandomState(13)
  tprev = (288.0 + 8.0 * rs.rand(Bn, *fp.shape)).astype(np.float32)
  q = np.stack([jr.input_q(fp, rs.uniform(-3000.0, 3000.0, Z)) for _ in range(Bn)])
  tinf = rs.uniform(265.0, 305.0, Bn)
  grid, iters, conv = sim.tap_jacobi(tprev, q, tinf)
  for b in range(Bn):
    want, wi, wc = jr.fd_timestep(tt, tprev[b], q[b], tinf[b], cfg.time_step_sec, cfg.convergence_threshold,
                                  cfg.iteration_limit)
    assert (iters[b], bool(conv[b])) == (wi, wc), (b, iters[b], wi)
    assert np.array_equal(np.asarray(grid[b], np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
  init = zl.initial_grids(fp, Bn)
  acts = zl.actions(3, Bn)
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  obs = torch.zeros((Bn, sim.O), dtype=torch.float32, device="cuda")
  rew = torch.zeros((Bn,), dtype=torch.float32, device="cuda")
  info = torch.zeros((Bn, _ffi.SB_INFO_STRIDE), dtype=torch.float32, device="cuda")
  zlab = fp.zone_label.reshape(-1)
  for t in range(3):
    sim.step(torch.tensor(acts[t], device="cuda"), _step_in(g, 96 + t), obs, rew, info)
    flat = sim.temps().cpu().numpy().reshape(Bn, -1)
    assert np.array_equal(flat, flat.astype(np.float32).astype(np.float64))       # a float32 grid, widened
    means = np.stack([flat[:, zlab == z].mean(axis=1) for z in range(Z)], axis=1)
    zt = sim.zone_temps().cpu().numpy()
    assert np.abs(zt - means).max() <= JACOBI_ZONE_TOL, (t, np.abs(zt - means).max())
  sim.close()
