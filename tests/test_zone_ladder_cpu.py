"""CPU checks of the zone ladder (tests/zone_ladder.py): what the launch planner picks for each case (sb_plan_info,
host only) on both sides of every capacity edge, the NumPy schedule models of tests/kernel_model.py against the oracle
on the cases they fit, and the conditions tests/test_zone_ladder_gpu.py needs of its inputs, on the oracle alone."""
import numpy as np
import pytest

from oracle import oracle as orc
from sbsim_amd import _ffi
from sbsim_amd.environment import SimConfig
from sbsim_amd.floorplan import jacobi_cv_tensors
from tests import zone_ladder as zl
from tests.twins import oracle_plan_of, plan_info

KIB160 = 160 * 1024


def _info(name, monkeypatch):
  c = zl.CASES[name]
  for k, v in c.env:
    monkeypatch.setenv(k, v)
  fp = zl.device_plan(name)
  cp = fp.compile(300.0, 12.0)
  rc, info = plan_info(fp, n_obs=3 * cp.Z + 19)
  assert rc == 0, _ffi.load().sb_last_error()
  return fp, cp, info


@pytest.mark.parametrize("name", list(zl.CASES))
def test_planner_picks_the_pinned_kernel(name, monkeypatch):
  c = zl.CASES[name]
  fp, cp, info = _info(name, monkeypatch)
  assert (cp.n_classes, cp.Z) == (c.n_classes, c.n_zones)
  assert (info["kernel"], info["waves_per_building"], info["sweep_steps"]) == (c.kernel, c.waves, c.steps)
  assert info["lds_bytes_per_workgroup"] <= KIB160
  cells = fp.zone_cell_lists()
  assert min(len(x) for x in cells) >= 1                      # no empty zone
  d = fp.diffusers.reshape(-1)
  for x in cells:                                             # diffusers sum to 1 in a zone that has any
    assert d[x].sum() == 0.0 or d[x].sum() == 1.0
  assert (fp.diffusers[fp.zone_label < 0] == 0.0).all()


def test_cases_sit_on_both_sides_of_every_edge():
  """The table of edges ("Zone edges per kernel"): every Z the table names, on the kernel it names."""
  def zs(kernel, waves=None, prefix=""):
    return {c.n_zones for n, c in zl.CASES.items()
            if c.kernel == kernel and (waves is None or c.waves == waves) and n.startswith(prefix)}
  assert {1, 15, 16, 17, 30, 31} <= zs(zl.ROLL) and max(zs(zl.ROLL)) == 31
  assert zl.CASES["roll-z32-lds"].kernel == zl.LDS and not zl.CASES["roll-z32-lds"].env       # Z = 32 falls off
  assert {1, 15, 16, 17, 30} <= zs(zl.REG, prefix="reg-z") and zl.CASES["reg-z31-lds"].kernel == zl.LDS
  assert zl.CASES["reg-z31-lds"].env == zl.CASES["reg-z30"].env                                # the same switches
  for kernel, waves in ((zl.TWO, 1), (zl.BAND, 2), (zl.BAND, 3)):
    for lay in ("bands", "columns", "cells"):
      assert {63, 64, 65} <= {c.n_zones for n, c in zl.CASES.items()
                              if (c.kernel, c.waves) == (kernel, waves) and f"-{lay}-" in n}
    assert any(c.orientation == "columns" for c in zl.CASES.values() if (c.kernel, c.waves) == (kernel, waves))
    assert max(zs(kernel, waves)) >= 150
  assert 1000 in zs(zl.TWO) and 1000 in zs(zl.BAND)
  assert any(c.orientation == "columns" for c in zl.CASES.values() if c.kernel == zl.ROLL)
  assert any(c.orientation == "columns" for c in zl.CASES.values() if c.kernel == zl.REG)
  assert {1, 2, 3, 64, 65} <= zs(zl.LDS, prefix="lds-z") and {1, 64, 65} <= zs(zl.STREAM)
  # k_pre (16 zones a pass), k_post (8 a group, Z = 1 mod 8 past the first), write_obs (4 zones a store)
  every = {c.n_zones for c in zl.CASES.values()}
  assert {1, 15, 16, 17, 31, 32, 33} <= every and {17, 33, 65} <= every and {1, 2, 3} <= {z % 4 for z in every}
  # k_sweep_lds' 512-cell index blocks, six to a batch
  sizes = {n: sorted(len(x) for x in zl.plan(n).zone_cell_lists()) for n in ("lds-sized-6blocks", "lds-sized-7blocks")}
  blocks = {n: sum((s + 511) // 512 for s in v) for n, v in sizes.items()}
  assert blocks == {"lds-sized-6blocks": 6, "lds-sized-7blocks": 7}
  assert {1, 511, 512, 513, 1024, 1025} <= set(sizes["lds-sized-6blocks"]) | set(sizes["lds-sized-7blocks"])
  for kind, (_, nw) in zl.JACOBI.items():
    assert zl.jacobi_zone_counts(nw) == (1, nw - 1, nw, nw + 1)


def test_lds_requests_at_the_capacity_edges(monkeypatch):
  """k_sweep_two's compact zone scratch outgrows A between the two "cells" cases; the LDS-grid case near the cap asks
  for more than 159 of the 160 KiB; k_sweep_roll and k_sweep_reg refuse one zone more than their largest case."""
  lds = {}
  for name in ("two-cells-z65", "two-cells-z150", "band2-cells-z65", "band2-cells-z150", "lds-z1060-cap"):
    with monkeypatch.context() as m:
      lds[name] = _info(name, m)[2]["lds_bytes_per_workgroup"]
  assert lds["two-cells-z65"] < lds["two-cells-z150"] <= KIB160
  assert lds["band2-cells-z65"] < lds["band2-cells-z150"] <= KIB160
  assert 159 * 1024 < lds["lds-z1060-cap"] <= KIB160


def _inputs(fp, seed):
  rs = np.random.RandomState(seed)
  H, W = fp.shape
  prev = np.clip(293.0 + 1.5 * rs.randn(H, W), 285.0, 300.0)
  qz = rs.uniform(-400.0, 900.0, size=fp.n_zones)
  q = np.zeros((H, W))
  for z, cells in enumerate(fp.zone_cell_lists()):
    q.reshape(-1)[cells] = qz[z] * fp.diffusers.reshape(-1)[cells]
  oplan = oracle_plan_of(fp)
  return prev, q, qz, oplan


@pytest.mark.parametrize("name", ["roll-z17", "roll-z31", "reg-z30", "roll-z16-columns", "two-cells-z65", "lds-z65",
                                  "lds-sized-7blocks"])
def test_lds_grid_schedule_models_match_the_oracle(name):
  """model_fd_timestep and FastSweepModel (the LDS-grid kernel's schedule) on compile()'s tables, one step."""
  from tests.kernel_model import FastSweepModel, model_fd_timestep
  fp = zl.device_plan(name)
  dt, h = 300.0, 100.0
  cp = fp.compile(dt, h)
  prev, q, qz, oplan = _inputs(fp, 5)
  ref, n_ref, _ = orc.fd_timestep(oplan, prev, q, 279.5, h, dt, 0.05, 40)
  got, n_got = model_fd_timestep(cp, prev, 279.5, qz, 0.05, 40)
  assert n_got == n_ref and n_ref >= 3
  assert np.abs(got - ref).max() < 1e-10
  got2, n2 = FastSweepModel(cp).fd_timestep(prev, 279.5, qz, 0.05, 40)
  assert n2 == n_ref
  assert np.abs(got2 - ref).max() < 1e-10


@pytest.mark.parametrize("name", ["roll-z1", "roll-z17", "roll-z31", "roll-z16-columns"])
def test_register_schedule_models_match_the_oracle(name, schedule="tight"):
  """RegSweepModel on the 38-row plans (its rolling schedule models the 96-slot instantiation only: 30 columns do
  not fit it)."""
  from tests.kernel_model import RegSweepModel
  fp = zl.device_plan(name)
  dt, h = 300.0, 100.0
  m = RegSweepModel(fp.compile(dt, h))
  prev, q, qz, oplan = _inputs(fp, 7)
  ref, n_ref, _ = orc.fd_timestep(oplan, prev, q, 279.5, h, dt, 0.05, 40)
  got, n_got = m.fd_timestep(prev, 279.5, qz, 0.05, 40, schedule=schedule)
  assert n_got == n_ref and n_ref >= 3
  assert np.abs(got - ref).max() < 1e-10


# ---- the conditions tests/test_zone_ladder_gpu.py needs of its inputs: on the oracle alone, every case, every step
def _setpoints(g, t, cfg):
  comfort = bool(g["comfort_now"][96 + t])
  return cfg.comfort_temp_window if comfort else cfg.eco_temp_window


@pytest.mark.parametrize("name", list(zl.CASES))
def test_inputs_keep_the_thermostats_decided_and_the_zones_apart(name):
  """(1) Every zone mean the oracle forms (before and after every step) is at least 1e-6 K from the heating setpoint,
  the cooling setpoint and their midpoint: a 1e-8 K difference between device and oracle cannot flip a mode.
  (2) In every building, at least two steps have two or more thermostat modes among the zones (Z >= 2: one zone has
  one mode).  (3) Z >= 4: at least two steps have more than Z / 2 distinct zone powers."""
  g, cfg = zl.step_rows(), SimConfig.sb1()
  Z = zl.CASES[name].n_zones
  outs = zl.oracle_rollout(name)
  for b in range(zl.B):
    mixed = distinct = 0
    for t in range(zl.T):
      o = outs[t][b]
      hsp, csp = _setpoints(g, t, cfg)
      for tz in (o["zone_temp_pre"], o["zone_temp_post"], o["zone_air_temp"]):
        for edge in (hsp, csp, 0.5 * (csp - hsp) + hsp):
          assert np.abs(tz - edge).min() >= 1e-6, (t, b, edge)
      mixed += len(set(o["mode"].tolist())) >= 2
      distinct += len(set(o["q_zone"].tolist())) > Z / 2
    assert Z < 2 or mixed >= 2, (b, mixed)
    assert Z < 4 or distinct >= 2, (b, distinct)


def test_first_step_has_every_mode_among_the_zones():
  for name in ("roll-z31", "two-cells-z65", "lds-z1060-cap"):
    for b in range(zl.B):
      assert set(zl.oracle_rollout(name)[0][b]["mode"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", zl.CAP_CASES)
def test_ahu_cap_first_binds_inside_the_second_sixteen_zone_pass(name):
  """With ahu_max_air_flow_rate = AHU_CAP the oracle's running sum of the zones' air flows (air_handler.py:254-268,
  zone after zone) first exceeds the cap at a zone of k_pre's second pass (zones 16..31) in every building at steps 0
  and 1, and the cap changes the air handler's flow there."""
  cfg = SimConfig.sb1()
  capped, free = zl.oracle_rollout(name, zl.AHU_CAP), zl.oracle_rollout(name)
  for t in (0, 1):
    for b in range(zl.B):
      run = np.cumsum(capped[t][b]["damper"] * cfg.vav_max_air_flow_rate)
      first = int(np.argmax(run > zl.AHU_CAP))
      assert run[-1] > zl.AHU_CAP and 16 <= first < 32, (t, b, first)
      assert capped[t][b]["ahu_flow"] == zl.AHU_CAP < free[t][b]["ahu_flow"]
      assert capped[t][b]["ahu_count"] == free[t][b]["ahu_count"] == 33


@pytest.mark.parametrize("kind", list(zl.JACOBI))
def test_jacobi_plans_qualify(kind):
  for Z in zl.jacobi_zone_counts(zl.JACOBI[kind][1]):
    fp = zl.jacobi_plan(Z)
    assert fp.n_zones == Z
    jacobi_cv_tensors(fp, 300.0, 100.0)
