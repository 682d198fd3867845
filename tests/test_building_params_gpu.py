"""Per-building HVAC, setpoint and reward parameters (sb_set_building_params) on the GPU: against oracle twins built
with each building's own parameters, bitwise identity with a table of the defaults, bitwise permutation of rows, a
mixed batch against stand-alone environments, and the reset / fork semantics."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from sbsim_amd.host_inputs import BUILDING_PARAM_NAMES, BuildingParams  # noqa: E402
from tests.golden_util import load, oracle_params, oracle_plan  # noqa: E402
from tests.params_cases import c_row, random_params  # noqa: E402
from tests.parity import need_gpu, step_buffers  # noqa: E402
from tests.twins import T_TOL, oracle_rates, plan_from_npz, rates_match, step_in, step_kwargs  # noqa: E402

SB1 = SimConfig.sb1()


def _r9():
  return FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)


def _col(sim, suffix):
  return [i for i, n in enumerate(sim.field_names) if n.endswith("/" + suffix)]


@pytest.mark.parametrize("kernel", ["default", "lds"])
def test_every_building_against_an_oracle_twin_of_its_own_parameters(kernel, monkeypatch):
  need_gpu()
  from oracle import oracle as orc
  if kernel == "lds":
    monkeypatch.setenv("SBSIM_FORCE_LDS_PATH", "1")
  g = load("h2_sb1_r9_random.npz")
  p = load("plan_r9_sb1.npz")
  B, T = 8, 12
  rs = np.random.RandomState(11)
  init = np.clip(294.0 + rs.randn(B, 1, 1) + 0.8 * rs.randn(B, 68, 98), 285.0, 305.0)
  acts = rs.uniform(-1, 1, size=(T, B, 2)).astype(np.float32)
  bp = random_params(B, seed=3)
  sim = BatchedSimulator(plan_from_npz(p), SB1, B, float(g["h_conv"]))
  assert sim.launch_info["path"] == (0 if kernel == "lds" else 1)
  sim.set_building_params(bp)
  sim.reset(temps=torch.tensor(init.reshape(B, -1), dtype=torch.float64, device="cuda"))
  rows = [c_row(bp, b) for b in range(B)]
  sc = sim.scalars().cpu().numpy()
  for b in range(B):   # the reset's setpoints come from the building's row
    assert (sc[b, 0], sc[b, 1], sc[b, 4], sc[b, 8]) == (rows[b]["ahu_heat_sp"], rows[b]["ahu_cool_sp"],
                                                       rows[b]["blr_setpoint"], rows[b]["blr_setpoint"]), b
  plan = oracle_plan(p)
  twins = [orc.OracleBuilding(plan, oracle_params(g["params_json"], **rows[b]), 0.0, reset_temps=init[b].reshape(-1))
           for b in range(B)]
  obs, rew, info = step_buffers(sim)
  c_dp = _col(sim, "differential_pressure_setpoint")
  c_fan = _col(sim, "discharge_fan_speed_percentage_command") + _col(sim, "supply_fan_speed_percentage_command")
  c_oa = _col(sim, "outside_air_flowrate_sensor")
  c_vav = _col(sim, "supply_air_flowrate_setpoint")
  assert len(c_dp) == len(c_oa) == 1 and len(c_fan) == 2 and len(c_vav) == sim.Z
  f32 = np.float32
  for t in range(T):
    tt = t + 100
    sim.step(torch.tensor(acts[t], device="cuda"), step_in(g, tt), obs, rew, info)
    i = info.cpu().numpy().astype(np.float64)
    r = rew.cpu().numpy().astype(np.float64)
    o_dev = obs.cpu().numpy()
    zt = sim.zone_temps().cpu().numpy()
    for b in range(B):
      o = twins[b].step(**step_kwargs(g, tt, t, SB1, acts[t, b]))
      assert i[b, 4] == o["n_sweeps"], (t, b, i[b, 4], o["n_sweeps"])
      assert np.abs(zt[b] - o["zone_temp_post"]).max() < T_TOL, (t, b)
      assert rates_match(i[b, :4], oracle_rates(o)), (t, b, i[b, :4], oracle_rates(o))
      assert abs(float(r[b]) - o["reward"]) < 1e-6, (t, b, r[b], o["reward"])
      # the reward's constants in the info row, and the observation columns that carry a parameter (no normaliser
      # here: an observation is the native value as a proto float)
      row = rows[b]
      assert list(i[b, 13:17]) == [float(f32(row[k])) for k in ("w_prod", "w_cost", "w_carbon", "max_prod")], (t, b)
      assert o_dev[b, c_dp[0]] == f32(row["ahu_dp"]), (t, b)
      assert (o_dev[b, c_vav] == f32(row["vav_max_air_flow"])).all(), (t, b)
      flow = o["ahu_flow"]
      assert np.allclose(o_dev[b, c_fan], flow / row["ahu_max_flow"], rtol=1e-6, atol=0), (t, b)
      assert np.allclose(o_dev[b, c_oa[0]], (1.0 - row["ahu_recirc"]) * flow, rtol=1e-6, atol=0), (t, b)
  sim.close()


def _run(env, acts, steps):
  """obs, reward, info and temperatures of every step (clones)."""
  out = []
  env.reset()
  for t in range(steps):
    ts = env.step(acts[t])
    out.append((ts.observation.clone(), ts.reward.clone(), env.info.clone(), env.sim.temps()))
  return out


def _same(x, y):
  for t, (a, b) in enumerate(zip(x, y)):
    for k, (u, v) in enumerate(zip(a, b)):
      assert torch.equal(u, v), (t, k)


@pytest.mark.parametrize("solver", ["gauss_seidel", "jacobi_fp32"])
def test_a_table_of_the_defaults_is_bitwise_no_table(solver):
  need_gpu()
  B, T = 8, 20
  gen = torch.Generator(device="cuda")
  gen.manual_seed(21)
  acts = torch.rand((T, B, 2), generator=gen, device="cuda") * 2 - 1
  defaults = BuildingParams({name: np.broadcast_to(np.asarray(getattr(SB1, name), dtype=np.float64),
                                                   (B,) + np.asarray(getattr(SB1, name)).shape)
                             for name in BUILDING_PARAM_NAMES})
  plain = BatchedEnvironment(_r9(), B, collect_info=True, solver=solver)
  table = BatchedEnvironment(_r9(), B, collect_info=True, solver=solver, building_params=defaults)
  cleared = BatchedEnvironment(_r9(), B, collect_info=True, solver=solver, building_params=random_params(B, 5))
  cleared.set_building_params(None)
  ref = _run(plain, acts, T)
  _same(ref, _run(table, acts, T))
  _same(ref, _run(cleared, acts, T))
  for k, v in table.building_params().items():
    assert np.array_equal(v, plain.building_params()[k]), k
  for env in (plain, table, cleared):
    env.close()


@pytest.mark.parametrize("solver", ["gauss_seidel", "jacobi_fp32"])
def test_permuted_rows_permute_the_outputs_bitwise(solver):
  need_gpu()
  B, T = 16, 12
  gen = torch.Generator(device="cuda")
  gen.manual_seed(22)
  acts = torch.rand((T, B, 2), generator=gen, device="cuda") * 2 - 1
  bp = random_params(B, seed=7, keep_default=())
  perm = np.random.RandomState(1).permutation(B)
  pi = torch.tensor(perm, device="cuda")
  bp_pi = BuildingParams({k: v[perm] for k, v in bp.fields.items()})
  a = BatchedEnvironment(_r9(), B, collect_info=True, solver=solver, building_params=bp)
  b = BatchedEnvironment(_r9(), B, collect_info=True, solver=solver, building_params=bp_pi)
  x = _run(a, acts, T)              # every building starts from the same reset state
  y = _run(b, acts[:, pi], T)
  _same([tuple(u[pi] for u in step) for step in x], y)
  assert not torch.equal(x[-1][1], x[-1][1][pi])   # (the rows do make the buildings differ)
  a.close()
  b.close()


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_mixed_batch_slices_equal_stand_alone_environments(rank, world):
  need_gpu()
  plans = [_r9(), FloorPlan.from_file_input(rectangular_floor_plan((2, 3), (9, 10)), Materials.sb1(), 10.0, 300.0)]
  totals = [6, 5]
  bp = random_params(sum(totals), seed=9, keep_default=())
  mixed = MixedBatchedEnvironment(list(zip(plans, totals)), rank=rank, world=world, collect_info=True,
                                  building_params=bp)
  singles = [BatchedEnvironment(p, hi - lo, collect_info=True, building_params=bp.rows(glo, ghi))
             for p, (lo, hi), (glo, ghi) in zip(plans, mixed.class_ranges, mixed.global_rows)]
  B = mixed.batch_size
  gen = torch.Generator(device="cuda")
  gen.manual_seed(23)
  acts = torch.rand((10, B, 2), generator=gen, device="cuda") * 2 - 1
  mixed.reset()
  for s in singles:
    s.reset()
  for t in range(10):
    ts = mixed.step(acts[t])
    for k, (s, (a, b)) in enumerate(zip(singles, mixed.slices)):
      tk = s.step(acts[t, a:b].contiguous())
      assert torch.equal(ts.observation[a:b, :mixed.observation_widths[k]], tk.observation), (t, k)
      assert torch.equal(ts.reward[a:b], tk.reward), (t, k)
      assert torch.equal(mixed.envs[k].info, s.info), (t, k)
  for k, s in enumerate(singles):
    assert torch.equal(mixed.envs[k].sim.temps(), s.sim.temps()), k
    for name, v in s.building_params().items():
      assert np.array_equal(mixed.envs[k].building_params()[name], v), (k, name)
  mixed.set_building_params(None)   # clears every class's table
  assert mixed.envs[1].building_params()["ahu_fan_efficiency"].tolist() == [SB1.ahu_fan_efficiency] * mixed.envs[1].batch_size
  with pytest.raises(ValueError, match="global building number"):
    mixed.set_building_params(bp.rows(0, 10))
  mixed.close()
  for s in singles:
    s.close()


@pytest.mark.parametrize("solver", ["gauss_seidel", "jacobi_fp32"])
def test_reset_sets_each_buildings_own_setpoints(solver):
  need_gpu()
  B = 8
  env = BatchedEnvironment(_r9(), B, collect_info=True, solver=solver)
  env.reset()
  sc0 = env.sim.scalars().cpu().numpy()
  assert (sc0[:, 0] == SB1.ahu_heating_air_temp_setpoint).all() and (sc0[:, 4] == SB1.boiler_reheat_water_setpoint).all()
  bp = random_params(B, seed=13)
  env.set_building_params(bp)
  # a new table does not rewrite the setpoints in force ...
  assert np.array_equal(env.sim.scalars().cpu().numpy(), sc0)
  ts = env.reset()   # ... the next reset sets them from the rows
  sc = env.sim.scalars().cpu().numpy()
  eff = env.building_params()
  assert np.array_equal(sc[:, 0], eff["ahu_heating_air_temp_setpoint"])
  assert np.array_equal(sc[:, 1], eff["ahu_cooling_air_temp_setpoint"])
  assert np.array_equal(sc[:, 4], eff["boiler_reheat_water_setpoint"])
  # the reset's observation (k_observe) shows each building's own VAV flow setpoint
  c_vav = _col(env.sim, "supply_air_flowrate_setpoint")
  o = ts.observation.cpu().numpy()
  assert (o[:, c_vav] == eff["vav_max_air_flow_rate"].astype(np.float32)[:, None]).all()
  env.close()


def test_a_forked_building_keeps_its_slots_row():
  need_gpu()
  B = 8
  bp = random_params(B, seed=17, keep_default=(0, 1, 2, 3))   # buildings 0..3: one row; 4..7: rows of their own
  env = BatchedEnvironment(_r9(), B, collect_info=True, building_params=bp)
  gen = torch.Generator(device="cuda")
  gen.manual_seed(24)
  acts = torch.rand((4, B, 2), generator=gen, device="cuda") * 2 - 1
  env.reset()
  for t in range(3):
    env.step(acts[t])
  env.fork(torch.zeros(B, dtype=torch.int64, device="cuda"))   # every slot takes building 0's state
  same = acts[3, :1].expand(B, 2).contiguous()
  ts = env.step(same)
  obs, rew, info = ts.observation.cpu().numpy(), ts.reward.cpu().numpy(), env.info.cpu().numpy()
  for b in range(1, 4):   # equal rows, equal state: equal outputs
    assert np.array_equal(obs[b], obs[0]) and rew[b] == rew[0] and np.array_equal(info[b], info[0]), b
  for b in range(4, 8):   # equal state, their own rows: different outputs
    assert not np.array_equal(obs[b], obs[0]), b
    assert rew[b] != rew[0] and not np.array_equal(info[b], info[0]), b
  env.close()


def test_the_c_entry_names_the_building_and_the_field():
  need_gpu()
  B = 4
  sim = BatchedSimulator(_r9(), SB1, B, 10.0)
  fn = _ffi.entry("sb_set_building_params")
  lib = _ffi.load()

  def call(fields, values):
    f = np.asarray(fields, dtype=np.int32)
    v = np.ascontiguousarray(values, dtype=np.float64)
    return fn(sim._h, len(fields), f.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), None)

  k = {name: i for i, name in enumerate(_ffi.BUILDING_PARAM_FIELDS)}
  assert call([k["ahu_cool_sp"]], [[298.0, 298.0, 280.0, 298.0]]) == -1
  msg = lib.sb_last_error().decode()
  assert "building 2" in msg and "cooling_air_temp_setpoint must greater than heating_air_temp_setpoint" in msg, msg
  assert call([k["ahu_eff"]], [[0.9, 0.0, 0.9, 0.9]]) == -1
  assert "building 1" in lib.sb_last_error().decode() and "ahu_eff" in lib.sb_last_error().decode()
  assert call([k["eco_lo"]], [[289.0, 289.0, 289.0, 299.0]]) == -1
  assert "building 3" in lib.sb_last_error().decode() and "eco_temp_window" in lib.sb_last_error().decode()
  assert call([k["w_prod"]], [[0.2, np.nan, 0.2, 0.2]]) == -1
  assert "w_prod is not finite" in lib.sb_last_error().decode()
  assert call([k["w_prod"], k["w_prod"]], [[0.2] * 4, [0.2] * 4]) == -1
  assert call([32], [[0.2] * 4]) == -1
  assert call([k["ahu_eff"]], [[0.8, 0.9, 0.7, 0.6]]) == 0
  with pytest.raises(ValueError, match="4 buildings"):
    sim.set_building_params(BuildingParams({"ahu_fan_efficiency": [0.9] * 3}))
  sim.close()
