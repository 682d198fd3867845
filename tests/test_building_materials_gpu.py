"""Per-building materials and convection coefficient (sb_create_materials) on the GPU: k_class_coef bitwise against the
NumPy restatement, every building against a one-building default handle and an oracle twin on the plan with its
materials substituted, bitwise identity with a default handle on k_sweep_lds for the plan's own values, the hand-over
of the per-wavefront coefficient table between buildings, set_building_materials between steps, snapshots and the
stochastic models, the refusals, and a mixed batch under two shardings."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd import host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan, structural_class_coef  # noqa: E402
from sbsim_amd.host_inputs import BuildingMaterials  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.materials_cases import random_sets, substituted, the_plan  # noqa: E402
from tests.parity import need_gpu, step_buffers  # noqa: E402
from tests.twins import T_TOL, assert_step_matches, oracle_twin, step_in, step_kwargs  # noqa: E402

SB1 = SimConfig.sb1()
MANY = "roll66-48sets"   # irregular plan with more than 32 structural classes: the ts = 128 sweep body
LDS = 0                  # sb_sweep_kernel


def _table(plan, B, seed):
  """B random rows around the plan's own materials (tests/materials_cases.py, random_sets)."""
  ids, table = plan.material_slots()
  sets, hs = random_sets(table, B, seed)
  bm = BuildingMaterials(conductivity=sets[:, :, 0], heat_capacity=sets[:, :, 1], density=sets[:, :, 2],
                         convection_coefficient=hs)
  return ids, sets, hs, bm


def _own(plan, B, h_conv):
  """A table that repeats the plan's own values in every row."""
  table = plan.material_slots()[1]
  return BuildingMaterials(conductivity=np.tile(table[:, 0], (B, 1)), heat_capacity=np.tile(table[:, 1], (B, 1)),
                           density=np.tile(table[:, 2], (B, 1)), convection_coefficient=np.full(B, h_conv))


def _two_sets(plan, B):
  """Rows alternating between two very different material sets."""
  table = plan.material_slots()[1]
  a = table * np.array([0.2, 3.0, 2.0])
  b = table * np.array([4.0, 0.3, 0.5])
  sets = np.stack([a if i % 2 == 0 else b for i in range(B)])
  hs = np.array([5.0 if i % 2 == 0 else 150.0 for i in range(B)])
  return BuildingMaterials(conductivity=sets[:, :, 0], heat_capacity=sets[:, :, 1], density=sets[:, :, 2],
                           convection_coefficient=hs)


FOURTH = "r9-fourth-material"   # the plan and its transpose meet the materials in different orders (columns: transposed)


@pytest.mark.parametrize("name,orientation", [("plan_small_test", "auto"), ("plan_weird_test", "auto"), (MANY, "auto"),
                                              (FOURTH, "columns"), (FOURTH, "rows")])
def test_coefficient_tap_is_bitwise_the_numpy_restatement(name, orientation):
  need_gpu()
  plan = the_plan(name)
  B = 7
  ids, sets, hs, bm = _table(plan, B, seed=31)
  sim = BatchedSimulator(plan, SB1, B, 12.0, building_materials=bm, orientation=orientation)
  assert sim.launch_info["kernel"] == LDS and (orientation == "auto" or sim.transposed == (orientation == "columns"))
  sp = sim.compiled
  if name == MANY:
    assert sp.n_classes > 32
  assert np.array_equal(sp.slot_table, plan.material_slots()[1])   # the caller's slot numbering in either orientation
  got = sim.building_coef().cpu().numpy()
  for b in range(B):
    want = structural_class_coef(sp, sets[b, :, 0], sets[b, :, 1], sets[b, :, 2], hs[b], SB1.time_step_sec, sp.dx, sp.zh)
    assert np.array_equal(got[b].view(np.uint64), want.view(np.uint64)), (b, np.argwhere(got[b] != want)[:4])
    # per cell, the value-keyed compile() of the plan with row b substituted, in the device's orientation
    pb = substituted(plan, ids, sets[b])
    cp = (pb.transposed() if sim.transposed else pb).compile(SB1.time_step_sec, float(hs[b]))
    assert np.array_equal(got[b][sp.cell_class].view(np.uint64), cp.class_coef[cp.cell_class].view(np.uint64)), b
  sim.set_building_materials(None)   # n_fields == 0: the plan's own values
  own = sp.class_coef(h_conv=12.0)
  got = sim.building_coef().cpu().numpy()
  assert all(np.array_equal(got[b].view(np.uint64), own.view(np.uint64)) for b in range(B))
  eff = sim.building_materials()
  assert np.array_equal(eff["conductivity"], np.tile(sp.slot_table[:, 0], (B, 1))) and (eff["convection_coefficient"] == 12.0).all()
  sim.close()


@pytest.mark.parametrize("name,orientation", [("plan_small_test", "auto"), ("plan_weird_test", "auto"), (MANY, "auto"),
                                              ("plan_r9_test", "auto"), (FOURTH, "columns")])
def test_every_building_against_a_default_handle_and_an_oracle_twin(name, orientation, monkeypatch):
  need_gpu()
  g = load("h2_sb1_r9_random.npz")
  plan = the_plan(name)
  H, W = plan.shape
  B, T = 6, 12
  ids, sets, hs, bm = _table(plan, B, seed=41)
  rs = np.random.RandomState(43)
  init = np.clip(294.0 + rs.randn(B, 1) + 0.5 * rs.randn(B, H * W), 285.0, 305.0)
  acts = rs.uniform(-1, 1, size=(T, B, 2)).astype(np.float32)
  sim = BatchedSimulator(plan, SB1, B, 12.0, building_materials=bm, orientation=orientation)
  assert sim.launch_info["kernel"] == LDS and (orientation == "auto" or sim.transposed)
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  # building b alone: a default handle on the plan with row b's materials and h_conv, forced onto k_sweep_lds in the
  # same orientation -- the same kernel body on the same coefficients: bitwise
  monkeypatch.setenv("SBSIM_FORCE_LDS_PATH", "1")
  singles, twins = [], []
  for b in range(B):
    pb = substituted(plan, ids, sets[b])
    s = BatchedSimulator(pb, SB1, 1, float(hs[b]), orientation="columns" if sim.transposed else "rows")
    assert s.launch_info["kernel"] == LDS and s.transposed == sim.transposed
    s.reset(temps=torch.tensor(init[b:b + 1], dtype=torch.float64, device="cuda"))
    singles.append((s,) + step_buffers(s))
    twins.append(oracle_twin(pb, SB1, init[b]))
  obs, rew, info = step_buffers(sim)
  for t in range(T):
    tt = 100 + t
    sim.step(torch.tensor(acts[t], device="cuda"), step_in(g, tt), obs, rew, info)
    i = info.cpu().numpy().astype(np.float64)
    zt, grid = sim.zone_temps().cpu().numpy(), sim.temps().cpu().numpy()
    for b, (s, o1, r1, i1) in enumerate(singles):
      s.step(torch.tensor(acts[t, b:b + 1], device="cuda"), step_in(g, tt), o1, r1, i1)
      assert i[b, 4] == float(i1[0, 4]), (t, b, i[b, 4], float(i1[0, 4]))   # sweep counts
      z1, g1 = s.zone_temps().cpu().numpy()[0], s.temps().cpu().numpy()[0]
      assert np.abs(zt[b] - z1).max() < T_TOL and np.abs(grid[b] - g1).max() < T_TOL, (t, b)
      assert np.array_equal(zt[b], z1) and np.array_equal(grid[b], g1), (t, b)
      assert torch.equal(obs[b], o1[0]) and torch.equal(rew[b], r1[0]) and torch.equal(info[b], i1[0]), (t, b)
      o = twins[b].step(**step_kwargs(g, tt, t, SB1, acts[t, b], h_conv=hs[b]))
      assert_step_matches(i[b], zt[b], float(rew[b]), o, (t, b))
      assert abs(float(rew[b]) - o["reward"]) < 1e-6, (t, b)
  final = sim.temps().cpu().numpy()
  for b in range(B):
    assert np.abs(final[b].reshape(-1) - twins[b].temp).max() < T_TOL, b
  assert len({int(x) for x in info.cpu().numpy()[:, 4]}) > 1 or name != "plan_r9_test"   # (the rows do make buildings differ)
  for s, *_ in singles:
    s.close()
  sim.close()


def _run(env, acts, steps, start=0):
  out = []
  for t in range(start, start + steps):
    ts = env.step(acts[t])
    out.append((ts.observation.clone(), ts.reward.clone(), env.info.clone(), env.sim.temps()))
  return out


def _same(x, y):
  assert len(x) == len(y)
  for t, (a, b) in enumerate(zip(x, y)):
    for k, (u, v) in enumerate(zip(a, b)):
      assert torch.equal(u, v), (t, k)


def _acts(T, B, seed):
  gen = torch.Generator(device="cuda")
  gen.manual_seed(seed)
  return torch.rand((T, B, 2), generator=gen, device="cuda") * 2 - 1


def _r9():
  return FloorPlan.from_file_input(rectangular_floor_plan((3, 3), (20, 30)), Materials.sb1(), 10.0, 300.0)


@pytest.mark.parametrize("name", ["r9", "plan_small_test"])
def test_the_plans_own_values_are_bitwise_a_default_handle_on_k_sweep_lds(name, monkeypatch):
  need_gpu()
  plan = _r9() if name == "r9" else the_plan(name)
  B, T = 8, 12
  acts = _acts(T, B, 51)
  table = BatchedEnvironment(plan, B, collect_info=True, building_materials=_own(plan, B, 100.0))
  assert table.sim.launch_info["kernel"] == LDS
  monkeypatch.setenv("SBSIM_FORCE_LDS_PATH", "1")
  plain = BatchedEnvironment(plan, B, collect_info=True)
  assert plain.sim.launch_info["kernel"] == LDS and plain.sim.transposed == table.sim.transposed
  plain.reset()
  table.reset()
  _same(_run(plain, acts, T), _run(table, acts, T))
  # default fingerprints are unchanged; a materials handle hashes the structural tables and says so
  fp0, fp1 = plain.sim.state_fingerprint(), table.sim.state_fingerprint()
  assert ("building_materials",) not in fp0 and fp1[-1] == ("building_materials",) and fp0[1] != fp1[1]
  plain.close()
  table.close()


def test_hand_over_between_buildings_reloads_the_wavefronts_table():
  need_gpu()
  plan = the_plan("plan_small_test")
  # enough buildings for every wavefront of a full launch to draw a second and a third one
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  full = BatchedSimulator(plan, SB1, cus * 64, 12.0, building_materials=_own(plan, cus * 64, 12.0))
  li = full.launch_info
  full.close()
  B = 2 * li["workgroups"] * li["waves_per_workgroup"] + 3
  T = 3
  big = BatchedEnvironment(plan, B, collect_info=True, building_materials=_two_sets(plan, B))
  assert big.sim.launch_info["kernel"] == LDS
  assert B > 2 * big.sim.launch_info["workgroups"] * big.sim.launch_info["waves_per_workgroup"]
  two = BatchedEnvironment(plan, 2, collect_info=True, building_materials=_two_sets(plan, 2))
  a2 = _acts(T, 2, 61)
  aB = a2.repeat(1, (B + 1) // 2, 1)[:, :B].contiguous()   # building b gets the actions of building b % 2
  big.reset()
  two.reset()
  x, y = _run(big, aB, T), _run(two, a2, T)
  for t in range(T):
    for k in range(4):
      u, v = x[t][k], y[t][k]
      assert torch.equal(u[0::2], v[0:1].expand_as(u[0::2])), (t, k, "even")
      assert torch.equal(u[1::2], v[1:2].expand_as(u[1::2])), (t, k, "odd")
  assert not torch.equal(y[-1][3][0], y[-1][3][1])   # (the two sets do differ)
  big.close()
  two.close()


def test_a_new_table_applies_from_the_next_step():
  need_gpu()
  plan = the_plan("plan_small_test")
  B = 6
  acts = _acts(8, B, 71)
  _, _, _, bm1 = _table(plan, B, seed=73)
  _, _, _, bm2 = _table(plan, B, seed=74)
  env = BatchedEnvironment(plan, B, collect_info=True, building_materials=bm1)
  env.reset()
  _run(env, acts, 3)
  snap = env.snapshot()
  env.set_building_materials(bm2)
  after = _run(env, acts, 2, start=3)
  fresh = BatchedEnvironment(plan, B, collect_info=True, building_materials=bm2)
  fresh.restore(snap)   # snapshots do not carry the table: the restored state runs under the fresh handle's rows
  _same(after, _run(fresh, acts, 2, start=3))
  stale = BatchedEnvironment(plan, B, collect_info=True, building_materials=bm1)
  stale.restore(snap)
  assert not torch.equal(after[0][3], _run(stale, acts, 1, start=3)[0][3])   # (the new rows did change the step)
  # n_fields == 0: back to the plan's own values, equal to a handle that repeats them in every row
  env.restore(snap)
  env.set_building_materials(None)
  own = BatchedEnvironment(plan, B, collect_info=True, building_materials=_own(plan, B, 100.0))
  own.restore(snap)
  _same(_run(env, acts, 2, start=3), _run(own, acts, 2, start=3))
  for e in (env, fresh, stale, own):
    e.close()


def test_snapshots_and_stochastic_models_on_a_materials_handle():
  """snapshot / restore / fork, the convection shuffle, device occupancy, BuildingParams and the dollar reward see the
  LDS state layout and the k_pre / k_post hand-over only -- none of them reads a coefficient table -- so they work on a
  materials handle unchanged."""
  need_gpu()
  plan = _r9()
  B = 6
  acts = _acts(10, B, 81)
  _, _, _, bm = _table(plan, B, seed=83)
  occ = host_inputs.BatchedRandomizedArrivalDepartureOccupancy(10, 7, 10, 16, 19, 300.0, seed=5)
  conv = host_inputs.StochasticConvectionSimulator(0.3, 2, seed=9)
  bp = host_inputs.BuildingParams({"ahu_fan_efficiency": np.linspace(0.6, 0.9, B)})
  rf = host_inputs.SetpointEnergyCarbonReward(1.0, 1.0, 0.05, 0.0, 1.0)
  env = BatchedEnvironment(plan, B, collect_info=True, building_materials=bm, occupancy=occ, convection_simulator=conv,
                           building_params=bp, reward_function=rf)
  assert env.sim.launch_info["kernel"] == LDS
  env.reset()
  _run(env, acts, 3)
  snap = env.snapshot()
  first = _run(env, acts, 3, start=3)
  env.restore(snap)
  _same(first, _run(env, acts, 3, start=3))   # grid, occupants and shuffle counters replay bitwise
  # fork: every slot takes building 0's state and keeps its own row
  env.restore(snap)
  env.fork(torch.zeros(B, dtype=torch.int64, device="cuda"))
  t0 = env.sim.temps()
  assert all(torch.equal(t0[b], t0[0]) for b in range(B))
  env.step(acts[3, :1].expand(B, 2).contiguous())
  t1 = env.sim.temps()
  assert not torch.equal(t1[1], t1[0])
  env.close()


def test_refusals():
  need_gpu()
  plan = the_plan("plan_small_test")
  B = 4
  own = _own(plan, B, 12.0)
  with pytest.raises(ValueError, match="jacobi_fp32"):
    BatchedSimulator(plan, SB1, B, 12.0, solver="jacobi_fp32", building_materials=own)
  with pytest.raises(ValueError, match="4 rows, the simulator 5"):
    BatchedSimulator(plan, SB1, 5, 12.0, building_materials=own)
  huge = FloorPlan.from_file_input(rectangular_floor_plan((14, 9), (20, 43)), Materials.sb1(), 10.0, 300.0)
  assert huge.shape == (299, 401)
  with pytest.raises(ValueError, match="k_sweep_lds, which cannot hold this floor plan"):
    BatchedSimulator(huge, SB1, 2, 12.0, building_materials=_own(huge, 2, 12.0))
  plain = BatchedSimulator(plan, SB1, B, 12.0)
  with pytest.raises(ValueError, match="created with building_materials"):
    plain.set_building_materials(own)
  lib = _ffi.load()
  setm = _ffi.materials_entry("sb_set_building_materials")

  def call(sim, fields, values, stream=None):
    f = np.asarray(fields, dtype=np.int32)
    v = np.ascontiguousarray(values, dtype=np.float64)
    return setm(sim._h, len(fields), f.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), stream)

  assert call(plain, [0], [[1.0] * B]) == -5   # SB_ERR_UNSUPPORTED
  assert "sb_create_materials" in lib.sb_last_error().decode()
  out = torch.zeros(8, dtype=torch.float64, device="cuda")
  assert _ffi.materials_entry("sb_get_building_coef")(plain._h, C.c_void_p(out.data_ptr()), None) == -5
  plain.close()
  sim = BatchedSimulator(plan, SB1, B, 12.0, building_materials=own)
  M = len(plan.material_slots()[1])
  before = sim.building_coef().clone()
  assert call(sim, [M + 1], [[700.0, 700.0, np.nan, 700.0]]) == -1
  msg = lib.sb_last_error().decode()
  assert "building 2" in msg and "heat_capacity[1] is not finite" in msg, msg
  assert call(sim, [0], [[50.0, 0.0, 50.0, 50.0]]) == -1
  msg = lib.sb_last_error().decode()
  assert "building 1" in msg and "conductivity[0] must be positive" in msg, msg
  assert call(sim, [3 * M], [[1.0, 1.0, 1.0, -2.0]]) == -1
  msg = lib.sb_last_error().decode()
  assert "building 3" in msg and "h_conv must not be negative" in msg, msg
  assert call(sim, [0, 0], [[1.0] * B, [1.0] * B]) == -1 and "named twice" in lib.sb_last_error().decode()
  assert call(sim, [3 * M + 1], [[1.0] * B]) == -1 and "unknown field" in lib.sb_last_error().decode()
  assert torch.equal(sim.building_coef(), before)   # nothing changed
  bad = BuildingMaterials(convection_coefficient=[1.0, 2.0, 3.0])
  with pytest.raises(ValueError, match="3 rows, the simulator 4"):
    sim.set_building_materials(bad)
  # a stream under capture
  s = torch.cuda.Stream()
  graph = torch.cuda.CUDAGraph()
  scratch = torch.zeros(4, device="cuda")
  with torch.cuda.stream(s):
    graph.capture_begin()
    try:
      scratch.add_(1.0)
      rc = call(sim, [3 * M], [[1.0] * B], C.c_void_p(s.cuda_stream))
      msg = lib.sb_last_error().decode()
    finally:
      graph.capture_end()
  assert rc == -1 and "captured" in msg, (rc, msg)
  assert torch.equal(sim.building_coef(), before)
  assert call(sim, [3 * M], [[1.0, 2.0, 3.0, 4.0]]) == 0
  assert not torch.equal(sim.building_coef(), before)
  sim.close()


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_mixed_batch_does_not_depend_on_the_sharding(rank, world):
  need_gpu()
  plans = [the_plan("plan_small_test"), FloorPlan.from_file_input(rectangular_floor_plan((2, 3), (9, 10)), Materials.sb1(), 10.0, 300.0)]
  totals = [6, 5]
  _, _, _, bm0 = _table(plans[0], totals[0], seed=91)
  mixed = MixedBatchedEnvironment(list(zip(plans, totals)), rank=rank, world=world, collect_info=True,
                                  building_materials=[bm0, None])
  assert mixed.envs[0].sim._materials_handle and not mixed.envs[1].sim._materials_handle
  # stand-alone environments of each class's whole population: the rank's buildings must equal their rows
  wholes = [BatchedEnvironment(plans[0], totals[0], collect_info=True, building_materials=bm0),
            BatchedEnvironment(plans[1], totals[1], collect_info=True)]
  T = 6
  acts = [_acts(T, n, 93 + k) for k, n in enumerate(totals)]
  mixed.reset()
  for w in wholes:
    w.reset()
  for t in range(T):
    a = torch.cat([acts[k][t, lo:hi] for k, (lo, hi) in enumerate(mixed.class_ranges)]).contiguous()
    ts = mixed.step(a)
    for k, (w, (lo, hi), (s0, s1)) in enumerate(zip(wholes, mixed.class_ranges, mixed.slices)):
      tk = w.step(acts[k][t])
      assert torch.equal(ts.observation[s0:s1, :mixed.observation_widths[k]], tk.observation[lo:hi]), (t, k)
      assert torch.equal(ts.reward[s0:s1], tk.reward[lo:hi]), (t, k)
      assert torch.equal(mixed.envs[k].info, w.info[lo:hi]), (t, k)
  for k, (w, (lo, hi)) in enumerate(zip(wholes, mixed.class_ranges)):
    assert torch.equal(mixed.envs[k].sim.temps(), w.sim.temps()[lo:hi]), k
  lo, hi = mixed.class_ranges[0]
  assert np.array_equal(mixed.envs[0].building_materials()["conductivity"], bm0.fields["conductivity"][lo:hi])
  with pytest.raises(ValueError, match="one row per building of class 0"):
    mixed.set_building_materials([bm0.rows(0, 3), None])
  with pytest.raises(ValueError, match="class 1 was created without"):
    mixed.set_building_materials([None, _own(plans[1], totals[1], 100.0)])
  mixed.close()
  for w in wholes:
    w.close()
