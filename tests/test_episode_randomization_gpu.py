"""Episode randomisation on the GPU (sb_randomization_attach; host_inputs.EpisodeRandomization through BatchedSimulator,
BatchedEnvironment and MixedBatchedEnvironment).

The yardsticks: the rows in force against ``EpisodeRandomization.values`` (tests/randomization_cases.py), the coefficient
rows against FloorPlan's host fold of those materials, and an environment with the randomisation against a hand-driven
twin without it, which gets the same rows through set_building_params / set_building_materials.  Both sides run the
same kernels on rows of the same bits: every comparison is bitwise.

5 to 7 buildings of the 12 x 23 test plan or of the two-room 7 x 9 plan, episodes of 2 to 4 steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment  # noqa: E402
from sbsim_amd.floorplan import structural_class_coef  # noqa: E402
from sbsim_amd.host_inputs import BuildingMaterials, BuildingParams, Choice, EpisodeRandomization, Uniform  # noqa: E402
from tests import randomization_cases as rc  # noqa: E402
from tests.parity import need_gpu  # noqa: E402

LDS, REG, JACOBI = 0, 1, 7   # sb_sweep_kernel
SHORT = dict(num_days_in_episode=16 / 288, start_timestamp=rc.START, holiday_calendar=None)


def _np(t):
  return t.cpu().numpy()


def _assert_tables(sim, er, base, episodes, what, buildings=None):
  """The handle's two tables and coefficient rows are those of ``episodes`` (building b: values(b, episodes[b]))."""
  rows = rc.rows_in_force(er, base, episodes, buildings)
  pick = slice(None) if buildings is None else list(buildings)
  assert rc.same_bits(_np(sim.building_param_rows())[:, pick], rc.param_table(rows)[:, pick]), f"{what}: the parameter rows differ"
  if not sim._materials_handle:
    return rows
  assert rc.same_bits(_np(sim.building_material_rows())[:, pick], rc.material_table(rows)[:, pick]), f"{what}: the material rows differ"
  sp, coef = sim.compiled, _np(sim.building_coef())
  for b in (range(sim.B) if buildings is None else buildings):
    want = structural_class_coef(sp, rows["conductivity"][b], rows["heat_capacity"][b], rows["density"][b],
                                 rows["convection_coefficient"][b], sim.config.time_step_sec, sp.dx, sp.zh)
    assert rc.same_bits(coef[b], want), f"{what}: building {b}'s coefficient rows differ"
  return rows


def _sim(plan, B, materials=True, params=True, **kw):
  bm = rc.building_materials(plan, B) if materials else None
  bp = rc.building_params(B) if params else None
  sim = BatchedSimulator(plan, rc.config(), B, rc.H_CONV, building_materials=bm, **kw)
  if bp is not None:
    sim.set_building_params(bp)
  return sim, rc.base_rows(B, bp, bm, plan if materials else None)


# ---------------------------------------------------------------- 1. the rows in force
def test_rows_in_force_are_the_restatement_and_a_partial_reset_touches_no_other_building():
  need_gpu()
  B, plan = 7, rc.plan_small()
  sim, base = _sim(plan, B)
  assert sim.launch_info["kernel"] == LDS
  er = rc.randomization(materials=True)
  sim.randomization_attach(er)
  episodes = np.full(B, -1)
  _assert_tables(sim, er, base, episodes, "attached")              # nothing is drawn before a reset
  assert sim.randomization_episodes().tolist() == [0] * B
  for n in range(2):
    sim.reset()
    episodes += 1
    _assert_tables(sim, er, base, episodes, f"reset {n}")
    assert sim.randomization_episodes().tolist() == [n + 1] * B
    # the reset kernel read the new row
    scal = _np(sim.scalars())
    rows = rc.rows_in_force(er, base, episodes)
    assert rc.same_bits(scal[:, 0], rows["ahu_heating_air_temp_setpoint"]) and rc.same_bits(scal[:, 1], rows["ahu_cooling_air_temp_setpoint"])
    assert rc.same_bits(scal[:, 4], rows["boiler_reheat_water_setpoint"])
  for mask in (np.zeros(B, bool), np.arange(B) == 4, np.ones(B, bool), np.arange(B) % 2 == 0):
    before = [_np(t).copy() for t in (sim.building_param_rows(), sim.building_material_rows(), sim.building_coef(), sim.randomization_episodes())]
    sim.reset_buildings(mask)
    episodes = episodes + mask
    _assert_tables(sim, er, base, episodes, f"mask {mask.astype(int)}")
    after = [_np(t) for t in (sim.building_param_rows(), sim.building_material_rows(), sim.building_coef(), sim.randomization_episodes())]
    assert after[3].tolist() == (episodes + 1).tolist()
    keep = ~mask
    assert np.array_equal(before[0][:, keep].view(np.uint64), after[0][:, keep].view(np.uint64))
    assert np.array_equal(before[1][:, keep].view(np.uint64), after[1][:, keep].view(np.uint64))
    assert np.array_equal(before[2][keep].view(np.uint64), after[2][keep].view(np.uint64))
    assert np.array_equal(before[3][keep], after[3][keep])
  # the base rows stay what building_params() / building_materials() return, and the fingerprint names the randomisation
  assert rc.same_bits(rc.param_table(sim.building_params()), rc.param_table(base))
  assert ("episode_randomization", er.digest()) in sim.state_fingerprint()
  sim.randomization_detach()
  assert not any(isinstance(x, tuple) and x and x[0] == "episode_randomization" for x in sim.state_fingerprint())
  sim.close()


# ---------------------------------------------------------------- 2. the autoreset against a hand-driven twin
LAYOUTS = {   # name -> (materials, BatchedEnvironment arguments, the kernel)
    "register": (False, {}, REG),
    "lds-materials": (True, {}, LDS),
    "jacobi": (False, dict(solver="jacobi_fp32"), JACOBI),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_autoreset_is_a_twin_given_the_same_rows_by_hand(layout):
  need_gpu()
  materials, extra, kernel = LAYOUTS[layout]
  B, plan, lengths = 5, rc.plan_small(), np.array([2, 3, 4, 2, 3])
  bp = rc.building_params(B)
  bm = rc.building_materials(plan, B) if materials else None
  base = rc.base_rows(B, bp, bm, plan if materials else None)
  er = rc.randomization(materials)

  def tables(episodes):
    p, m = rc.split(rc.rows_in_force(er, base, episodes))
    return BuildingParams(p), (BuildingMaterials(**m) if m else None)

  common = dict(SHORT, collect_info=True, **extra)
  a = BatchedEnvironment(plan, B, episode_steps=lengths, building_params=bp, building_materials=bm, episode_randomization=er, **common)
  p0, m0 = tables(np.zeros(B, int))
  t = BatchedEnvironment(plan, B, per_building_episodes=True, building_params=p0, building_materials=m0, **common)
  assert a.sim.launch_info["kernel"] == kernel == t.sim.launch_info["kernel"], (a.sim.launch_info, t.sim.launch_info)
  ra, rt = a.reset(), t.reset()
  assert torch.equal(ra.observation, rt.observation)
  acts = torch.tensor(np.random.RandomState(5).uniform(-1, 1, size=(12, B, 2)).astype(np.float32), device="cuda")
  episodes, position, restarts = np.zeros(B, int), np.zeros(B, int), 0
  for n in range(12):
    sa = a.step(acts[n])
    st = t.step(acts[n])
    t_obs, t_rew = st.observation.clone(), st.reward.clone()
    assert torch.equal(sa.reward, t_rew), (layout, n)          # the last step of the old episode ran with the old row
    position += 1
    mask = position == lengths + 1   # (episode_steps transitions plus the terminal step)
    if mask.any():
      restarts += int(mask.sum())
      episodes = episodes + mask
      position[mask] = 0
      p, m = tables(episodes)
      t.set_building_params(p)
      if m is not None:
        t.set_building_materials(m)
      first = t.reset_buildings(mask).observation
      on, off = torch.from_numpy(mask).cuda(), torch.from_numpy(~mask).cuda()
      assert torch.equal(a.final_observation[on], t_obs[on]), (layout, n)
      assert torch.equal(sa.observation[on], first[on]), (layout, n)
      assert torch.equal(sa.observation[off], t_obs[off]), (layout, n)
    else:
      assert torch.equal(sa.observation, t_obs), (layout, n)
  assert restarts == 4 + 3 + 2 + 4 + 3 and a.sim.randomization_episodes().tolist() == (episodes + 1).tolist()
  _assert_tables(a.sim, er, base, episodes, layout)
  vals = a.randomized_values()
  rows = rc.rows_in_force(er, base, episodes)
  assert set(vals) == set(rc.param_fields()) | (set(rc.material_fields()) if materials else set())
  for name, v in vals.items():
    assert rc.same_bits(_np(v), rows[name]), name
  a.close(), t.close()


# ---------------------------------------------------------------- 3. shards
def test_shards_draw_what_the_whole_batch_draws():
  need_gpu()
  B, plan = 6, rc.plan_small()
  lengths = np.array([2, 3, 4, 2, 3, 4])
  bp, bm = rc.building_params(B), rc.building_materials(plan, B)
  er = rc.randomization(materials=True, seed=21)
  whole = BatchedEnvironment(plan, B, episode_steps=lengths, building_params=bp, building_materials=bm, episode_randomization=er, **SHORT)
  parts = [BatchedEnvironment(plan, 3, episode_steps=lengths[lo:lo + 3], building_params=bp.rows(lo, lo + 3),
                              building_materials=bm.rows(lo, lo + 3), episode_randomization=er.rows(lo), **SHORT) for lo in (0, 3)]
  assert [p.episode_randomization.first_building for p in parts] == [0, 3]
  acts = torch.tensor(np.random.RandomState(6).uniform(-1, 1, size=(6, B, 2)).astype(np.float32), device="cuda")
  outs = [whole.reset().observation.clone()] + [None] * 6
  part_outs = [[p.reset().observation.clone() for p in parts]] + [None] * 6
  for n in range(6):
    outs[n + 1] = whole.step(acts[n]).observation.clone()
    part_outs[n + 1] = [p.step(acts[n, lo:lo + 3].contiguous()).observation.clone() for p, lo in zip(parts, (0, 3))]
  for n in range(7):
    assert torch.equal(outs[n], torch.cat(part_outs[n])), n
  for get in ("building_param_rows", "building_material_rows"):
    assert torch.equal(getattr(whole.sim, get)(), torch.cat([getattr(p.sim, get)() for p in parts], dim=1)), get
  for e in [whole] + parts:
    e.close()


def test_a_mixed_batch_draws_what_its_single_class_environments_draw():
  need_gpu()
  plans = [rc.plan_small(), rc.plan_two_rooms()]
  er = EpisodeRandomization(params=rc.param_fields(), seed=33)
  mixed = MixedBatchedEnvironment([(plans[0], 3), (plans[1], 3)], episode_randomization=er, **SHORT)
  singles = [BatchedEnvironment(plans[k], 3, episode_randomization=er.rows(3 * k), **SHORT) for k in range(2)]
  assert [e.episode_randomization.first_building for e in mixed.envs] == [0, 3]
  acts = torch.tensor(np.random.RandomState(7).uniform(-1, 1, size=(2, 6, 2)).astype(np.float32), device="cuda")
  for episode in range(2):
    steps = [mixed.reset().observation.clone()] + [mixed.step(acts[n]).observation.clone() for n in range(2)]
    for k, (lo, hi) in enumerate(mixed.slices):
      s = singles[k]
      want = [s.reset().observation.clone()] + [s.step(acts[n, lo:hi].contiguous()).observation.clone() for n in range(2)]
      for n in range(3):
        assert torch.equal(steps[n][lo:hi, :s.sim.O], want[n]), (episode, k, n)
      torch.cuda.synchronize()   # (the classes run on streams of their own)
      assert torch.equal(mixed.envs[k].sim.building_param_rows(), s.sim.building_param_rows())
      base = rc.base_rows(3)
      _assert_tables(s.sim, er.rows(3 * k), base, np.full(3, episode), f"class {k}")
  mixed.close()
  for s in singles:
    s.close()


# ---------------------------------------------------------------- 4. checkpoint
def test_the_counters_are_the_checkpoint_and_detach_returns_the_base_rows():
  need_gpu()
  B, plan, lengths = 5, rc.plan_small(), np.array([1, 2, 3, 1, 6])   # episodes of 2, 3, 4, 2 and 7 steps
  bp, bm = rc.building_params(B), rc.building_materials(plan, B)
  base = rc.base_rows(B, bp, bm, plan)
  er = rc.randomization(materials=True, seed=44)
  env = BatchedEnvironment(plan, B, episode_steps=lengths, building_params=bp, building_materials=bm, episode_randomization=er, **SHORT)
  sim = env.sim
  env.reset()
  acts = torch.tensor(np.random.RandomState(8).uniform(-1, 1, size=(5, B, 2)).astype(np.float32), device="cuda")
  for n in range(5):
    env.step(acts[n])
  saved = sim.randomization_episodes().clone()
  assert saved.tolist() == [3, 2, 2, 3, 1]
  held = [t.clone() for t in (sim.building_param_rows(), sim.building_material_rows(), sim.building_coef())]
  sim.randomization_detach()
  with pytest.raises(ValueError, match="no randomisation"):
    sim.randomization_episodes()
  own = [sim.building_param_rows(), sim.building_material_rows(), sim.building_coef()]
  assert rc.same_bits(_np(own[0]), rc.param_table(base)) and rc.same_bits(_np(own[1]), rc.material_table(base))
  _assert_tables(sim, er, base, np.full(B, -1), "detached")        # ... and the coefficient rows are the base's fold
  sim.randomization_attach(er)
  assert sim.randomization_episodes().tolist() == [0] * B
  saved[4] = 0                                                    # a building that never drew keeps its base row
  sim.set_randomization_episodes(saved)
  assert torch.equal(sim.randomization_episodes(), saved)
  _assert_tables(sim, er, base, _np(saved).astype(int) - 1, "restored")
  now = [sim.building_param_rows(), sim.building_material_rows(), sim.building_coef()]
  for x, y in zip(held, now):
    idx = torch.arange(4, device="cuda")
    assert torch.equal(x.movedim(-1, 0)[idx] if x.dim() == 2 else x[idx], y.movedim(-1, 0)[idx] if y.dim() == 2 else y[idx])
  env.close()


# ---------------------------------------------------------------- 5. edges of the launch
def test_one_field_alone():
  need_gpu()
  B, plan = 5, rc.plan_small()
  sim, base = _sim(plan, B, materials=False, params=False)
  er = EpisodeRandomization(params={"boiler_reheat_water_setpoint": Uniform(330.0, 360.0)}, seed=1)
  sim.randomization_attach(er)   # a handle that never had a table: allocated from the SimConfig's values
  sim.reset()
  _assert_tables(sim, er, base, np.zeros(B, int), "one field")
  sim.randomization_detach()
  assert rc.same_bits(_np(sim.building_param_rows()), rc.param_table(base))
  sim.close()


def test_every_field_at_once_on_70_buildings():
  need_gpu()
  B, plan = 70, rc.plan_two_rooms()
  sim, base = _sim(plan, B)
  params, mats = rc.every_field(len(plan.material_slots()[1]))
  er = EpisodeRandomization(params=params, materials=mats, seed=2)
  assert len(er.fields) == _ffi.SB_NUM_BUILDING_PARAMS + 3 * len(plan.material_slots()[1]) + 1
  assert (B * len(er.fields)) % _ffi.SB_RAND_THREADS != 0 and B % 64 != 0
  sim.randomization_attach(er)
  sim.reset()
  mask = np.arange(B) % 3 == 1
  sim.reset_buildings(mask)
  _assert_tables(sim, er, base, mask.astype(int), "every field")
  sim.close()


def test_work_beyond_one_pass_of_the_capped_grid():
  need_gpu()
  plan = rc.plan_two_rooms()
  params, mats = rc.every_field(len(plan.material_slots()[1]))
  er = EpisodeRandomization(params=params, materials=mats, seed=3)
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  one_pass = cus * _ffi.SB_RAND_BLOCKS_PER_CU * _ffi.SB_RAND_THREADS
  B = one_pass // len(er.fields) + 4099
  assert B * len(er.fields) > one_pass and B < 40000
  sim, base = _sim(plan, B)
  sim.randomization_attach(er)
  sim.reset()
  mask = np.arange(B) % 5 == 2
  sim.reset_buildings(mask)
  sample = sorted({0, 1, 2, 63, 64, 255, 256, 257, B // 2, B // 2 + 1, one_pass // len(er.fields) - 1, one_pass // len(er.fields),
                   one_pass // len(er.fields) + 1, B - 3, B - 2, B - 1} | set(np.random.RandomState(9).randint(0, B, 24).tolist()))
  _assert_tables(sim, er, base, mask.astype(int), "grid stride", buildings=sample)
  assert sim.randomization_episodes().tolist() == (mask.astype(int) + 1).tolist()
  sim.close()


# ---------------------------------------------------------------- 6. what the library refuses
def test_device_side_refusals():
  need_gpu()
  B, plan = 5, rc.plan_small()
  sim, base = _sim(plan, B, materials=False)
  L = _ffi.load()
  err = lambda: (L.sb_last_error() or b"").decode()
  attach = _ffi.randomization_entry("sb_randomization_attach")
  er = EpisodeRandomization(params={"ahu_fan_efficiency": Uniform(0.7, 0.95)}, seed=1)
  arr, keep = er.c_fields(None)
  out = torch.zeros(B, dtype=torch.int32, device="cuda")
  stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
  # the counters of a handle without an attachment
  for name in ("sb_randomization_episodes_get", "sb_randomization_episodes_set"):
    assert _ffi.randomization_entry(name)(sim._h, C.c_void_p(out.data_ptr()), stream()) == -5 and "no randomisation" in err()
  # a material field on a handle sb_create made
  mat = (_ffi.RandField * 1)()
  mat[0].id, mat[0].kind, mat[0].lo, mat[0].hi = _ffi.SB_RAND_MATERIAL + 0, _ffi.SB_RAND_UNIFORM, 1.0, 2.0
  assert attach(sim._h, mat, 1, 1, 0) == -5 and "sb_create_materials" in err()
  assert rc.same_bits(_np(sim.building_param_rows()), rc.param_table(base))
  # the library's own range check (Python repeats it before the call)
  bad = (_ffi.RandField * 1)()
  bad[0].id, bad[0].kind, bad[0].lo, bad[0].hi = 3, _ffi.SB_RAND_UNIFORM, 285.0, 299.0   # ahu_heat_sp against 298
  assert attach(sim._h, bad, 1, 1, 0) == -1 and "ahu_heat_sp" in err() and "building 0" in err()
  assert attach(sim._h, arr, 1, 1, -1) == -1 and "first_building" in err()
  # attach while the stream is being captured: refused before the library is called (its hipDeviceSynchronize would be
  # refused too, but a refused synchronisation invalidates the capture in progress)
  s = torch.cuda.Stream()
  graph = torch.cuda.CUDAGraph()
  scratch = torch.zeros(4, device="cuda")
  with torch.cuda.stream(s):
    graph.capture_begin()
    try:
      scratch.add_(1.0)
      with pytest.raises(ValueError, match="captured"):
        sim.randomization_attach(er)
    finally:
      graph.capture_end()
  assert sim.randomization is None
  with pytest.raises(ValueError, match="no randomisation"):
    sim.randomization_episodes()
  # the tables belong to the randomisation while it is attached
  sim.randomization_attach(er)
  fields = np.array([0], dtype=np.int32)
  values = np.full((1, B), 0.04)
  set_params = _ffi.entry("sb_set_building_params")
  assert set_params(sim._h, 1, fields.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p), stream()) == -1
  assert "sb_randomization_detach first" in err()
  with pytest.raises(ValueError, match="randomization_detach first"):
    sim.set_building_params(rc.building_params(B))
  sim.randomization_detach()
  sim.set_building_params(rc.building_params(B))
  sim.close()
  # ... the materials' too
  msim, _ = _sim(plan, B)
  msim.randomization_attach(rc.randomization(materials=True))
  set_mats = _ffi.materials_entry("sb_set_building_materials")
  assert set_mats(msim._h, 0, None, None, stream()) == -1 and "sb_randomization_detach first" in err()
  with pytest.raises(ValueError, match="randomization_detach first"):
    msim.set_building_materials(None)
  msim.close()
