"""GPU: sb_spatial (zone {min, max, mean} and the pooled temperature map from the device state) against its NumPy
restatement (tests/spatial_restatement.py), bit for bit.

Comparison target: the restatement applied to `sim.temps()`, the library's own view of building.temp -- so the test does
not depend on the exterior-ring rule of the register layouts; that `temps()` is the input where the layout stores it is
asserted separately.  Inputs give every cell a value of its own, float(b * N + g) as tests/convection_cases.py does, with
B * N < 2^24 so that the Jacobi solver's float32 grid holds them exactly."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment, SimConfig  # noqa: E402
from sbsim_amd.host_inputs import BuildingMaterials, SpatialOutputs  # noqa: E402
from tests import convection_cases as cc  # noqa: E402
from tests import handover_cases as hc  # noqa: E402
from tests import spatial_restatement as sr  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import need_gpu  # noqa: E402
from tests.twins import plan_from_npz  # noqa: E402

SHORT = dict(num_days_in_episode=12 / 288, holiday_calendar=None)


def _small():
  return plan_from_npz(load("plan_small_test.npz"))


def _r9():
  return cc._plan("R9")


def _same_bits(got, want):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
  return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(u), want.view(u))


def _grids(fp, B):
  H, W = fp.shape
  assert B * H * W < 2 ** 24
  return np.arange(B * H * W, dtype=np.float64).reshape(B, H, W)


def _put(sim, fp, grids):
  """reset(temps=...) (the Jacobi solver refuses set_temps); temps() is the input wherever the layout stores the cell."""
  sim.reset(temps=torch.tensor(grids, dtype=torch.float64, device="cuda").reshape(sim.B, -1))
  seen = sim.temps().cpu().numpy()
  stored = ~np.asarray(fp.exterior_space, dtype=bool)
  assert np.array_equal(seen[:, stored], grids[:, stored])
  return seen


def _check(sim, fp, pool, rows=None, seen=None):
  """spatial() of the attached pool against the restatement of temps(); returns the device outputs."""
  seen = sim.temps().cpu().numpy() if seen is None else seen
  pick = None if rows is None else torch.as_tensor(rows, device="cuda")
  stats, tmap = sim.spatial(pick)
  want_stats, want_map = sr.spatial(seen, fp.zone_cell_lists(), pool, rows)
  assert _same_bits(stats.cpu().numpy(), want_stats), (pool, rows)
  if pool is None:
    assert tmap is None
  else:
    assert tuple(tmap.shape[1:]) == sr.map_shape(*fp.shape, pool) == sim.map_shape
    assert _same_bits(tmap.cpu().numpy(), want_map), (pool, rows)
  return stats, tmap


def _own_materials(plan, B):
  table = plan.material_slots()[1]
  return BuildingMaterials(conductivity=np.tile(table[:, 0], (B, 1)), heat_capacity=np.tile(table[:, 1], (B, 1)),
                           density=np.tile(table[:, 2], (B, 1)), convection_coefficient=np.full(B, 100.0))


# name -> (plan, orientation, switches, BatchedSimulator arguments, (kernel, path, waves_per_building) or (kernel, path))
LAYOUTS = {name: (spec, orient, env + ((("SBSIM_FORCE_LDS_PATH", "1"),) if pin[1] == 0 else ()), {}, pin)
           for name, spec, orient, env, pin in cc.LAYOUTS}
LAYOUTS.update({
    "materials": ("small", "auto", (), dict(building_materials=True), (hc.LDS, 0)),
    "jacobi": ("small", "rows", (), dict(solver="jacobi_fp32"), (hc.JACOBI, 0)),
    "jacobi-global": ("small", "rows", (("SBSIM_FORCE_JACOBI_GLOBAL", "1"),), dict(solver="jacobi_fp32"), (hc.JACOBI, 2)),
})
assert set(LAYOUTS) == {"reg", "pair", "roll", "two", "band2", "band3", "band4", "lds-rows", "lds-columns", "materials",
                        "jacobi", "jacobi-global"}


def _layout_sim(name, monkeypatch, B=2):
  spec, orient, switches, extra, pin = LAYOUTS[name]
  monkeypatch.delenv(hc.SWITCH, raising=False)
  for k, v in switches:
    monkeypatch.setenv(k, v)
  fp = _small() if spec == "small" else cc._plan(spec)
  extra = dict(extra)
  if extra.get("building_materials"):
    extra["building_materials"] = _own_materials(fp, B)
  sim = BatchedSimulator(fp, SimConfig.sb1(), B, 100.0, orientation=orient, **extra)
  info = sim.launch_info
  assert (info["kernel"], info["path"], info["waves_per_building"])[:len(pin)] == pin, (name, info)
  if orient != "auto":
    assert sim.transposed == (orient == "columns")
  return sim, fp


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_layout_against_the_restatement(name, monkeypatch):
  """Pools (1, 1): the map is temps() rounded to float32; (4, 4): on 68 x 98 the last column of tiles is ragged; (H, W):
  a 1 x 1 map, one wave-order tile; none: zone statistics only, a map request raises.  R9 also (5, 7) and a ragged
  wave-order pool (9, 8)."""
  need_gpu()
  sim, fp = _layout_sim(name, monkeypatch)
  H, W = fp.shape
  seen = _put(sim, fp, _grids(fp, sim.B))
  with pytest.raises(ValueError, match="spatial_attach"):
    sim.spatial()
  pools = [(1, 1), (4, 4), (H, W)] + ([(5, 7), (9, 8)] if name == "roll" else [])
  for pool in pools:
    sim.spatial_attach(pool)
    _, tmap = _check(sim, fp, pool, seen=seen)
    if pool == (1, 1):
      assert _same_bits(tmap.cpu().numpy(), seen.astype(np.float32))
    if pool == (H, W):
      assert tuple(tmap.shape) == (sim.B, 1, 1)
  if name == "roll":
    assert (H, W) == (68, 98) and sr.map_shape(H, W, (4, 4)) == (17, 25)
  sim.spatial_attach(None)
  assert sim.map_shape is None
  _check(sim, fp, None, seen=seen)
  with pytest.raises(ValueError, match="needs a pool size"):
    sim.temperature_map()
  assert _same_bits(sim.zone_temp_stats().cpu().numpy(), sr.zone_stats(seen, fp.zone_cell_lists()))
  sim.close()


@pytest.mark.parametrize("plan", ["sizes", "shapes", "quirks"])
def test_room_shapes(plan):
  """Rooms of 1, 2, 3, 64, 65 and 600 cells (a lone lane, one full round, one cell into the second); an L-shaped room
  and a zone of distant pieces; a zone made of two rooms."""
  need_gpu()
  fp = cc.PLANS[plan]()
  if plan == "sizes":
    assert sorted(len(c) for c in fp.zone_cell_lists()) == [1, 2, 3, 64, 65, 600]
  sim = BatchedSimulator(fp, SimConfig.sb1(), 3, 100.0)
  seen = _put(sim, fp, _grids(fp, 3))
  for pool in ((4, 4), (3, 5)):
    sim.spatial_attach(pool)
    _check(sim, fp, pool, seen=seen)
  sim.close()


def test_same_bits_on_every_layout(monkeypatch):
  """The same R9 input on the register layout, the LDS grid by rows and the LDS grid transposed: byte-identical."""
  need_gpu()
  outs = []
  for name in ("roll", "lds-rows", "lds-columns"):
    sim, fp = _layout_sim(name, monkeypatch, B=3)
    for k, _ in LAYOUTS[name][2]:
      monkeypatch.delenv(k, raising=False)
    grids = _grids(fp, 3)
    grids[:, np.asarray(fp.exterior_space, dtype=bool)] = 5.0   # (one value outside: what every layout reports there)
    seen = _put(sim, fp, grids)
    assert np.array_equal(seen, grids)
    sim.spatial_attach((4, 4))
    stats, tmap = sim.spatial()
    sim.spatial_attach((17, 14))
    outs.append((stats.cpu(), tmap.cpu(), sim.temperature_map().cpu()))
    sim.close()
  for other in outs[1:]:
    for a, b in zip(outs[0], other):
      assert _same_bits(a.numpy(), b.numpy())


def test_picks():
  need_gpu()
  fp = _small()
  B = 4
  sim = BatchedSimulator(fp, SimConfig.sb1(), B, 100.0)
  seen = _put(sim, fp, _grids(fp, B))
  sim.spatial_attach((4, 4))
  whole = _check(sim, fp, (4, 4), seen=seen)
  for rows in ([2, 0, 3, 0, 1], [3], [1, 2], list(range(B))):
    stats, tmap = _check(sim, fp, (4, 4), rows=rows, seen=seen)
    idx = torch.as_tensor(rows, device="cuda")
    assert torch.equal(stats, whole[0][idx]) and torch.equal(tmap, whole[1][idx])
  # rows the launch does not name keep what they held: outputs of 4 rows, a pick of 2 through the C entry
  fn = _ffi.spatial_entry("sb_spatial")
  stats = torch.full((B, sim.Z, 3), -7.0, dtype=torch.float64, device="cuda")
  tmap = torch.full((B,) + sim.map_shape, -7.0, dtype=torch.float32, device="cuda")
  pick = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
  assert fn(sim._h, C.c_void_p(pick.data_ptr()), 2, C.c_void_p(stats.data_ptr()), C.c_void_p(tmap.data_ptr()), sim._stream()) == 0
  assert torch.equal(stats[:2], whole[0][pick.long()]) and torch.equal(tmap[:2], whole[1][pick.long()])
  assert bool((stats[2:] == -7.0).all()) and bool((tmap[2:] == -7.0).all())
  # a pick outside [0, B) leaves its row untouched (Python refuses it before the launch; the C entry skips the row)
  stats.fill_(-7.0)
  pick = torch.tensor([B, 2, -1], dtype=torch.int32, device="cuda")
  assert fn(sim._h, C.c_void_p(pick.data_ptr()), 3, C.c_void_p(stats.data_ptr()), None, sim._stream()) == 0
  assert bool((stats[0] == -7.0).all()) and bool((stats[2:] == -7.0).all()) and torch.equal(stats[1], whole[0][2])
  # caller-owned outputs
  out = torch.zeros((2, sim.Z, 3), dtype=torch.float64, device="cuda")
  assert sim.zone_temp_stats(torch.tensor([1, 3], device="cuda"), out=out) is out and torch.equal(out, whole[0][[1, 3]])
  before = out.clone()
  for bad, msg in ((torch.tensor([0.0, 1.0], device="cuda"), "int32 or int64"),
                   (torch.tensor([[0, 1]], device="cuda"), "non-empty 1-D"),
                   (torch.zeros((0,), dtype=torch.int64, device="cuda"), "non-empty 1-D"),
                   (torch.tensor([0, 1]), "must be on"),
                   (torch.tensor([0, B], device="cuda"), "out of range"),
                   (torch.tensor([-1, 0], device="cuda"), "out of range"),
                   ([0, 1], "int32 or int64")):
    with pytest.raises(ValueError, match=msg):
      sim.zone_temp_stats(bad, out=out)
  with pytest.raises(ValueError, match="stats_out must be a contiguous"):
    sim.zone_temp_stats(torch.tensor([1], device="cuda"), out=out)
  with pytest.raises(ValueError, match="map_out must be a contiguous"):
    sim.temperature_map(out=torch.zeros((B,) + sim.map_shape, dtype=torch.float64, device="cuda"))
  assert torch.equal(out, before)
  sim.close()


def test_grid_stride_on_one_cu(monkeypatch):
  """The tiny plan under SBSIM_DEBUG_CUS=1 with B = 4 * 32 + 3: every workgroup runs several rows, the last round is
  partly empty; every row must be right, picked or not."""
  need_gpu()
  monkeypatch.setenv(hc.SWITCH, "1")
  fp = cc._plan(cc.TINY)
  B = cc.B_HANDOVER
  assert B == 4 * 32 + 3
  sim = BatchedSimulator(fp, SimConfig.sb1(), B, 100.0, orientation="rows")
  seen = _put(sim, fp, _grids(fp, B))
  sim.spatial_attach((4, 4))
  _check(sim, fp, (4, 4), seen=seen)
  _check(sim, fp, (4, 4), rows=list(range(B - 1, -1, -1)) + [5, 5], seen=seen)
  sim.close()


@pytest.mark.parametrize("solver", ["gauss_seidel", "jacobi_fp32"])
def test_after_real_steps(solver):
  """Three steps of random actions (R9 on the default kernel: the ring now holds the step's ambient temperature, the
  uniform case; the small plan on the Jacobi solver): the outputs are the restatement of temps() bit for bit, and the
  zone mean is within 1e-9 K of zone_temps()."""
  need_gpu()
  fp = _r9() if solver == "gauss_seidel" else _small()
  B = 4
  env = BatchedEnvironment(fp, B, solver=solver, spatial=SpatialOutputs(pool=(4, 4)), **SHORT)
  env.reset()
  rs = np.random.RandomState(5)
  for _ in range(3):
    env.step(torch.tensor(rs.uniform(-1, 1, (B, 2)), dtype=torch.float32, device="cuda"))
  stats, _ = _check(env.sim, fp, (4, 4))
  assert torch.equal(stats, env.zone_temp_stats)
  assert float((stats[:, :, 2] - env.sim.zone_temps()).abs().max()) <= 1e-9
  assert bool((stats[:, :, 0] <= stats[:, :, 2]).all()) and bool((stats[:, :, 2] <= stats[:, :, 1]).all())
  assert bool((stats[:, :, 0] < stats[:, :, 1]).any())
  env.close()


def _direct(env):
  return env.sim.spatial()


def test_environment_outputs_follow_reset_step_snapshot_and_fork():
  need_gpu()
  fp, B = _small(), 4
  env = BatchedEnvironment(fp, B, spatial=SpatialOutputs(pool=(4, 4)), **SHORT)
  assert env.final_temperature_map is None and env.final_zone_temp_stats is None
  rs = np.random.RandomState(9)
  act = lambda: torch.tensor(rs.uniform(-1, 1, (B, 2)), dtype=torch.float32, device="cuda")
  env.reset()
  assert tuple(env.temperature_map.shape) == (B,) + sr.map_shape(*fp.shape, (4, 4))
  assert tuple(env.zone_temp_stats.shape) == (B, fp.n_zones, 3)
  for k in range(3):
    stats, tmap = _direct(env)
    assert torch.equal(env.zone_temp_stats, stats) and torch.equal(env.temperature_map, tmap), k
    _check(env.sim, fp, (4, 4))
    env.step(act())
  snap = env.snapshot()
  assert not any("map" in k or "stats" in k for k in snap.state_dict()) and "spatial" not in repr(snap.sim.fingerprint)
  kept = (env.zone_temp_stats.clone(), env.temperature_map.clone())
  env.step(act())
  env.step(act())
  assert not torch.equal(env.zone_temp_stats, kept[0])
  env.restore(snap)
  assert torch.equal(env.zone_temp_stats, kept[0]) and torch.equal(env.temperature_map, kept[1])
  src = torch.tensor([2, 2, 0, 1], device="cuda")
  before = env.zone_temp_stats.clone()
  env.fork(src)
  assert torch.equal(env.zone_temp_stats, before[src]) and torch.equal(env.zone_temp_stats, _direct(env)[0])
  env.close()
  only_map = BatchedEnvironment(fp, B, spatial=SpatialOutputs(pool=(2, 3), zone_stats=False), **SHORT)
  only_map.reset()
  assert only_map.zone_temp_stats is None and torch.equal(only_map.temperature_map, only_map.sim.temperature_map())
  only_map.close()
  with pytest.raises(ValueError, match="must be a host_inputs.SpatialOutputs"):
    BatchedEnvironment(fp, B, spatial=(4, 4), **SHORT)


def test_environment_with_episodes_per_building():
  """Episode lengths 2, 3, 5, 2, 7, 12, 3.  The twin has every length 12 and runs the same actions: until a building's
  first episode ends, the two environments' copies of it are in the same state, so a direct call on the twin after the
  step is the call "just before the reset" of the buildings that end in that step."""
  need_gpu()
  fp = _small()
  steps = np.array([2, 3, 5, 2, 7, 12, 3])
  B = len(steps)
  sp = SpatialOutputs(pool=(4, 4))
  env = BatchedEnvironment(fp, B, episode_steps=steps, spatial=sp, **SHORT)
  twin = BatchedEnvironment(fp, B, per_building_episodes=True, spatial=sp, **SHORT)
  env.reset()
  twin.reset()
  assert bool((env.final_zone_temp_stats == 0).all()) and bool((env.final_temperature_map == 0).all())
  fresh = (env.zone_temp_stats.clone(), env.temperature_map.clone())   # every building at its reset state
  rs = np.random.RandomState(13)
  checked = 0
  for k in range(1, 9):   # (a building of episode_steps s returns LAST at its (s + 1)-th step, as the reference's counter does)
    a = torch.tensor(rs.uniform(-1, 1, (B, 2)), dtype=torch.float32, device="cuda")
    finals = (env.final_zone_temp_stats.clone(), env.final_temperature_map.clone())
    ts = env.step(a)
    twin.step(a)
    ended = ts.step_type.cpu().numpy() == 2
    assert ended.tolist() == [k % (s + 1) == 0 for s in steps.tolist()]
    first_end = ended & (steps + 1 == k)
    want = twin.sim.spatial()
    others = torch.as_tensor(~ended, device="cuda")
    for got, old, ref, cur, new in zip((env.final_zone_temp_stats, env.final_temperature_map), finals, want,
                                       (env.zone_temp_stats, env.temperature_map), fresh):
      assert torch.equal(got[others], old[others])                                           # the others keep their rows
      if first_end.any():
        idx = torch.as_tensor(np.nonzero(first_end)[0], device="cuda")
        assert torch.equal(got[idx], ref[idx])
        checked += len(idx)
      if ended.any():                                                                        # restarted: the reset state
        idx = torch.as_tensor(np.nonzero(ended)[0], device="cuda")
        assert torch.equal(cur[idx], new[idx]) and not torch.equal(got[idx], new[idx])
    direct = _direct(env)
    assert torch.equal(env.zone_temp_stats, direct[0]) and torch.equal(env.temperature_map, direct[1])
  assert checked == 2 * 6     # buildings 0, 3 (step 3), 1, 6 (4), 2 (6), 4 (8), both outputs
  mask = np.array([False, True, False, False, False, True, False])
  env.reset_buildings(mask)
  idx = torch.as_tensor(np.nonzero(mask)[0], device="cuda")
  assert torch.equal(env.zone_temp_stats[idx], fresh[0][idx]) and torch.equal(env.zone_temp_stats, _direct(env)[0])
  env.close()
  twin.close()


def test_mixed_batch_and_the_default():
  need_gpu()
  small, tiny = _small(), cc._plan(cc.TINY)
  assert small.shape != tiny.shape
  mixed = MixedBatchedEnvironment([(small, 3), (tiny, 2)], spatial=SpatialOutputs(pool=(4, 4)), **SHORT)
  mixed.reset()
  mixed.step(torch.zeros((5, 2), dtype=torch.float32, device="cuda"))
  torch.cuda.synchronize()
  for k, (fp, n) in enumerate(((small, 3), (tiny, 2))):
    assert tuple(mixed.temperature_maps[k].shape) == (n,) + sr.map_shape(*fp.shape, (4, 4))
    assert tuple(mixed.zone_temp_stats[k].shape) == (n, fp.n_zones, 3)
    stats, tmap = mixed.envs[k].sim.spatial()
    assert torch.equal(mixed.zone_temp_stats[k], stats) and torch.equal(mixed.temperature_maps[k], tmap)
    _check(mixed.envs[k].sim, fp, (4, 4))
  per_class = MixedBatchedEnvironment([(small, 3), (tiny, 2)], spatial=[SpatialOutputs(pool=(2, 2), zone_stats=False), None],
                                      **SHORT)
  per_class.reset()
  assert per_class.temperature_maps[1] is None and per_class.zone_temp_stats == [None, None]
  assert tuple(per_class.temperature_maps[0].shape) == (3,) + sr.map_shape(*small.shape, (2, 2))
  with pytest.raises(ValueError, match="spatial: one per class"):
    MixedBatchedEnvironment([(small, 3), (tiny, 2)], spatial=[None], **SHORT)
  # off (the default): nothing is built
  plain = BatchedEnvironment(small, 3, **SHORT)
  plain.reset()
  assert plain.spatial is None and plain.temperature_map is None and plain.zone_temp_stats is None
  assert plain.final_temperature_map is None and plain.final_zone_temp_stats is None
  assert plain.sim.launch_info == mixed.envs[0].sim.launch_info and plain.sim.map_shape is None
  for e in (mixed, per_class, plain):
    e.close()


def test_refusals_of_the_c_entries():
  need_gpu()
  fp, B = _small(), 2
  attach, run = _ffi.spatial_entry("sb_spatial_attach"), _ffi.spatial_entry("sb_spatial")
  err = lambda: _ffi.load().sb_last_error().decode()
  sim = BatchedSimulator(fp, SimConfig.sb1(), B, 100.0)
  stats = torch.full((B, sim.Z, 3), -7.0, dtype=torch.float64, device="cuda")
  mh, mw = sr.map_shape(*fp.shape, (4, 4))
  tmap = torch.full((B, mh, mw), -7.0, dtype=torch.float32, device="cuda")
  ps, pm, st = C.c_void_p(stats.data_ptr()), C.c_void_p(tmap.data_ptr()), sim._stream()
  assert attach(None, 4, 4, 0) == -1 and "null handle" in err()
  assert run(None, None, B, ps, pm, st) == -1 and "null handle" in err()
  for pool in ((-1, 4), (4, -1), (-2, -2)):
    assert attach(sim._h, *pool, 0) == -1 and "negative pool" in err()
  for pool in ((0, 4), (4, 0)):
    assert attach(sim._h, *pool, 0) == -1 and "both 0" in err()
  assert run(sim._h, None, B, ps, pm, st) == -1 and "sb_spatial_attach first" in err()    # (the refused attaches attached nothing)
  assert attach(sim._h, 4, 4, int(sim.transposed)) == 0
  # before the first sb_reset: sb_create resets once itself, so a handle is in that state only after sb_state_load put a
  # snapshot's "never reset" into it (tests/test_building_episodes_gpu.py does the same)
  snap = sim.save_state()
  snap.clock = (snap.clock[0], snap.clock[1], 0, 0)
  sim.load_state(snap)
  assert run(sim._h, None, B, ps, pm, st) == -1 and "sb_reset first" in err()
  sim.reset()
  for n in (0, -1):
    assert run(sim._h, None, n, ps, pm, st) == -1 and "n > 0" in err()
  assert run(sim._h, None, B - 1, ps, pm, st) == -1 and "n must be the batch size" in err()
  assert run(sim._h, None, B, None, None, st) == -1 and "both outputs are NULL" in err()
  assert attach(sim._h, 0, 0, int(sim.transposed)) == 0
  assert run(sim._h, None, B, ps, pm, st) == -1 and "a map needs a pool size" in err()
  assert run(sim._h, None, B, None, pm, st) == -1 and "a map needs a pool size" in err()
  torch.cuda.synchronize()
  assert bool((stats == -7.0).all()) and bool((tmap == -7.0).all())      # no refused call launched anything
  assert run(sim._h, None, B, ps, None, st) == 0
  torch.cuda.synchronize()
  assert bool((stats != -7.0).all())
  sim.close()
