"""GPU: the reference's seeded convection shuffle per building on the device (sb_convection_attach_seeded,
k_convect_seeded) against its host twin ``host_convection.SeededHostConvection`` -- which
tests/test_convection.py::test_seeded_host_convection_replays_the_reference_draw_for_draw holds to the reference's own
output.  Every comparison is exact."""
import random

import numpy as np
import pytest

from sbsim_amd.floorplan import EXTERIOR_SPACE, INTERIOR_SPACE, WALL, FloorPlan, Materials, rectangular_floor_plan
from sbsim_amd.host_convection import SeededHostConvection

pytestmark = pytest.mark.gpu

SEEDS = (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 11)
SHORT = dict(holiday_calendar=None, num_days_in_episode=12 * 300 / 86400.0)   # 12 steps per episode


def _plan(rooms, shape):
  return FloorPlan.from_file_input(rectangular_floor_plan(rooms, shape), Materials.sb1(), 10.0, 300.0)


def _mixed_plan():
  """Rooms of 1 cell (the smallest the floor-plan code admits), 63, 64, 65 cells (one wavefront's worth of cells, one
  less, one more) and 120 cells (at p = 1 more than 624 words per call: the block is regenerated inside a room)."""
  a = np.full((24, 34), WALL, dtype=np.int8)
  a[0, :] = a[-1, :] = EXTERIOR_SPACE
  a[:, 0] = a[:, -1] = EXTERIOR_SPACE
  for x0, y0, h, w in ((3, 3, 1, 1), (3, 6, 7, 9), (3, 16, 8, 8), (12, 3, 5, 13), (12, 17, 10, 12)):
    a[x0:x0 + h, y0:y0 + w] = INTERIOR_SPACE
  plan = FloorPlan.from_file_input(a, Materials.sb1(), 10.0, 300.0)
  assert [len(c) for c in plan.zone_cell_lists()] == [1, 63, 64, 65, 120]
  return plan


def _rooms(plan):
  return [[(int(x), int(y)) for x, y in zip(*np.unravel_index(cells, plan.shape))] for cells in plan.zone_cell_lists()]


class Twins:
  """One SeededHostConvection per building; the candidate tables (geometry only) are computed once and shared."""

  def __init__(self, plan, p, distance, seeds):
    self.rooms = _rooms(plan)
    self.twins = [SeededHostConvection(p, distance, int(s)) for s in seeds]
    for t in self.twins[1:]:
      t._windows = self.twins[0]._windows

  def apply(self, grids, buildings=None):
    """grids [n, H, W] numpy, in place; row i belongs to twin buildings[i] (default: i)."""
    for i, b in enumerate(range(len(grids)) if buildings is None else buildings):
      self.twins[b].apply(self.rooms, grids[i])


def _sim(plan, B, **kw):
  from sbsim_amd.environment import BatchedSimulator, SimConfig
  return BatchedSimulator(plan, SimConfig.sb1(), B, 100.0, **kw)


def _random_start(sim, seed, same=()):
  """reset(temps=X), X random per building (buildings of `same` get building same[0]'s); returns temps() after it."""
  import torch
  rs = np.random.RandomState(seed)
  x = 285.0 + 20.0 * rs.rand(sim.B, sim.H * sim.W)
  for b in same[1:]:
    x[b] = x[same[0]]
  sim.reset(temps=torch.tensor(x, dtype=torch.float64, device="cuda"))
  return sim.temps().cpu().numpy()


def _tap_against_twins(sim, plan, p, distance, seeds, calls=4, same=()):
  start = _random_start(sim, 11, same)
  sim.convection_attach_seeded(p, distance, seeds)
  seeds = [int(s) for s in (seeds if not isinstance(seeds, int) else [seeds + b for b in range(sim.B)])]
  twins = Twins(plan, p, distance, seeds)
  expect = start.copy()
  for k in range(calls):
    sim.convection_apply()
    twins.apply(expect)
    got = sim.temps().cpu().numpy()
    for b in range(sim.B):
      assert np.array_equal(got[b], expect[b]), (k, b)
  assert not np.array_equal(expect, start)
  if same:
    assert all(np.array_equal(got[b], got[same[0]]) for b in same[1:])
  return twins, expect


def _as_words(t):
  return t.cpu().numpy().view(np.uint32)


def test_seeding_is_pythons():
  from tests.parity import need_gpu
  need_gpu()
  sim = _sim(_plan((2, 2), (5, 9)), 5)
  sim.convection_attach_seeded(1.0, 5, np.array(SEEDS, dtype=np.uint64))
  rows = _as_words(sim.convection_rng())
  assert rows.shape == (5, 625)
  for b, s in enumerate(SEEDS):
    assert tuple(int(v) for v in rows[b]) == random.Random(s).getstate()[1], s
  sim.convection_attach_seeded(1.0, 5, 2 ** 32 - 2)    # an integer s: building b gets s + b
  rows = _as_words(sim.convection_rng())
  for b in range(5):
    assert tuple(int(v) for v in rows[b]) == random.Random(2 ** 32 - 2 + b).getstate()[1], b
  assert sim.state_fingerprint()[-1] == ("seeded", 1.0, 5)
  sim.close()


@pytest.mark.parametrize("p,distance", [(1.0, 5), (0.5, 3), (0.3, 19), (1.0, -1)])
@pytest.mark.parametrize("which", ["mixed", "room45"])
def test_tap_equals_the_host_twin_per_building(which, p, distance):
  """Four convection_apply() calls from random grids, B = 5: after each call every building's grid is its own twin's.
  Buildings 1 and 3 share a seed and a start and stay identical.  Rooms of 1, 63, 64, 65 and 120 cells; one room of
  45 x 45 = 2025 cells."""
  from tests.parity import need_gpu
  need_gpu()
  plan = _mixed_plan() if which == "mixed" else _plan((1, 1), (45, 45))
  sim = _sim(plan, 5)
  seeds = np.array([SEEDS[0], 5, SEEDS[2], 5, SEEDS[4]], dtype=np.uint64)
  _tap_against_twins(sim, plan, p, distance, seeds, same=(1, 3))
  sim.close()


@pytest.mark.parametrize("rooms,shape,force_lds,orientation,kernel", [
    ((3, 3), (20, 30), False, "auto", 3), ((2, 2), (5, 9), False, "auto", 1), ((8, 5), (12, 14), False, "auto", 4),
    ((9, 4), (16, 17), False, "auto", 5), ((3, 3), (20, 30), True, "auto", 0), ((2, 2), (5, 9), False, "columns", None)])
def test_tap_on_every_state_layout_and_orientation(rooms, shape, force_lds, orientation, kernel, monkeypatch):
  """The five state layouts of the adapter test (k_sweep_roll, k_sweep_reg, k_sweep_two, k_sweep_band, the LDS-grid
  kernel) and a transposed handle: cell and candidate order stay the caller's."""
  from tests.parity import need_gpu
  need_gpu()
  if force_lds:
    monkeypatch.setenv("SBSIM_FORCE_LDS_PATH", "1")
  plan = _plan(rooms, shape)
  sim = _sim(plan, 5, orientation=orientation)
  if kernel is not None:
    assert sim.launch_info["kernel"] == kernel
  assert sim.transposed == (orientation == "columns") or orientation == "auto"
  _tap_against_twins(sim, plan, 1.0, 5, 40)
  sim.close()


def _pair(plan, B, conv, **kw):
  from sbsim_amd.environment import BatchedEnvironment
  a = BatchedEnvironment(plan, B, convection_simulator=conv, **SHORT, **kw)
  c = BatchedEnvironment(plan, B, **SHORT, **kw)
  return a, c


def _step_in_lockstep(a, c, twins, action, sample=None):
  """One step of both: A's grid is the twin's shuffle of C's (the finite-difference grid); rewards and observations are
  equal; then both take A's grid, so both recompute zone means and the grid mean from the same grid."""
  import torch
  ta, tc = a.step(action), c.step(action)
  assert torch.equal(ta.reward, tc.reward) and torch.equal(ta.observation, tc.observation)
  got = a.sim.temps()
  idx = list(range(a.batch_size)) if sample is None else sample
  expect = c.sim.temps()[idx].cpu().numpy()
  before = expect.copy()
  twins.apply(expect, idx)
  assert np.array_equal(got[idx].cpu().numpy(), expect) and not np.array_equal(expect, before)
  a.sim.set_temps(got)
  c.sim.set_temps(got)


def test_inside_the_step_only_the_grid_depends_on_the_generator():
  from tests.parity import need_gpu
  need_gpu()
  import torch
  from sbsim_amd.host_inputs import SeededStochasticConvectionSimulator
  plan, B = _plan((2, 2), (5, 9)), 6
  a, c = _pair(plan, B, SeededStochasticConvectionSimulator(1.0, 5, 7))
  twins = Twins(plan, 1.0, 5, [7 + b for b in range(B)])
  a.reset(), c.reset()
  rs = np.random.RandomState(2)
  for t in range(6):
    act = torch.tensor(rs.uniform(-1, 1, (B, 2)).astype(np.float32), device="cuda")
    _step_in_lockstep(a, c, twins, act)
  assert a.sim.save_state().clock[1] == 6     # sb_state_clock.conv_calls still counts the calls
  a.close(), c.close()


def test_more_buildings_than_workgroups():
  """The grid is capped (_ffi.SB_CONV_SEEDED_MAX_WORKGROUPS): with more buildings a workgroup takes a second building in
  its grid-stride loop and reloads the generator, the room and the swap list for it."""
  from tests.parity import need_gpu
  need_gpu()
  import torch
  from sbsim_amd import _ffi
  from sbsim_amd.host_inputs import SeededStochasticConvectionSimulator
  B = _ffi.SB_CONV_SEEDED_MAX_WORKGROUPS + 904
  assert B > _ffi.SB_CONV_SEEDED_MAX_WORKGROUPS and B >= 3000      # a second round for 904 workgroups
  plan = _plan((2, 2), (5, 9))
  a, c = _pair(plan, B, SeededStochasticConvectionSimulator(0.5, 3, 1000))
  sample = sorted({0, 1, 903, 904, 2047, 2048, 4095, 4096, 4097, 4500, 4998, 4999, 777, 3333, 4100, 2500})
  assert len(sample) == 16
  twins = Twins(plan, 0.5, 3, [1000 + b for b in range(B)])
  a.reset(), c.reset()
  rs = np.random.RandomState(4)
  for t in range(3):
    act = torch.tensor(rs.uniform(-1, 1, (B, 2)).astype(np.float32), device="cuda")
    _step_in_lockstep(a, c, twins, act, sample)
  a.close(), c.close()


def test_snapshot_restore_fork_and_the_index_clamp():
  from tests.parity import need_gpu
  need_gpu()
  import torch
  from sbsim_amd.environment import BatchedEnvironment
  from sbsim_amd.host_inputs import SeededStochasticConvectionSimulator, StochasticConvectionSimulator
  plan, B = _plan((2, 2), (5, 9)), 4
  env = BatchedEnvironment(plan, B, convection_simulator=SeededStochasticConvectionSimulator(0.5, 3, 21), **SHORT)
  env.reset()
  rs = np.random.RandomState(6)
  acts = torch.tensor(rs.uniform(-1, 1, (4, B, 2)).astype(np.float32), device="cuda")
  env.step(acts[0])
  snap = env.snapshot()
  assert snap.sim.conv_rng is not None and torch.equal(snap.sim.conv_rng, env.sim.convection_rng())

  def run():
    out = []
    for t in range(1, 4):
      ts = env.step(acts[t])
      out.append((env.sim.temps(), env.sim.convection_rng(), ts.reward.clone(), ts.observation.clone()))
    return out
  first = run()
  assert not torch.equal(first[-1][1], snap.sim.conv_rng)
  env.restore(snap)
  assert torch.equal(env.sim.convection_rng(), snap.sim.conv_rng)
  for x, y in zip(first, run()):
    assert all(torch.equal(u, v) for u, v in zip(x, y))
  # a fork leaves every slot's stream in place
  rng = env.sim.convection_rng()
  env.fork(torch.zeros(B, dtype=torch.int64, device="cuda"))
  assert torch.equal(env.sim.convection_rng(), rng)
  t0 = env.sim.temps()
  assert all(torch.equal(t0[b], t0[0]) for b in range(B))
  assert env.sim.save_state(rows=torch.arange(2, device="cuda")).conv_rng is None
  # a state_dict carries the generators
  from sbsim_amd.environment import EnvSnapshot
  again = EnvSnapshot.from_state_dict(snap.state_dict(), env.sim.tdev)
  assert torch.equal(again.sim.conv_rng, snap.sim.conv_rng)
  # seeded and counter-based snapshots do not load into one another; a seeded state without generators does not load
  other = BatchedEnvironment(plan, B, convection_simulator=StochasticConvectionSimulator(0.5, 3, seed=21), **SHORT)
  other.reset()
  other.step(acts[0])
  with pytest.raises(ValueError, match="generator set"):
    other.restore(snap)
  with pytest.raises(ValueError, match="generator set"):
    env.restore(other.snapshot())
  import dataclasses
  bare = dataclasses.replace(snap, sim=dataclasses.replace(snap.sim, conv_rng=None))
  with pytest.raises(ValueError, match="conv_rng"):
    env.restore(bare)
  other.close()
  # an index word of 10^6 in one row: the kernel clamps it to 624, every other building is its twin's
  sim = env.sim
  start = _random_start(sim, 8)
  sim.convection_attach_seeded(0.5, 3, 21)
  words = sim.convection_rng()
  words[2, 624] = 10 ** 6
  sim.set_convection_rng(words)
  sim.convection_apply()
  twins = Twins(plan, 0.5, 3, [21 + b for b in range(B)])
  expect = start.copy()
  twins.apply(expect)
  got = sim.temps().cpu().numpy()
  for b in (0, 1, 3):
    assert np.array_equal(got[b], expect[b]), b
  assert np.array_equal(np.sort(got[2].ravel()), np.sort(start[2].ravel()))        # still a permutation
  assert int(_as_words(sim.convection_rng())[2, 624]) <= 624
  env.close()


def test_refusals_leave_the_attachment_in_force():
  from tests.parity import need_gpu
  need_gpu()
  from sbsim_amd import _ffi
  from sbsim_amd.environment import BatchedEnvironment, MixedBatchedEnvironment
  from sbsim_amd.host_inputs import SeededStochasticConvectionSimulator
  plan = _plan((2, 2), (5, 9))
  sim = _sim(plan, 3)
  twins, expect = _tap_against_twins(sim, plan, 1.0, 5, 9, calls=1)
  before = sim.convection_rng()
  with pytest.raises(ValueError, match="SeededHostConvection"):
    sim.convection_attach_seeded(1.0, 20, 9)
  with pytest.raises(ValueError, match="SeededHostConvection"):
    sim.convection_attach_seeded(0.4, -1, 9)
  with pytest.raises(ValueError, match="negative"):
    sim.convection_attach_seeded(1.0, 5, -1)
  import torch
  assert torch.equal(sim.convection_rng(), before) and sim.state_fingerprint()[-1] == ("seeded", 1.0, 5)
  sim.convection_apply()                       # the generator attached before goes on drawing
  twins.apply(expect)
  assert np.array_equal(sim.temps().cpu().numpy(), expect)
  # attaching the counter-based kind replaces it (and the other way round); either detach form detaches
  sim.convection_attach(1.0, 5, seed=3)
  with pytest.raises(_ffi.SbsimError, match="sb_convection_attach_seeded first"):
    sim.convection_rng()
  with pytest.raises(ValueError, match="SeededHostConvection"):
    sim.convection_attach_seeded(1.0, 20, 9)
  assert sim.state_fingerprint()[-1] == (1.0, 5, 3, 0)
  sim.convection_apply()                       # (the counter-based generator, still attached)
  sim.convection_attach_seeded(1.0, 5, 9)
  sim.convection_attach(0.0, 5, seed=3)
  with pytest.raises(_ffi.SbsimError, match="attach"):
    sim.convection_apply()
  sim.close()
  big = _sim(_plan((1, 1), (46, 46)), 2)       # a room of 2116 cells
  with pytest.raises(ValueError, match="2047 cells"):
    big.convection_attach_seeded(1.0, 5, 1)
  big.close()
  conv = SeededStochasticConvectionSimulator(1.0, 5, 1)
  with pytest.raises(ValueError, match="jacobi_fp32"):
    BatchedEnvironment(plan, 2, solver="jacobi_fp32", convection_simulator=conv, **SHORT)
  jac = _sim(plan, 2, solver="jacobi_fp32")
  with pytest.raises(ValueError, match="jacobi_fp32"):
    jac.convection_attach_seeded(1.0, 5, 1)
  jac.close()
  with pytest.raises(ValueError, match="SeededStochasticConvectionSimulator"):
    MixedBatchedEnvironment([(plan, 2), (_plan((1, 2), (6, 8)), 2)], convection_simulator=conv, **SHORT)
  with pytest.raises(ValueError, match="shape"):
    BatchedEnvironment(plan, 2, convection_simulator=SeededStochasticConvectionSimulator(1.0, 5, [1, 2, 3]), **SHORT)


def test_per_building_episodes_do_not_rewind_the_streams():
  """reset_buildings(mask): the restarted buildings' generators stay where they are -- the reference seeds in its
  constructor only -- and the next step is the twin's that kept drawing."""
  from tests.parity import need_gpu
  need_gpu()
  import torch
  from sbsim_amd.host_inputs import SeededStochasticConvectionSimulator
  plan, B = _plan((2, 2), (5, 9)), 4
  a, c = _pair(plan, B, SeededStochasticConvectionSimulator(1.0, 5, 30), per_building_episodes=True)
  twins = Twins(plan, 1.0, 5, [30 + b for b in range(B)])
  a.reset(), c.reset()
  rs = np.random.RandomState(9)
  act = lambda: torch.tensor(rs.uniform(-1, 1, (B, 2)).astype(np.float32), device="cuda")
  for t in range(2):
    _step_in_lockstep(a, c, twins, act())
  rng = a.sim.convection_rng()
  mask = np.array([True, False, True, False])
  a.reset_buildings(mask), c.reset_buildings(mask)
  assert torch.equal(a.sim.convection_rng(), rng)
  _step_in_lockstep(a, c, twins, act())
  a.reset(), c.reset()                          # a whole-batch reset: a second episode draws on too
  assert not torch.equal(a.sim.convection_rng(), rng)
  _step_in_lockstep(a, c, twins, act())
  a.close(), c.close()
