"""Several calendars in one batch (BatchedEnvironment(calendars=..., calendar_of=...)) on the GPU.  The oracle is the
single-calendar environment itself: the buildings of calendar k must equal, bit for bit, a plain ``BatchedEnvironment`` of
as many buildings that has the calendar's members as its own models -- both sides run the same kernels on inputs of the
same bits (tests/test_clock_gpu.py pins the clock path to the shared-clock path; the single-calendar tests pin every member
to the reference).  The calendars are tests/calendar_cases.py's: they differ in every member and each crosses its own
comfort switch inside the run, which is asserted on the host rows before the GPU is touched."""
import ctypes as C
import dataclasses
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.host_inputs import Calendar  # noqa: E402
from tests import calendar_cases as cc  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import need_gpu  # noqa: E402
from tests.twins import plan_from_npz  # noqa: E402

UTC, DT = cc.UTC, cc.DT
B, K, T = 12, 3, 30
CALENDAR_OF = np.arange(B) % K   # interleaved: neighbouring lanes read three different segments of the table
EPISODE = dict(num_days_in_episode=cc.episode_days(40))


def _actions(n_steps, n_buildings, seed=3):
  return torch.tensor(np.random.RandomState(seed).uniform(-1, 1, size=(n_steps, n_buildings, 2)).astype(np.float32),
                      device="cuda")


def _outputs(env, ts):
  out = dict(step_type=ts.step_type, observation=ts.observation, reward=ts.reward, discount=ts.discount,
             info=env.info, temps=env.sim.temps())
  if env.final_observation is not None:
    out["final_observation"] = env.final_observation
  if env._occ_count is not None:
    out["occupants"] = env._occ_count
  return {k: v.clone() for k, v in out.items()}


def _rollout(env, acts, between=None):
  """reset(), then one step per row of acts; between: {step: f(env) -> TimeStep} run before that step, its outputs kept."""
  outs = [_outputs(env, env.reset())]
  for t in range(acts.shape[0]):
    if between is not None and t in between:
      outs.append(_outputs(env, between[t](env)))
    outs.append(_outputs(env, env.step(acts[t])))
  return outs


def _assert_group_equals(got, want, rows, what):
  idx = torch.as_tensor(rows, device="cuda")
  assert len(got) == len(want)
  for t, (g, w) in enumerate(zip(got, want)):
    assert g.keys() == w.keys()
    for k in g:
      assert torch.equal(g[k][idx], w[k]), f"{what}: call {t}: {k} differs"


def _plain(plan, k, n, **kw):
  """A plain environment of n buildings with calendar k's members as its own models."""
  cfg = dataclasses.replace(SimConfig.sb1(), **cc.config_fields(k))
  return BatchedEnvironment(plan, n, config=cfg, collect_info=True, **cc.plain_kwargs(k), **EPISODE, **kw)


def test_a_mixed_batch_equals_its_single_calendar_environments():
  tl = host_inputs.CalendarTimeline(cc.calendars(), CALENDAR_OF, cc.base_models(), cc.STARTS[0], None, 40)
  assert all(cc.crosses_comfort(tl, b, T) for b in range(B))   # every calendar crosses its own comfort switch in the run
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  # member j of every group takes the same actions: what differs between the groups is their calendars'
  acts = _actions(T, B // K)[:, np.arange(B) // K].contiguous()
  env = BatchedEnvironment(plan, B, calendars=cc.calendars(), calendar_of=CALENDAR_OF, collect_info=True, **EPISODE)
  assert isinstance(env.timeline, host_inputs.CalendarTimeline) and np.array_equal(env.timeline.rows, tl.rows)
  got = _rollout(env, acts)
  assert env.current_simulation_timestamps() == [cc.STARTS[b % K] + T * DT for b in range(B)]
  assert env.current_simulation_timestamp == dt.datetime(2023, 7, 6, 7, 0, 0) + T * DT   # the base clock
  env.close()
  for k in range(K):
    rows = np.nonzero(CALENDAR_OF == k)[0]
    plain = _plain(plan, k, len(rows))
    assert plain.timeline is None
    want = _rollout(plain, acts[:, rows].contiguous())
    plain.close()
    _assert_group_equals(got, want, rows, f"calendar {k}")
  # the groups are not one calendar: member 0 of each (same actions, same initial state) sees other inputs and ends elsewhere
  last = got[-1]
  for i, j in ((0, 1), (0, 2), (1, 2)):
    for name in ("observation", "reward", "info", "temps"):
      assert not torch.equal(last[name][i], last[name][j]), (i, j, name)


def _generators(first_building=(0, 0, 0)):
  """Three device generators that differ in the four hours and in zone_assignment (1 and 32 among them), all inside
  their arrival window at 07:00 UTC."""
  mk = host_inputs.BatchedRandomizedArrivalDepartureOccupancy
  return [mk(1, 6, 9, 15, 18, 300, seed=99, time_zone="UTC", first_building=first_building[0]),
          mk(32, 5, 8, 14, 19, 300, seed=99, time_zone="UTC", first_building=first_building[1]),
          mk(5, 7, 10, 16, 20, 300, seed=99, time_zone="UTC", first_building=first_building[2])]


def test_device_occupancy_per_group():
  bounds = [(0, 7), (7, 13), (13, 20)]   # contiguous groups; 20 buildings: the last wavefront's tail lanes are idle
  n = bounds[-1][1]
  group_of = np.concatenate([np.full(hi - lo, k) for k, (lo, hi) in enumerate(bounds)])
  start = dt.datetime(2023, 7, 6, 7, 0, tzinfo=UTC)   # Thursday 07:00 UTC
  starts = [start, start + dt.timedelta(days=7), start + dt.timedelta(days=14)]
  for gen, s in zip(_generators(), starts):
    assert gen.hours[0] <= s.hour <= gen.hours[1] and gen.is_work_day(s)
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  acts = _actions(T, n, seed=5)
  kw = dict(occupancy_normalization_constant=2.0, holiday_calendar=None, collect_info=True, **EPISODE)
  env = BatchedEnvironment(plan, n, calendars=[Calendar(occupancy=g, start_timestamp=s) for g, s in zip(_generators(), starts)],
                           calendar_of=group_of, start_timestamp=start, **kw)
  assert env.sim._occ_attached[0] == "groups" and len(env.sim._occ_attached[1]) == 3
  got = _rollout(env, acts)
  env.close()
  for k, (lo, hi) in enumerate(bounds):
    single = BatchedEnvironment(plan, hi - lo, occupancy=_generators(first_building=(lo, lo, lo))[k], start_timestamp=starts[k], **kw)
    want = _rollout(single, acts[:, lo:hi].contiguous())
    single.close()
    _assert_group_equals(got, want, np.arange(lo, hi), f"group {k}")
  counts = [got[-1]["occupants"][lo:hi] for lo, hi in bounds]
  assert all(float(c.sum()) > 0 for c in counts)
  assert float(counts[0].max()) <= 1 and float(counts[1].max()) > 5 and 1 < float(counts[2].max()) <= 5
  means = [float(c.mean()) for c in counts]
  assert len(set(means)) == 3


def test_per_building_episodes_with_calendars():
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  steps = np.array([5, 9, 12, 7, 12, 6, 11, 8, 5, 10, 12, 9], dtype=np.int64)   # mixed; autoresets inside the run
  offsets = np.array([0, 3, 1, 0, 2, 5, 4, 0, 0, 1, 0, 2], dtype=np.int64)
  mask = np.zeros(B, dtype=bool)
  mask[[1, 2, 7, 9]] = True   # calendars 1, 2, 1, 0: one reset_buildings call across the calendars
  assert len(set(CALENDAR_OF[mask])) == 3
  acts = _actions(T, B, seed=9)
  short = dict(num_days_in_episode=cc.episode_days(12))
  env = BatchedEnvironment(plan, B, calendars=cc.calendars(), calendar_of=CALENDAR_OF, collect_info=True, episode_steps=steps,
                           start_offsets=offsets, **short)
  got = _rollout(env, acts, between={14: lambda e: e.reset_buildings(mask)})
  positions = env.episode_positions()
  stamps = env.current_simulation_timestamps()
  assert stamps == [cc.STARTS[b % K] + (int(offsets[b]) + int(positions[b])) * DT for b in range(B)]
  env.close()
  kinds = torch.stack([g["step_type"] for g in got]).cpu().numpy()
  assert (kinds == 2).any(axis=0).all() and len(set((kinds == 2).sum(axis=0))) > 1   # every building ended, not all alike
  for k in range(K):
    rows = np.nonzero(CALENDAR_OF == k)[0]
    cfg = dataclasses.replace(SimConfig.sb1(), **cc.config_fields(k))
    single = BatchedEnvironment(plan, len(rows), config=cfg, collect_info=True, episode_steps=steps[rows],
                                start_offsets=offsets[rows], **cc.plain_kwargs(k), **short)
    want = _rollout(single, acts[:, rows].contiguous(), between={14: lambda e: e.reset_buildings(mask[rows])})
    single.close()
    _assert_group_equals(got, want, rows, f"calendar {k}")


def test_snapshot_and_restore_replay_bitwise_and_refuse_another_calendar_of():
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  acts = _actions(9, B, seed=4)
  offsets = np.arange(B, dtype=np.int64) % 5
  make = lambda cal_of: BatchedEnvironment(plan, B, calendars=cc.calendars(), calendar_of=cal_of, collect_info=True,
                                           start_offsets=offsets, **EPISODE)
  env = make(CALENDAR_OF)
  fp = env.sim.state_fingerprint()
  assert fp[-1][0] == "calendars" and len(fp[-1]) == 3 and fp[-2][0] == "clock"
  env.reset()
  for t in range(4):
    env.step(acts[t])
  snap = env.snapshot()
  first = [_outputs(env, env.step(acts[t])) for t in range(4, 9)]
  env.restore(snap)
  again = [_outputs(env, env.step(acts[t])) for t in range(4, 9)]
  for t, (a, f) in enumerate(zip(again, first)):
    for name in f:
      assert torch.equal(a[name], f[name]), (t, name)
  # through the state_dict too (another process would load it like this)
  env.restore(type(snap).from_state_dict(snap.state_dict(), "cuda"))
  assert torch.equal(env.step(acts[4]).observation, first[0]["observation"])
  other = make(CALENDAR_OF[::-1].copy())
  other.reset()
  with pytest.raises(ValueError, match="another floor plan, configuration"):
    other.restore(snap)
  other.close()
  env.close()
  plain = BatchedEnvironment(plan, B, collect_info=True, start_offsets=offsets, **EPISODE)
  assert not any(isinstance(f, tuple) and f and f[0] == "calendars" for f in plain.sim.state_fingerprint())
  plain.close()


def test_attach_groups_validates_before_anything_changes():
  need_gpu()
  n = 6
  sim = BatchedSimulator(plan_from_npz(load("plan_small_test.npz")), SimConfig.sb1(), n, 12.0)
  L = _ffi.load()
  attach = _ffi.occupancy_entry("sb_occupancy_attach_groups")
  cfg = lambda z, hours, seed=7, first=0, step=300.0: _ffi.OccupancyConfig(z, *hours, step, seed, first)
  good = (_ffi.OccupancyConfig * 2)(cfg(3, (6, 9, 15, 18)), cfg(32, (5, 8, 14, 19)))
  group_of = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
  ptr = lambda a: a.ctypes.data_as(C.c_void_p)
  count, total = torch.zeros((n, sim.Z), device="cuda"), torch.zeros(n, device="cuda")
  g0, g1 = torch.as_tensor(group_of == 0, device="cuda"), torch.as_tensor(group_of == 1, device="cuda")

  def peeks():
    """Re-attaches the good groups, asks eight times inside both arrival windows; -> the counts."""
    assert attach(sim._h, good, 2, ptr(group_of)) == 0
    for _ in range(8):
      sim.occupancy_peek(7, True, count, total)
    return count.clone()

  want = peeks()
  assert float(want[g0].max()) <= 3 < float(want[g1].max())
  assert attach(sim._h, good, 2, ptr(group_of)) == 0   # the attachment every refused call below must leave alone
  for _ in range(3):
    sim.occupancy_peek(7, True, count, total)
  after3 = count.clone()

  def refused(rc, *needles):
    assert rc == -1   # SB_ERR_INVALID
    msg = L.sb_last_error()
    assert msg.startswith(b"sb_occupancy_attach_groups") and all(s in msg for s in needles), msg

  refused(attach(sim._h, None, 2, ptr(group_of)), b"null")
  refused(attach(sim._h, good, 2, None), b"null")
  refused(attach(None, good, 2, ptr(group_of)), b"null")
  refused(attach(sim._h, good, 0, ptr(group_of)), b"n_groups must be 1..65535")
  refused(attach(sim._h, good, 65536, ptr(group_of)), b"n_groups must be 1..65535")
  bad_index = group_of.copy(); bad_index[4] = 2
  refused(attach(sim._h, good, 2, ptr(bad_index)), b"building 4", b"group 2 is outside 0..1")
  bad_index[4] = -1
  refused(attach(sim._h, good, 2, ptr(bad_index)), b"building 4", b"group -1")
  refused(attach(sim._h, (_ffi.OccupancyConfig * 2)(cfg(3, (6, 9, 15, 18)), cfg(32, (5, 8, 8, 19))), 2, ptr(group_of)),
          b"group 1", b"hours must be strictly increasing")
  refused(attach(sim._h, (_ffi.OccupancyConfig * 2)(cfg(3, (6, 9, 15, 18)), cfg(33, (5, 8, 14, 19))), 2, ptr(group_of)),
          b"group 1", b"zone_assignment must be 1..32")
  refused(attach(sim._h, (_ffi.OccupancyConfig * 2)(cfg(3, (6, 9, 15, 18)), cfg(32, (5, 8, 14, 19), seed=8)), 2, ptr(group_of)),
          b"group 1", b"seed differs")
  refused(attach(sim._h, (_ffi.OccupancyConfig * 2)(cfg(3, (6, 9, 15, 18)), cfg(32, (5, 8, 14, 19), first=6)), 2, ptr(group_of)),
          b"group 1", b"first_building differs")
  refused(attach(sim._h, (_ffi.OccupancyConfig * 2)(cfg(3, (6, 9, 15, 18)), cfg(32, (5, 8, 14, 19), step=600.0)), 2, ptr(group_of)),
          b"group 1", b"time_step_sec differs")
  with pytest.raises(ValueError, match="group 1: hours must be strictly increasing"):
    sim.occupancy_attach_groups([(3, (6, 9, 15, 18), 300.0, 7, 0), (32, (5, 8, 8, 19), 300.0, 7, 0)], group_of)
  with pytest.raises(ValueError, match=r"group_of must be integers of shape \[6\]"):
    sim.occupancy_attach_groups([(3, (6, 9, 15, 18), 300.0, 7, 0)], group_of[:5])
  # the previous attachment kept working through all of it: its occupants and its query counter went on untouched
  torch.cuda.synchronize()
  assert torch.equal(count, after3)
  for _ in range(5):
    sim.occupancy_peek(7, True, count, total)
  assert torch.equal(count, want)
  # sb_occupancy_attach afterwards returns the handle to one configuration: group 1's for every building
  sim.occupancy_attach(32, (5, 8, 14, 19), 300.0, 7)
  for _ in range(8):
    sim.occupancy_peek(7, True, count, total)
  assert torch.equal(count[g1], want[g1]) and not torch.equal(count[g0], want[g0])
  torch.cuda.synchronize()
  sim.close()


def test_a_state_forked_across_groups_keeps_the_groups_headcount():
  """A fork moves the occupants' state word with the building's state; the slot keeps its group (its configuration is
  the slot's, like its calendar): building 0 (3 occupants per zone) takes building 1's word (32 per zone) and counts
  only its own three."""
  need_gpu()
  n = 6
  sim = BatchedSimulator(plan_from_npz(load("plan_small_test.npz")), SimConfig.sb1(), n, 12.0)
  group_of = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
  sim.occupancy_attach_groups([(3, (6, 9, 15, 18), 300.0, 7, 0), (32, (5, 8, 14, 19), 300.0, 7, 0)], group_of)
  sim.reset()
  count = torch.zeros((n, sim.Z), device="cuda")
  for _ in range(12):
    sim.occupancy_peek(7, True, count, None)
  assert float(count[1].min()) > 3   # more of building 1's occupants are at work than building 0 has
  state = sim.save_state()
  sim.load_state(state, pick=torch.tensor([1, 1, 2, 3, 4, 5], device="cuda"), clock=False)
  sim.occupancy_peek(12, True, count, None)   # noon: between the windows, nobody moves
  assert float(count[0].max()) <= 3 and float(count[1].min()) > 3
  torch.cuda.synchronize()
  sim.close()
