"""A calendar per building (BatchedEnvironment(start_offsets=...)) on the GPU.  The oracle is the shared-clock path itself:
building b of an environment with offsets must equal, bit for bit, building b of a plain environment of the same 70
buildings started at ``start + offset[b] * dt`` -- both sides run the same arithmetic on inputs of the same bits.

B = 70 crosses a 64-thread k_post block and several k_pre blocks; building b gets offs[b % 5], the five offsets shuffled
so that neighbouring lanes differ: a gather by the wrong building index hands some building another building's row.
The offsets come from the timeline itself: within 12 steps the five clocks cross a comfort switch, midnight into a weekend,
an hour's electricity-price change and a month's gas-price change (asserted before the GPU is touched).  The replay-weather
case runs on tests/golden/local_weather_test_data.csv, whose trace is ten hours of one Saturday (UTC): its offsets are
chosen inside it, where a comfort switch and the hourly carbon rate's change are there to cross, with 12-step episodes."""
import datetime as dt
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, SimConfig  # noqa: E402
from tests.golden_util import GOLDEN, load  # noqa: E402
from tests.parity import need_gpu  # noqa: E402
from tests.twins import plan_from_npz  # noqa: E402

UTC = dt.timezone.utc
DT = dt.timedelta(seconds=300)
B, T = 70, 12
START = dt.datetime(2023, 9, 1, tzinfo=UTC) - 300 * DT   # Wednesday 30 August 2023, 23:00 UTC
CSV = os.path.join(GOLDEN, "local_weather_test_data.csv")
START_TRACE = dt.datetime(2023, 7, 1, tzinfo=UTC)        # the trace's first time stamp
SHORT = dict(num_days_in_episode=(T + 0.5) * 300.0 / 86400.0)   # episodes of T transitions
F = {name: i for i, name in enumerate(host_inputs.CLOCK_FIELDS)}


def _host_rows(start, n):
  cfg = SimConfig.sb1()
  m = host_inputs.StepModels(host_inputs.WeatherController(273.0, 283.0, convection_coefficient=100.0), cfg.schedule(),
                             host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1),
                             host_inputs.ElectricityEnergyCost(), host_inputs.NaturalGasEnergyCost(), DT, ("z",), 0.0)
  return host_inputs.Timeline(m, start, [0], n).rows


def _first_change(rows, field, also=lambda r: True):
  col = rows[:, F[field]]
  return next(r for r in range(1, len(col)) if col[r] != col[r - 1] and also(r))


def _crosses(rows, off, field):
  """The clock at `off` sees `field` change between two of the rows its T steps read (now: off .. off + T - 1, next: + 1)."""
  return len(set(rows[off:off + T + 1, F[field]])) > 1


def _offsets(seed=7):
  """Five offsets from the timeline (see the module docstring), shuffled; asserts what they cross."""
  rows = _host_rows(START, 800)
  comfort = _first_change(rows, "comfort") - 6
  weekend = _first_change(rows, "aux3", lambda r: (START + r * DT).weekday() == 5 and (START + r * DT).hour == 0) - 6
  price = _first_change(rows, "e_price") - 6
  gas = _first_change(rows, "g_price") - 6
  assert _crosses(rows, comfort, "comfort") and _crosses(rows, price, "e_price") and _crosses(rows, gas, "g_price")
  assert _crosses(rows, weekend, "aux2") and _crosses(rows, weekend, "aux3")   # the day of the week turns: midnight
  assert (START + (weekend + 6) * DT).weekday() == 5                            # ... into a Saturday
  assert (START + (gas + 6) * DT).day == 1                                      # the month's gas price
  offs = np.array([0, comfort, weekend, price, gas], dtype=np.int64)
  assert len(set(offs.tolist())) == 5 and (offs >= 0).all()
  np.random.RandomState(seed).shuffle(offs)
  return offs


def _trace_offsets(seed=7):
  rows = _host_rows(START_TRACE, 110)
  comfort = _first_change(rows, "comfort") - 6
  carbon = _first_change(rows, "e_carbon", lambda r: r > 50) - 6
  assert _crosses(rows, comfort, "comfort") and _crosses(rows, carbon, "e_carbon")
  offs = np.array([0, comfort, carbon, 37, 85], dtype=np.int64)
  assert len(set(offs.tolist())) == 5 and offs.max() + T + 1 < 110
  np.random.RandomState(seed).shuffle(offs)
  return offs


def _outputs(env, ts):
  sim = env.sim
  out = dict(step_type=ts.step_type, observation=ts.observation, reward=ts.reward, discount=ts.discount,
             temps=sim.temps(), zone_temps=sim.zone_temps(), modes=sim.modes(), scalars=sim.scalars())
  if env.info is not None:
    out["info"] = env.info
  return {k: v.clone() for k, v in out.items()}


def _rollout(env, acts, rejected=None):
  """reset(), then one step per row of acts (rejected: {step: flags}); every call's outputs."""
  outs = [_outputs(env, env.reset())]
  for t in range(acts.shape[0]):
    flags = None if rejected is None or t not in rejected else torch.as_tensor(rejected[t], device="cuda")
    outs.append(_outputs(env, env.step(acts[t], flags)))
  return outs


def _assert_rows_equal(got, want, rows, what):
  idx = torch.as_tensor(rows, device="cuda")
  for t, (g, w) in enumerate(zip(got, want)):
    assert g.keys() == w.keys()
    for k in g:
      assert torch.equal(g[k][idx], w[k][idx]), f"{what}: call {t}: {k} differs"


def _actions(n, seed=3):
  return torch.tensor(np.random.RandomState(seed).uniform(-1, 1, size=(n, B, 2)).astype(np.float32), device="cuda")


def _check_against_plain(plan, offs, start, make_kwargs, n_calls=T, rejected=None, acts=None):
  """The clock environment against one plain environment per offset, every output of every call."""
  acts = _actions(n_calls) if acts is None else acts
  per_building = offs[np.arange(B) % 5]
  env = BatchedEnvironment(plan, B, start_timestamp=start, collect_info=True, start_offsets=per_building, **make_kwargs())
  assert env.timeline is not None and env.current_simulation_timestamps()[1] == start + int(per_building[1]) * DT
  got = _rollout(env, acts, rejected)
  env.close()
  for k, off in enumerate(offs):
    plain = BatchedEnvironment(plan, B, start_timestamp=start + int(off) * DT, collect_info=True, **make_kwargs())
    assert plain.timeline is None
    want = _rollout(plain, acts, rejected)
    plain.close()
    _assert_rows_equal(got, want, np.arange(k, B, 5), f"offset {int(off)}")
  return got, per_building


def _case(name):
  """-> (offsets, start, a function that makes the keyword arguments of one environment, the rejected flags)."""
  rs = np.random.RandomState(11)
  offs, start, rejected = _offsets(), START, None
  if name == "shared_weather":
    kw = lambda: dict(weather=host_inputs.WeatherController(268.0, 289.0, convection_coefficient=100.0))
  elif name == "sinusoid_weather":
    lo = rs.uniform(262.0, 280.0, size=B)
    hi = lo + rs.uniform(3.0, 15.0, size=B)
    kw = lambda: dict(weather=host_inputs.BatchedSinusoidWeather(lo, hi, 100.0))
  elif name == "replay_weather":
    offs, start = _trace_offsets(), START_TRACE
    shift = rs.permutation(B) * 20.0   # distinct, up to 1380 s
    kw = lambda: dict(weather=host_inputs.BatchedReplayWeather(CSV, shift, 100.0), **SHORT)
  elif name == "partial_rejection":
    flags = np.arange(B) % 3 == 1   # (a third of the buildings; on the device in _rollout)
    rejected = {t: flags for t in (3, 4, 5)}
    kw = lambda: {}
  elif name == "building_params":
    lo = 292.0 + rs.uniform(0.0, 3.0, size=B)
    bp = host_inputs.BuildingParams({"comfort_temp_window": np.stack([lo, lo + rs.uniform(1.0, 4.0, size=B)], axis=1),
                                     "ahu_fan_efficiency": rs.uniform(0.7, 0.95, size=B)})
    kw = lambda: dict(building_params=bp)
  elif name == "jacobi":
    kw = lambda: dict(solver="jacobi_fp32")
  elif name == "device_occupancy":
    # the hour's price change is at 06:00 UTC: that clock's 12 steps lie in the arrival window 05 .. 08 UTC of a Thursday
    kw = lambda: dict(occupancy=host_inputs.BatchedRandomizedArrivalDepartureOccupancy(
        4, 5, 8, 15, 19, 300, seed=99, time_zone="UTC", first_building=1000), occupancy_normalization_constant=2.0)
  else:
    raise AssertionError(name)
  return offs, start, kw, rejected


@pytest.mark.parametrize("case", ["shared_weather", "sinusoid_weather", "replay_weather", "partial_rejection",
                                  "building_params", "jacobi", "device_occupancy"])
def test_every_building_equals_a_plain_environment_started_at_its_own_time(case):
  offs, start, kw, rejected = _case(case)   # (the crossings are asserted here, on the host)
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  got, per_building = _check_against_plain(plan, offs, start, kw, rejected=rejected)
  # the batch is not one clock: the time features of two neighbouring buildings differ at every call
  env = BatchedEnvironment(plan, B)
  aux = env.field_names.index("hod_cos_000")
  env.close()
  assert all(not torch.equal(g["observation"][0, aux:aux + 4], g["observation"][1, aux:aux + 4]) for g in got)
  if case == "device_occupancy":   # somebody arrived where the clock is inside the arrival window, nobody elsewhere
    price = int(_first_change(_host_rows(START, 800), "e_price") - 6)
    n_occ = got[-1]["observation"][:, aux + 6]
    inside = torch.as_tensor(per_building == price, device="cuda")
    assert (n_occ[inside] != n_occ[~inside][0]).any() and (n_occ[~inside] == n_occ[~inside][0]).all()
  if case == "partial_rejection":
    assert torch.isinf(got[4]["reward"][1]) and not torch.isinf(got[4]["reward"][0]) and not torch.isinf(got[7]["reward"]).any()


def test_offsets_of_zero_equal_an_environment_without_offsets():
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  acts = _actions(T)
  outs = []
  for offsets in (np.zeros(B, np.int64), None):
    env = BatchedEnvironment(plan, B, start_timestamp=START, collect_info=True, start_offsets=offsets)
    assert (env.timeline is None) == (offsets is None)
    fp = env.sim.state_fingerprint()
    assert (isinstance(fp[-1], tuple) and fp[-1][0] == "clock") == (offsets is not None)
    outs.append(_rollout(env, acts) + [_outputs(env, env.reset())])
    env.close()
  assert len(outs[0]) == T + 2
  _assert_rows_equal(outs[0], outs[1], np.arange(B), "offsets 0")


def test_second_episode_starts_from_the_last_stepped_instant():
  """Episodes of 6 transitions: reset, 6 steps, the terminal step, the step that resets, the second episode's first step,
  whose thermostats see the comfort flag of the first episode's LAST instant (Thermostat._previous_timestamp survives
  reset): the clock whose 7 steps end after a comfort switch while its episode starts before it tells the two apart."""
  rows = _host_rows(START, 800)
  switch = _first_change(rows, "comfort")
  offs = np.array([0, switch - 3, switch - 6, switch - 1, switch + 20], dtype=np.int64)
  assert rows[switch - 3, F["comfort"]] != rows[switch - 3 + 6, F["comfort"]]   # first instant vs the terminal step's
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  short = lambda: dict(num_days_in_episode=6.5 * 300.0 / 86400.0)
  got, _ = _check_against_plain(plan, offs, START, short, n_calls=10)
  kinds = [int(g["step_type"][0]) for g in got]
  assert kinds == [0, 1, 1, 1, 1, 1, 1, 2, 0, 1, 1]


def test_snapshot_restore_and_fork_keep_the_slots_offsets():
  need_gpu()
  plan = plan_from_npz(load("plan_small_test.npz"))
  offs = _offsets()
  per_building = offs[np.arange(B) % 5]
  acts = _actions(9)
  env = BatchedEnvironment(plan, B, start_timestamp=START, collect_info=True, start_offsets=per_building)
  env.reset()
  for t in range(4):
    env.step(acts[t])
  snap = env.snapshot()
  first = [_outputs(env, env.step(acts[t])) for t in range(4, 9)]
  env.restore(snap)
  again = [_outputs(env, env.step(acts[t])) for t in range(4, 9)]
  _assert_rows_equal(again, first, np.arange(B), "after restore")
  other = BatchedEnvironment(plan, B, start_timestamp=START, collect_info=True, start_offsets=per_building[::-1].copy())
  other.reset()
  with pytest.raises(ValueError, match="another floor plan, configuration"):   # offsets are part of the fingerprint
    other.restore(snap)
  other.close()
  # a fork moves state, not the calendar: slot 10 takes building 3's state and keeps its own offset
  env.restore(snap)
  src = torch.arange(B, device="cuda")
  src[10] = 3
  assert per_building[10] != per_building[3]
  env.fork(src)
  obs = env.step(acts[4]).observation.clone()
  aux = env.field_names.index("hod_cos_000")
  _assert_rows_equal([dict(aux=obs[:, aux:aux + 6])], [dict(aux=first[0]["observation"][:, aux:aux + 6])], np.arange(B),
                     "time features after fork")
  assert not torch.equal(obs[10, aux:aux + 4], obs[3, aux:aux + 4])
  dev = [i for i, n in enumerate(env.field_names) if n.endswith("zone_air_temperature_sensor")]
  assert torch.equal(obs[10, dev], obs[3, dev])   # ... while the state is building 3's
  env.close()


def test_the_c_entries_validate_before_anything_changes():
  need_gpu()
  import ctypes as C
  from sbsim_amd import _ffi
  from sbsim_amd.environment import BatchedSimulator
  sim = BatchedSimulator(plan_from_npz(load("plan_small_test.npz")), SimConfig.sb1(), 6, 12.0)
  L, NF = _ffi.load(), _ffi.SB_CLOCK_FIELDS
  attach, seek = _ffi.clock_entry("sb_clock_attach"), _ffi.clock_entry("sb_clock_seek")
  rows, offs = np.zeros((10, NF)), np.array([0, 1, 2, 3, 4, 8], np.int32)
  rows[:, 0] = 280.0   # (the ambient temperature)
  ptr = lambda a: a.ctypes.data_as(C.c_void_p)
  assert attach(sim._h, None, 10, NF, ptr(offs)) == -1 and attach(sim._h, ptr(rows), 10, NF, None) == -1
  assert attach(sim._h, ptr(rows), 10, NF - 1, ptr(offs)) == -1 and b"n_fields" in L.sb_last_error()
  assert attach(sim._h, ptr(rows), (1 << 22) + 1, NF, ptr(offs)) == -4   # SB_ERR_TOO_LARGE, before a row is read
  bad = offs.copy(); bad[4] = -1
  assert attach(sim._h, ptr(rows), 10, NF, ptr(bad)) == -1 and b"building 4: negative offset" in L.sb_last_error()
  bad[4] = 9
  assert attach(sim._h, ptr(rows), 10, NF, ptr(bad)) == -1 and b"building 4" in L.sb_last_error()
  nan = rows.copy(); nan[7, 12] = np.inf
  assert attach(sim._h, ptr(nan), 10, NF, ptr(offs)) == -1 and b"row 7: e_price is not finite" in L.sb_last_error()
  assert seek(sim._h, 0, -1) == -1 and b"sb_clock_attach first" in L.sb_last_error()   # nothing was attached so far
  with pytest.raises(ValueError, match="n_fields"):
    sim.clock_attach(np.zeros((10, NF + 1)), offs)
  sim.clock_attach(rows, offs)
  sim.reset()
  obs, rew = torch.zeros((6, sim.O), device="cuda"), torch.zeros(6, device="cuda")
  si = _ffi.StepIn()
  with pytest.raises(_ffi.SbsimError, match="never sought"):
    sim.step(None, si, obs, rew)
  assert seek(sim._h, 1, 9) == -1 and seek(sim._h, -1, -1) == -1 and seek(sim._h, 0, -2) == -1
  with pytest.raises(ValueError, match="runs past the table's 10 rows"):
    sim.clock_seek(1, 0)    # 8 + 1 + 1 > 9
  sim.clock_seek(0, -1)
  sim.step(None, si, obs, rew)   # a thermostat-only step on the rows
  sim.clock_detach()
  sim.step(None, si, obs, rew)   # ... and on sb_step_in's scalars again
  torch.cuda.synchronize()
  sim.close()
