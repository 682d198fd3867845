"""A calendar per building (BatchedEnvironment(start_offsets=...)), the parts that need no GPU: the Timeline's rows against
the shared-clock path's own step inputs, the choice of rows through two episodes, the refusals, the C entries' null checks."""
import ctypes as C
import datetime as dt
import os
import types

import numpy as np
import pytest

from sbsim_amd import _ffi, host_inputs
from sbsim_amd.environment import SimConfig

UTC = dt.timezone.utc
DT = dt.timedelta(seconds=300)
F = {name: i for i, name in enumerate(host_inputs.CLOCK_FIELDS)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _models(weather=None, occupancy=None, occ_norm=0.0):
  cfg = SimConfig.sb1()   # the default SB1 configuration: US/Pacific schedule, 300 s steps
  assert cfg.time_step_sec == 300.0
  return host_inputs.StepModels(
      weather or host_inputs.WeatherController(273.0, 283.0, convection_coefficient=100.0), cfg.schedule(),
      occupancy or host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1),
      host_inputs.ElectricityEnergyCost(), host_inputs.NaturalGasEnergyCost(), DT, ("room_1", "room_2"), occ_norm)


def _device_occupancy():
  return host_inputs.BatchedRandomizedArrivalDepartureOccupancy(4, 7, 10, 15, 19, 300, seed=5, time_zone="US/Pacific")


def _changes(rows, field):
  return int(np.count_nonzero(np.diff(rows[:, F[field]])))


def _check_rows_against_shared_clock(m, start, n_steps, offsets=(0,)):
  """Row r against what make_step_in computes (host_inputs.step_inputs) for a step at t_r on the shared-clock path: its
  "now" half from row r, its "next" half from row r + 1, comfort_prev from row r - 1; and the reset observation's
  features (_aux at t_r) from row r."""
  tl = host_inputs.Timeline(m, start, list(offsets), n_steps)
  assert tl.rows.shape == (n_steps + 2, len(host_inputs.CLOCK_FIELDS)) and tl.rows.dtype == np.float64
  for r in range(tl.n_rows - 1):
    t = start + r * DT
    d = host_inputs.step_inputs(m, t, None if r == 0 else t - DT)
    now, nxt = tl.rows[r], tl.rows[r + 1]
    assert (now[F["t_amb"]], now[F["weather_f"]], now[F["weather_t"]]) == (d["t_amb_now"], d["weather_f_now"], d["weather_t_now"]), r
    assert (nxt[F["t_amb"]], nxt[F["weather_f"]], nxt[F["weather_t"]]) == (d["t_amb_next"], d["weather_f_next"], d["weather_t_next"]), r
    assert now[F["comfort"]] == d["comfort_now"] and nxt[F["comfort"]] == d["comfort_next"], r
    if r:
      assert tl.rows[r - 1, F["comfort"]] == d["comfort_prev"], r
    for i, v in enumerate(d["aux"]):   # float32 values, stored as the doubles of the same value
      assert nxt[F["aux0"] + i] == float(v) and np.float32(nxt[F["aux0"] + i]) == v, (r, i)
    for i, v in enumerate(host_inputs.aux_features(m, t)):
      assert now[F["aux0"] + i] == float(v), (r, i)
    assert nxt[F["occupancy"]] == d["occupancy"], r
    assert tuple(nxt[F["e_price"]:F["g_carbon"] + 1]) == (d["e_price"], d["e_carbon"], d["g_price"], d["g_carbon"]), r
    # ... and against the host classes asked directly
    assert now[F["comfort"]] == m.schedule.is_comfort_mode(t) and now[F["aux5"]] == m.schedule.is_comfort_mode(t + dt.timedelta(minutes=60))
    utc = host_inputs.reward_start_time_utc(t)
    assert tuple(now[F["e_price"]:F["g_carbon"] + 1]) == m.electricity.rates(utc) + m.gas.rates(utc)
    assert (now[F["occ_hour"]], now[F["occ_workday"]]) == host_inputs.occupancy_clock(m.occupancy, t)
    assert (now[F["occ_hour5"]], now[F["occ_workday5"]]) == host_inputs.occupancy_clock(m.occupancy, t - dt.timedelta(minutes=5))
  return tl


def test_rows_equal_the_shared_clock_inputs_across_a_month_end():
  start = dt.datetime(2023, 9, 1, tzinfo=UTC) - 300 * DT   # Wednesday 30 August, 16:00 in US/Pacific
  tl = _check_rows_against_shared_clock(_models(), start, 864)
  for field in ("comfort", "e_price", "g_price", "occupancy"):   # the range means something: each of them changes in it
    assert _changes(tl.rows, field) >= 1, field
  assert tl.rows[300, F["g_price"]] != tl.rows[299, F["g_price"]]   # the month's gas price, at midnight UTC
  occ = _check_rows_against_shared_clock(_models(occupancy=_device_occupancy(), occ_norm=3.0), start, 864)
  assert _changes(occ.rows, "occ_workday") >= 1 and _changes(occ.rows, "occ_hour") >= 24
  assert (occ.rows[:, F["occupancy"]] == 0.0).all()   # the device generator's buildings have their own


def test_rows_equal_the_shared_clock_inputs_across_a_daylight_saving_change():
  # US/Pacific leaves daylight saving on Sunday 5 November 2023, 09:00 UTC: the local hour 01 comes twice
  start = dt.datetime(2023, 11, 5, 6, 0, tzinfo=UTC)
  tl = _check_rows_against_shared_clock(_models(occupancy=_device_occupancy()), start, 100)
  hours = tl.rows[:, F["occ_hour"]]
  assert list(hours[::12][:6]) == [23.0, 0.0, 1.0, 1.0, 2.0, 3.0]
  start = dt.datetime(2024, 3, 8, 8, 0, tzinfo=UTC)   # ... and enters it on Sunday 10 March 2024: a Friday-to-Monday range
  tl = _check_rows_against_shared_clock(_models(), start, 864)
  assert _changes(tl.rows, "comfort") >= 2


def test_rows_of_the_per_building_weather_forms():
  start = dt.datetime(2023, 7, 6, 7, 0)   # the default, naive start
  sin = host_inputs.BatchedSinusoidWeather([270.0, 275.0], [280.0, 291.0])
  tl = _check_rows_against_shared_clock(_models(weather=sin), start, 40)
  assert _changes(tl.rows, "weather_f") == tl.n_rows - 1 and (tl.rows[:, F["t_amb"]] == 0.0).all()
  csv = os.path.join(GOLDEN, "local_weather_test_data.csv")
  rep = host_inputs.BatchedReplayWeather(csv, [0.0, 1800.0])
  t0 = dt.datetime.fromtimestamp(float(rep.times.min()), tz=UTC) + dt.timedelta(hours=1)
  tl = _check_rows_against_shared_clock(_models(weather=rep), t0, 40, offsets=(0, 0))
  assert (np.diff(tl.rows[:, F["weather_t"]]) == 300.0).all()


def test_row_selection_through_two_episodes():
  offsets = np.array([0, 1, 13, 287, 288, 7400])
  n = 6   # transitions per episode; the terminal step is a step too
  cur = host_inputs.ClockCursor()
  seen_none = 0
  for episode in range(2):
    cur.reset()
    assert cur.pos == 0
    for s in range(n + 1):
      rows = cur.rows(offsets)
      assert (rows["now"] == offsets + s).all() and (rows["next"] == offsets + s + 1).all()
      if episode == 0 and s == 0:   # "none" only before the first step ever
        assert rows["prev"] is None and cur.seek_args() == (0, -1)
        seen_none += 1
      elif s == 0:                  # after a reset: the last stepped instant, the terminal step of the episode before
        assert (rows["prev"] == offsets + n).all() and cur.seek_args() == (0, n)
      else:
        assert (rows["prev"] == offsets + s - 1).all() and cur.seek_args() == (s, s - 1)
      assert rows["next"].max() <= int(offsets.max()) + n + 1   # inside Timeline(..., steps_per_episode=n)'s rows
      cur.advance()
  assert seen_none == 1
  tl = host_inputs.Timeline(_models(), dt.datetime(2023, 7, 6, 7, 0), [0, 3], n)
  assert tl.n_rows == 3 + n + 2 and tl.instant(3) == dt.datetime(2023, 7, 6, 7, 15)


def test_refusals_name_the_building_or_the_argument():
  with pytest.raises(ValueError, match=r"start_offsets must have shape \[4\]"):
    host_inputs.check_start_offsets([0, 1, 2], 4)
  with pytest.raises(ValueError, match=r"start_offsets must have shape \[4\]"):
    host_inputs.check_start_offsets(np.zeros((4, 1), np.int64), 4)
  with pytest.raises(ValueError, match="start_offsets must be integers"):
    host_inputs.check_start_offsets([0.0, 1.5, 2.0, 3.0], 4)
  with pytest.raises(ValueError, match="start_offsets must be integers"):
    host_inputs.check_start_offsets([True, False, True, False], 4)
  with pytest.raises(ValueError, match="building 2: negative offset -7"):
    host_inputs.check_start_offsets([0, 1, -7, 3], 4)
  assert host_inputs.check_start_offsets([0, 5, 2, 3], 4).dtype == np.int32
  start = dt.datetime(2023, 7, 6, 7, 0)
  shared = host_inputs.RandomizedArrivalDepartureOccupancy(4, 7, 10, 15, 19, 300)
  with pytest.raises(ValueError, match="RandomizedArrivalDepartureOccupancy.*BatchedRandomizedArrivalDepartureOccupancy"):
    host_inputs.Timeline(_models(occupancy=shared), start, [0, 1], 10)
  csv = os.path.join(GOLDEN, "local_weather_test_data.csv")
  rep = host_inputs.BatchedReplayWeather(csv, [0.0, 0.0, 0.0])
  steps = int((rep.times.max() - rep.times.min()) / 300.0) - 20
  t0 = dt.datetime.fromtimestamp(float(rep.times.min()), tz=UTC)
  host_inputs.Timeline(_models(weather=rep), t0, [0, 5, 0], 10)   # (covered: no complaint)
  with pytest.raises(ValueError, match="building 1: its episode ends at .* after the weather trace's last time stamp"):
    host_inputs.Timeline(_models(weather=rep), t0, [0, 30, 0], steps)
  late = host_inputs.BatchedReplayWeather(csv, [0.0, 0.0, 7200.0])   # the building's own replay offset counts too
  with pytest.raises(ValueError, match="building 2: its episode ends at"):
    host_inputs.Timeline(_models(weather=late), t0, [0, 0, 0], steps)
  from sbsim_amd.episode_writer import BuildingLogger
  env = types.SimpleNamespace(start_offsets=np.zeros(2, np.int32), info=None)
  with pytest.raises(ValueError, match="start_offsets"):
    BuildingLogger(env, "unused", buildings=[0])


def test_entries_refuse_a_null_handle_and_the_binding_knows_them():
  L = _ffi.load()
  rows = np.zeros((4, _ffi.SB_CLOCK_FIELDS))
  offs = np.zeros(1, np.int32)
  assert _ffi.clock_entry("sb_clock_attach")(None, rows.ctypes.data_as(C.c_void_p), 4, _ffi.SB_CLOCK_FIELDS,
                                             offs.ctypes.data_as(C.c_void_p)) == -1
  assert b"null" in L.sb_last_error()
  assert _ffi.clock_entry("sb_clock_seek")(None, 0, -1) == -1
  assert _ffi.clock_entry("sb_clock_detach")(None) == -1
  assert _ffi.clock_entry("sb_observe_step_in")(None, None, None, None) == -1
  assert _ffi.CLOCK_FIELDS == host_inputs.CLOCK_FIELDS and _ffi.SB_CLOCK_FIELDS == 20
  header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "sbsim_amd.h")).read()
  assert "#define SB_ABI_VERSION 8" in header and "SB_CLOCK_FIELDS" in header


def test_no_offsets_builds_no_timeline(monkeypatch):
  """start_offsets=None takes the path it always took: BatchedEnvironment builds a Timeline (and a cursor, and attaches a
  clock) only inside ``if start_offsets is not None``."""
  import inspect
  from sbsim_amd import environment
  src = inspect.getsource(environment.BatchedEnvironment.__init__)
  assert src.count("host_inputs.Timeline(") == 1
  guard = src.index("if start_offsets is not None:")
  assert guard < src.index("host_inputs.Timeline(") < src.index("self._action_spec")
  assert inspect.signature(environment.BatchedEnvironment.__init__).parameters["start_offsets"].default is None
  # the shared-clock step inputs do not touch the Timeline either
  monkeypatch.setattr(host_inputs, "Timeline", None)
  d = host_inputs.step_inputs(_models(), dt.datetime(2023, 7, 6, 7, 0))
  assert d["comfort_prev"] == -1 and len(d["aux"]) == _ffi.SB_NUM_AUX
