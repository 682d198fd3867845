"""Several calendars in one batch, host side (no GPU): ``host_inputs.Calendar`` / ``CalendarTimeline`` build, for every
building, exactly the rows its own calendar's models give at its own instants; one default calendar is ``Timeline``; and
every refusal fires before anything is created, naming the building, calendar or group."""
import datetime as dt
import os
import re

import numpy as np
import pytest

from sbsim_amd import _ffi, host_inputs
from sbsim_amd.environment import BatchedEnvironment, MixedBatchedEnvironment, SimConfig
from sbsim_amd.host_inputs import Calendar, CalendarTimeline
from tests import calendar_cases as cc
from tests.golden_util import GOLDEN, load
from tests.twins import plan_from_npz

UTC, DT = cc.UTC, cc.DT
STEPS = 30
B = 12
CALENDAR_OF = np.arange(B) % 3                                            # interleaved
START_OFFSETS = np.array([0, 5, 17, 3, 0, 2, 9, 40, 1, 6, 11, 4])          # calendar 1's largest: 40 (building 7)
CSV = os.path.join(GOLDEN, "local_weather_test_data.csv")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timeline(**kw):
  args = dict(calendars=cc.calendars(), calendar_of=CALENDAR_OF, models=cc.base_models(),
              start_timestamp=dt.datetime(2023, 3, 1, tzinfo=UTC), start_offsets=START_OFFSETS, steps_per_episode=STEPS)
  args.update(kw)
  return CalendarTimeline(**args)


def test_every_building_reads_its_own_calendars_rows_at_its_own_instants():
  tl = _timeline()
  assert len({s.month for s in cc.STARTS}) == 3 and len({z for _, _, z in cc.SCHEDULES}) == 3
  assert tl.rows.shape == (tl.n_rows, len(host_inputs.CLOCK_FIELDS)) and tl.offsets.dtype == np.int32
  sizes = [int(START_OFFSETS[CALENDAR_OF == k].max()) + STEPS + 2 for k in range(3)]
  assert tl.base.tolist() == [0, sizes[0], sizes[0] + sizes[1]] and tl.n_rows == sum(sizes)
  assert np.array_equal(tl.offsets, tl.base[CALENDAR_OF] + START_OFFSETS)
  for b in range(B):
    k = int(CALENDAR_OF[b])
    models = host_inputs.Calendar(**cc.members(k)).models(cc.base_models())   # fresh objects: not the timeline's own
    for p in range(STEPS + 2):
      ts = cc.STARTS[k] + (int(START_OFFSETS[b]) + p) * DT
      assert tl.instant(b, p) == ts
      want = np.array(host_inputs.instant_row(models, ts), dtype=np.float64)
      assert np.array_equal(tl.rows[tl.offsets[b] + p], want), (b, p)
  # the calendars are not one: the same position of three neighbouring buildings holds three different rows
  assert len({tl.rows[tl.offsets[b]].tobytes() for b in (0, 1, 2)}) == 3
  # ... and every calendar crosses its own comfort switch within 30 steps of its start (buildings 0, 4, 8: offsets 0, 0, 1)
  assert all(cc.crosses_comfort(tl, b, STEPS) for b in (0, 4, 8)) and set(CALENDAR_OF[[0, 4, 8]]) == {0, 1, 2}


def test_one_default_calendar_is_timeline():
  start = dt.datetime(2023, 7, 6, 7, 0, 0)
  offs = np.array([3, 0, 11, 7, 2], dtype=np.int64)
  want = host_inputs.Timeline(cc.base_models(), start, offs, STEPS)
  got = CalendarTimeline([Calendar()], np.zeros(5, dtype=np.int64), cc.base_models(), start, offs, STEPS)
  assert np.array_equal(got.rows, want.rows) and np.array_equal(got.offsets, want.offsets)
  assert got.offsets.dtype == want.offsets.dtype and got.n_rows == want.n_rows and got.base.tolist() == [0]
  none = CalendarTimeline([Calendar()], np.zeros(5, dtype=np.int64), cc.base_models(), start, None, STEPS)
  assert np.array_equal(none.offsets, np.zeros(5, np.int32)) and none.n_rows == STEPS + 2


def test_the_seek_bound_holds_at_the_last_position():
  """sb_clock_seek refuses ``largest offset + pos > n_rows - 2``: the terminal step at pos = steps reads rows pos and
  pos + 1 of every building, inside its own segment."""
  tl = _timeline()
  assert int(tl.offsets.max()) + STEPS <= tl.n_rows - 2
  ends = np.concatenate([tl.base[1:], [tl.n_rows]])
  for b in range(B):   # no building's last row (the terminal step's "next") lies in the next calendar's segment
    assert tl.offsets[b] + STEPS + 1 < ends[CALENDAR_OF[b]]


def test_calendar_timeline_refusals_name_the_global_building():
  with pytest.raises(ValueError, match="calendar 2 is used by no building"):
    _timeline(calendar_of=np.arange(B) % 2)
  with pytest.raises(ValueError, match=r"building 5: calendar 3 is outside 0 \.\. 2"):
    _timeline(calendar_of=np.where(np.arange(B) == 5, 3, CALENDAR_OF))
  with pytest.raises(ValueError, match=r"calendar_of must have shape \[12\]"):
    _timeline(calendar_of=CALENDAR_OF[:11], start_offsets=START_OFFSETS)
  with pytest.raises(ValueError, match="calendar_of must be integers"):
    _timeline(calendar_of=CALENDAR_OF.astype(np.float64))
  # Timeline's refusals, per calendar: the host-side randomized model ...
  cals = cc.calendars()
  cals[1] = Calendar(occupancy=host_inputs.RandomizedArrivalDepartureOccupancy(3, 7, 9, 16, 18, 300))
  with pytest.raises(ValueError, match=r"calendar 1 \(building 1\): a host-side RandomizedArrivalDepartureOccupancy"):
    _timeline(calendars=cals)
  # ... the 2^22 rows of the concatenated table ...
  far = START_OFFSETS.copy(); far[[0, 1, 2]] = 1 << 21
  with pytest.raises(ValueError, match=r"more than 2\^22 \(reached in calendar 1, whose building 1 "):
    _timeline(start_offsets=far)
  # ... and a replay trace (ten hours from 2023-07-01 00:00 UTC) that ends before building 7 of calendar 1 does
  trace = host_inputs.ReplayWeatherController(CSV, convection_coefficient=cc.H_CONV)
  cals = [Calendar(start_timestamp=dt.datetime(2023, 7, 1, tzinfo=UTC)),
          Calendar(weather=trace, start_timestamp=dt.datetime(2023, 7, 1, 4, 30, tzinfo=UTC)),
          Calendar(start_timestamp=dt.datetime(2023, 7, 1, tzinfo=UTC))]
  with pytest.raises(ValueError, match=r"building 7 \(calendar 1\): its episode ends at .* after the weather trace"):
    _timeline(calendars=cals)
  ok = START_OFFSETS.copy(); ok[7] = 20
  _timeline(calendars=cals, start_offsets=ok)   # 04:30 + (20 + 31) * 5 min = 08:45: inside
  cals[1] = Calendar(weather=trace, start_timestamp=dt.datetime(2023, 6, 30, 23, tzinfo=UTC))
  with pytest.raises(ValueError, match=r"building 4 \(calendar 1\): its episode starts before"):
    _timeline(calendars=cals, start_offsets=ok)


def test_a_calendar_takes_only_a_batch_shared_weather():
  with pytest.raises(ValueError, match="BatchedSinusoidWeather"):
    Calendar(weather=host_inputs.BatchedSinusoidWeather(np.full(B, 270.0), np.full(B, 280.0), cc.H_CONV))
  with pytest.raises(ValueError, match="BatchedReplayWeather"):
    Calendar(weather=host_inputs.BatchedReplayWeather(CSV, np.zeros(B), cc.H_CONV))
  assert Calendar(weather=host_inputs.ReplayWeatherController(CSV)).weather is not None


def _env(**kw):
  """The constructor with calendars: every refusal below comes before a simulator is created, so none needs a GPU."""
  args = dict(calendars=cc.calendars(), calendar_of=CALENDAR_OF,
              weather=host_inputs.WeatherController(273.0, 283.0, convection_coefficient=cc.H_CONV))
  args.update(kw)
  return BatchedEnvironment(plan_from_npz(load("plan_small_test.npz")), B, **args)


def _device_occupancy(k, **kw):
  args = dict(zone_assignment=4, hours=(5 + k, 9 + k, 15, 19), time_step_sec=300, seed=99, first_building=0)
  args.update(kw)
  return host_inputs.BatchedRandomizedArrivalDepartureOccupancy(args["zone_assignment"], *args["hours"], args["time_step_sec"],
                                                                seed=args["seed"], first_building=args["first_building"])


def test_the_environment_refuses_before_anything_is_created():
  with pytest.raises(ValueError, match=r"calendar_of must have shape \[12\]"):
    _env(calendar_of=CALENDAR_OF[:5])
  with pytest.raises(ValueError, match="calendar_of must be integers"):
    _env(calendar_of=CALENDAR_OF.astype(np.float32))
  with pytest.raises(ValueError, match=r"building 11: calendar -1 is outside 0 \.\. 2"):
    _env(calendar_of=np.where(np.arange(B) == 11, -1, CALENDAR_OF))
  with pytest.raises(ValueError, match="calendars needs calendar_of"):
    _env(calendar_of=None)
  with pytest.raises(ValueError, match="calendar_of needs calendars"):
    _env(calendars=None)
  with pytest.raises(ValueError, match="calendar 1 is used by no building"):
    _env(calendar_of=np.where(CALENDAR_OF == 1, 0, CALENDAR_OF))
  # a schedule with windows of its own: those are per-building parameter rows
  cals = cc.calendars()
  cals[2] = Calendar(schedule=host_inputs.SetpointSchedule(7, 20, (293.0, 297.0), cc.ECO))
  with pytest.raises(ValueError, match=r"calendar 2: its schedule's comfort_temp_window .* building_params"):
    _env(calendars=cals)
  cals[2] = Calendar(schedule=host_inputs.SetpointSchedule(7, 20, cc.COMFORT, (288.0, 298.0)))
  with pytest.raises(ValueError, match=r"calendar 2: its schedule's eco_temp_window .* building_params"):
    _env(calendars=cals)
  # a weather with another convection coefficient: the coefficient tables are one per handle
  cals = cc.calendars()
  cals[1] = Calendar(weather=host_inputs.WeatherController(262.0, 270.0, convection_coefficient=12.0))
  with pytest.raises(ValueError, match=r"calendar 1: its weather's convection coefficient 12.0 .* building_materials"):
    _env(calendars=cals)
  # a calendar's weather next to a per-building weather of the environment
  with pytest.raises(ValueError, match="calendar 0 carries a weather, but the environment's BatchedSinusoidWeather"):
    _env(weather=host_inputs.BatchedSinusoidWeather(np.full(B, 270.0), np.full(B, 280.0), cc.H_CONV))
  # device and host occupancy models mixed
  cals = cc.calendars()
  cals[1] = Calendar(occupancy=_device_occupancy(1))
  with pytest.raises(ValueError, match="calendar 0 has a host-side occupancy model .* calendar 1 the device generator"):
    _env(calendars=cals)
  # device models that differ in what a handle has once
  for name, other in (("seed", 100), ("first_building", 12), ("time_step_sec", 600)):
    cals = [Calendar(occupancy=_device_occupancy(k, **({name: other} if k == 2 else {}))) for k in range(3)]
    with pytest.raises(ValueError, match=rf"calendar 2 \(occupancy group 2\): {name} = "):
      _env(calendars=cals)
  with pytest.raises(ValueError, match="per_building_episodes: BatchedRandomizedArrivalDepartureOccupancy is not supported"):
    _env(calendars=[Calendar(occupancy=_device_occupancy(k)) for k in range(3)], per_building_episodes=True)
  with pytest.raises(ValueError, match="building 3: negative offset"):
    _env(start_offsets=np.where(np.arange(B) == 3, -1, 0))
  with pytest.raises(ValueError, match="non-empty list of host_inputs.Calendar"):
    _env(calendars=[cc.members(0)] * 3)


def test_the_mixed_environment_and_the_logger_refuse_calendars():
  plan = plan_from_npz(load("plan_small_test.npz"))
  with pytest.raises(ValueError, match="calendars is not implemented for MixedBatchedEnvironment"):
    MixedBatchedEnvironment([(plan, B)], calendars=cc.calendars(), calendar_of=CALENDAR_OF)
  from sbsim_amd.episode_writer import BuildingLogger

  class _Env:   # (what the logger looks at first)
    calendars, start_offsets, per_building_episodes, info = cc.calendars(), None, False, None
  with pytest.raises(ValueError, match="not for an environment with calendars"):
    BuildingLogger(_Env(), "unused", buildings=[0])


def test_the_new_entry_is_declared_exported_and_bound_when_present():
  text = open(os.path.join(ROOT, "include", "sbsim_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  assert re.search(r"\bint\s+sb_occupancy_attach_groups\s*\(\s*sb_handle\s*\*\s*h\s*,\s*const\s+sb_occupancy_config\s*\*\s*cfgs\s*,"
                   r"\s*int32_t\s+n_groups\s*,\s*const\s+int32_t\s*\*\s*group_of_building_host\s*\)\s*;", text)
  assert "sb_occupancy_attach_groups" in _ffi.EXPORTS and _ffi.OCCUPANCY_ENTRIES == ("sb_occupancy_attach_groups",)
  assert _ffi.SB_ABI_VERSION == 8
  fn = _ffi.occupancy_entry("sb_occupancy_attach_groups")
  assert fn.argtypes[1:3] == [_ffi.C.POINTER(_ffi.OccupancyConfig), _ffi.C.c_int32]
  with pytest.raises(_ffi.SbsimError, match="has no sb_no_such_entry: rebuild it"):
    _ffi.occupancy_entry("sb_no_such_entry")
