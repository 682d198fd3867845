"""Host-side, per-step inputs of the batched step: weather, schedule, occupancy, tariffs.

These are the pieces SURVEY.md section 8(a) rows a14/a17/a18 marks "host-side; fed as a
per-step scalar": every building of a batch shares the simulator clock, so calendar logic
(time zones, holidays, schedules) runs once per step on the host and reaches the kernel as
a small struct (include/sbsim_amd.h ``sb_step_in``).  Each class mirrors the reference
class of the same name (same constructor arguments, same method names) and cites it.

Timestamps are ``datetime.datetime`` (``pandas.Timestamp`` is accepted: it is a subclass).
Naive timestamps are interpreted exactly as the reference does: as UTC wall-clock
(``setpoint_schedule.py:100-106``, ``conversion_utils.py:39-49``).
"""
from __future__ import annotations

import copy
import csv
import dataclasses
import datetime as dt
import hashlib
import math
from typing import Dict, Iterable, List, Mapping, NamedTuple, Optional, Sequence, Set, Tuple
from zoneinfo import ZoneInfo

import numpy as np

from . import _ffi

UTC = dt.timezone.utc
_SECONDS_IN_A_DAY = 24 * 3600
_DAYS_IN_A_YEAR = 365
_MIN_RADIANS = -math.pi / 2.0
_MAX_RADIANS = 3.0 * math.pi / 2.0


def as_datetime(ts) -> dt.datetime:
  if hasattr(ts, "to_pydatetime"):
    return ts.to_pydatetime()
  return ts


def _tz(time_zone) -> dt.tzinfo:
  if isinstance(time_zone, dt.tzinfo):
    return time_zone
  if time_zone in ("UTC", None):
    return UTC
  return ZoneInfo(str(time_zone))


def epoch_seconds(ts: dt.datetime) -> float:
  """pandas ``Timestamp.timestamp()``: naive values are taken as UTC."""
  ts = as_datetime(ts)
  if ts.tzinfo is None:
    ts = ts.replace(tzinfo=UTC)
  return ts.timestamp()


def seconds_since_midnight(ts: dt.datetime) -> float:
  return ts.hour * 3600 + ts.minute * 60 + ts.second + ts.microsecond * 1e-6


# --------------------------------------------------------------------------- weather
class WeatherController:
  """Sinusoid: low at midnight, high at noon (simulator/weather_controller.py:47-132)."""

  def __init__(self, default_low_temp: float, default_high_temp: float,
               special_days: Optional[Mapping[int, Tuple[float, float]]] = None,
               convection_coefficient: float = 12.0):
    if default_low_temp > default_high_temp:
      raise ValueError("default_low_temp cannot be greater than default_high_temp.")
    self.default_low_temp = default_low_temp
    self.default_high_temp = default_high_temp
    self.special_days = dict(special_days) if special_days else {}
    self.convection_coefficient = convection_coefficient
    for day, (low, high) in self.special_days.items():
      if low > high:
        raise ValueError(f"Low temp cannot be greater than high temp for special day: {day}.")

  def seconds_to_rads(self, seconds_in_day: float) -> float:
    return (seconds_in_day / _SECONDS_IN_A_DAY) * (_MAX_RADIANS - _MIN_RADIANS) + _MIN_RADIANS

  def get_current_temp(self, timestamp) -> float:
    ts = as_datetime(timestamp)
    today = ts.timetuple().tm_yday
    tomorrow = (today + 1) % _DAYS_IN_A_YEAR
    today_low, today_high = self.special_days.get(
        today, (self.default_low_temp, self.default_high_temp))
    tomorrow_low = self.special_days.get(tomorrow, (self.default_low_temp, None))[0]
    high = today_high
    low = today_low if ts.hour < 12 else tomorrow_low
    rad = self.seconds_to_rads(seconds_since_midnight(ts))
    return 0.5 * (math.sin(rad) + 1) * (high - low) + low

  def get_air_convection_coefficient(self, timestamp) -> float:
    return self.convection_coefficient


class BatchedSinusoidWeather:
  """One sinusoid WeatherController per building (per-building low / high bounds): the same
  formula as ``WeatherController.get_current_temp`` (weather_controller.py:93-123),
  ``T_b = 0.5*(sin(rad)+1) * (high_b - low_b) + low_b``.  The time-only factor is computed on
  the host, the per-building temperatures on the device (sb_step_in.weather_lohi_dev), so no
  per-building host work is left in a step.  Special days are not modelled."""

  def __init__(self, low_temps, high_temps, convection_coefficient: float = 12.0):
    import numpy as np
    self.low = np.ascontiguousarray(low_temps, dtype=np.float64)
    self.high = np.ascontiguousarray(high_temps, dtype=np.float64)
    if self.low.shape != self.high.shape or self.low.ndim != 1:
      raise ValueError("low_temps and high_temps must be 1-D arrays of the same length")
    if (self.low > self.high).any():
      raise ValueError("default_low_temp cannot be greater than default_high_temp.")
    self.convection_coefficient = convection_coefficient
    self._one = WeatherController(0.0, 1.0)

  def factor(self, timestamp) -> float:
    """0.5*(sin(rad(t))+1): what a (low=0, high=1) controller returns."""
    return self._one.get_current_temp(timestamp)

  def temps(self, timestamp):
    """[B] float64 ambient temperatures, bit-identical to B separate WeatherControllers."""
    f = self.factor(timestamp)
    return f * (self.high - self.low) + self.low

  def get_air_convection_coefficient(self, timestamp) -> float:
    return self.convection_coefficient


def _parse_weather_time(text: str) -> dt.datetime:
  """``pd.Timestamp(t, tz='UTC')`` on the CSV's ``Time`` column (weather_controller.py:183-185): the
  sbsim weather files write ``YYYYMMDD-HHMM`` (UTC); ISO strings are accepted as well."""
  text = text.strip()
  try:
    t = dt.datetime.strptime(text, "%Y%m%d-%H%M")
  except ValueError:
    t = dt.datetime.fromisoformat(text.replace("Z", "+00:00").replace(" UTC", "+00:00"))
  return t.replace(tzinfo=UTC) if t.tzinfo is None else t


class ReplayWeatherController:
  """Linear interpolation of an hourly ``Time,TempF`` CSV
  (simulator/weather_controller.py:166-218)."""

  def __init__(self, local_weather_path: str, convection_coefficient: float = 12.0):
    times, temps = [], []
    with open(local_weather_path, newline="") as fh:
      for row in csv.DictReader(fh):
        t = _parse_weather_time(row["Time"])
        times.append(t.timestamp())
        temps.append(float(row["TempF"]))
    self._times = np.asarray(times, dtype=np.float64)
    self._temps = np.asarray(temps, dtype=np.float64)
    self.convection_coefficient = convection_coefficient

  def get_current_temp(self, timestamp) -> float:
    ts = as_datetime(timestamp)
    if ts.tzinfo is None:
      raise TypeError("ReplayWeatherController needs a tz-aware timestamp (reference: tz_convert)")
    target = ts.timestamp()
    if target < self._times.min():
      raise ValueError(f"Attempting to get weather data at {ts}, before the latest timestamp.")
    if target > self._times.max():
      raise ValueError(f"Attempting to get weather data at {ts}, after the latest timestamp.")
    temp_f = float(np.interp(target, self._times, self._temps))
    return (temp_f - 32.0) * 5.0 / 9.0 + 273.15   # conversion_utils.py:155-171

  def get_air_convection_coefficient(self, timestamp) -> float:
    return self.convection_coefficient


class BatchedReplayWeather(ReplayWeatherController):
  """One ``ReplayWeatherController`` per building over the same CSV, building b reading the trace
  ``offsets_sec[b]`` seconds ahead (per-building weather diversity).  The
  interpolation runs on the device (``sb_step_in.weather_times_dev``): np.interp's arithmetic and
  the reference's Fahrenheit -> kelvin conversion, bit-identical to ``temps()`` below."""

  def __init__(self, local_weather_path: str, offsets_sec, convection_coefficient: float = 12.0):
    super().__init__(local_weather_path, convection_coefficient)
    self.offsets_sec = np.ascontiguousarray(offsets_sec, dtype=np.float64)
    if self.offsets_sec.ndim != 1:
      raise ValueError("offsets_sec must be one offset per building")

  @property
  def times(self) -> np.ndarray:
    return self._times

  @property
  def temps_f(self) -> np.ndarray:
    return self._temps

  def query_time(self, timestamp) -> float:
    ts = as_datetime(timestamp)
    if ts.tzinfo is None:
      raise TypeError("ReplayWeatherController needs a tz-aware timestamp (reference: tz_convert)")
    target = ts.timestamp()
    lo, hi = target + self.offsets_sec.min(), target + self.offsets_sec.max()
    if lo < self._times.min():   # weather_controller.py:196-205, for every building
      raise ValueError(f"Attempting to get weather data at {ts}, before the latest timestamp.")
    if hi > self._times.max():
      raise ValueError(f"Attempting to get weather data at {ts}, after the latest timestamp.")
    return target

  def temps(self, timestamp) -> np.ndarray:
    """[B] ambient temperatures, K."""
    x = self.query_time(timestamp) + self.offsets_sec
    temp_f = np.array([np.interp(v, self._times, self._temps) for v in x])   # scalar calls: arr_interp's scalar path
    return (temp_f - 32.0) * 5.0 / 9.0 + 273.15

  def get_current_temp(self, timestamp) -> float:
    raise TypeError("per-building weather: use temps() / BatchedEnvironment")


# --------------------------------------------------------------------------- schedule
class SetpointSchedule:
  """Day (comfort) / night (eco) temperature windows (simulator/setpoint_schedule.py:29-128)."""

  def __init__(self, morning_start_hour: int, evening_start_hour: int,
               comfort_temp_window: Tuple[float, float], eco_temp_window: Tuple[float, float],
               holidays: Optional[Set[int]] = None, time_zone="UTC"):
    if morning_start_hour > evening_start_hour:
      raise ValueError("morning_start_hour must be less than evening_start_hour")
    if comfort_temp_window[0] > comfort_temp_window[1]:
      raise ValueError("comfort_temp_window[0] must be less than comfort_temp_window[1]")
    if eco_temp_window[0] > eco_temp_window[1]:
      raise ValueError("eco_temp_window[0] must be less than eco_temp_window[1]")
    self.morning_start_hour = morning_start_hour
    self.evening_start_hour = evening_start_hour
    self.comfort_temp_window = comfort_temp_window
    self.eco_temp_window = eco_temp_window
    self._time_zone = _tz(time_zone)
    self.holidays = set(holidays) if holidays else set()

  def _localize_or_convert_timezone(self, ts: dt.datetime) -> dt.datetime:
    ts = as_datetime(ts)
    if ts.tzinfo is not None:
      return ts.astimezone(self._time_zone)
    return ts.replace(tzinfo=UTC)   # naive -> localized as UTC, NOT converted (:100-106)

  def is_weekend(self, ts) -> bool:
    return self._localize_or_convert_timezone(ts).weekday() >= 5

  def is_comfort_mode(self, ts) -> bool:
    local = self._localize_or_convert_timezone(ts)
    return (self.morning_start_hour <= local.hour < self.evening_start_hour
            and local.timetuple().tm_yday not in self.holidays
            and local.weekday() < 5)

  def get_temperature_window(self, ts) -> Tuple[float, float]:
    return self.comfort_temp_window if self.is_comfort_mode(ts) else self.eco_temp_window


# --------------------------------------------------------------------------- work days
def _nth_weekday(year: int, month: int, weekday: int, n: int) -> dt.date:
  d = dt.date(year, month, 1)
  d += dt.timedelta(days=(weekday - d.weekday()) % 7 + 7 * (n - 1))
  return d


def _last_weekday(year: int, month: int, weekday: int) -> dt.date:
  d = dt.date(year + (month == 12), month % 12 + 1, 1) - dt.timedelta(days=1)
  return d - dt.timedelta(days=(d.weekday() - weekday) % 7)


def us_federal_holidays(year: int) -> Set[dt.date]:
  """The default ``holidays.US()`` calendar the reference consults
  (utils/conversion_utils.py:62-70): federal holidays with Friday/Monday observance."""
  days = [dt.date(year, 1, 1), _nth_weekday(year, 1, 0, 3), _nth_weekday(year, 2, 0, 3),
          _last_weekday(year, 5, 0), dt.date(year, 7, 4), _nth_weekday(year, 9, 0, 1),
          _nth_weekday(year, 10, 0, 2), dt.date(year, 11, 11), _nth_weekday(year, 11, 3, 4),
          dt.date(year, 12, 25)]
  if year >= 2021:
    days.append(dt.date(year, 6, 19))
  out = set(days)
  for d in days:
    if d.weekday() == 5:
      out.add(d - dt.timedelta(days=1))
    elif d.weekday() == 6:
      out.add(d + dt.timedelta(days=1))
  if dt.date(year + 1, 1, 1).weekday() == 5:   # next New Year's Day observed on Dec 31
    out.add(dt.date(year, 12, 31))
  return out


_HOLIDAY_CACHE: Dict[int, Set[dt.date]] = {}


def is_work_day(ts, holiday_calendar: Optional[Iterable[dt.date]] = "us") -> bool:
  """conversion_utils.py:67-70: weekday < 5 and the date is not a US holiday.
  ``holiday_calendar=None`` disables the holiday test (what the golden harness ran with,
  because the ``holidays`` package is not installed here)."""
  ts = as_datetime(ts)
  if ts.weekday() >= 5:
    return False
  if holiday_calendar is None:
    return True
  if holiday_calendar == "us":
    cal = _HOLIDAY_CACHE.get(ts.year)
    if cal is None:   # (setdefault would rebuild the year's calendar on every call)
      cal = _HOLIDAY_CACHE[ts.year] = us_federal_holidays(ts.year)
  else:
    cal = holiday_calendar
  return ts.date() not in cal


# --------------------------------------------------------------------------- occupancy
class StepFunctionOccupancy:
  """Constant occupancy inside / outside working hours
  (simulator/step_function_occupancy.py:36-173)."""

  def __init__(self, work_start_time: dt.timedelta, work_end_time: dt.timedelta,
               work_occupancy: float, nonwork_occupancy: float,
               holiday_calendar: Optional[Iterable[dt.date]] = "us"):
    for t in (work_start_time, work_end_time):
      if t > dt.timedelta(hours=24) or t.total_seconds() < 0.0:
        raise ValueError("Time delta must be positive and less than one day.")
    self._work_start_time = work_start_time
    self._work_end_time = work_end_time
    self._work_occupancy = work_occupancy
    self._nonwork_occupancy = nonwork_occupancy
    self._holiday_calendar = holiday_calendar

  def _split_workday(self, start: dt.timedelta, end: dt.timedelta):
    if start > end:
      raise ValueError("Cannot have an end time before start time.")
    before = during = after = 0.0
    current = start
    interval_end = min(end, dt.timedelta(hours=24))
    nxt = min(interval_end, self._work_start_time)
    if current < nxt:
      before = (nxt - current).total_seconds()
      current = max(current, nxt)
    nxt = min(interval_end, self._work_end_time)
    if current < nxt:
      during = (nxt - current).total_seconds()
      current = nxt
    nxt = interval_end
    if current < nxt:
      after = (nxt - current).total_seconds()
    return before, during, after

  def average_zone_occupancy(self, zone_id, start_time, end_time) -> float:
    start_time, end_time = as_datetime(start_time), as_datetime(end_time)
    if start_time >= end_time:
      raise ValueError("End time may not occur before start time.")
    work = nonwork = 0.0
    day = start_time.replace(hour=0, minute=0, second=0, microsecond=0)
    if start_time.tzinfo is not None:
      day = day.replace(tzinfo=None)   # pd.Timestamp(year=, month=, day=) is naive (:88-90)
      start_time, end_time = start_time.replace(tzinfo=None), end_time.replace(tzinfo=None)
    current = start_time - day
    while day <= end_time:
      day_end = min(dt.timedelta(days=1), end_time - day)
      if is_work_day(day, self._holiday_calendar):
        b, d, a = self._split_workday(current, day_end)
        work += d
        nonwork += b + a
      else:
        nonwork += (day_end - current).total_seconds()
      day += dt.timedelta(days=1)
      current = dt.timedelta(0)
    return (work * self._work_occupancy + nonwork * self._nonwork_occupancy) / (work + nonwork)


class RandomizedArrivalDepartureOccupancy:
  """Occupants that arrive and leave at random times of a working day
  (simulator/randomized_arrival_departure_occupancy.py:41-218).  Host mirror: the same
  ``np.random.RandomState(seed)`` stream consumed in the same order, so one instance
  reproduces the reference call for call (tests/golden/occupancy_randomized.npz).  Every
  ``average_zone_occupancy`` call ADVANCES each occupant of the zone (one Bernoulli trial inside
  the arrival / departure window), exactly as in the reference -- the result depends on how
  often it is asked, not only on the time."""

  AWAY, WORK = 1, 2

  def __init__(self, zone_assignment: int, earliest_expected_arrival_hour: int,
               latest_expected_arrival_hour: int, earliest_expected_departure_hour: int,
               latest_expected_departure_hour: int, time_step_sec: int, seed: Optional[int] = 17321,
               time_zone="UTC", holiday_calendar: Optional[Iterable[dt.date]] = "us"):
    assert (earliest_expected_arrival_hour < latest_expected_arrival_hour
            < earliest_expected_departure_hour < latest_expected_departure_hour)   # :68-73
    self.zone_assignment = int(zone_assignment)
    self.hours = (int(earliest_expected_arrival_hour), int(latest_expected_arrival_hour),
                  int(earliest_expected_departure_hour), int(latest_expected_departure_hour))
    self.time_step_sec = float(time_step_sec)
    self.seed = seed
    self.p_arrival = self.event_probability(self.hours[0], self.hours[1], self.time_step_sec)
    self.p_departure = self.event_probability(self.hours[2], self.hours[3], self.time_step_sec)
    self._random_state = np.random.RandomState(seed)
    self._tz = _tz(time_zone)
    self._holiday_calendar = holiday_calendar
    self._zone_occupants: Dict[str, list] = {}

  @staticmethod
  def event_probability(start_hour: int, end_hour: int, time_step_sec: float) -> float:
    """:100-112: geometric distribution whose mean is half the window."""
    n_halfway = (end_hour - start_hour) * 3600.0 / time_step_sec / 2.0
    return 1.0 / n_halfway

  def local(self, ts) -> dt.datetime:
    ts = as_datetime(ts)
    return ts if ts.tzinfo is None else ts.astimezone(self._tz)   # :93-98

  def is_work_day(self, ts) -> bool:
    loc = self.local(ts)
    return is_work_day(dt.datetime(loc.year, loc.month, loc.day), self._holiday_calendar)   # :141-150

  def _peek(self, state: int, ts) -> int:
    """ZoneOccupant.peek (:138-160)."""
    hour = self.local(ts).hour
    e_arr, l_arr, e_dep, _ = self.hours
    if not self.is_work_day(ts):
      return self.AWAY
    if state == self.AWAY:
      if hour < e_arr or hour > l_arr:
        return state
      return self.WORK if self._random_state.rand() < self.p_arrival else state
    if hour < e_dep:
      return state
    return self.AWAY if self._random_state.rand() < self.p_departure else state

  def average_zone_occupancy(self, zone_id, start_time, end_time) -> float:
    """:183-218: the number of occupants at work at ``start_time``."""
    occ = self._zone_occupants.setdefault(zone_id, [self.AWAY] * self.zone_assignment)
    n = 0.0
    for i in range(len(occ)):
      occ[i] = self._peek(occ[i], start_time)
      if occ[i] == self.WORK:
        n += 1.0
    return n


class BatchedRandomizedArrivalDepartureOccupancy(RandomizedArrivalDepartureOccupancy):
  """One independent ``RandomizedArrivalDepartureOccupancy`` per building, generated on the
  device (``sb_occupancy_attach`` / ``sb_occupancy_peek``): the per-occupant state machine is the
  reference's, the Bernoulli trials come from a counter-based generator (Philox4x32-10 keyed by
  seed, counter = global building index, zone, query number), so the streams cannot be those of
  ``np.random.RandomState`` -- statistically equivalent, not bitwise --
  but they do not depend on how the batch is sharded over GPUs.  ``BatchedEnvironment`` asks
  twice per step like the reference's environment: the reward's query, then ``num_occupants``'
  query five minutes earlier.  ``first_building``: global index of the batch's building 0."""

  def __init__(self, *args, first_building: int = 0, **kwargs):
    super().__init__(*args, **kwargs)
    if not 1 <= self.zone_assignment <= 32:
      raise ValueError("the device generator keeps a zone's occupants in one 32-bit word")
    self.first_building = int(first_building)

  def average_zone_occupancy(self, zone_id, start_time, end_time) -> float:
    raise TypeError("per-building occupancy lives on the device; use BatchedEnvironment")


class StochasticConvectionSimulator:
  """Parameters of the reference's StochasticConvectionSimulator(p, distance, seed)
  (simulator/stochastic_convection_simulator.py:35-60; SB1: p = 1, distance = 5,
  sim_config.gin:36-39).  The shuffle itself runs on the device after every FD update
  (``sb_convection_attach``, ``BatchedEnvironment(convection_simulator=...)``): the reference's
  random process with counter-based draws per building -- statistically equivalent to the
  reference (which uses Python's global ``random``), independent of batch sharding."""

  def __init__(self, p: float, distance: int, seed: Optional[int], first_building: int = 0):
    self.p, self.distance, self.seed, self.first_building = float(p), int(distance), seed, int(first_building)


class SeededStochasticConvectionSimulator:
  """StochasticConvectionSimulator(p, distance, seed) with the reference's OWN draws, one seeded generator per building
  (``sb_convection_attach_seeded``, ``BatchedEnvironment(convection_simulator=...)``): building b is the reference
  process that called ``random.seed(seeds[b])`` -- its grid after every step is the reference's, bit for bit
  (``host_convection.SeededHostConvection(p, distance, seeds[b])`` is the host twin).  ``seeds``: an integer s -- building
  b gets s + b, so building 0 is the reference run with seed s -- or an integer array [B].  Seeds are uint64: a
  non-integer dtype, a negative value, a value of 2^64 or more or another shape is a ValueError.  Slower than the
  counter-based ``StochasticConvectionSimulator`` (one serial chain of draws per building); windows of more than 64
  offsets (distance >= 20, or -1 with p < 1) and rooms of more than 2047 cells are refused."""

  def __init__(self, p: float, distance: int, seeds):
    self.p, self.distance = float(p), int(distance)
    if isinstance(seeds, (int, np.integer)) and not isinstance(seeds, (bool, np.bool_)):
      self.seeds = int(seeds)
      self._check_range(self.seeds, self.seeds)
    else:
      if isinstance(seeds, (list, tuple)) and seeds and all(
          isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in seeds):
        self._check_range(min(int(v) for v in seeds), max(int(v) for v in seeds))   # (Python ints beyond int64)
        a = np.array([int(v) for v in seeds], dtype=np.uint64)
      else:
        a = np.asarray(seeds)
      if a.dtype.kind not in "iu":
        raise ValueError(f"seeds must be an integer or an integer array [B], got dtype {a.dtype}")
      if a.ndim != 1 or a.size == 0:
        raise ValueError(f"seeds must be an integer or an integer array [B], got shape {a.shape}")
      self._check_range(int(a.min()), int(a.max()))
      self.seeds = a.astype(np.uint64)

  @staticmethod
  def _check_range(lo: int, hi: int) -> None:
    if lo < 0:
      raise ValueError(f"seeds must not be negative (random.seed takes the absolute value: two buildings would share a "
                       f"stream), got {lo}")
    if hi >= 1 << 64:
      raise ValueError(f"seeds must be below 2^64, got {hi}")

  def seeds_for(self, n_buildings: int) -> np.ndarray:
    """The buildings' seeds, uint64 [n_buildings]; ValueError for an array of another length or s + B - 1 >= 2^64."""
    B = int(n_buildings)
    if isinstance(self.seeds, int):
      self._check_range(self.seeds, self.seeds + B - 1)
      return np.array([self.seeds + b for b in range(B)], dtype=np.uint64)
    if self.seeds.shape != (B,):
      raise ValueError(f"seeds must be an integer or an integer array [{B}], got shape {self.seeds.shape}")
    return self.seeds.copy()


# --------------------------------------------------------------------------- tariffs
# Units: kg carbon / MWh (reward/electricity_energy_cost.py:39-64).
CARBON_EMISSION_BY_HOUR = (
    88.19666493, 87.79190866, 87.87607686, 87.83054163, 88.00279618, 88.19648183,
    89.70663283, 93.97947901, 98.85868291, 100.7853521, 101.3866866, 101.7795612,
    102.5919168, 103.4403736, 104.1380294, 104.7359292, 102.0714466, 97.04226176,
    93.57895651, 92.46355045, 91.72914657, 90.69209747, 89.76552213, 88.99950995)
# cents / kWh (reward/electricity_energy_cost.py:72-123).
WEEKDAY_PRICE_BY_HOUR = (16.0,) * 6 + (18.0,) * 6 + (20.0,) * 7 + (16.0,) * 5
WEEKEND_PRICE_BY_HOUR = (16.0,) * 24
# USD / 1000 ft3, 2020 (reward/natural_gas_energy_cost.py:31-44).
GAS_PRICE_BY_MONTH = (9.02, 8.35, 7.77, 7.26, 6.69, 6.86, 6.77, 6.76, 6.99, 7.19, 7.96, 8.98)
KWH_PER_KFT3_GAS = 293.07107   # utils/constants.py:40
JOULES_PER_KWH = 3.6e6         # utils/constants.py:29
GAS_CO2 = 53.12                # utils/constants.py:44


class ElectricityEnergyCost:
  """reward/electricity_energy_cost.py:125-224, reduced to the two rates the kernel needs."""

  def __init__(self, weekday_energy_prices: Sequence[float] = WEEKDAY_PRICE_BY_HOUR,
               weekend_energy_prices: Sequence[float] = WEEKEND_PRICE_BY_HOUR,
               carbon_emission_rates: Sequence[float] = CARBON_EMISSION_BY_HOUR,
               holiday_calendar: Optional[Iterable[dt.date]] = "us"):
    if len(weekday_energy_prices) != 24 or len(weekend_energy_prices) != 24:
      raise ValueError("Energy cost rates must have 24 entries.")
    if len(carbon_emission_rates) != 24:
      raise ValueError("Carbon emission rates must have 24 entries.")
    self.carbon_emission_rates = np.array(carbon_emission_rates) / 1.0e6 / 3600.0
    self.weekday_energy_prices = np.array(weekday_energy_prices) / 100.0 / 1000.0 / 3600.0
    self.weekend_energy_prices = np.array(weekend_energy_prices) / 100.0 / 1000.0 / 3600.0
    self._holiday_calendar = holiday_calendar

  def rates(self, start_time_utc: dt.datetime) -> Tuple[float, float]:
    """(USD per W per s, kg per W per s) at ``start_time.hour`` (UTC: SURVEY.md 7.8)."""
    hour = start_time_utc.hour
    if is_work_day(start_time_utc, self._holiday_calendar):
      price = self.weekday_energy_prices[hour]
    else:
      price = self.weekend_energy_prices[hour]
    return float(price), float(self.carbon_emission_rates[hour])


class NaturalGasEnergyCost:
  """reward/natural_gas_energy_cost.py:47-138."""

  def __init__(self, gas_price_by_month: Sequence[float] = GAS_PRICE_BY_MONTH):
    assert len(gas_price_by_month) == 12, "Gas price per month must have exactly 12 values."
    self.month_gas_price = np.array(gas_price_by_month) / KWH_PER_KFT3_GAS / JOULES_PER_KWH
    self.carbon_rate = GAS_CO2 / KWH_PER_KFT3_GAS / JOULES_PER_KWH

  def rates(self, start_time_utc: dt.datetime) -> Tuple[float, float]:
    return float(self.month_gas_price[start_time_utc.month - 1]), float(self.carbon_rate)


class SetpointEnergyCarbonReward:
  """reward/setpoint_energy_carbon_reward.py:84-190, SetpointEnergyCarbonRewardFunction: the absolute reward in dollars,
  ``(productivity - energy_cost_weight * (electricity + gas cost) - carbon_cost_weight * carbon_cost -
  reward_normalizer_shift) / reward_normalizer_scale`` with ``carbon_cost = carbon_emitted * carbon_cost_factor``.
  The constructor's productivity arguments (max_productivity_personhour_usd, productivity_midpoint_delta,
  productivity_decay_stiffness) and the energy cost models are the SimConfig's and the environment's, as for the default
  regret function; the regret's own fields (min productivity, the rate caps, the three weights) play no part.

      env = BatchedEnvironment(plan, B, reward_function=SetpointEnergyCarbonReward(1.0, 1.0, 0.2, 250.0, 5000.0))

  The reference constructor checks nothing; the values here must be finite and the scale non-zero (the reward divides
  by it) -- ValueError otherwise."""
  kind = 1   # SB_REWARD_SETPOINT_ENERGY_CARBON

  def __init__(self, energy_cost_weight: float, carbon_cost_weight: float, carbon_cost_factor: float,
               reward_normalizer_shift: float = 0.0, reward_normalizer_scale: float = 1.0):
    vals = dict(energy_cost_weight=energy_cost_weight, carbon_cost_weight=carbon_cost_weight,
                carbon_cost_factor=carbon_cost_factor, reward_normalizer_shift=reward_normalizer_shift,
                reward_normalizer_scale=reward_normalizer_scale)
    for name, v in vals.items():
      if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
      if not np.isfinite(v):
        raise ValueError(f"{name} is not finite")
      setattr(self, name, float(v))
    if self.reward_normalizer_scale == 0.0:
      raise ValueError("reward_normalizer_scale must not be 0 (the reward divides by it)")

  def as_tuple(self) -> Tuple:
    """(kind, the five constants): what a snapshot's fingerprint carries."""
    return (self.kind, self.energy_cost_weight, self.carbon_cost_weight, self.carbon_cost_factor,
            self.reward_normalizer_shift, self.reward_normalizer_scale)

  def __eq__(self, other) -> bool:
    return isinstance(other, SetpointEnergyCarbonReward) and self.as_tuple() == other.as_tuple()

  def __hash__(self) -> int:
    return hash(self.as_tuple())

  def __repr__(self) -> str:
    return "SetpointEnergyCarbonReward(%r, %r, %r, %r, %r)" % self.as_tuple()[1:]


class SpatialOutputs:
  """What ``BatchedEnvironment(..., spatial=SpatialOutputs(...))`` keeps beside the observation, refreshed with one
  launch by every ``reset()`` / ``step()`` / ``reset_buildings()`` / ``restore()`` / ``fork()``:

  ``pool``: None -- no map; ``(pool_h, pool_w)``, two integers >= 1 -- ``env.temperature_map`` [B, map_h, map_w] float32,
  the mean of every ``pool_h x pool_w`` tile of the [H, W] grid (the last row / column of tiles may be ragged).
  ``zone_stats``: ``env.zone_temp_stats`` [B, Z, 3] float64 {min, max, mean} over each zone's air control volumes
  (Building.get_zone_temp_stats, building.py:564-577).
  ValueError for a pool that is not two integers >= 1, and when neither output is asked for."""

  def __init__(self, pool: Optional[Sequence[int]] = None, zone_stats: bool = True):
    if pool is not None:
      try:
        ok = not any(isinstance(x, (bool, np.bool_)) for x in pool)
        pool = tuple(x.__index__() for x in pool)   # (integers only: a float pool is refused, not truncated)
        ok = ok and len(pool) == 2 and all(1 <= x < 1 << 31 for x in pool)
      except (TypeError, ValueError, AttributeError):
        ok = False
      if not ok:
        raise ValueError("pool must be (pool_h, pool_w), two integers >= 1, or None")
    if not isinstance(zone_stats, (bool, np.bool_)):
      raise ValueError("zone_stats must be a bool")
    if pool is None and not zone_stats:
      raise ValueError("SpatialOutputs with neither a pool nor zone_stats asks for nothing")
    self.pool, self.zone_stats = pool, bool(zone_stats)

  def __eq__(self, other) -> bool:
    return isinstance(other, SpatialOutputs) and (self.pool, self.zone_stats) == (other.pool, other.zone_stats)

  def __hash__(self) -> int:
    return hash((self.pool, self.zone_stats))

  def __repr__(self) -> str:
    return f"SpatialOutputs(pool={self.pool!r}, zone_stats={self.zone_stats!r})"


def reward_start_time_utc(ts: dt.datetime) -> dt.datetime:
  """conversion_utils.py:39-59: the reward sees pandas_to_proto -> proto_to_pandas, i.e. UTC."""
  return dt.datetime.fromtimestamp(int(epoch_seconds(ts)), tz=UTC)


# --------------------------------------------------------------------------- time features
def get_radian_time(ts, hour_of_day: bool) -> float:
  """conversion_utils.py:107-134 (in the timestamp's own zone)."""
  ts = as_datetime(ts)
  if hour_of_day:
    frac = seconds_since_midnight(ts) / _SECONDS_IN_A_DAY
  else:
    frac = float(ts.weekday()) / 7.0
  return 2.0 * np.pi * frac


# --------------------------------------------------------------------------- what a step derives from an instant
class StepModels(NamedTuple):
  """The host models one environment resolves its step inputs with, and the three constants that go with them."""
  weather: object
  schedule: SetpointSchedule
  occupancy: object
  electricity: ElectricityEnergyCost
  gas: NaturalGasEnergyCost
  step_interval: dt.timedelta
  zone_names: Tuple[str, ...]
  occupancy_norm: float


def weather_inputs(weather, ts) -> Tuple[float, float, float]:
  """(t_amb, weather_f, weather_t) of sb_step_in at ``ts``: the form the weather model uses, 0.0 for the other two."""
  if isinstance(weather, BatchedReplayWeather):
    return 0.0, 0.0, weather.query_time(ts)
  if isinstance(weather, BatchedSinusoidWeather):
    return 0.0, weather.factor(ts), 0.0
  return weather.get_current_temp(ts), 0.0, 0.0


def host_num_occupants(m: StepModels, ts) -> float:
  """SimulatorBuilding.num_occupants at ``ts`` (simulator_building.py:305-315) of a host occupancy model: the sum over
  the zones of its ``[ts - 5 min, ts]`` query.  0 for the device generator, whose buildings have their own."""
  t5 = ts - dt.timedelta(minutes=5)
  n_occ = 0.0
  if isinstance(m.occupancy, BatchedRandomizedArrivalDepartureOccupancy):
    pass
  elif isinstance(m.occupancy, StepFunctionOccupancy):
    v = m.occupancy.average_zone_occupancy("", t5, ts)   # stateless, the same for every zone: one query,
    for _ in m.zone_names:                                 # the reference's sum
      n_occ += v
  else:
    for z in m.zone_names:
      n_occ += m.occupancy.average_zone_occupancy(z, t5, ts)
  return n_occ


def aux_features(m: StepModels, ts) -> list:
  """environment.py:916-956: the SB_NUM_AUX auxiliary features of an observation at ``ts``, float32."""
  hod = get_radian_time(ts, hour_of_day=True)
  dow = get_radian_time(ts, hour_of_day=False)
  n_occ = int(host_num_occupants(m, ts))
  return [np.float32(np.cos(hod)), np.float32(np.sin(hod)), np.float32(np.cos(dow)),
          np.float32(np.sin(dow)), np.float32(m.schedule.is_comfort_mode(ts)),
          np.float32(m.schedule.is_comfort_mode(ts + dt.timedelta(minutes=60))),
          np.float32((n_occ - m.occupancy_norm) / (m.occupancy_norm + 1))]


def reward_occupancy(m: StepModels, ts):
  """average_zone_occupancy over [ts, ts + dt] as the reward's RewardInfo holds it: one value for every zone; a list per
  zone for a shared RandomizedArrivalDepartureOccupancy; 0.0 for the device generator (its buildings have their own)."""
  if isinstance(m.occupancy, BatchedRandomizedArrivalDepartureOccupancy):
    return 0.0
  if isinstance(m.occupancy, RandomizedArrivalDepartureOccupancy):
    return [m.occupancy.average_zone_occupancy(z, ts, ts + m.step_interval) for z in m.zone_names]
  return m.occupancy.average_zone_occupancy("", ts, ts + m.step_interval)


def reward_rates(m: StepModels, ts) -> Tuple[float, float, float, float]:
  """(e_price, e_carbon, g_price, g_carbon) of a reward whose interval starts at ``ts``."""
  start_utc = reward_start_time_utc(ts)
  return m.electricity.rates(start_utc) + m.gas.rates(start_utc)


def occupancy_clock(occupancy, ts) -> Tuple[int, int]:
  """sb_occupancy_peek's (local hour, working day) at ``ts``; (0, 0) for a model that is not the device generator."""
  if not isinstance(occupancy, BatchedRandomizedArrivalDepartureOccupancy):
    return 0, 0
  return occupancy.local(ts).hour, int(occupancy.is_work_day(ts))


# sb_step_in's time-dependent scalars, as step_inputs names them
STEP_INPUT_SCALARS = ("t_amb_now", "t_amb_next", "weather_f_now", "weather_f_next", "weather_t_now", "weather_t_next",
                      "comfort_now", "comfort_prev", "comfort_next", "e_price", "e_carbon", "g_price", "g_carbon")


def step_inputs(m: StepModels, ts, prev_thermostat_ts=None) -> Dict[str, object]:
  """Everything ``BatchedEnvironment.make_step_in`` derives from the step's instant ``ts`` (and the instant of the
  previous thermostat update, None: none): STEP_INPUT_SCALARS, ``aux`` (the observation's features at ts + dt) and
  ``occupancy`` (the reward's, over [ts + dt, ts + 2 dt]: one value, or a list per zone for a shared randomized model).
  The occupancy model is asked in the reference's order (environment.py:1310-1330): the observation's num_occupants, then
  the reward's query -- it matters for the randomized model, whose every query advances the occupants."""
  nxt = ts + m.step_interval
  d: Dict[str, object] = {}
  d["t_amb_now"], d["weather_f_now"], d["weather_t_now"] = weather_inputs(m.weather, ts)
  d["t_amb_next"], d["weather_f_next"], d["weather_t_next"] = weather_inputs(m.weather, nxt)
  d["comfort_now"] = int(m.schedule.is_comfort_mode(ts))
  d["comfort_prev"] = -1 if prev_thermostat_ts is None else int(m.schedule.is_comfort_mode(prev_thermostat_ts))
  d["comfort_next"] = int(m.schedule.is_comfort_mode(nxt))
  d["aux"] = aux_features(m, nxt)
  d["occupancy"] = reward_occupancy(m, nxt)
  d["e_price"], d["e_carbon"], d["g_price"], d["g_carbon"] = reward_rates(m, nxt)
  return d


# --------------------------------------------------------------------------- a calendar per building
# enum sb_clock_field (include/sbsim_amd.h): the fields of a Timeline row, in order
CLOCK_FIELDS = ("t_amb", "weather_f", "weather_t", "comfort", "aux0", "aux1", "aux2", "aux3", "aux4", "aux5", "aux6",
                "occupancy", "e_price", "e_carbon", "g_price", "g_carbon", "occ_hour", "occ_workday", "occ_hour5",
                "occ_workday5")


def instant_row(m: StepModels, ts) -> List[float]:
  """One Timeline row: everything ``BatchedEnvironment.make_step_in``, ``_aux`` and ``reset`` derive from the instant
  ``ts``, by the functions they call themselves -- as "now" (weather, comfort), as "next" (the auxiliary features, the
  reward's occupancy and rates) or as the previous thermostat update (comfort)."""
  occupancy = reward_occupancy(m, ts)   # (a Timeline refuses the shared randomized model: one value)
  return [*weather_inputs(m.weather, ts), float(int(m.schedule.is_comfort_mode(ts))), *(float(v) for v in aux_features(m, ts)),
          float(occupancy), *reward_rates(m, ts), *occupancy_clock(m.occupancy, ts),
          *occupancy_clock(m.occupancy, ts - dt.timedelta(minutes=5))]


def check_start_offsets(start_offsets, n_buildings: int) -> np.ndarray:
  """``BatchedEnvironment(start_offsets=...)`` as int32 [B]: whole step intervals, >= 0.  ValueError otherwise, naming
  the building."""
  a = np.asarray(start_offsets)
  if a.shape != (int(n_buildings),):
    raise ValueError(f"start_offsets must have shape [{int(n_buildings)}] (one offset per building), got {a.shape}")
  if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
    raise ValueError(f"start_offsets must be integers (whole step intervals), got dtype {a.dtype}")
  if (a < 0).any():
    bad = int(np.argmax(a < 0))
    raise ValueError(f"start_offsets: building {bad}: negative offset {a[bad]}")
  if (a > (1 << 22)).any():
    bad = int(np.argmax(a > (1 << 22)))
    raise ValueError(f"start_offsets: building {bad}: offset {a[bad]} is beyond the 2^22 rows a timeline may have")
  return np.ascontiguousarray(a, dtype=np.int32)


class Timeline:
  """The calendar of a batch whose buildings start at different times (``BatchedEnvironment(start_offsets=...)``): one
  ``instant_row`` per instant ``t_r = start_timestamp + r * step_interval`` for ``r = 0 .. max(offsets) +
  steps_per_episode + 1``, float64 ``rows [n_rows, len(CLOCK_FIELDS)]`` (sb_clock_attach's table).  Building b lives at
  row ``offsets[b] + position``; an episode of N transitions steps at positions 0 .. N (the last is the terminal step)
  and reads one row beyond.

  ValueError: a shared host-side ``RandomizedArrivalDepartureOccupancy`` (one stateful instance that answers for one
  instant per query; ``BatchedRandomizedArrivalDepartureOccupancy``, the device generator, is the supported form), and a
  replay weather whose trace ends before the latest building's episode does -- the message names that building."""

  def __init__(self, models: StepModels, start_timestamp, offsets, steps_per_episode: int, episode_starts=None,
               max_offset: Optional[int] = None):
    """``max_offset``: the table also holds an episode that starts at this row (``BatchedEnvironment.set_start_offsets``).
    ``episode_starts``: an ``EpisodeStarts`` -- the table is sized for the largest offset a building may draw (with
    ``relative``: its own offset plus the largest draw), and a replay weather's trace is checked over the worst possible
    draw of offset and shift."""
    m = models
    self.offsets = check_start_offsets(offsets, len(np.atleast_1d(np.asarray(offsets))))
    self.start = as_datetime(start_timestamp)
    self.step_interval = m.step_interval
    self.episode_starts = episode_starts
    self._span = int(steps_per_episode) + 1   # rows an episode reads beyond its first
    top = int(self.offsets.max()) if episode_starts is None else int(episode_starts.largest_offsets(self.offsets).max())
    if max_offset is not None:
      if isinstance(max_offset, bool) or not isinstance(max_offset, (int, np.integer)) or max_offset < 0:
        raise ValueError(f"max_start_offset must be an integer >= 0, got {max_offset!r}")
      top = max(top, int(max_offset))
    self.n_rows = top + int(steps_per_episode) + 2
    if self.n_rows > (1 << 22):
      raise ValueError(("start_offsets" if episode_starts is None else "offsets")
                       + f": the timeline would have {self.n_rows} rows, more than 2^22")
    if (isinstance(m.occupancy, RandomizedArrivalDepartureOccupancy)
        and not isinstance(m.occupancy, BatchedRandomizedArrivalDepartureOccupancy)):
      raise ValueError("start_offsets: a host-side RandomizedArrivalDepartureOccupancy is one stateful instance queried at "
                       "one instant per step; use BatchedRandomizedArrivalDepartureOccupancy (the device generator)")
    if isinstance(m.weather, ReplayWeatherController):
      self._check_trace(m.weather)
    if episode_starts is not None and isinstance(m.weather, BatchedReplayWeather):
      # (the rows hold the query time alone; which rows and shifts a building can reach was checked just above)
      w0 = copy.copy(m.weather)
      w0.offsets_sec = np.zeros(1)
      m = m._replace(weather=w0)
    self.rows = np.array([instant_row(m, self.instant(r)) for r in range(self.n_rows)], dtype=np.float64)
    self.rows.setflags(write=False)

  def instant(self, row: int) -> dt.datetime:
    return self.start + row * self.step_interval

  def check_starts(self, es, weather, base_offsets=None) -> None:
    """New starts on the table there is (``BatchedEnvironment.set_episode_starts``): the largest offset ``es`` may draw
    over ``base_offsets`` (None: the offsets of the constructor) leaves an episode's rows, and a replay weather's trace
    holds the worst possible draw of offset and shift -- what the constructor checks for its own ``episode_starts``.
    ValueError naming the building and the draw."""
    base = self.offsets if base_offsets is None else check_start_offsets(base_offsets, len(self.offsets))
    top = es.largest_offsets(base)
    b = int(np.argmax(top))
    if int(top[b]) + self._span + 1 > self.n_rows:
      raise ValueError(f"offsets: building {b}: an episode that starts at the largest possible offset {int(top[b])} needs "
                       f"{int(top[b]) + self._span + 1} rows, the timeline has {self.n_rows} (create the environment with "
                       "these episode_starts, or with max_start_offset)")
    if isinstance(weather, ReplayWeatherController):
      self._check_trace(weather, es, base)

  def _check_trace(self, weather, es=None, offsets=None) -> None:
    """Every building's last query (the row after its terminal step, plus its own replay offset) inside the trace.
    ``es`` / ``offsets``: these starts over these attached offsets (None: the constructor's)."""
    if self.start.tzinfo is None:
      raise TypeError("ReplayWeatherController needs a tz-aware timestamp (reference: tz_convert)")
    shift = getattr(weather, "offsets_sec", None)
    if shift is not None and shift.shape != self.offsets.shape:
      raise ValueError("BatchedReplayWeather needs one offset per building")
    t_min, t_max = float(weather._times.min()), float(weather._times.max())
    es = self.episode_starts if es is None else es
    if es is not None:   # the worst possible draw of offset and shift, per building
      offsets = self.offsets if offsets is None else offsets
      hi_off, lo_off = es.largest_offsets(offsets), es.smallest_offsets(offsets)
      base = np.zeros(self.offsets.shape) if shift is None else shift
      s_lo, s_hi = es.fields["weather_shift"].span() if "weather_shift" in es.fields else (None, None)
      hi_shift = base if s_hi is None else np.maximum(base, s_hi)
      lo_shift = base if s_lo is None else np.minimum(base, s_lo)
      dt_sec = self.step_interval.total_seconds()
      last = self.start.timestamp() + (hi_off + self._span) * dt_sec + hi_shift
      first = self.start.timestamp() + lo_off * dt_sec + lo_shift
      if (last > t_max).any():
        b = int(np.argmax(last))
        raise ValueError(f"episode_starts: building {b}: with offset {int(hi_off[b])} and weather shift {float(hi_shift[b])} s "
                         f"drawn, its episode ends at {dt.datetime.fromtimestamp(float(last[b]), tz=UTC)}, after the weather "
                         f"trace's last time stamp {dt.datetime.fromtimestamp(t_max, tz=UTC)}")
      if (first < t_min).any():
        b = int(np.argmin(first))
        raise ValueError(f"episode_starts: building {b}: with offset {int(lo_off[b])} and weather shift {float(lo_shift[b])} s "
                         "drawn, its episode starts before the weather trace's first time stamp")
      return
    last_row = self.offsets.astype(np.int64) + (self.n_rows - 1 - int(self.offsets.max()))
    last = self.start.timestamp() + last_row * self.step_interval.total_seconds() + (0.0 if shift is None else shift)
    first = self.start.timestamp() + self.offsets * self.step_interval.total_seconds() + (0.0 if shift is None else shift)
    if (last > t_max).any():
      b = int(np.argmax(last))
      raise ValueError(f"start_offsets: building {b}: its episode ends at "
                       f"{dt.datetime.fromtimestamp(float(last[b]), tz=UTC)}, after the weather trace's last time stamp "
                       f"{dt.datetime.fromtimestamp(t_max, tz=UTC)}")
    if (first < t_min).any():
      b = int(np.argmin(first))
      raise ValueError(f"start_offsets: building {b}: its episode starts before the weather trace's first time stamp")


class ClockCursor:
  """Which Timeline rows a batch reads: ``pos``, the position of the next step (0 after a ``reset``), and ``prev``, the
  position of the last step taken -- the previous thermostat update, which survives ``reset`` as
  ``Thermostat._previous_timestamp`` does (thermostat.py:66-69) and is None only before the first step ever."""

  def __init__(self, pos: int = 0, prev: Optional[int] = None):
    self.pos, self.prev = int(pos), (None if prev is None else int(prev))

  def reset(self) -> None:
    self.pos = 0

  def advance(self) -> None:
    """One step taken at ``pos``."""
    self.prev = self.pos
    self.pos += 1

  def rows(self, offsets) -> Dict[str, Optional[np.ndarray]]:
    """Per building: the rows a step at ``pos`` reads as now, next and the previous thermostat update (None: none)."""
    o = np.asarray(offsets, dtype=np.int64)
    return dict(now=o + self.pos, next=o + self.pos + 1, prev=None if self.prev is None else o + self.prev)

  def seek_args(self) -> Tuple[int, int]:
    """sb_clock_seek's (pos, prev_pos)."""
    return self.pos, (-1 if self.prev is None else self.prev)


def check_episode_steps(episode_steps, n_buildings: int, steps_per_episode: int) -> np.ndarray:
  """``BatchedEnvironment(episode_steps=...)`` as int64 [B]: building b's step returns LAST when its own step count has
  reached ``episode_steps[b]`` (an episode of ``episode_steps[b] + 1`` steps, as ``steps_per_episode`` counts for the
  batch); ``1 <= episode_steps[b] <= steps_per_episode``, the length the calendar was built for.  ValueError otherwise,
  naming the building."""
  a = np.asarray(episode_steps)
  if a.shape != (int(n_buildings),):
    raise ValueError(f"episode_steps must have shape [{int(n_buildings)}] (one length per building), got {a.shape}")
  if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
    raise ValueError(f"episode_steps must be integers (whole steps), got dtype {a.dtype}")
  bad = (a < 1) | (a > int(steps_per_episode))
  if bad.any():
    b = int(np.argmax(bad))
    raise ValueError(f"episode_steps: building {b}: {a[b]} is outside 1 .. {int(steps_per_episode)} (steps_per_episode)")
  return np.ascontiguousarray(a, dtype=np.int64)


class EpisodeCursor:
  """``ClockCursor`` for a batch whose buildings have episodes of their own (``BatchedEnvironment(per_building_episodes=
  True)``): the batch position ``pos`` of the next step, which only ``reset`` rewinds; ``prev``, the batch position of
  the last step taken since then (None after a ``reset``: the batch position grows across the buildings' restarts, beyond
  any row of the restored calendar -- and nothing reads that row in this mode, where every building's previous thermostat
  update is its own, on the device); and per building the batch position at which its current episode started
  (``restart_pos``).  Building b's own episode position is ``pos - restart_pos[b]``: the number of steps it has taken in
  its episode, and the Timeline row it reads next, counted from its start offset."""

  def __init__(self, n_buildings: int, pos: int = 0, prev: Optional[int] = None):
    self.pos, self.prev = int(pos), (None if prev is None else int(prev))
    self.restart_pos = np.zeros(int(n_buildings), dtype=np.int64)

  def reset(self) -> None:
    """Every building at the start of an episode, the batch at position 0, no previous position."""
    self.pos = 0
    self.prev = None
    self.restart_pos[:] = 0

  def advance(self) -> None:
    """One step taken at ``pos`` by every building."""
    self.prev = self.pos
    self.pos += 1

  def positions(self) -> np.ndarray:
    """Every building's own episode position, int64 [B]."""
    return self.pos - self.restart_pos

  def rows(self, offsets) -> Dict[str, np.ndarray]:
    """Per building: the Timeline rows its next step reads as now and next."""
    now = np.asarray(offsets, dtype=np.int64) + self.positions()
    return dict(now=now, next=now + 1)

  def ended(self, episode_steps) -> np.ndarray:
    """bool [B], after ``advance``: the buildings whose step just taken was the last of their episode -- their own step
    count before it had reached ``episode_steps[b]`` (the batch's rule, environment.py:1366-1368: an episode of
    ``episode_steps[b]`` transitions plus one terminal step)."""
    return self.positions() - 1 >= np.asarray(episode_steps, dtype=np.int64)

  def restart(self, mask) -> None:
    """The buildings of ``mask`` (bool [B]) start a new episode at the batch position of the next step."""
    self.restart_pos[np.asarray(mask, dtype=bool)] = self.pos

  def seek_args(self) -> Tuple[int, int]:
    """sb_clock_seek's (pos, prev_pos)."""
    return self.pos, (-1 if self.prev is None else self.prev)


# --------------------------------------------------------------------------- several calendars in one batch
class Calendar:
  """The exogenous models of one group of buildings (``BatchedEnvironment(calendars=[...], calendar_of=...)``): the
  setpoint schedule (hours, holidays, time zone), the occupancy model, the two tariffs, a weather shared by the group and
  the date the group's episode starts on.  Every member left None is the environment's own.

      office = Calendar(schedule=SetpointSchedule(7, 18, comfort, eco, time_zone="Europe/Berlin"),
                        occupancy=StepFunctionOccupancy(dt.timedelta(hours=8), dt.timedelta(hours=16), 12.0, 0.1),
                        weather=WeatherController(263.0, 275.0, convection_coefficient=100.0),
                        start_timestamp=dt.datetime(2023, 1, 9, 5, tzinfo=UTC))

  ``weather`` is a batch-shared form (``WeatherController`` / ``ReplayWeatherController``): the per-building forms
  (``BatchedSinusoidWeather``, ``BatchedReplayWeather``) have one row per building of the whole batch and stay
  arguments of the environment.  ValueError otherwise."""

  def __init__(self, schedule: Optional[SetpointSchedule] = None, occupancy=None, electricity_energy_cost=None,
               natural_gas_energy_cost=None, weather=None, start_timestamp=None):
    if weather is not None and (isinstance(weather, (BatchedSinusoidWeather, BatchedReplayWeather))
                                or not isinstance(weather, (WeatherController, ReplayWeatherController))):
      raise ValueError("a Calendar's weather is shared by its buildings: a WeatherController or a ReplayWeatherController "
                       f"(the per-building forms are arguments of the environment), got {type(weather).__name__}")
    if schedule is not None and not isinstance(schedule, SetpointSchedule):
      raise ValueError(f"a Calendar's schedule is a SetpointSchedule, got {type(schedule).__name__}")
    self.schedule, self.occupancy, self.weather = schedule, occupancy, weather
    self.electricity_energy_cost, self.natural_gas_energy_cost = electricity_energy_cost, natural_gas_energy_cost
    self.start_timestamp = None if start_timestamp is None else as_datetime(start_timestamp)

  def models(self, base: StepModels) -> StepModels:
    """``base`` with this calendar's members in place of the environment's."""
    own = lambda mine, theirs: theirs if mine is None else mine
    return base._replace(weather=own(self.weather, base.weather), schedule=own(self.schedule, base.schedule),
                         occupancy=own(self.occupancy, base.occupancy),
                         electricity=own(self.electricity_energy_cost, base.electricity),
                         gas=own(self.natural_gas_energy_cost, base.gas))

  def start(self, base_start) -> dt.datetime:
    return as_datetime(base_start) if self.start_timestamp is None else self.start_timestamp


def check_calendar_of(calendar_of, n_buildings: int, n_calendars: int) -> np.ndarray:
  """``BatchedEnvironment(calendar_of=...)`` as int32 [B]: building b's index into ``calendars``, 0 .. K-1, every
  calendar used by some building.  ValueError otherwise, naming the building or the calendar."""
  if calendar_of is None:
    raise ValueError("calendars needs calendar_of: an integer array [B], every building's index into calendars")
  a = np.asarray(calendar_of)
  if a.shape != (int(n_buildings),):
    raise ValueError(f"calendar_of must have shape [{int(n_buildings)}] (one calendar index per building), got {a.shape}")
  if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
    raise ValueError(f"calendar_of must be integers (indices into calendars), got dtype {a.dtype}")
  bad = (a < 0) | (a >= int(n_calendars))
  if bad.any():
    b = int(np.argmax(bad))
    raise ValueError(f"calendar_of: building {b}: calendar {a[b]} is outside 0 .. {int(n_calendars) - 1}")
  unused = np.setdiff1d(np.arange(int(n_calendars)), a)
  if unused.size:
    raise ValueError(f"calendars: calendar {int(unused[0])} is used by no building (calendar_of)")
  return np.ascontiguousarray(a, dtype=np.int32)


def device_occupancy_groups(calendars: Sequence[Calendar], occupancy) -> Optional[List]:
  """The calendars' occupancy models (``occupancy``: the environment's, for a calendar without one) when they are the
  device generator -- one ``BatchedRandomizedArrivalDepartureOccupancy`` per calendar, sb_occupancy_attach_groups'
  configurations -- or None when none of them is.  ValueError, naming the calendar, when device and host models are
  mixed (the device generator's counts override every building's occupancy) or the generators differ in what one handle
  has once: ``seed``, ``first_building``, ``time_step_sec``."""
  occ = [occupancy if c.occupancy is None else c.occupancy for c in calendars]
  dev = [isinstance(o, BatchedRandomizedArrivalDepartureOccupancy) for o in occ]
  if not any(dev):
    return None
  if not all(dev):
    k = dev.index(False)
    raise ValueError(f"calendars: calendar {k} has a host-side occupancy model ({type(occ[k]).__name__}), calendar "
                     f"{dev.index(True)} the device generator: BatchedRandomizedArrivalDepartureOccupancy overrides every "
                     "building's occupancy, so it is every calendar's model or none's")
  for k, o in enumerate(occ):
    for name in ("seed", "first_building", "time_step_sec"):
      if (getattr(o, name) or 0) != (getattr(occ[0], name) or 0):
        raise ValueError(f"calendars: calendar {k} (occupancy group {k}): {name} = {getattr(o, name)!r} differs from "
                         f"calendar 0's {getattr(occ[0], name)!r}: the device generator has one {name} per handle")
  return occ


def check_calendars(calendars: Sequence[Calendar], calendar_of, n_buildings: int, weather, occupancy, start_timestamp,
                    comfort_temp_window, eco_temp_window) -> np.ndarray:
  """What ``BatchedEnvironment(calendars=...)`` refuses before it creates anything; ``weather``, ``occupancy``,
  ``start_timestamp`` and the two windows are the environment's own (the windows: its SimConfig's).  Returns
  ``calendar_of`` as int32 [B].  ValueError, naming the calendar: a member of ``calendars`` that is no ``Calendar``; a
  schedule whose temperature windows are not the SimConfig's (the windows are per-building parameter rows:
  ``building_params``); a weather next to a per-building weather of the environment, or whose convection coefficient at
  the calendar's start is not the environment's (one coefficient table per handle: ``building_materials``); and
  ``device_occupancy_groups``' refusals."""
  calendars = list(calendars) if isinstance(calendars, (list, tuple)) else None
  if not calendars or not all(isinstance(c, Calendar) for c in calendars):
    raise ValueError("calendars must be a non-empty list of host_inputs.Calendar")
  cal_of = check_calendar_of(calendar_of, n_buildings, len(calendars))
  h_conv = weather.get_air_convection_coefficient(as_datetime(start_timestamp))
  for k, c in enumerate(calendars):
    if c.schedule is not None:
      for name, want in (("comfort_temp_window", comfort_temp_window), ("eco_temp_window", eco_temp_window)):
        got = tuple(float(v) for v in getattr(c.schedule, name))
        if got != tuple(float(v) for v in want):
          raise ValueError(f"calendars: calendar {k}: its schedule's {name} {got} is not the SimConfig's "
                           f"{tuple(float(v) for v in want)}: the windows are per-building parameters, set them with "
                           "building_params (BuildingParams)")
    if c.weather is not None:
      if isinstance(weather, (BatchedSinusoidWeather, BatchedReplayWeather)):
        raise ValueError(f"calendars: calendar {k} carries a weather, but the environment's {type(weather).__name__} "
                         "already gives every building its own")
      got = c.weather.get_air_convection_coefficient(c.start(start_timestamp))
      if got != h_conv:
        raise ValueError(f"calendars: calendar {k}: its weather's convection coefficient {got} is not the environment's "
                         f"{h_conv}: the coefficient tables are one per handle, give buildings their own with "
                         "building_materials (BuildingMaterials)")
  device_occupancy_groups(calendars, occupancy)
  return cal_of


class CalendarTimeline:
  """``Timeline`` for a batch whose buildings live on K calendars: for calendar k the rows ``Timeline`` builds --
  ``instant_row(calendars[k].models(models), t)`` at ``t = start_k + r * step_interval``, ``start_k`` the calendar's own
  start or ``start_timestamp`` -- for ``r = 0 .. max(start_offsets of its buildings) + steps_per_episode + 1``, the K
  segments one after the other in ``rows [n_rows, len(CLOCK_FIELDS)]`` (sb_clock_attach's table).  ``base[k]`` is the
  first row of calendar k's segment; building b lives at row ``offsets[b] + position`` with ``offsets[b] =
  base[calendar_of[b]] + start_offsets[b]`` (int32 [B]), at the instant ``instant(b, position)``.

  ValueError, naming the global building and its calendar: ``Timeline``'s refusals per calendar (a host-side
  ``RandomizedArrivalDepartureOccupancy``, a replay weather whose trace does not hold a building's episode, more than
  2^22 rows in the concatenated table), a wrong ``calendar_of`` and a calendar no building uses."""

  def __init__(self, calendars: Sequence[Calendar], calendar_of, models: StepModels, start_timestamp, start_offsets,
               steps_per_episode: int):
    self.calendars = list(calendars)
    n_buildings = len(np.atleast_1d(np.asarray(calendar_of if start_offsets is None else start_offsets)))
    self.calendar_of = check_calendar_of(calendar_of, n_buildings, len(self.calendars))
    self.start_offsets = check_start_offsets(np.zeros(n_buildings, dtype=np.int32) if start_offsets is None
                                             else start_offsets, n_buildings)
    self.step_interval = models.step_interval
    self.models = [c.models(models) for c in self.calendars]
    self.starts = [c.start(start_timestamp) for c in self.calendars]
    steps = int(steps_per_episode)
    # Segment k has max(start_offsets of its buildings) + steps + 2 rows.  sb_clock_seek's bound -- largest offset + pos <=
    # n_rows - 2 -- therefore holds up to pos = steps for the concatenation as it does for one Timeline: every calendar
    # has a building, so the largest offset is base[K-1] + (the last segment's largest start offset), and the last
    # segment is sized for exactly that one: n_rows = base[K-1] + that offset + steps + 2.
    members = [np.nonzero(self.calendar_of == k)[0] for k in range(len(self.calendars))]
    sizes = np.array([int(self.start_offsets[idx].max()) + steps + 2 for idx in members], dtype=np.int64)
    self.base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    self.n_rows = int(sizes.sum())
    if self.n_rows > (1 << 22):
      k = int(np.argmax(np.cumsum(sizes) > (1 << 22)))
      raise ValueError(f"calendars: the concatenated timeline would have {self.n_rows} rows, more than 2^22 (reached in "
                       f"calendar {k}, whose building {int(members[k][np.argmax(self.start_offsets[members[k]])])} starts "
                       f"at offset {int(self.start_offsets[members[k]].max())})")
    segments = []
    for k, (m, idx) in enumerate(zip(self.models, members)):
      if (isinstance(m.occupancy, RandomizedArrivalDepartureOccupancy)
          and not isinstance(m.occupancy, BatchedRandomizedArrivalDepartureOccupancy)):
        raise ValueError(f"calendars: calendar {k} (building {int(idx[0])}): a host-side RandomizedArrivalDepartureOccupancy "
                         "is one stateful instance queried at one instant per step; use "
                         "BatchedRandomizedArrivalDepartureOccupancy (the device generator)")
      if isinstance(m.weather, ReplayWeatherController):
        self._check_trace(k, m.weather, idx, int(sizes[k]))
      segments.append(np.array([instant_row(m, self.starts[k] + r * self.step_interval) for r in range(int(sizes[k]))],
                               dtype=np.float64).reshape(int(sizes[k]), len(CLOCK_FIELDS)))
    self.rows = np.concatenate(segments, axis=0)
    self.rows.setflags(write=False)
    self.offsets = np.ascontiguousarray(self.base[self.calendar_of] + self.start_offsets, dtype=np.int32)

  def instant(self, building: int, position: int = 0) -> dt.datetime:
    """Building ``building``'s instant at ``position`` of its episode, on its own calendar."""
    k = int(self.calendar_of[building])
    return self.starts[k] + (int(self.start_offsets[building]) + int(position)) * self.step_interval

  def _check_trace(self, k: int, weather, idx: np.ndarray, n_rows: int) -> None:
    """Timeline._check_trace for calendar k's buildings ``idx`` (global indices) on its segment of ``n_rows`` rows."""
    start = self.starts[k]
    if start.tzinfo is None:
      raise TypeError("ReplayWeatherController needs a tz-aware timestamp (reference: tz_convert)")
    shift = getattr(weather, "offsets_sec", None)
    if shift is not None and shift.shape != self.calendar_of.shape:
      raise ValueError("BatchedReplayWeather needs one offset per building")
    shift = 0.0 if shift is None else shift[idx]
    offs = self.start_offsets[idx].astype(np.int64)
    step = self.step_interval.total_seconds()
    last = start.timestamp() + (offs + (n_rows - 1 - int(offs.max()))) * step + shift
    first = start.timestamp() + offs * step + shift
    t_min, t_max = float(weather._times.min()), float(weather._times.max())
    if (last > t_max).any():
      b = int(idx[np.argmax(last)])
      raise ValueError(f"calendars: building {b} (calendar {k}): its episode ends at "
                       f"{dt.datetime.fromtimestamp(float(last.max()), tz=UTC)}, after the weather trace's last time stamp "
                       f"{dt.datetime.fromtimestamp(t_max, tz=UTC)}")
    if (first < t_min).any():
      b = int(idx[np.argmin(first)])
      raise ValueError(f"calendars: building {b} (calendar {k}): its episode starts before the weather trace's first "
                       "time stamp")


# --------------------------------------------------------------------------- per-building plant parameters
# SimConfig field -> the sb_params fields it sets (include/sbsim_amd.h sb_building_param), in the enum's order
BUILDING_PARAM_NAMES: Dict[str, Tuple[str, ...]] = {
    "vav_max_air_flow_rate": ("vav_max_air_flow",),
    "vav_reheat_max_water_flow_rate": ("vav_max_water_flow",),
    "ahu_recirculation": ("ahu_recirc",),
    "ahu_heating_air_temp_setpoint": ("ahu_heat_sp",),
    "ahu_cooling_air_temp_setpoint": ("ahu_cool_sp",),
    "ahu_fan_differential_pressure": ("ahu_dp",),
    "ahu_fan_efficiency": ("ahu_eff",),
    "ahu_max_air_flow_rate": ("ahu_max_flow",),
    "boiler_reheat_water_setpoint": ("blr_setpoint",),
    "boiler_water_pump_differential_head": ("blr_head",),
    "boiler_water_pump_efficiency": ("blr_pump_eff",),
    "boiler_heating_rate": ("blr_heating_rate",),
    "boiler_cooling_rate": ("blr_cooling_rate",),
    "boiler_convection_coefficient": ("blr_conv",),
    "boiler_tank_length": ("blr_len",),
    "boiler_tank_radius": ("blr_radius",),
    "boiler_water_capacity": ("blr_capacity",),
    "boiler_insulation_conductivity": ("blr_ins_k",),
    "boiler_insulation_thickness": ("blr_ins_thick",),
    "comfort_temp_window": ("comfort_lo", "comfort_hi"),
    "eco_temp_window": ("eco_lo", "eco_hi"),
    "max_productivity_personhour_usd": ("max_prod",),
    "min_productivity_personhour_usd": ("min_prod",),
    "max_electricity_rate": ("max_elec",),
    "max_natural_gas_rate": ("max_gas",),
    "productivity_midpoint_delta": ("prod_delta",),
    "productivity_decay_stiffness": ("prod_stiff",),
    "productivity_weight": ("w_prod",),
    "energy_cost_weight": ("w_cost",),
    "carbon_emission_weight": ("w_carbon",),
}
# SimConfig fields that stay one value per batch: the solver's (dt, threshold, iteration limit, the plan's materials and
# geometry), the host's (schedule hours, holidays, time zone: resolved once per step), the observation and action layout
PER_BATCH_CONFIG_FIELDS = ("time_step_sec", "convergence_threshold", "iteration_limit", "cv_size_cm", "floor_height_cm",
                           "initial_temp", "materials", "morning_start_hour", "evening_start_hour", "schedule_holidays",
                           "time_zone", "ahu_has_weather_sensor", "action_ranges", "action_names", "action_zones")
# fields the device algebra divides by (sb_device.h), and the rest of the boiler's geometry: must be > 0
_POSITIVE_PARAMS = ("vav_max_air_flow_rate", "ahu_fan_efficiency", "ahu_max_air_flow_rate", "boiler_water_pump_efficiency",
                    "boiler_convection_coefficient", "boiler_tank_length", "boiler_tank_radius",
                    "boiler_insulation_conductivity", "boiler_insulation_thickness")
_WINDOWS = {"comfort_temp_window": "comfort_temp_window[0] must be less than comfort_temp_window[1]",  # setpoint_schedule.py:66-75
            "eco_temp_window": "eco_temp_window[0] must be less than eco_temp_window[1]"}


class BuildingParams:
  """Per-building plant, setpoint-window and reward parameters of one batch (sb_set_building_params): SimConfig field
  names mapped to float64 arrays with one row per building -- shape [B], or [B, 2] for ``comfort_temp_window`` /
  ``eco_temp_window``.  A field that is not given keeps the SimConfig's value for every building.

      bp = BuildingParams({"ahu_fan_efficiency": eff, "comfort_temp_window": np.stack([lo, hi], axis=1)})
      env = BatchedEnvironment(plan, B, building_params=bp)

  Raises ValueError for an unknown name (listing the allowed ones), a per-batch SimConfig field, a wrong shape, and the
  reference's constructor checks row by row; the checks that involve a field not given here run against the SimConfig
  in ``validate``."""

  def __init__(self, values: Optional[Mapping[str, object]] = None, **kw):
    merged = dict(values or {}, **kw)
    if not merged:
      raise ValueError("BuildingParams needs at least one field (pass None instead of a table to clear one)")
    self.fields: Dict[str, np.ndarray] = {}
    self.n_buildings = None
    for name, arr in merged.items():
      if name in PER_BATCH_CONFIG_FIELDS:
        raise ValueError(f"{name!r} is one value per batch (the sweep or the host reads it), not per building")
      if name not in BUILDING_PARAM_NAMES:
        raise ValueError(f"unknown per-building parameter {name!r}; allowed: {', '.join(BUILDING_PARAM_NAMES)}")
      a = np.array(arr, dtype=np.float64)
      width = len(BUILDING_PARAM_NAMES[name])
      if a.ndim != (1 if width == 1 else 2) or (width > 1 and a.shape[1] != width) or a.shape[0] == 0:
        raise ValueError(f"{name} must have shape [B]" + ("" if width == 1 else f" x {width}") + f", got {a.shape}")
      if self.n_buildings is None:
        self.n_buildings = int(a.shape[0])
      elif a.shape[0] != self.n_buildings:
        raise ValueError(f"{name} has {a.shape[0]} rows, the other fields {self.n_buildings}: one row per building")
      bad = np.nonzero(~np.isfinite(a).reshape(a.shape[0], -1).all(axis=1))[0]
      if bad.size:
        raise ValueError(f"building {int(bad[0])}: {name} is not finite")
      if name in _POSITIVE_PARAMS and not (a > 0.0).all():
        raise ValueError(f"building {int(np.argmin(a > 0.0))}: {name} must be positive")
      if name in _WINDOWS and not (a[:, 0] <= a[:, 1]).all():
        raise ValueError(f"building {int(np.argmin(a[:, 0] <= a[:, 1]))}: {_WINDOWS[name]}")
      a.setflags(write=False)
      self.fields[name] = a

  def rows(self, lo: int, hi: int) -> "BuildingParams":
    """Buildings lo .. hi-1 (a class's or a rank's share of a larger batch)."""
    if not 0 <= lo < hi <= self.n_buildings:
      raise ValueError(f"rows [{lo}, {hi}) outside the table's {self.n_buildings} buildings")
    return BuildingParams({k: v[lo:hi] for k, v in self.fields.items()})

  def effective(self, config) -> Dict[str, np.ndarray]:
    """Every per-building SimConfig field of every building: this table's rows, the SimConfig's value elsewhere."""
    return effective_building_params(self, config, self.n_buildings)

  def validate(self, config) -> None:
    """The reference's checks that tie two fields together, on the effective rows (a field not given: the config's)."""
    eff = self.effective(config)
    heat, cool = eff["ahu_heating_air_temp_setpoint"], eff["ahu_cooling_air_temp_setpoint"]
    if not (cool > heat).all():   # air_handler.py:60-64
      raise ValueError(f"building {int(np.argmin(cool > heat))}: cooling_air_temp_setpoint must greater than "
                       "heating_air_temp_setpoint")
    for name, msg in _WINDOWS.items():
      w = eff[name]
      if not (w[:, 0] <= w[:, 1]).all():
        raise ValueError(f"building {int(np.argmin(w[:, 0] <= w[:, 1]))}: {msg}")
    wsum = eff["productivity_weight"] + eff["energy_cost_weight"] + eff["carbon_emission_weight"]
    if not (wsum > 0.0).all():
      raise ValueError(f"building {int(np.argmin(wsum > 0.0))}: productivity_weight + energy_cost_weight + "
                       "carbon_emission_weight must be positive (the reward divides by it)")

  def c_table(self) -> Tuple[np.ndarray, np.ndarray]:
    """sb_set_building_params' arguments: the named sb_building_param fields (int32 [n]) and their rows ([n][B])."""
    from . import _ffi
    index = {name: k for k, name in enumerate(_ffi.BUILDING_PARAM_FIELDS)}
    fields, rows = [], []
    for name, a in self.fields.items():
      for j, c_name in enumerate(BUILDING_PARAM_NAMES[name]):
        fields.append(index[c_name])
        rows.append(a if a.ndim == 1 else a[:, j])
    return np.asarray(fields, dtype=np.int32), np.ascontiguousarray(np.stack(rows))


def effective_building_params(params: Optional[BuildingParams], config, n_buildings: int) -> Dict[str, np.ndarray]:
  """The per-building SimConfig fields of n_buildings buildings: ``params``' rows where it has the field, the config's
  value elsewhere (``params`` None: every building the config's)."""
  out = {}
  for name, c_fields in BUILDING_PARAM_NAMES.items():
    if params is not None and name in params.fields:
      out[name] = params.fields[name].copy()
    else:
      v = np.asarray(getattr(config, name), dtype=np.float64)
      out[name] = np.broadcast_to(v, (n_buildings,) + v.shape).copy()
  return out


_MATERIAL_KINDS = ("conductivity", "heat_capacity", "density")   # sb_material_kind, in order


class BuildingMaterials:
  """Per-building envelope physics of one batch (sb_set_building_materials): the conductivity, heat capacity and density
  of each of the floor plan's M material slots (``FloorPlan.material_slots()``: the plan's distinct materials in raster
  order -- for a ``from_file_input`` plan the exterior wall, the interior wall and the air, in the order the plan meets
  them), float64 [B, M] each, and the outside convection coefficient, float64 [B].  What is left out keeps the plan's own
  value (the ``h_conv`` of the weather controller for the convection coefficient) for every building.

      ids, table = plan.material_slots()
      bm = BuildingMaterials(conductivity=table[:, 0] * np.random.uniform(0.5, 2.0, size=(B, len(table))),
                             convection_coefficient=np.random.uniform(5.0, 50.0, size=B))
      env = BatchedEnvironment(plan, B, building_materials=bm)

  Raises ValueError, naming the building, for a wrong shape, a value that is not finite, a material value <= 0 or a
  negative convection coefficient."""

  def __init__(self, conductivity=None, heat_capacity=None, density=None, convection_coefficient=None):
    given = dict(conductivity=conductivity, heat_capacity=heat_capacity, density=density,
                 convection_coefficient=convection_coefficient)
    if all(v is None for v in given.values()):
      raise ValueError("BuildingMaterials needs at least one field (pass None instead of a table to clear one)")
    self.fields: Dict[str, np.ndarray] = {}
    self.n_buildings = None
    self.n_slots = None   # M; None when only the convection coefficient is given
    for name, arr in given.items():
      if arr is None:
        continue
      a = np.array(arr, dtype=np.float64)
      material = name in _MATERIAL_KINDS
      if a.ndim != (2 if material else 1) or 0 in a.shape:
        raise ValueError(f"{name} must have shape [B" + (", M]" if material else "]") + f", got {a.shape}")
      if self.n_buildings is None:
        self.n_buildings = int(a.shape[0])
      elif a.shape[0] != self.n_buildings:
        raise ValueError(f"{name} has {a.shape[0]} rows, the other fields {self.n_buildings}: one row per building")
      if material:
        if self.n_slots is None:
          self.n_slots = int(a.shape[1])
        elif a.shape[1] != self.n_slots:
          raise ValueError(f"{name} has {a.shape[1]} material slots, the other fields {self.n_slots}")
      bad = np.nonzero(~np.isfinite(a).reshape(a.shape[0], -1).all(axis=1))[0]
      if bad.size:
        raise ValueError(f"building {int(bad[0])}: {name} is not finite")
      ok = (a > 0.0) if material else (a >= 0.0)
      if not ok.all():
        b = int(np.argmin(ok.reshape(a.shape[0], -1).all(axis=1)))
        raise ValueError(f"building {b}: {name} must " + ("be positive" if material else "not be negative"))
      a.setflags(write=False)
      self.fields[name] = a

  def rows(self, lo: int, hi: int) -> "BuildingMaterials":
    """Buildings lo .. hi-1 (a class's or a rank's share of a larger batch)."""
    if not 0 <= lo < hi <= self.n_buildings:
      raise ValueError(f"rows [{lo}, {hi}) outside the table's {self.n_buildings} buildings")
    return BuildingMaterials(**{k: v[lo:hi] for k, v in self.fields.items()})

  def check_plan(self, n_buildings: int, n_slots: int) -> None:
    if self.n_buildings != n_buildings:
      raise ValueError(f"BuildingMaterials has {self.n_buildings} rows, the simulator {n_buildings} buildings")
    if self.n_slots is not None and self.n_slots != n_slots:
      raise ValueError(f"BuildingMaterials has {self.n_slots} material slots, the floor plan {n_slots} "
                       "(FloorPlan.material_slots())")

  def c_table(self, n_slots: int) -> Tuple[np.ndarray, np.ndarray]:
    """sb_set_building_materials' arguments for a plan of n_slots slots: the named fields (kind * M + slot; 3 M: the
    convection coefficient; int32 [n]) and their rows ([n][B])."""
    fields, rows = [], []
    for name, a in self.fields.items():
      if name == "convection_coefficient":
        fields.append(3 * n_slots)
        rows.append(a)
      else:
        for s in range(n_slots):
          fields.append(_MATERIAL_KINDS.index(name) * n_slots + s)
          rows.append(a[:, s])
    return np.asarray(fields, dtype=np.int32), np.ascontiguousarray(np.stack(rows))


def effective_building_materials(materials: Optional[BuildingMaterials], slot_table: np.ndarray, h_conv: float,
                                 n_buildings: int) -> Dict[str, np.ndarray]:
  """The materials every building runs with: ``materials``' rows where it has the field, the plan's own slot table
  ([M, 3]) and convection coefficient elsewhere.  conductivity / heat_capacity / density [B, M],
  convection_coefficient [B]."""
  out = {}
  for j, name in enumerate(_MATERIAL_KINDS):
    out[name] = np.broadcast_to(np.asarray(slot_table, dtype=np.float64)[:, j], (n_buildings, len(slot_table))).copy()
  out["convection_coefficient"] = np.full(n_buildings, float(h_conv))
  if materials is not None:
    for name, a in materials.fields.items():
      out[name] = a.copy()
  return out


# ---------------------------------------------------------------- start temperatures per building
# the three attachments' draws: the last counter word is the tag (| the field's number); _ffi states them from include/sbsim_amd.h
INITIAL_CONDITIONS_TAG, RANDOMIZATION_TAG, EPISODE_STARTS_TAG = (
    _ffi.SB_INITIAL_CONDITIONS_TAG, _ffi.SB_RANDOMIZATION_TAG, _ffi.SB_EPISODE_STARTS_TAG)
RAND_MATERIAL = _ffi.SB_RAND_MATERIAL            # id of material field f
RAND_MAX_CHOICES = _ffi.SB_RAND_MAX_CHOICES
START_MAX_K = _ffi.SB_START_MAX_K
_M32 = 0xFFFFFFFF


def _philox_block(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
  """One Philox4x32-10 block on Python integers (csrc/philox.h): the four output words of a four-word counter under a
  two-word key."""
  c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
  k0, k1 = (int(k) & _M32 for k in key)
  for _ in range(10):
    hi0, lo0 = divmod(0xD2511F53 * c0, 1 << 32)
    hi1, lo1 = divmod(0xCD9E8D57 * c2, 1 << 32)
    c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
  return c0, c1, c2, c3


class Uniform:
  """d = lo + (hi - lo) * u, u the 53-bit uniform of the field's Philox block: a value in [lo, hi].  ``scale``: the
  field's value is the building's own base row times d.  For a window field (``comfort_temp_window``,
  ``eco_temp_window``) lo and hi are pairs, one interval per edge: ``Uniform((293.0, 296.5), (295.0, 299.0))`` draws
  edge 0 in [293, 295] and edge 1 in [296.5, 299]."""

  def __init__(self, lo, hi, scale: bool = False):
    self.lo, self.hi, self.scale = lo, hi, bool(scale)

  def __repr__(self) -> str:
    return f"Uniform({self.lo!r}, {self.hi!r}, scale={self.scale})"


class Choice:
  """d = values[(c0 * K) >> 32], c0 the first word of the field's Philox block: one of K <= 65,536 values, integer
  arithmetic only (a log-spaced table is how a log-uniform draw stays bit for bit).  ``scale`` as ``Uniform``'s."""

  def __init__(self, values, scale: bool = False):
    self.values, self.scale = values, bool(scale)

  def __repr__(self) -> str:
    return f"Choice({self.values!r}, scale={self.scale})"


class UniformInt:
  """d = lo + step * ((c0 * K) >> 32), K = (hi - lo) // step + 1, c0 the first word of the field's Philox block: one of
  the K <= 2^22 whole numbers lo, lo + step, ... <= hi, integer arithmetic only (``EpisodeStarts(offsets=...)``)."""

  def __init__(self, lo, hi, step=1):
    self.lo, self.hi, self.step = lo, hi, step

  def __repr__(self) -> str:
    return f"UniformInt({self.lo!r}, {self.hi!r}, step={self.step!r})"


class _Dist(NamedTuple):
  """One parsed distribution, as the three per-episode attachments keep it."""
  kind: int                    # sb_rand_kind: 0 Uniform, 1 Choice, 2 UniformInt
  lo: float
  hi: float
  step: int
  values: Tuple[float, ...]
  scale: bool

  @property
  def k(self) -> int:
    return len(self.values) if self.kind == _ffi.SB_RAND_CHOICE else (int(self.hi) - int(self.lo)) // self.step + 1

  def span(self) -> Tuple[float, float]:
    """The smallest and the largest possible draw."""
    if self.kind == _ffi.SB_RAND_CHOICE:
      return min(self.values), max(self.values)
    if self.kind == _ffi.SB_RAND_UNIFORM_INT:
      return self.lo, float(int(self.lo) + self.step * (self.k - 1))
    return self.lo, self.hi


def _whole(v) -> bool:
  if isinstance(v, (bool, np.bool_)):
    return False
  if isinstance(v, (int, np.integer)):
    return True
  return isinstance(v, (float, np.floating)) and math.isfinite(v) and float(v) == math.floor(v)


def _parse_dist(name: str, dist, *, offset: bool = False, allow_scale: bool = True) -> _Dist:
  """``dist`` of field ``name`` checked: a ``Uniform`` or a ``Choice``; ``offset`` (rows of a timeline): a ``UniformInt``
  or a ``Choice`` of whole numbers in 0 .. 2^22.  ValueError naming the field."""
  if isinstance(dist, UniformInt) and offset:
    if not (_whole(dist.lo) and _whole(dist.hi)):
      raise ValueError(f"{name}: UniformInt needs whole numbers of rows, got ({dist.lo!r}, {dist.hi!r})")
    lo, hi = int(dist.lo), int(dist.hi)
    if lo < 0:
      raise ValueError(f"{name}: negative offset {lo}")
    if lo > hi:
      raise ValueError(f"{name}: lo {lo} > hi {hi}")
    if not _whole(dist.step) or int(dist.step) < 1:
      raise ValueError(f"{name}: step must be an integer >= 1, got {dist.step!r}")
    if hi > (1 << 22):
      raise ValueError(f"{name}: offset {hi} is beyond the 2^22 rows a timeline may have")
    d = _Dist(_ffi.SB_RAND_UNIFORM_INT, float(lo), float(hi), int(dist.step), (), False)
    if d.k > START_MAX_K:
      raise ValueError(f"{name}: K == {d.k} is more than 2^22")
    return d
  if isinstance(dist, Choice):
    if dist.scale and not allow_scale:
      raise ValueError(f"{name}: scale is not supported here" + (" (relative=True adds the draw to the attached offset)" if offset else ""))
    try:
      v = np.array(dist.values, dtype=np.float64)
    except (TypeError, ValueError):
      raise ValueError(f"{name}: Choice needs a list of numbers, got {dist.values!r}") from None
    if v.ndim != 1:
      raise ValueError(f"{name}: Choice needs a list of values, got shape {v.shape}")
    if v.size == 0 or v.size > RAND_MAX_CHOICES:
      raise ValueError(f"{name}: a Choice needs 1 .. 65,536 values, got K == {v.size}")
    if not np.isfinite(v).all():
      raise ValueError(f"{name}: choice {int(np.argmin(np.isfinite(v)))} is not finite")
    if offset:
      for j, x in enumerate(np.asarray(dist.values).tolist()):
        if not _whole(x):
          raise ValueError(f"{name}: choice {j} must be a whole number of rows, got {x!r}")
        if x < 0:
          raise ValueError(f"{name}: choice {j}: negative offset {x}")
        if x > (1 << 22):
          raise ValueError(f"{name}: choice {j}: offset {x} is beyond the 2^22 rows a timeline may have")
    return _Dist(_ffi.SB_RAND_CHOICE, 0.0, 0.0, 1, tuple(float(x) for x in v), dist.scale)
  if isinstance(dist, Uniform) and not offset:
    if dist.scale and not allow_scale:
      raise ValueError(f"{name}: scale is not supported here")
    try:
      lo, hi = float(dist.lo), float(dist.hi)
    except (TypeError, ValueError):
      raise ValueError(f"{name}: Uniform needs one lo and one hi, got ({dist.lo!r}, {dist.hi!r})") from None
    if not (math.isfinite(lo) and math.isfinite(hi)):
      raise ValueError(f"{name}: lo and hi must be finite, got ({lo}, {hi})")
    if lo > hi:
      raise ValueError(f"{name}: lo {lo} > hi {hi}")
    return _Dist(_ffi.SB_RAND_UNIFORM, lo, hi, 1, (), dist.scale)
  raise ValueError(f"{name}: the distribution must be " + ("a UniformInt or a Choice of integer rows" if offset else "a Uniform or a Choice")
                   + f", got {dist!r}")


def _episode_draw(dist: _Dist, tag_word: int, seed: int, gb: int, e: int):
  """d of one field for global building gb in its episode number e (the formulas of include/sbsim_amd.h, on Python integers
  and IEEE doubles: one rounding per operation): from the Philox4x32-10 block keyed by the seed with counter (gb lo, gb hi,
  e, tag_word).  An int for a ``UniformInt``."""
  c = _philox_block((gb & _M32, gb >> 32, int(e) & _M32, tag_word), (seed & _M32, seed >> 32))
  if dist.kind == _ffi.SB_RAND_UNIFORM:
    r = (c[1] << 32) | c[0]
    return dist.lo + (dist.hi - dist.lo) * (float(r >> 11) * 2.0 ** -53)
  i = (c[0] * dist.k) >> 32
  return dist.values[i] if dist.kind == _ffi.SB_RAND_CHOICE else int(dist.lo) + dist.step * i


def _fill_c_dist(cf, dist: _Dist, keep: list) -> None:
  """kind and lo / hi or choices / n_choices of a sb_rand_field or a sb_start_field; ``keep`` gets what ``choices`` points into."""
  cf.kind = dist.kind
  if dist.kind == _ffi.SB_RAND_CHOICE:
    v = np.ascontiguousarray(dist.values, dtype=np.float64)
    keep.append(v)
    cf.n_choices, cf.choices = len(dist.values), v.ctypes.data_as(_ffi._dp)
  else:
    cf.lo, cf.hi = dist.lo, dist.hi


def _check_seed_first(seed, first_building) -> Tuple[int, int]:
  if isinstance(seed, (bool, float)) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
    raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
  if isinstance(first_building, (bool, float)) or int(first_building) != first_building or first_building < 0:
    raise ValueError(f"first_building must be an integer >= 0, got {first_building!r}")
  return int(seed), int(first_building)


def _moved_first(self, lo: int):
  """``rows(lo)`` of an attachment without [B] arrays: a copy with ``first_building`` moved, so that buildings lo .. of a
  larger batch draw what they drew in the whole batch."""
  if lo < 0:
    raise ValueError(f"rows: lo must be >= 0, got {lo}")
  out = copy.copy(self)
  out.first_building = self.first_building + int(lo)
  return out


def _per_building(name: str, arr, dtype) -> np.ndarray:
  a = np.array(arr)
  if a.ndim != 1 or a.shape[0] == 0:
    raise ValueError(f"{name} must have shape [B], got {a.shape}")
  if dtype is np.int32:
    if a.dtype.kind not in "iu":
      raise ValueError(f"{name} must be an integer array, got dtype {a.dtype}")
    return a.astype(np.int64)
  a = a.astype(np.float64)
  bad = np.nonzero(~np.isfinite(a))[0]
  if bad.size:
    raise ValueError(f"building {int(bad[0])}: {name} is not finite")
  return a


@dataclasses.dataclass
class InitialConditions:
  """Start temperatures per building (sb_initial_conditions_attach): what every ``reset()`` of a building -- of the
  whole batch, of a mask, an autoreset -- writes into its grid, kept on the device.  The reference's
  ``FloorPlanBasedBuilding(initial_temp=, reset_temp_values=)`` (simulator/building.py:650,680,784-792) for a batch.

      ic = InitialConditions(reset_temp_values=recorded_grid)                       # every building, every episode
      ic = InitialConditions(reset_temp_values=grids, grid_of=which)                # K grids [K, H, W], one per building
      ic = InitialConditions(initial_temp=t0, jitter=(-0.5, 0.5, seed))             # a number per building and a draw
      env = BatchedEnvironment(plan, B, initial_conditions=ic)

  ``reset_temp_values``: float64 [H, W] or [K, H, W] in the caller's orientation; ``grid_of``: int [B], building b's
  grid (None: grid 0); ``initial_temp``: float64 [B], only without grids; ``offset``: float64 [B], added to every cell
  of the building; ``jitter``: (lo, hi, seed), one uniform draw in [lo, hi) per building and episode, added to every
  cell, seed a uint64; ``first_building``: the global index of building 0 (shards of one batch draw the same numbers).
  ``start_temps`` states the value of every cell.  ValueError, naming the field (and the building): K == 0, K > 1
  without ``grid_of``, a ``grid_of`` out of range or without grids, ``initial_temp`` together with grids, a value that
  is not finite, lo > hi, a seed outside uint64, [B] arrays of different lengths, no field at all; ``check`` adds what
  needs the batch: a grid of another shape than the plan's, [B] arrays of another length."""
  reset_temp_values: Optional[np.ndarray] = None
  grid_of: Optional[np.ndarray] = None
  initial_temp: Optional[np.ndarray] = None
  offset: Optional[np.ndarray] = None
  jitter: Optional[Tuple[float, float, int]] = None
  first_building: int = 0

  def __post_init__(self):
    if self.reset_temp_values is not None:
      g = np.array(self.reset_temp_values, dtype=np.float64)
      if g.ndim == 2:
        g = g[None]
      if g.ndim != 3 or 0 in g.shape[1:]:
        raise ValueError(f"reset_temp_values must have shape [H, W] or [K, H, W], got {np.shape(self.reset_temp_values)}")
      if g.shape[0] == 0:
        raise ValueError("reset_temp_values: K == 0 grids (pass None for no grids)")
      bad = np.argwhere(~np.isfinite(g))
      if bad.size:
        raise ValueError(f"reset_temp_values: grid {int(bad[0][0])} cell ({int(bad[0][1])}, {int(bad[0][2])}) is not finite")
      g.setflags(write=False)
      self.reset_temp_values = g
    if self.grid_of is not None:
      if self.reset_temp_values is None:
        raise ValueError("grid_of needs reset_temp_values: the grids it indexes")
      k = _per_building("grid_of", self.grid_of, np.int32)
      bad = np.nonzero((k < 0) | (k >= self.n_grids))[0]
      if bad.size:
        raise ValueError(f"building {int(bad[0])}: grid_of {int(k[bad[0]])} is outside the {self.n_grids} grids")
      self.grid_of = k.astype(np.int32)
      self.grid_of.setflags(write=False)
    elif self.n_grids > 1:
      raise ValueError(f"reset_temp_values holds {self.n_grids} grids: grid_of must say which one a building starts from")
    if self.initial_temp is not None:
      if self.reset_temp_values is not None:
        raise ValueError("initial_temp and reset_temp_values are two bases for the same cells: give one")
      self.initial_temp = _per_building("initial_temp", self.initial_temp, np.float64)
      self.initial_temp.setflags(write=False)
    if self.offset is not None:
      self.offset = _per_building("offset", self.offset, np.float64)
      self.offset.setflags(write=False)
    if self.jitter is not None:
      try:
        lo, hi, seed = self.jitter
      except (TypeError, ValueError):
        raise ValueError("jitter must be (lo, hi, seed)") from None
      lo, hi = float(lo), float(hi)
      if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"jitter: lo and hi must be finite, got ({lo}, {hi})")
      if lo > hi:
        raise ValueError(f"jitter: lo {lo} > hi {hi}")
      if isinstance(seed, (bool, float)) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"jitter: seed must be an integer in [0, 2^64), got {seed!r}")
      self.jitter = (lo, hi, int(seed))
    if isinstance(self.first_building, bool) or int(self.first_building) != self.first_building or self.first_building < 0:
      raise ValueError(f"first_building must be an integer >= 0, got {self.first_building!r}")
    self.first_building = int(self.first_building)
    if self.reset_temp_values is None and self.initial_temp is None and self.offset is None and self.jitter is None:
      raise ValueError("InitialConditions needs at least one field (pass None instead of an InitialConditions to clear them)")
    lengths = {name: int(a.shape[0]) for name, a in self._per_building_fields().items()}
    if len(set(lengths.values())) > 1:
      raise ValueError("the [B] arrays have different lengths: " + ", ".join(f"{n} {l}" for n, l in lengths.items()))

  def _per_building_fields(self) -> Dict[str, np.ndarray]:
    return {n: a for n, a in (("grid_of", self.grid_of), ("initial_temp", self.initial_temp), ("offset", self.offset))
            if a is not None}

  @property
  def n_grids(self) -> int:
    return 0 if self.reset_temp_values is None else int(self.reset_temp_values.shape[0])

  @property
  def n_buildings(self) -> Optional[int]:
    """B of the [B] arrays; None when there is none (one grid, a jitter): such conditions fit every batch size."""
    for a in self._per_building_fields().values():
      return int(a.shape[0])
    return None

  @property
  def has_base(self) -> bool:
    """Whether the conditions say what a cell starts from (grids or ``initial_temp``) and not only what is added."""
    return self.reset_temp_values is not None or self.initial_temp is not None

  def check(self, n_buildings: int, shape: Tuple[int, int]) -> None:
    """What needs the batch: the grids have the plan's shape, the [B] arrays the batch's length."""
    if self.reset_temp_values is not None and tuple(self.reset_temp_values.shape[1:]) != tuple(shape):
      raise ValueError(f"reset_temp_values: grids of shape {tuple(self.reset_temp_values.shape[1:])}, the floor plan is "
                       f"{tuple(shape)}")
    for name, a in self._per_building_fields().items():
      if a.shape[0] != n_buildings:
        raise ValueError(f"{name} has {a.shape[0]} rows, the batch {n_buildings} buildings")

  def rows(self, lo: int, hi: int) -> "InitialConditions":
    """Buildings lo .. hi-1 (a class's or a rank's share of a larger batch): their rows, and ``first_building`` moved so
    that they draw what they drew in the whole batch."""
    n = self.n_buildings
    if lo < 0 or hi <= lo or (n is not None and hi > n):
      raise ValueError(f"rows [{lo}, {hi}) outside the conditions' {n} buildings")
    cut = lambda a: None if a is None else a[lo:hi]
    return InitialConditions(self.reset_temp_values, cut(self.grid_of), cut(self.initial_temp), cut(self.offset), self.jitter,
                             self.first_building + lo)

  def draw(self, b: int, e: int) -> float:
    """u(b, e): the jitter of building b's episode number e -- lo + (hi - lo) * ((r >> 11) * 2^-53), r the first two
    words of the Philox4x32-10 block keyed by the seed with counter (global building lo, hi, e, INITIAL_CONDITIONS_TAG)."""
    lo, hi, seed = self.jitter
    return _episode_draw(_Dist(_ffi.SB_RAND_UNIFORM, lo, hi, 1, (), False), INITIAL_CONDITIONS_TAG, seed, self.first_building + int(b), e)

  def start_temps(self, b: int, e: int, initial_temp: Optional[float] = None, shape: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The grid [H, W] (caller's orientation) building b starts its episode number e from, in float64 with one rounding
    per operation -- what the device writes.  ``initial_temp`` / ``shape``: the reset call's scalar
    (``SimConfig.initial_temp``) and the plan's shape, needed where the conditions hold neither grids nor ``initial_temp``
    (``shape`` also with ``initial_temp`` alone)."""
    if self.reset_temp_values is not None:
      v = self.reset_temp_values[0 if self.grid_of is None else int(self.grid_of[b])].copy()
    else:
      if shape is None:
        raise ValueError("start_temps needs the plan's shape without grids")
      if self.initial_temp is None and initial_temp is None:
        raise ValueError("start_temps needs the reset call's initial_temp: the conditions hold no base")
      v = np.full(tuple(shape), float(self.initial_temp[b]) if self.initial_temp is not None else float(initial_temp))
    if self.offset is not None:
      v = v + float(self.offset[b])
    if self.jitter is not None:
      v = v + self.draw(b, e)
    return v

  def digest(self) -> str:
    """A hash of everything attached (``BatchedSimulator.state_fingerprint``)."""
    h = hashlib.sha256()
    for a in (self.reset_temp_values, self.grid_of, self.initial_temp, self.offset):
      h.update(b"-" if a is None else str((a.dtype.str, a.shape)).encode() + np.ascontiguousarray(a).tobytes())
    h.update(repr((None if self.jitter is None else (self.jitter[0].hex(), self.jitter[1].hex(), self.jitter[2]),
                   self.first_building)).encode())
    return h.hexdigest()


# ---------------------------------------------------------------- parameters and materials re-drawn per episode
class _RandField(NamedTuple):
  name: str        # as messages and ``values`` name it: the SimConfig field (with [edge]), kind[slot], convection_coefficient
  param: Optional[int]                  # sb_building_param, or None for a material field
  material: Optional[Tuple[int, int]]   # (kind, slot); kind 3: the convection coefficient
  dist: _Dist

  def ident(self, n_slots: Optional[int]) -> int:
    if self.param is not None:
      return self.param
    if n_slots is None:
      raise ValueError(f"{self.name}: a material field's number needs the plan's slot count (n_slots)")
    kind, slot = self.material
    return RAND_MATERIAL + (3 * n_slots if kind == 3 else kind * n_slots + slot)


def _items(table, what: str):
  if table is None:
    return []
  if isinstance(table, Mapping):
    return list(table.items())
  try:
    return [(k, v) for k, v in table]
  except (TypeError, ValueError):
    raise ValueError(f"{what} must be a mapping (or a list of pairs) of field -> distribution") from None


class EpisodeRandomization:
  """Per-building parameters and materials re-drawn at every episode start, on the device (sb_randomization_attach;
  INTEGRATION.md 4p): domain randomisation for batches whose buildings restart on their own.

      er = EpisodeRandomization(
          params={"ahu_fan_efficiency": Uniform(0.7, 0.95),
                  "vav_max_air_flow_rate": Uniform(0.8, 1.2, scale=True),
                  "comfort_temp_window": Uniform((293.0, 296.5), (295.0, 299.0))},
          materials={"conductivity": {0: Choice([20., 35., 50., 80.])}, "convection_coefficient": Uniform(6.0, 25.0)},
          seed=7)
      env = BatchedEnvironment(plan, B, episode_steps=lengths, building_materials=bm, episode_randomization=er)

  ``params``: SimConfig field name (``BUILDING_PARAM_NAMES``) -> ``Uniform`` / ``Choice``; a window field takes a
  ``Uniform`` with pair bounds or a pair of distributions, one per edge.  ``materials``: "conductivity" / "heat_capacity"
  / "density" -> {slot of ``FloorPlan.material_slots()``: distribution}, "convection_coefficient" -> distribution.
  ``values`` states the value of every field of building b in its episode e; a field's draw depends on (seed, global
  building, e, field) alone.  ValueError, naming the field: an unknown, per-batch or repeated field, lo > hi, a bound or
  choice that is not finite, K == 0 or K > 65,536, a seed outside uint64, first_building < 0; ``check`` adds what needs
  the batch."""

  def __init__(self, params=None, materials=None, seed: int = 0, first_building: int = 0):
    index = {name: k for k, name in enumerate(_ffi.BUILDING_PARAM_FIELDS)}
    fields: List[_RandField] = []
    seen = set()

    def add(name, param, material, dist):
      key = (param, material)
      if key in seen:
        raise ValueError(f"{name} is named twice")
      seen.add(key)
      fields.append(_RandField(name, param, material, _parse_dist(name, dist)))

    for name, dist in _items(params, "params"):
      if name in PER_BATCH_CONFIG_FIELDS:
        raise ValueError(f"{name!r} is one value per batch (the sweep or the host reads it), not per building")
      if name not in BUILDING_PARAM_NAMES:
        raise ValueError(f"unknown per-building parameter {name!r}; allowed: {', '.join(BUILDING_PARAM_NAMES)}")
      c_names = BUILDING_PARAM_NAMES[name]
      if len(c_names) == 1:
        add(name, index[c_names[0]], None, dist)
        continue
      if isinstance(dist, Uniform):   # pair bounds: one interval per edge
        try:
          edges = [Uniform(dist.lo[j], dist.hi[j], dist.scale) for j in range(len(c_names))]
          if len(dist.lo) != len(c_names) or len(dist.hi) != len(c_names):
            raise TypeError
        except (TypeError, IndexError):
          raise ValueError(f"{name}: a window's Uniform takes pairs, (lo0, lo1) and (hi0, hi1): one interval per edge") from None
      elif isinstance(dist, (list, tuple)) and len(dist) == len(c_names):
        edges = list(dist)
      else:
        raise ValueError(f"{name}: a window takes a Uniform with pair bounds or a pair of distributions, one per edge")
      for j, c_name in enumerate(c_names):
        add(f"{name}[{j}]", index[c_name], None, edges[j])
    for kind, table in _items(materials, "materials"):
      if kind == "convection_coefficient":
        add(kind, None, (3, 0), table)
      elif kind in _MATERIAL_KINDS:
        for slot, dist in _items(table, kind):
          if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or slot < 0 or slot >= 255:
            raise ValueError(f"{kind}: a material slot is an integer in 0 .. 254 (FloorPlan.material_slots()), got {slot!r}")
          add(f"{kind}[{int(slot)}]", None, (_MATERIAL_KINDS.index(kind), int(slot)), dist)
      else:
        raise ValueError(f"unknown material field {kind!r}; allowed: {', '.join(_MATERIAL_KINDS)}, convection_coefficient")
    if not fields:
      raise ValueError("EpisodeRandomization needs at least one field (pass None instead of one to clear it)")
    self.seed, self.first_building = _check_seed_first(seed, first_building)
    self.fields = tuple(fields)

  @property
  def has_materials(self) -> bool:
    return any(f.material is not None for f in self.fields)

  @property
  def has_params(self) -> bool:
    return any(f.param is not None for f in self.fields)

  def rows(self, lo: int, hi: int = None) -> "EpisodeRandomization":
    """The same randomisation for buildings lo .. of a larger batch: ``first_building`` moved so that they draw what they
    drew in the whole batch."""
    return _moved_first(self, lo)

  def draw(self, field: _RandField, b: int, e: int, n_slots: Optional[int] = None) -> float:
    """d of ``field`` for building b in its episode number e (the formula of include/sbsim_amd.h, on Python integers and
    IEEE doubles: one rounding per operation)."""
    return _episode_draw(field.dist, RANDOMIZATION_TAG | field.ident(n_slots), self.seed, self.first_building + int(b), e)

  @staticmethod
  def _base_of(field: _RandField, base, b: int) -> float:
    if field.param is not None:
      name, _, edge = field.name.partition("[")
      a = base[name][b]
      return float(a[int(edge[:-1])]) if edge else float(a)
    kind, slot = field.material
    return float(base["convection_coefficient"][b]) if kind == 3 else float(base[_MATERIAL_KINDS[kind]][b][slot])

  @staticmethod
  def _base_column(field: _RandField, base) -> np.ndarray:
    """``_base_of`` for every building at once: float64 [B]."""
    if field.param is not None:
      name, _, edge = field.name.partition("[")
      a = np.asarray(base[name], dtype=np.float64)
      return a[:, int(edge[:-1])] if edge else a
    kind, slot = field.material
    return np.asarray(base["convection_coefficient"] if kind == 3 else np.asarray(base[_MATERIAL_KINDS[kind]])[:, slot], dtype=np.float64)

  def values(self, b: int, e: int, base: Optional[Mapping[str, np.ndarray]] = None, n_slots: Optional[int] = None) -> Dict[str, object]:
    """The value of every randomised field of building b in its episode number e -- what the device writes.  ``base``:
    the rows in force at attach, by name (``building_params()`` merged with ``building_materials()``: float64 [B],
    [B, 2] for a window, [B, M] for a material kind); needed for ``scale`` fields and for material fields (whose numbers
    depend on M; ``n_slots`` gives M without a base).  Returns SimConfig field -> float ([2] for a window, with the edge
    that is not randomised from ``base``), material kind -> float64 [M] (the slots not randomised from ``base``),
    "convection_coefficient" -> float."""
    if n_slots is None and base is not None and "conductivity" in base:
      n_slots = int(np.asarray(base["conductivity"]).shape[1])
    out: Dict[str, object] = {}
    for f in self.fields:
      d = self.draw(f, b, e, n_slots)
      if f.dist.scale:
        if base is None:
          raise ValueError(f"{f.name}: a scale field needs the base rows")
        d = self._base_of(f, base, b) * d
      if f.param is not None:
        name, _, edge = f.name.partition("[")
        if edge:
          if name not in out:
            if base is None and sum(g.name.startswith(name + "[") for g in self.fields) < 2:
              raise ValueError(f"{name}: one edge is randomised, the other needs the base rows")
            out[name] = np.array(base[name][b], dtype=np.float64) if base is not None else np.zeros(2)
          out[name][int(edge[:-1])] = d
        else:
          out[name] = d
      elif f.material[0] == 3:
        out["convection_coefficient"] = d
      else:
        kind = _MATERIAL_KINDS[f.material[0]]
        if kind not in out:
          if base is None:
            raise ValueError(f"{f.name}: a material field needs the base rows (the slots that are not randomised)")
          out[kind] = np.array(base[kind][b], dtype=np.float64)
        out[kind][f.material[1]] = d
    return out

  def check(self, n_buildings: int, base_params: Mapping[str, np.ndarray], base_materials: Optional[Mapping[str, np.ndarray]],
            solver: str = "gauss_seidel") -> None:
    """What needs the batch, as sb_randomization_attach checks it: material fields need a simulator created with
    ``building_materials`` (``base_materials`` None: there is none) and not solver="jacobi_fp32"; a slot beyond the
    plan's; and every possible draw against the rows' checks, on the closed range of every field, per building where
    ``scale`` makes the range depend on the base row.  ValueError naming the field and, for these, the building."""
    B = int(n_buildings)
    if self.has_materials:
      if solver == "jacobi_fp32":
        f = next(f for f in self.fields if f.material is not None)
        raise ValueError(f"{f.name}: material fields are not implemented for solver='jacobi_fp32' (its float32 class table "
                         "is one per batch)")
      if base_materials is None:
        f = next(f for f in self.fields if f.material is not None)
        raise ValueError(f"{f.name}: material fields need an environment created with building_materials=... (its floor "
                         "plan is compiled into structural classes)")
    base = dict(base_params)
    if base_materials is not None:
      base.update(base_materials)
    M = None if base_materials is None else int(np.asarray(base_materials["conductivity"]).shape[1])
    span: Dict[Tuple, Tuple[np.ndarray, np.ndarray]] = {}

    def first_bad(ok) -> int:
      return int(np.argmin(ok))

    for f in self.fields:
      if f.material is not None and f.material[0] != 3 and f.material[1] >= M:
        raise ValueError(f"{f.name}: the floor plan has {M} material slots (FloorPlan.material_slots())")
      lo, hi = f.dist.span()
      scale = f.dist.scale
      b0 = self._base_column(f, base) if scale else None
      with np.errstate(over="ignore", invalid="ignore"):   # (an overflow is what the next lines refuse)
        x, y = (b0 * lo, b0 * hi) if scale else (np.full(B, lo), np.full(B, hi))
      ok = np.isfinite(x) & np.isfinite(y)
      if not ok.all():
        raise ValueError(f"building {first_bad(ok)}: {f.name} can be drawn not finite")
      span[(f.param, f.material)] = (np.minimum(x, y), np.maximum(x, y))
      mn = span[(f.param, f.material)][0]
      if f.material is not None:
        ok = (mn >= 0.0) if f.material[0] == 3 else (mn > 0.0)
        if not ok.all():
          b = first_bad(ok)
          raise ValueError(f"building {b}: {f.name} must " + ("not be negative" if f.material[0] == 3 else "be positive")
                           + f", and can be drawn as {mn[b]}")
      elif f.name in _POSITIVE_PARAMS and not (mn > 0.0).all():
        b = first_bad(mn > 0.0)
        raise ValueError(f"building {b}: {f.name} must be positive, and can be drawn as {mn[b]}")
    if not self.has_params:
      return
    index = {name: k for k, name in enumerate(_ffi.BUILDING_PARAM_FIELDS)}

    def rng(name: str, edge: Optional[int] = None):
      """(drawn, lowest, highest) possible value per building of a SimConfig field (or a window's edge)."""
      k = index[BUILDING_PARAM_NAMES[name][edge or 0]]
      if (k, None) in span:
        return (True,) + span[(k, None)]
      a = np.asarray(base[name], dtype=np.float64)
      a = a[:, edge] if edge is not None else a
      return False, a, a

    dh, _, heat_hi = rng("ahu_heating_air_temp_setpoint")
    dc, cool_lo, _ = rng("ahu_cooling_air_temp_setpoint")
    if (dh or dc) and not (cool_lo > heat_hi).all():   # air_handler.py:60-64
      b = first_bad(cool_lo > heat_hi)
      which = "ahu_heating_air_temp_setpoint" if dh else "ahu_cooling_air_temp_setpoint"
      raise ValueError(f"building {b}: {which}: the largest possible heating setpoint {heat_hi[b]} must be below the "
                       f"smallest possible cooling setpoint {cool_lo[b]}")
    for name, msg in _WINDOWS.items():
      d0, _, lo_hi = rng(name, 0)
      d1, hi_lo, _ = rng(name, 1)
      if (d0 or d1) and not (lo_hi <= hi_lo).all():
        raise ValueError(f"building {first_bad(lo_hi <= hi_lo)}: {name}: {msg} in every possible draw")
    w = [rng(n) for n in ("productivity_weight", "energy_cost_weight", "carbon_emission_weight")]
    if any(x[0] for x in w) and not (w[0][1] + w[1][1] + w[2][1] > 0.0).all():
      b = first_bad(w[0][1] + w[1][1] + w[2][1] > 0.0)
      which = ("productivity_weight", "energy_cost_weight", "carbon_emission_weight")[[x[0] for x in w].index(True)]
      raise ValueError(f"building {b}: {which}: productivity_weight + energy_cost_weight + carbon_emission_weight must be "
                       "positive at their smallest draws (the reward divides by it)")

  def c_fields(self, n_slots: Optional[int]):
    """sb_randomization_attach's ``fields`` for a plan of n_slots material slots: the ctypes array and what it points into."""
    arr = (_ffi.RandField * len(self.fields))()
    keep = []
    for i, f in enumerate(self.fields):
      arr[i].id, arr[i].scale = f.ident(n_slots), int(f.dist.scale)
      _fill_c_dist(arr[i], f.dist, keep)
    return arr, keep

  def digest(self) -> str:
    """A hash of everything attached (``BatchedSimulator.state_fingerprint``): the fields in the order of their numbers."""
    rows = sorted((f.param is None, f.param, f.material, d.kind == _ffi.SB_RAND_CHOICE, d.scale, d.lo.hex(), d.hi.hex(),
                   tuple(v.hex() for v in d.values)) for f, d in ((f, f.dist) for f in self.fields))
    return hashlib.sha256(repr((rows, self.seed, self.first_building)).encode()).hexdigest()


# ---------------------------------------------------------------- a start time and weather per building drawn per episode
START_FIELDS = ("offsets", "weather_low", "weather_high", "weather_shift")   # sb_start_field_id, in order


class EpisodeStarts:
  """A start time and weather per building, drawn anew at every episode start, on the device (sb_episode_starts_attach;
  INTEGRATION.md 4q): every reset of a building moves it to a new row of the timeline under new weather.

      es = EpisodeStarts(offsets=UniformInt(0, 364 * 288, step=288),      # rows of the timeline (whole step intervals)
                         weather_low=Uniform(268.0, 285.0), weather_high=Uniform(286.0, 305.0), seed=11)
      env = BatchedEnvironment(plan, B, weather=BatchedSinusoidWeather(low, high), episode_steps=lengths, episode_starts=es)

  ``offsets``: ``UniformInt`` or a ``Choice`` of integer rows; ``relative=True`` adds the draw to the building's attached
  offset (``start_offsets``).  ``weather_low`` / ``weather_high``: ``Uniform`` / ``Choice``, ``BatchedSinusoidWeather``
  only.  ``weather_shift``: likewise, ``BatchedReplayWeather``'s ``offsets_sec``.  A field left out stays what it is.
  ``values`` states every field of building b in its episode e; a draw depends on (seed, global building, e, field)
  alone.  ValueError, naming the field: offsets that are negative or no whole numbers, lo > hi, step < 1, K > 2^22, a
  bound or choice that is not finite, no field at all, a seed outside uint64, first_building < 0; ``check`` adds what
  needs the batch."""

  def __init__(self, offsets=None, relative: bool = False, weather_low=None, weather_high=None, weather_shift=None,
               seed: int = 0, first_building: int = 0):
    given = dict(zip(START_FIELDS, (offsets, weather_low, weather_high, weather_shift)))
    self.fields: Dict[str, _Dist] = {name: _parse_dist(name, dist, offset=name == "offsets", allow_scale=False)
                                     for name, dist in given.items() if dist is not None}
    if not self.fields:
      raise ValueError("EpisodeStarts needs at least one field (pass None instead of one to clear it)")
    if "weather_low" in self.fields and "weather_high" in self.fields:
      lo_max, hi_min = self.fields["weather_low"].span()[1], self.fields["weather_high"].span()[0]
      if lo_max > hi_min:
        raise ValueError(f"weather_low: low can be drawn as {lo_max}, above a high of {hi_min}")
    self.seed, self.first_building = _check_seed_first(seed, first_building)
    self.relative = bool(relative)

  @property
  def has_offsets(self) -> bool:
    return "offsets" in self.fields

  def rows(self, lo: int, hi: int = None) -> "EpisodeStarts":
    """The same starts for buildings lo .. of a larger batch: ``first_building`` moved so that they draw what they drew
    in the whole batch."""
    return _moved_first(self, lo)

  def draw(self, name: str, b: int, e: int):
    """d of field ``name`` for building b in its episode number e (the formula of include/sbsim_amd.h, on Python integers
    and IEEE doubles: one rounding per operation); an int for the offsets."""
    d = _episode_draw(self.fields[name], EPISODE_STARTS_TAG | START_FIELDS.index(name), self.seed, self.first_building + int(b), e)
    return int(d) if name == "offsets" else d

  def values(self, b: int, e: int, base_offsets=None) -> Dict[str, object]:
    """The value of every drawn field of building b in its episode number e -- what the device writes: "offsets" -> int
    (with ``relative``: ``base_offsets[b]`` + the draw; ``base_offsets`` None: zeros), the weather fields -> float."""
    out: Dict[str, object] = {}
    for name in self.fields:
      d = self.draw(name, b, e)
      if name == "offsets" and self.relative and base_offsets is not None:
        d = int(np.asarray(base_offsets)[b]) + d
      out[name] = d
    return out

  def largest_offsets(self, base_offsets) -> np.ndarray:
    """int64 [B]: the largest offset building b may have while this is attached -- its attached offset, or the largest
    possible draw (added to it with ``relative``)."""
    base = np.asarray(base_offsets, dtype=np.int64)
    if not self.has_offsets:
      return base
    top = int(self.fields["offsets"].span()[1])
    return base + top if self.relative else np.maximum(base, top)

  def smallest_offsets(self, base_offsets) -> np.ndarray:
    base = np.asarray(base_offsets, dtype=np.int64)
    if not self.has_offsets:
      return base
    low = int(self.fields["offsets"].span()[0])
    return base + low if self.relative else np.minimum(base, low)

  def check(self, n_buildings: int, weather, calendars=None) -> None:
    """What needs the batch, as sb_episode_starts_attach checks it: weather fields need the matching per-building weather
    class; a drawn low must not exceed the building's own high (and the other way round) where only one of the two is
    drawn; ``calendars`` together with drawn offsets.  ValueError naming the field and, where it depends on one, the
    building."""
    if calendars is not None and self.has_offsets:
      raise ValueError("offsets: episode_starts is not supported together with calendars (the calendars' tables lie one "
                       "after the other: a drawn offset would walk from one into the next)")
    for name in ("weather_low", "weather_high"):
      if name in self.fields and not isinstance(weather, BatchedSinusoidWeather):
        raise ValueError(f"{name}: needs weather=BatchedSinusoidWeather(...) (one (low, high) pair per building on the device)")
    if "weather_shift" in self.fields and not isinstance(weather, BatchedReplayWeather):
      raise ValueError("weather_shift: needs weather=BatchedReplayWeather(...) (one offset into the trace per building)")
    if "weather_low" in self.fields and "weather_high" not in self.fields:
      bad = self.fields["weather_low"].span()[1] > weather.high
      if bad.any():
        b = int(np.argmax(bad))
        raise ValueError(f"weather_low: building {b}: low can be drawn as {self.fields['weather_low'].span()[1]}, above its high of {weather.high[b]}")
    if "weather_high" in self.fields and "weather_low" not in self.fields:
      bad = weather.low > self.fields["weather_high"].span()[0]
      if bad.any():
        b = int(np.argmax(bad))
        raise ValueError(f"weather_high: building {b}: high can be drawn as {self.fields['weather_high'].span()[0]}, below its low of {weather.low[b]}")

  def c_desc(self, weather_lohi_ptr: int = 0, weather_offset_ptr: int = 0):
    """sb_episode_starts_attach's descriptor: the ctypes struct and what it points into."""
    d = _ffi.EpisodeStartsDesc()
    keep = []
    for name, f in self.fields.items():
      cf = d.field[START_FIELDS.index(name)]
      cf.present, cf.step = 1, f.step
      _fill_c_dist(cf, f, keep)
    d.relative = int(self.relative)
    d.weather_lohi_dev, d.weather_offset_dev = weather_lohi_ptr or None, weather_offset_ptr or None
    d.seed, d.first_building = self.seed, self.first_building
    return d, keep

  def digest(self) -> str:
    """A hash of everything attached (``BatchedSimulator.state_fingerprint``)."""
    rows = [(name, f.kind, f.lo.hex(), f.hi.hex(), f.step, tuple(v.hex() for v in f.values)) for name, f in sorted(self.fields.items())]
    return hashlib.sha256(repr((rows, self.relative, self.seed, self.first_building)).encode()).hexdigest()


# ---- episode totals per building (sb_episode_metrics_attach; include/sbsim_amd.h states the table) ----
EPISODE_METRIC_NAMES = _ffi.EPISODE_METRIC_NAMES


class EpisodeMetricsTwin:
  """The episode totals of B buildings in NumPy, written from the table of include/sbsim_amd.h (sb_episode_metrics_attach):
  ``running`` and ``completed``, float64 [B, 20] with the columns ``EPISODE_METRIC_NAMES``.  ``step`` is what one
  sb_step adds, ``close`` the latch in front of a reset.  Every operation is one IEEE double operation on fp32 inputs
  widened, in the table's order, so the device rows equal these bit for bit."""

  K = 1.0 / 3600.0 / 1000.0   # W s -> kWh

  def __init__(self, n_buildings: int, dt: float):
    self.B, self.dt = int(n_buildings), np.float64(dt)
    self.running = self._fresh(self.B, 0.0)
    self.completed = self._fresh(self.B, -1.0)   # no episode closed yet

  @staticmethod
  def _fresh(n: int, episode) -> np.ndarray:
    rows = np.zeros((n, _ffi.SB_EM_FIELDS), dtype=np.float64)
    rows[:, 0] = episode
    rows[:, 18], rows[:, 19] = np.inf, -np.inf
    return rows

  def step(self, reward, info, zone_means) -> None:
    """reward: float32 [B] as the step returned it (-inf: rejected); info: float32 [B, 24] as k_post wrote it;
    zone_means: float64 [B, Z], the post-update zone means."""
    reward = np.asarray(reward)
    info = np.asarray(info)
    if reward.dtype != np.float32 or info.dtype != np.float32:
      raise ValueError("reward and info are the step's float32 outputs")
    zm = np.asarray(zone_means, dtype=np.float64).reshape(self.B, -1)
    r = reward.astype(np.float64)
    I = info.astype(np.float64)
    dt, K = self.dt, np.float64(self.K)
    rejected = np.isneginf(reward)
    R = self.running
    with np.errstate(invalid="ignore"):
      R[:, 1] += 1.0
      R[:, 2] += rejected
      R[:, 3] += r
      R[~rejected, 4] += r[~rejected]
      R[:, 5] += (I[:, 0] * dt * K + I[:, 1] * dt * K) + I[:, 3] * dt * K
      R[:, 6] += I[:, 2] * dt * K
      for col, src in ((7, 9), (8, 10), (9, 11), (10, 17), (11, 20), (12, 21), (13, 22), (14, 23), (15, 8), (16, 4)):
        R[:, col] += I[:, src]
      R[:, 17] += info[:, 5] == 0
      R[:, 18] = np.minimum(R[:, 18], zm.min(axis=1))
      R[:, 19] = np.maximum(R[:, 19], zm.max(axis=1))

  def close(self, mask=None) -> np.ndarray:
    """The latch: every building of ``mask`` (None: all) with steps > 0 has its running row copied to its completed row
    and its running row re-initialised with episode + 1; the others keep both rows.  Returns which buildings closed."""
    m = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    closing = m & (self.running[:, 1] > 0)
    self.completed[closing] = self.running[closing]
    fresh = self._fresh(int(closing.sum()), 0.0)
    fresh[:, 0] = self.running[closing, 0] + 1.0
    self.running[closing] = fresh
    return closing


# ---- buildings scored against recorded zone temperatures (sb_telemetry_attach; include/sbsim_amd.h states the table) ----
TELEMETRY_SCORE_NAMES = _ffi.TELEMETRY_SCORE_NAMES
TELEMETRY_ZONE_SCORE_NAMES = _ffi.TELEMETRY_ZONE_SCORE_NAMES


class Telemetry:
  """Recorded zone temperatures to score every building of a batch against, on the device (sb_telemetry_attach).

      tel = Telemetry(recorded, actions=recorded_setpoints)          # one recording [n_rows, Z] for every building
      tel = Telemetry(recordings, trace_of=which, first_row=where)   # [n_traces, n_rows, Z]; a trace and a first row per building
      env = BatchedEnvironment(plan, B, telemetry=tel)

  ``zone_temps``: float32 or float64 [n_rows, Z] or [n_traces, n_rows, Z], kelvin, widened to float64; NaN is "no
  sample", +-inf is refused.  ``trace_of``: int [B], building b's trace (None: 0).  ``first_row``: int [B] in
  [0, n_rows), the row building b's first step after a reset is compared with (None: 0); row r goes with the building's
  (r - first_row)-th step since its reset, rows at or beyond n_rows count as missing.  ``zone_weights``: float64 [Z],
  finite and >= 0 (None: all 1).  ``actions``: float32 [n_rows, A] or [n_traces, n_rows, A], the normalised setpoints
  recorded with the temperatures (``telemetry_actions()`` hands each building its next row; past the end, the last).
  ``per_zone``: also keep samples, sum_err, sum_abs_err, sum_sq_err per zone.
  ValueError, naming what is at fault: here whatever the arrays themselves show, in ``check`` what needs the batch."""

  def __init__(self, zone_temps, trace_of=None, first_row=None, zone_weights=None, actions=None, per_zone: bool = False):
    t = np.asarray(zone_temps)
    if t.dtype not in (np.float32, np.float64):
      raise ValueError(f"zone_temps must be float32 or float64, got {t.dtype}")
    t = np.array(t, dtype=np.float64)
    if t.ndim == 2:
      t = t[None]
    if t.ndim != 3 or 0 in t.shape:
      raise ValueError(f"zone_temps must have shape [n_rows, Z] or [n_traces, n_rows, Z], got {np.shape(zone_temps)}")
    bad = np.argwhere(np.isinf(t))
    if bad.size:
      raise ValueError(f"zone_temps: trace {int(bad[0][0])} row {int(bad[0][1])} zone {int(bad[0][2])} is infinite (NaN is \"no sample\")")
    t.setflags(write=False)
    self.zone_temps = t
    self.trace_of = self._index("trace_of", trace_of, self.n_traces, "traces")
    self.first_row = self._index("first_row", first_row, self.n_rows, "rows")
    if self.trace_of is not None and self.first_row is not None and len(self.trace_of) != len(self.first_row):
      raise ValueError(f"trace_of has {len(self.trace_of)} rows, first_row {len(self.first_row)}")
    self.zone_weights = None
    if zone_weights is not None:
      w = np.array(zone_weights, dtype=np.float64)
      if w.shape != (self.n_zones,):
        raise ValueError(f"zone_weights must have shape [{self.n_zones}], got {w.shape}")
      bad = np.nonzero(~np.isfinite(w) | (w < 0))[0]
      if bad.size:
        raise ValueError(f"zone_weights[{int(bad[0])}] = {w[bad[0]]} must be finite and >= 0")
      w.setflags(write=False)
      self.zone_weights = w
    self.actions = None
    if actions is not None:
      a = np.array(actions, dtype=np.float32)
      if a.ndim == 2:
        a = a[None]
      if a.ndim != 3 or a.shape[2] == 0:
        raise ValueError(f"actions must have shape [n_rows, A] or [n_traces, n_rows, A], got {np.shape(actions)}")
      if a.shape[:2] != t.shape[:2]:
        raise ValueError(f"actions hold {a.shape[0]} traces of {a.shape[1]} rows, zone_temps {t.shape[0]} of {t.shape[1]}")
      if not np.isfinite(a).all():
        raise ValueError("actions must be finite")
      a.setflags(write=False)
      self.actions = a
    self.per_zone = bool(per_zone)

  @staticmethod
  def _index(name, values, n, what):
    if values is None:
      return None
    k = _per_building(name, values, np.int32)
    bad = np.nonzero((k < 0) | (k >= n))[0]
    if bad.size:
      raise ValueError(f"building {int(bad[0])}: {name} {int(k[bad[0]])} is outside the {n} {what}")
    k = k.astype(np.int32)
    k.setflags(write=False)
    return k

  @property
  def n_traces(self) -> int:
    return int(self.zone_temps.shape[0])

  @property
  def n_rows(self) -> int:
    return int(self.zone_temps.shape[1])

  @property
  def n_zones(self) -> int:
    return int(self.zone_temps.shape[2])

  @property
  def n_actions(self) -> int:
    return 0 if self.actions is None else int(self.actions.shape[2])

  def check(self, n_buildings: int, n_zones: int, n_actions: Optional[int] = None) -> None:
    """What needs the batch: Z zones, [B] arrays of the batch's length, actions of the simulator's A columns."""
    if self.n_zones != n_zones:
      raise ValueError(f"zone_temps hold {self.n_zones} zones, the floor plan {n_zones}")
    for name, a in (("trace_of", self.trace_of), ("first_row", self.first_row)):
      if a is not None and a.shape[0] != n_buildings:
        raise ValueError(f"{name} has {a.shape[0]} rows, the batch {n_buildings} buildings")
    if self.actions is not None and n_actions is not None and self.n_actions != n_actions:
      raise ValueError(f"actions have {self.n_actions} columns, the simulator {n_actions}")

  def per_building(self, n_buildings: int) -> Tuple[np.ndarray, np.ndarray]:
    """(trace_of, first_row) as int32 [B], the defaults filled in."""
    zeros = np.zeros(n_buildings, dtype=np.int32)
    return (zeros if self.trace_of is None else self.trace_of, zeros if self.first_row is None else self.first_row)


class TelemetryTwin:
  """csrc/telemetry.h restated in NumPy float64 with plain loops, for B buildings of Z zones: ``running`` and
  ``completed``, float64 [B, 13] with the columns ``TELEMETRY_SCORE_NAMES``, and with ``tel.per_zone`` ``zone_running``
  and ``zone_completed``, float64 [B, Z, 4] (``TELEMETRY_ZONE_SCORE_NAMES``).  ``step`` is what one sb_step adds,
  ``close`` the latch in front of a reset.  Every operation is one IEEE double operation in the header's order, so the
  device tables equal these bit for bit."""

  def __init__(self, tel: Telemetry, n_buildings: int, n_zones: Optional[int] = None):
    self.tel, self.B, self.Z = tel, int(n_buildings), tel.n_zones if n_zones is None else int(n_zones)
    tel.check(self.B, self.Z)
    self.trace_of, self.first_row = tel.per_building(self.B)
    self.weights = np.ones(self.Z) if tel.zone_weights is None else tel.zone_weights
    self.running = self._fresh(self.B, 0.0)
    self.completed = self._fresh(self.B, -1.0)   # no episode closed yet
    self.zone_running = np.zeros((self.B, self.Z, _ffi.SB_TL_ZONE_FIELDS)) if tel.per_zone else None
    self.zone_completed = np.zeros((self.B, self.Z, _ffi.SB_TL_ZONE_FIELDS)) if tel.per_zone else None

  @staticmethod
  def _fresh(n: int, episode) -> np.ndarray:
    rows = np.zeros((n, _ffi.SB_TL_FIELDS), dtype=np.float64)
    rows[:, 0] = episode
    rows[:, 7:10] = -1.0
    return rows

  def step(self, zone_means) -> None:
    """zone_means: float64 [B, Z], the post-update zone means (``sim.zone_temps()``)."""
    zm = np.asarray(zone_means, dtype=np.float64).reshape(self.B, self.Z)
    traces, n_rows = self.tel.zone_temps, self.tel.n_rows
    with np.errstate(all="ignore"):
      for b in range(self.B):
        R = self.running[b]
        r = np.float64(self.first_row[b]) + R[1]
        R[1] += 1.0
        if not (r >= 0.0 and r < n_rows):
          R[3] += np.float64(self.Z)
          continue
        row = traces[self.trace_of[b], int(r)]
        for z in range(self.Z):
          obs = row[z]
          if np.isnan(obs):
            R[3] += 1.0
            continue
          e = zm[b, z] - obs
          a = np.abs(e)
          q = e * e
          w = self.weights[z]
          R[2] += 1.0
          R[4] += e
          R[5] += a
          R[6] += q
          if a > R[7]:
            R[7], R[8], R[9] = a, r, np.float64(z)
          R[10] += w * a
          R[11] += w * q
          R[12] += w
          if self.zone_running is not None:
            zr = self.zone_running[b, z]
            zr[0] += 1.0
            zr[1] += e
            zr[2] += a
            zr[3] += q

  def close(self, mask=None) -> np.ndarray:
    """The latch: every building of ``mask`` (None: all) with steps > 0 has its running rows copied to its completed rows
    and re-initialised with episode + 1; the others keep every row.  Returns which buildings closed."""
    m = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    closing = m & (self.running[:, 1] > 0)
    self.completed[closing] = self.running[closing]
    fresh = self._fresh(int(closing.sum()), 0.0)
    fresh[:, 0] = self.running[closing, 0] + 1.0
    self.running[closing] = fresh
    if self.zone_running is not None:
      self.zone_completed[closing] = self.zone_running[closing]
      self.zone_running[closing] = 0.0
    return closing

  def action_rows(self) -> np.ndarray:
    """The row of the recording every building's next step is scored on, the last row past the end: int [B]."""
    r = self.first_row.astype(np.float64) + self.running[:, 1]
    return np.where(r < self.tel.n_rows, np.maximum(r, 0.0), self.tel.n_rows - 1).astype(np.int64)

  def actions(self) -> np.ndarray:
    """What ``telemetry_actions()`` returns: float32 [B, A]."""
    if self.tel.actions is None:
      raise ValueError("the telemetry holds no actions")
    return self.tel.actions[self.trace_of, self.action_rows()]
