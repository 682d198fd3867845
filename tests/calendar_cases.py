"""The calendars of tests/test_calendars_cpu.py and tests/test_calendars_gpu.py: three sets of exogenous models that differ
in every member -- setpoint schedule (hours, time zone), StepFunctionOccupancy (hours, headcount), electricity tariff
(holiday calendar), gas tariff, shared sinusoid weather (low / high) and the start date (three months, three weekdays) --
with starts chosen so that each crosses its own comfort switch inside a 30-step run (asserted by ``crosses_comfort``).
The temperature windows are the SimConfig's and the convection coefficient is the environment's, as a calendar must have
them."""
import datetime as dt

import numpy as np

from sbsim_amd import host_inputs

UTC = dt.timezone.utc
DT = dt.timedelta(seconds=300)
COMFORT, ECO = (294.0, 297.0), (289.0, 298.0)   # SimConfig.sb1()'s windows
H_CONV = 100.0
F = {name: i for i, name in enumerate(host_inputs.CLOCK_FIELDS)}

# (morning hour, evening hour, time zone) of the schedule; the comfort switch each start is placed before
SCHEDULES = ((6, 19, "US/Pacific"), (8, 17, "Europe/Berlin"), (7, 20, "UTC"))
STARTS = (dt.datetime(2023, 7, 6, 12, 0, tzinfo=UTC),     # Thursday 05:00 PDT: the morning switch at step 12
          dt.datetime(2023, 1, 10, 6, 0, tzinfo=UTC),     # Tuesday 07:00 CET: the morning switch at step 12
          dt.datetime(2023, 10, 4, 18, 30, tzinfo=UTC))   # Wednesday 18:30 UTC: the evening switch at step 18
WORK = ((9, 17, 10.0, 0.1), (7, 15, 6.0, 0.5), (8, 20, 25.0, 0.0))   # StepFunctionOccupancy: start h, end h, work, nonwork
TARIFF_HOLIDAYS = ("us", None, (dt.date(2023, 10, 4),))   # calendar 2: its own start date is a holiday (weekend prices)
GAS = (host_inputs.GAS_PRICE_BY_MONTH, tuple(2.0 * v for v in host_inputs.GAS_PRICE_BY_MONTH),
       tuple(v + 1.0 for v in host_inputs.GAS_PRICE_BY_MONTH))
WEATHER = ((273.0, 283.0), (262.0, 270.0), (280.0, 296.0))


def schedule(k):
  morning, evening, zone = SCHEDULES[k]
  return host_inputs.SetpointSchedule(morning, evening, COMFORT, ECO, set(), zone)


def members(k):
  """Calendar k's members as ``host_inputs.Calendar``'s keyword arguments (fresh objects on every call)."""
  ws, we, work, nonwork = WORK[k]
  return dict(schedule=schedule(k),
              occupancy=host_inputs.StepFunctionOccupancy(dt.timedelta(hours=ws), dt.timedelta(hours=we), work, nonwork),
              electricity_energy_cost=host_inputs.ElectricityEnergyCost(holiday_calendar=TARIFF_HOLIDAYS[k]),
              natural_gas_energy_cost=host_inputs.NaturalGasEnergyCost(GAS[k]),
              weather=host_inputs.WeatherController(*WEATHER[k], convection_coefficient=H_CONV),
              start_timestamp=STARTS[k])


def calendars():
  return [host_inputs.Calendar(**members(k)) for k in range(3)]


def plain_kwargs(k):
  """Calendar k's members as the keyword arguments of a plain ``BatchedEnvironment`` that has them as its own models
  (the schedule goes through the SimConfig: ``config_fields``)."""
  m = members(k)
  return dict(weather=m["weather"], occupancy=m["occupancy"], electricity_energy_cost=m["electricity_energy_cost"],
              natural_gas_energy_cost=m["natural_gas_energy_cost"], start_timestamp=m["start_timestamp"])


def config_fields(k):
  morning, evening, zone = SCHEDULES[k]
  return dict(morning_start_hour=morning, evening_start_hour=evening, time_zone=zone)


def base_models(zone_names=("room_1", "room_2"), occupancy_norm=0.0):
  """The models of an environment created with defaults (what a member left None falls back to)."""
  return host_inputs.StepModels(host_inputs.WeatherController(273.0, 283.0, convection_coefficient=H_CONV),
                                host_inputs.SetpointSchedule(6, 19, COMFORT, ECO, set(), "US/Pacific"),
                                host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1),
                                host_inputs.ElectricityEnergyCost(), host_inputs.NaturalGasEnergyCost(), DT,
                                tuple(zone_names), float(occupancy_norm))


def crosses_comfort(timeline, building, steps):
  """Building ``building`` sees its comfort flag change among the rows its ``steps`` steps read (now and next)."""
  o = int(timeline.offsets[building])
  return len(set(timeline.rows[o:o + steps + 1, F["comfort"]])) > 1


def episode_days(steps):
  """``num_days_in_episode`` of an episode of ``steps`` transitions."""
  return (steps + 0.5) * 300.0 / 86400.0
