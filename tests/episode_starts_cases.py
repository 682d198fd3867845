"""Shared cases of the episode-starts tests (host_inputs.EpisodeStarts, sb_episode_starts_attach): the weather models, the
starts, and what a handle must hold after a given history of resets, restated from ``EpisodeStarts.values``.  No device
needed.

The sinusoid case starts at 07:00 on the SB1 schedule (comfort until 19:00: row 144 of a 5-minute timeline) and draws
offsets from {132, 136, .., 148}: an episode of up to five steps crosses the comfort switch from some of them and not
from others.  The replay case lives inside tests/golden/local_weather_test_data.csv, ten hours of one Saturday.

The replay case crosses no comfort switch: the trace covers Saturday 00:00 to 10:00 only, a weekend day on the SB1
schedule, so every row of its timeline is in eco mode.  ``comfort_prev`` under moved offsets is therefore exercised by
the sinusoid runs alone (test_episode_starts_cpu asserts the crossing for them and returns before it for the replay
case); the replay runs check the drawn shift and the trace rows."""
import datetime as dt
import os
import types

import numpy as np

from sbsim_amd import host_inputs
from sbsim_amd.host_inputs import Choice, EpisodeStarts, Uniform, UniformInt
from tests import calendar_cases as cc
from tests import randomization_cases as rc
from tests.golden_util import GOLDEN

UTC = dt.timezone.utc
DT = dt.timedelta(seconds=300)
START = rc.START                                          # Thursday 6 July 2023, 07:00
START_TRACE = dt.datetime(2023, 7, 1, tzinfo=UTC)         # the trace's first time stamp
CSV = os.path.join(GOLDEN, "local_weather_test_data.csv")
EPISODE_ROWS = 16                                         # steps_per_episode of SHORT
SHORT = dict(num_days_in_episode=EPISODE_ROWS / 288, holiday_calendar=None)
SEED = 1                                                  # (test_episode_starts_cpu asserts what it has to show)
LENGTHS = np.array([2, 3, 4, 2, 3])
MAX_OFFSET = 148


def sinusoid_weather(B):
  low = np.linspace(270.0, 280.0, B)
  return host_inputs.BatchedSinusoidWeather(low, low + np.linspace(8.0, 14.0, B), 100.0)


def replay_weather(B):
  return host_inputs.BatchedReplayWeather(CSV, np.arange(B) * 40.0, 100.0)


def sinusoid_starts(seed=SEED, first_building=0):
  return EpisodeStarts(offsets=UniformInt(132, MAX_OFFSET, step=4), weather_low=Uniform(268.0, 280.0),
                       weather_high=Uniform(282.0, 300.0), seed=seed, first_building=first_building)


REPLAY_OFFSETS = (0, 30, 60, 85)
REPLAY_SHIFTS = (0.0, 300.0, 900.0, 1380.0)


def replay_starts(seed=SEED, first_building=0):
  return EpisodeStarts(offsets=Choice(list(REPLAY_OFFSETS)), weather_shift=Choice(list(REPLAY_SHIFTS)), seed=seed,
                       first_building=first_building)


def case(name, B):
  """-> (weather factory, starts, start time stamp, largest offset) of the sinusoid or the replay case."""
  if name == "sinusoid":
    return (lambda: sinusoid_weather(B)), sinusoid_starts(), START, MAX_OFFSET
  return (lambda: replay_weather(B)), replay_starts(), START_TRACE, max(REPLAY_OFFSETS)


def base_values(weather, B, base_offsets=None):
  """The values in force without starts, by name (what ``in_force`` falls back to)."""
  out = {"offsets": np.zeros(B, dtype=np.int64) if base_offsets is None else np.asarray(base_offsets, dtype=np.int64)}
  if isinstance(weather, host_inputs.BatchedSinusoidWeather):
    out["weather_low"], out["weather_high"] = weather.low.copy(), weather.high.copy()
  if isinstance(weather, host_inputs.BatchedReplayWeather):
    out["weather_shift"] = weather.offsets_sec.copy()
  return out


def in_force(es, base, episodes, buildings=None):
  """The values by name after the given history: building b holds ``values(b, episodes[b])``, its base values where
  episodes[b] < 0 (never drawn).  ``buildings``: only these are computed (the others stay at their base)."""
  out = {k: np.array(v) for k, v in base.items()}
  for b in (range(len(episodes)) if buildings is None else buildings):
    if episodes[b] < 0:
      continue
    for name, v in es.values(b, int(episodes[b]), base["offsets"]).items():
      out[name][b] = v
  return out


def models(weather, zone_names=("z",)):
  from sbsim_amd.environment import SimConfig   # (imports torch: this module must load without it)
  return host_inputs.StepModels(weather, SimConfig.sb1().schedule(),
                                host_inputs.StepFunctionOccupancy(dt.timedelta(hours=9), dt.timedelta(hours=17), 10.0, 0.1,
                                                                  holiday_calendar=None),
                                host_inputs.ElectricityEnergyCost(holiday_calendar=None), host_inputs.NaturalGasEnergyCost(),
                                DT, tuple(zone_names), 0.0)


def crosses(timeline, offsets, building, steps):
  """``calendar_cases.crosses_comfort`` for a building that starts at ``offsets[building]`` of ``timeline``."""
  return cc.crosses_comfort(types.SimpleNamespace(offsets=np.asarray(offsets), rows=timeline.rows), building, steps)


def same_bits(a, b):
  return rc.same_bits(a, b)
