"""Episode starts without a device: the draw of csrc/episode_draw.h (compiled for the host into a small program) against
its restatement ``EpisodeStarts.values``, bit for bit; pinned draws; UniformInt's range; independence of the field list and
of the shard; that the seeds of the GPU tests can show a failure; the Timeline's size and trace check; the refusals of
host_inputs and of BatchedEnvironment, raised before anything is created."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from sbsim_amd import _ffi, environment, host_inputs
from sbsim_amd.environment import BatchedEnvironment, MixedBatchedEnvironment
from sbsim_amd.host_inputs import Choice, EpisodeStarts, Timeline, Uniform, UniformInt
from tests import episode_starts_cases as ec
from tests import randomization_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: one draw per line -- seed gb e id kind lo hi step K t0 t1 (choice table v[j] = t0 + j * t1); stdout: the draw's
# bits (the offset's as a double)
PROGRAM = textwrap.dedent("""
    #include <cinttypes>
    #include <cstdio>
    #include <cstring>
    #include <vector>
    #include "episode_draw.h"
    int main() {
      unsigned long long seed, gb;
      unsigned e;
      int id, kind, step, K;
      double lo, hi, t0, t1;
      while (std::scanf("%llu %llu %u %d %d %la %la %d %d %la %la", &seed, &gb, &e, &id, &kind, &lo, &hi, &step, &K, &t0, &t1) == 11) {
        std::vector<double> v((size_t)K + 3);
        for (int j = 0; j < K; ++j) v[3 + j] = t0 + (double)j * t1;
        sb::StartField f{};
        f.d = sb::RandField{id, 0, 0, kind, 0, 3, K, 0, lo, hi};
        f.present = 1; f.ilo = (int)lo; f.step = step; f.k = kind == SB_RAND_UNIFORM_INT ? ((int)hi - (int)lo) / step + 1 : 0;
        const double x = id == SB_START_OFFSET ? (double)sb::start_offset_draw(f, v.data(), seed, gb, e) : sb::start_draw(f, v.data(), seed, gb, e);
        uint64_t bits;
        std::memcpy(&bits, &x, 8);
        std::printf("%016" PRIx64 "\\n", bits);
      }
      return 0;
    }
""")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
  d = tmp_path_factory.mktemp("episode_starts")
  src, exe = os.path.join(d, "draw.cpp"), os.path.join(d, "draw")
  open(src, "w").write(PROGRAM)
  subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "sbsim_amd", "csrc"),
                  "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
  return exe


def _restated(t):
  seed, gb, e, ident, kind, lo, hi, step, K, t0, t1 = t
  table = [t0 + float(j) * t1 for j in range(K)]
  dist = UniformInt(int(lo), int(hi), step) if kind == 2 else Choice(table) if kind == 1 else Uniform(lo, hi)
  name = host_inputs.START_FIELDS[ident]
  kw = {("offsets" if ident == 0 else name): dist}
  return float(EpisodeStarts(seed=seed, first_building=gb, **kw).values(0, e)[name])


def test_the_host_build_of_the_draw_equals_the_restatement(program):
  rng = np.random.RandomState(3)
  tuples = []
  for _ in range(60):
    seed = int(rng.randint(0, 2 ** 62)) * 4 + int(rng.randint(0, 4))
    gb = int(rng.choice([0, 1, 69, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 17]))
    e = int(rng.choice([0, 1, 2, 1000, 2 ** 31, 2 ** 32 - 1]))
    tuples.append((seed, gb, e, 0, 2, 0.0, float(364 * 288), 288, 1, 0.0, 0.0))
    tuples.append((seed, gb, e, 0, 2, 0.0, float((1 << 22) - 1), 1, 1, 0.0, 0.0))      # K == 2^22
    tuples.append((seed, gb, e, 0, 1, 0.0, 0.0, 1, 7, 3.0, 11.0))
    tuples.append((seed, gb, e, 1, 0, 268.0, 285.0, 1, 1, 0.0, 0.0))
    tuples.append((seed, gb, e, 2, 1, 0.0, 0.0, 1, 65536, 286.0, 0.001))
    tuples.append((seed, gb, e, 3, 0, -3600.0, 86400.0 * 7, 1, 1, 0.0, 0.0))
  text = "".join(f"{s} {gb} {e} {i} {k} {float(lo).hex()} {float(hi).hex()} {st} {K} {float(t0).hex()} {float(t1).hex()}\n"
                 for s, gb, e, i, k, lo, hi, st, K, t0, t1 in tuples)
  out = subprocess.run([program], input=text, check=True, capture_output=True, text=True).stdout.split()
  got = np.array([int(x, 16) for x in out], dtype=np.uint64).view(np.float64)
  want = np.array([_restated(t) for t in tuples])
  assert len(got) == len(tuples) and ec.same_bits(got, want)


# ---------------------------------------------------------------- 1. the restatement
def test_known_answers():
  kw = dict(offsets=UniformInt(0, 364 * 288, step=288), weather_low=Uniform(268.0, 285.0), weather_high=Uniform(286.0, 305.0))
  pinned = {(11, 0, 0): (8064, "0x1.1706ba3797c8ap+8", "0x1.25b1adb2bfc9fp+8"),
            (11, 3, 2): (98784, "0x1.1a47688952c40p+8", "0x1.1f0974d9ca49cp+8"),
            ((1 << 40) + 5, (1 << 33) + 7, 4000000000): (45216, "0x1.0e47184897fd7p+8", "0x1.264a492bf0163p+8")}
  table = {(11, 0, 0): (5, 604800.0), (11, 3, 2): (4000, 604800.0), ((1 << 40) + 5, (1 << 33) + 7, 4000000000): (17, -3600.0)}
  for (seed, gb, e), (off, low, high) in pinned.items():
    v = EpisodeStarts(seed=seed, first_building=gb, **kw).values(0, e)
    assert (v["offsets"], float(v["weather_low"]).hex(), float(v["weather_high"]).hex()) == (off, low, high)
    assert isinstance(v["offsets"], int) and v["offsets"] % 288 == 0
    c = EpisodeStarts(offsets=Choice([5, 17, 4000]), weather_shift=Choice([0.0, 86400.0 * 7, -3600.0]), seed=seed,
                      first_building=gb).values(0, e)
    assert (c["offsets"], c["weather_shift"]) == table[(seed, gb, e)]
  # the counter words: the tag lies outside every other generator's
  assert host_inputs.EPISODE_STARTS_TAG == _ffi.SB_EPISODE_STARTS_TAG == 0xE5A70000
  others = [(host_inputs.RANDOMIZATION_TAG, host_inputs.RANDOMIZATION_TAG | 0x3FD), (host_inputs.INITIAL_CONDITIONS_TAG,) * 2,
            (0x80000000, 0x8000FFFF), (0, (1 << 21) - 1)]
  assert all(not lo <= host_inputs.EPISODE_STARTS_TAG | i <= hi for lo, hi in others for i in range(4))


def test_uniform_int_covers_both_ends_and_nothing_else():
  es = EpisodeStarts(offsets=UniformInt(3, 24, step=7), seed=5)     # 3, 10, 17, 24
  draws = [es.values(b, e)["offsets"] for b in range(64) for e in range(64)]
  assert len(draws) == 4096 and set(draws) == {3, 10, 17, 24}
  odd = EpisodeStarts(offsets=UniformInt(3, 23, step=7), seed=5)    # hi is no member: 3, 10, 17
  assert {odd.values(b, 0)["offsets"] for b in range(4096)} == {3, 10, 17}
  assert odd.largest_offsets(np.zeros(2, int)).tolist() == [17, 17]
  one = EpisodeStarts(offsets=UniformInt(9, 9), seed=5)
  assert {one.values(b, 1)["offsets"] for b in range(64)} == {9}
  rel = EpisodeStarts(offsets=UniformInt(0, 4), relative=True, seed=5)
  base = np.array([100, 200, 300])
  assert all(rel.values(b, 2, base)["offsets"] == base[b] + rel.values(b, 2)["offsets"] for b in range(3))
  assert rel.largest_offsets(base).tolist() == [104, 204, 304] and rel.smallest_offsets(base).tolist() == [100, 200, 300]


def test_a_draw_depends_on_seed_building_episode_and_field_alone():
  full = ec.sinusoid_starts(seed=9)
  for name, dist in (("offsets", UniformInt(132, 148, step=4)), ("weather_low", Uniform(268.0, 280.0)), ("weather_high", Uniform(282.0, 300.0))):
    alone = EpisodeStarts(seed=9, **{name: dist})
    assert all(alone.values(b, e)[name] == full.values(b, e)[name] for b in range(6) for e in range(3))
  shard = full.rows(4)
  assert shard.first_building == 4 and full.first_building == 0
  assert all(shard.values(b, e) == full.values(b + 4, e) for b in range(3) for e in range(3))
  assert full.values(0, 0) != full.values(0, 1) and full.values(0, 0) != full.values(1, 0)
  assert ec.sinusoid_starts(seed=10).values(0, 0) != full.values(0, 0)
  assert full.digest() != shard.digest() and full.digest() == ec.sinusoid_starts(seed=9).digest()


# ---------------------------------------------------------------- 2. inputs that can show a failure
@pytest.mark.parametrize("name", ["sinusoid", "replay"])
def test_the_gpu_tests_seeds_draw_distinct_offsets_and_cross_a_comfort_switch(name):
  B = len(ec.LENGTHS)
  weather, es, start, top = ec.case(name, B)
  offs = np.array([[es.values(b, e)["offsets"] for b in range(B)] for e in range(3)])
  assert len(set(offs.ravel().tolist())) >= 3 and offs.max() <= top
  if name == "replay":
    shifts = {es.values(b, e)["weather_shift"] for b in range(B) for e in range(3)}
    assert len(shifts) >= 3
    return
  tl = Timeline(ec.models(weather()), start, np.zeros(B, int), ec.EPISODE_ROWS, episode_starts=es)
  cross = np.array([[ec.crosses(tl, offs[e], b, int(ec.LENGTHS[b]) + 1) for b in range(B)] for e in range(3)])
  assert any(cross[:, b].any() and not cross[:, b].all() for b in range(B)), cross


# ---------------------------------------------------------------- 3. the Timeline
def test_the_timeline_is_sized_for_the_largest_draw():
  B = 3
  m = ec.models(ec.sinusoid_weather(B))
  plain = Timeline(m, ec.START, [0, 5, 9], 16)
  assert plain.n_rows == 9 + 16 + 2
  es = EpisodeStarts(offsets=UniformInt(10, 41, step=10), seed=1)      # 10, 20, 30, 40
  assert Timeline(m, ec.START, [0, 5, 9], 16, episode_starts=es).n_rows == 40 + 16 + 2
  assert Timeline(m, ec.START, [0, 5, 90], 16, episode_starts=es).n_rows == 90 + 16 + 2      # an attached offset beyond every draw
  rel = EpisodeStarts(offsets=Choice([0, 7, 3]), relative=True, seed=1)
  tl = Timeline(m, ec.START, [0, 5, 9], 16, episode_starts=rel)
  assert tl.n_rows == 9 + 7 + 16 + 2
  assert ec.same_bits(tl.rows[:plain.n_rows], plain.rows)
  assert Timeline(m, ec.START, [0, 5, 9], 16, max_offset=50).n_rows == 50 + 16 + 2
  weather_only = EpisodeStarts(weather_low=Uniform(260.0, 265.0), seed=1)
  assert Timeline(m, ec.START, [0, 5, 9], 16, episode_starts=weather_only).n_rows == plain.n_rows
  with pytest.raises(ValueError, match="offsets: the timeline would have .* rows, more than 2\\^22"):
    Timeline(m, ec.START, [0, 0, 0], 16, episode_starts=EpisodeStarts(offsets=UniformInt(0, (1 << 22) - 10), seed=1))


def test_the_replay_trace_is_checked_over_the_worst_draw():
  B = 4
  m = ec.models(ec.replay_weather(B))
  tl = Timeline(m, ec.START_TRACE, np.zeros(B, int), 16, episode_starts=ec.replay_starts())
  assert tl.n_rows == 85 + 16 + 2
  # ten hours are 120 rows: an offset of 100 ends at row 117, and a shift of 1,380 s carries it past the trace's end
  late = EpisodeStarts(offsets=Choice([0, 100]), weather_shift=Choice([0.0, 1380.0]), seed=1)
  with pytest.raises(ValueError, match="episode_starts: building 0: with offset 100 and weather shift 1380.0 s drawn, its episode ends at .* after the weather trace's last time stamp"):
    Timeline(m, ec.START_TRACE, np.zeros(B, int), 16, episode_starts=late)
  Timeline(m, ec.START_TRACE, np.zeros(B, int), 16, episode_starts=EpisodeStarts(offsets=Choice([0, 100]), seed=1))   # (without the shift: inside)
  early = EpisodeStarts(weather_shift=Choice([0.0, -60.0]), seed=1)
  with pytest.raises(ValueError, match="episode_starts: building 0: with offset 0 and weather shift -60.0 s drawn, its episode starts before"):
    Timeline(m, ec.START_TRACE, np.zeros(B, int), 16, episode_starts=early)
  rel = EpisodeStarts(offsets=Choice([0, 20]), relative=True, seed=1)
  with pytest.raises(ValueError, match="episode_starts: building 2: with offset 110"):
    Timeline(m, ec.START_TRACE, [0, 0, 90, 0], 16, episode_starts=rel)


def test_new_starts_are_checked_against_the_table_there_is():
  """Timeline.check_starts: what BatchedEnvironment.set_episode_starts asks before it attaches."""
  B = 4
  w = ec.replay_weather(B)
  tl = Timeline(ec.models(w), ec.START_TRACE, np.zeros(B, int), 16, episode_starts=ec.replay_starts())     # 85 + 16 + 2 rows
  tl.check_starts(ec.replay_starts(seed=5), w)
  tl.check_starts(EpisodeStarts(offsets=Choice([0, 85]), seed=1), w)
  with pytest.raises(ValueError, match="offsets: building 0: an episode that starts at the largest possible offset 86 needs 104 rows, the timeline has 103"):
    tl.check_starts(EpisodeStarts(offsets=Choice([0, 86]), seed=1), w)
  with pytest.raises(ValueError, match="offsets: building 2: an episode that starts at the largest possible offset 90 needs"):
    tl.check_starts(EpisodeStarts(offsets=Choice([0, 20]), relative=True, seed=1), w, base_offsets=[0, 0, 70, 0])
  # 85 + 17 rows end at 08:30; a shift of two hours carries the last query past the trace's ten hours
  with pytest.raises(ValueError, match="episode_starts: building 0: with offset 85 and weather shift 7200.0 s drawn, its episode ends at .* after the weather trace's last time stamp"):
    tl.check_starts(EpisodeStarts(offsets=Choice([0, 85]), weather_shift=Choice([0.0, 7200.0]), seed=1), w)
  with pytest.raises(ValueError, match="episode_starts: building 0: with offset 0 and weather shift -60.0 s drawn, its episode starts before"):
    tl.check_starts(EpisodeStarts(weather_shift=Choice([0.0, -60.0]), seed=1), w)
  # a sinusoid weather has no trace: the table's size alone
  ws = ec.sinusoid_weather(B)
  ts = Timeline(ec.models(ws), ec.START, np.zeros(B, int), 16, episode_starts=ec.sinusoid_starts())
  ts.check_starts(ec.sinusoid_starts(seed=2), ws)
  with pytest.raises(ValueError, match="largest possible offset 149"):
    ts.check_starts(EpisodeStarts(offsets=UniformInt(0, 149), seed=1), ws)


# ---------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("kw, message", [
    (dict(offsets=UniformInt(0.5, 4)), "offsets: UniformInt needs whole numbers"),
    (dict(offsets=UniformInt(-1, 4)), "offsets: negative offset -1"),
    (dict(offsets=UniformInt(5, 4)), "offsets: lo 5 > hi 4"),
    (dict(offsets=UniformInt(0, 4, step=0)), "offsets: step must be an integer >= 1"),
    (dict(offsets=UniformInt(0, 4, step=1.5)), "offsets: step must be an integer >= 1"),
    (dict(offsets=UniformInt(0, 1 << 22)), "offsets: K == 4194305 is more than 2\\^22"),
    (dict(offsets=UniformInt(0, (1 << 22) + 1)), "offsets: offset 4194305 is beyond the 2\\^22 rows"),
    (dict(offsets=Choice([0, 2.5])), "offsets: choice 1 must be a whole number"),
    (dict(offsets=Choice([0, -3])), "offsets: choice 1: negative offset"),
    (dict(offsets=Choice([0, 1 << 23])), "offsets: choice 1: offset 8388608 is beyond"),
    (dict(offsets=Choice([])), "offsets: a Choice needs 1 .. 65,536 values"),
    (dict(offsets=Uniform(0.0, 4.0)), "offsets: the distribution must be a UniformInt or a Choice of integer rows"),
    (dict(offsets=Choice([1, 2], scale=True)), "offsets: scale is not supported"),
    (dict(weather_low=UniformInt(1, 2)), "weather_low: the distribution must be a Uniform or a Choice"),
    (dict(weather_low=Uniform(280.0, 270.0)), "weather_low: lo 280.0 > hi 270.0"),
    (dict(weather_high=Uniform(280.0, float("inf"))), "weather_high: lo and hi must be finite"),
    (dict(weather_shift=Choice([0.0, float("nan")])), "weather_shift: choice 1 is not finite"),
    (dict(weather_low=Uniform(270.0, 290.0), weather_high=Choice([300.0, 285.0])), "weather_low: low can be drawn as 290.0, above a high of 285.0"),
    (dict(), "needs at least one field"),
    (dict(offsets=UniformInt(0, 4), seed=-1), "seed must be an integer"),
    (dict(offsets=UniformInt(0, 4), first_building=-1), "first_building must be an integer >= 0"),
])
def test_what_episode_starts_refuses_by_itself(kw, message):
  with pytest.raises(ValueError, match=message):
    EpisodeStarts(**kw)


def _no_simulator(monkeypatch):
  def boom(*a, **k):
    raise AssertionError("a BatchedSimulator was created")
  monkeypatch.setattr(environment, "BatchedSimulator", boom)


def test_what_the_environment_refuses_before_anything_is_created(monkeypatch):
  _no_simulator(monkeypatch)
  plan, B = rc.plan_small(), 4
  offs = EpisodeStarts(offsets=UniformInt(0, 8), seed=1)
  low = EpisodeStarts(weather_low=Uniform(260.0, 275.0), seed=1)
  shift = EpisodeStarts(weather_shift=Choice([0.0, 60.0]), seed=1)
  with pytest.raises(ValueError, match="episode_starts must be a host_inputs.EpisodeStarts"):
    BatchedEnvironment(plan, B, episode_starts=UniformInt(0, 8), **ec.SHORT)
  with pytest.raises(ValueError, match="weather_low: needs weather=BatchedSinusoidWeather"):
    BatchedEnvironment(plan, B, episode_starts=low, **ec.SHORT)
  with pytest.raises(ValueError, match="weather_low: needs weather=BatchedSinusoidWeather"):
    BatchedEnvironment(plan, B, episode_starts=low, weather=ec.replay_weather(B), start_timestamp=ec.START_TRACE, **ec.SHORT)
  with pytest.raises(ValueError, match="weather_shift: needs weather=BatchedReplayWeather"):
    BatchedEnvironment(plan, B, episode_starts=shift, weather=ec.sinusoid_weather(B), **ec.SHORT)
  # only one of the pair is drawn: against the building's own other entry (building 3's high is 294)
  with pytest.raises(ValueError, match="weather_low: building 0: low can be drawn as 279.0, above its high of 278.0"):
    BatchedEnvironment(plan, B, episode_starts=EpisodeStarts(weather_low=Uniform(260.0, 279.0), seed=1), weather=ec.sinusoid_weather(B), **ec.SHORT)
  with pytest.raises(ValueError, match="weather_high: building 3: high can be drawn as 279.0, below its low of 280.0"):
    BatchedEnvironment(plan, B, episode_starts=EpisodeStarts(weather_high=Uniform(279.0, 300.0), seed=1), weather=ec.sinusoid_weather(B), **ec.SHORT)
  from tests import calendar_cases as cc
  with pytest.raises(ValueError, match="offsets: episode_starts is not supported together with calendars"):
    BatchedEnvironment(plan, B, episode_starts=offs, calendars=cc.calendars(), calendar_of=np.arange(B) % 3, **ec.SHORT)
  with pytest.raises(ValueError, match="episode_starts is not implemented for MixedBatchedEnvironment"):
    MixedBatchedEnvironment([(plan, 2), (plan, 2)], episode_starts=offs, **ec.SHORT)
  with pytest.raises(ValueError, match="max_start_offset must be an integer >= 0"):
    BatchedEnvironment(plan, B, max_start_offset=-2, **ec.SHORT)


def test_episode_starts_entry_asks_for_a_rebuild_on_a_library_without_the_entries(monkeypatch):
  class Stub:   # a library of the same ABI version built before the entries existed
    def sb_reset(self):
      pass
  monkeypatch.setattr(_ffi, "_lib", Stub())
  for name in _ffi.EPISODE_STARTS_ENTRIES:
    with pytest.raises(_ffi.SbsimError, match=f"has no {name}: rebuild"):
      _ffi.episode_starts_entry(name)
  assert {"sb_episode_starts_attach", "sb_episode_starts_detach", "sb_episode_starts_episodes_get", "sb_episode_starts_episodes_set",
          "sb_episode_starts_values_get"} <= set(_ffi.EPISODE_STARTS_ENTRIES) <= set(_ffi.EXPORTS)


def test_null_arguments_are_refused_without_a_gpu():
  from sbsim_amd import build
  build.build()
  for name, args in (("sb_episode_starts_attach", (None,)), ("sb_episode_starts_detach", ()), ("sb_episode_starts_episodes_get", (None, None)),
                     ("sb_episode_starts_episodes_set", (None, None)), ("sb_episode_starts_values_get", (None, None, None)),
                     ("sb_clock_set_offsets", (None, None))):
    assert _ffi.episode_starts_entry(name)(None, *args) == -1, name
    assert b"null" in _ffi.load().sb_last_error()


def test_the_descriptor_matches_the_header():
  import ctypes as C
  import tempfile
  src = '#include <stdio.h>\n#include "sbsim_amd.h"\nint main(void) { printf("%zu %zu\\n", sizeof(sb_start_field), sizeof(sb_episode_starts)); return 0; }\n'
  with tempfile.TemporaryDirectory() as d:
    c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    sizes = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
  assert sizes == [C.sizeof(_ffi.StartField), C.sizeof(_ffi.EpisodeStartsDesc)]
  d, keep = ec.sinusoid_starts().c_desc(0x1000, 0)
  assert [f.present for f in d.field] == [1, 1, 1, 0] and d.field[0].kind == _ffi.SB_RAND_UNIFORM_INT and d.field[0].step == 4
  assert d.weather_lohi_dev == 0x1000 and d.weather_offset_dev is None and d.seed == ec.SEED
