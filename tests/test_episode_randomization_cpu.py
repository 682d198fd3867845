"""Episode randomisation without a device: the draw of csrc/episode_draw.h (compiled for the host into a small program)
against its NumPy restatement ``EpisodeRandomization.values``, bit for bit; pinned draws; ranges and independence of the
field list; the refusals of host_inputs and of BatchedEnvironment, raised before anything is created."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from sbsim_amd import _ffi, environment, host_inputs
from sbsim_amd.environment import BatchedEnvironment
from sbsim_amd.host_inputs import BuildingMaterials, BuildingParams, Choice, EpisodeRandomization, Uniform
from tests import randomization_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: one draw per line -- seed gb e id kind scale lo hi base K t0 t1 (choice table v[j] = t0 + j * t1); stdout: the
# value's bits
PROGRAM = textwrap.dedent("""
    #include <cinttypes>
    #include <cstdio>
    #include <cstring>
    #include <vector>
    #include "episode_draw.h"
    int main() {
      unsigned long long seed, gb;
      unsigned e;
      int id, kind, scale, K;
      double lo, hi, base, t0, t1;
      while (std::scanf("%llu %llu %u %d %d %d %la %la %la %d %la %la", &seed, &gb, &e, &id, &kind, &scale, &lo, &hi, &base, &K, &t0, &t1) == 12) {
        std::vector<double> v((size_t)K + 3);
        for (int j = 0; j < K; ++j) v[3 + j] = t0 + (double)j * t1;
        sb::RandField f{id, 0, 0, kind, scale, 3, K, 0, lo, hi};
        const double x = sb::rand_value(f, sb::rand_draw(f, v.data(), seed, gb, e), base);
        uint64_t bits;
        std::memcpy(&bits, &x, 8);
        std::printf("%016" PRIx64 "\\n", bits);
      }
      return 0;
    }
""")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
  d = tmp_path_factory.mktemp("randomize")
  src, exe = os.path.join(d, "draw.cpp"), os.path.join(d, "draw")
  open(src, "w").write(PROGRAM)
  subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "sbsim_amd", "csrc"),
                  "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
  return exe


def _run(program, tuples):
  text = "".join(f"{s} {gb} {e} {i} {k} {sc} {float(lo).hex()} {float(hi).hex()} {float(base).hex()} {K} {float(t0).hex()} {float(t1).hex()}\n"
                 for s, gb, e, i, k, sc, lo, hi, base, K, t0, t1 in tuples)
  out = subprocess.run([program], input=text, check=True, capture_output=True, text=True).stdout.split()
  assert len(out) == len(tuples)
  return np.array([int(x, 16) for x in out], dtype=np.uint64).view(np.float64)


def _restated(t):
  """The tuple's value through EpisodeRandomization.values: the field whose number is the tuple's id."""
  s, gb, e, ident, kind, scale, lo, hi, base, K, t0, t1 = t
  dist = Choice([t0 + float(j) * t1 for j in range(K)], scale=bool(scale)) if kind else Uniform(lo, hi, scale=bool(scale))
  if ident < host_inputs.RAND_MATERIAL:
    name = next(n for n, c in host_inputs.BUILDING_PARAM_NAMES.items() if _ffi.BUILDING_PARAM_FIELDS[ident] in c)
    edge = host_inputs.BUILDING_PARAM_NAMES[name].index(_ffi.BUILDING_PARAM_FIELDS[ident])
    window = len(host_inputs.BUILDING_PARAM_NAMES[name]) == 2
    other = Uniform(0.0, 0.0)
    er = EpisodeRandomization(params={name: ((dist, other) if edge == 0 else (other, dist)) if window else dist}, seed=s, first_building=gb)
    got = er.values(0, e, {name: np.full((1, 2) if window else (1,), base)})[name]
    return float(got[edge]) if window else float(got)
  M = 255
  f = ident - host_inputs.RAND_MATERIAL
  base_rows = {k: np.full((1, M), base) for k in rc.KINDS}
  base_rows["convection_coefficient"] = np.full(1, base)
  if f == 3 * M:
    er = EpisodeRandomization(materials={"convection_coefficient": dist}, seed=s, first_building=gb)
    return float(er.values(0, e, base_rows)["convection_coefficient"])
  er = EpisodeRandomization(materials={rc.KINDS[f // M]: {f % M: dist}}, seed=s, first_building=gb)
  return float(er.values(0, e, base_rows)[rc.KINDS[f // M]][f % M])


def _tuples():
  rng = np.random.RandomState(11)
  largest = host_inputs.RAND_MATERIAL + 3 * 255   # the convection coefficient of a plan of 255 slots
  ids = list(range(_ffi.SB_NUM_BUILDING_PARAMS)) + [host_inputs.RAND_MATERIAL + f for f in (0, 1, 254, 255, 600, 764)] + [largest]
  out = []
  for n in range(300):
    seed = int(rng.randint(0, 1 << 32)) << 32 | int(rng.randint(0, 1 << 32))
    gb = int(rng.randint(0, 1 << 20)) if n % 3 else (1 << 32) + int(rng.randint(0, 1 << 31)) * 7
    e = 0 if n % 5 == 0 else int(rng.randint(0, 1 << 31))
    ident = ids[n % len(ids)]
    kind, scale = n % 2, (n // 2) % 2
    lo = float(rng.uniform(-5, 5))
    hi = lo if n % 7 == 0 else lo + float(rng.uniform(0, 50))
    K = 1 if n % 11 == 1 else 65536 if n % 11 == 3 else int(rng.randint(2, 40))
    out.append((seed, gb, e, ident, kind, scale, lo, hi, float(rng.uniform(0.5, 300.0)), K, float(rng.uniform(0.1, 9)), float(rng.uniform(0.01, 2))))
  out.append(((1 << 64) - 1, (1 << 40) + 5, 0, largest, 1, 1, 0.0, 0.0, 3.25, 65536, 0.5, 0.125))
  out.append((0, 1 << 32, 0, largest, 0, 0, 2.5, 2.5, 1.0, 1, 0.0, 0.0))
  return out


def test_the_device_draw_is_the_numpy_restatement_bit_for_bit(program):
  tuples = _tuples()
  assert any(t[1] >= 1 << 32 for t in tuples) and any(t[2] == 0 for t in tuples)
  assert any(t[4] == 1 and t[9] == 1 for t in tuples) and any(t[4] == 1 and t[9] == 65536 for t in tuples)
  assert any(t[4] == 0 and t[6] == t[7] for t in tuples) and any(t[3] == host_inputs.RAND_MATERIAL + 765 for t in tuples)
  got = _run(program, tuples)
  want = np.array([_restated(t) for t in tuples])
  bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
  assert bad.size == 0, [(tuples[i], got[i], want[i]) for i in bad[:3]]


# (seed, global building, episode, id, kind, scale, lo, hi, base, K, t0, t1) -> the value's bits, computed once by the program
PINNED = [
    ((7, 0, 0, 6, 0, 0, 0.7, 0.95, 1.0, 1, 0.0, 0.0), 0x3FEAC765FA2F13C6),
    ((7, (1 << 32) + 3, 2, 0, 0, 1, 0.8, 1.2, 0.04, 1, 0.0, 0.0), 0x3FA235E8C39B52FE),
    ((12345678901234567890, 41, 9, 0x100 + 12, 1, 0, 0.0, 0.0, 1.0, 5, 20.0, 15.0), 0x4041800000000000),
]


def test_pinned_draws(program):
  got = _run(program, [t for t, _ in PINNED]).view(np.uint64)
  assert [int(x) for x in got] == [bits for _, bits in PINNED], [hex(int(x)) for x in got]
  assert [np.float64(_restated(t)).view(np.uint64) for t, _ in PINNED] == [bits for _, bits in PINNED]


def test_ranges_and_independence_of_the_field_list():
  er = EpisodeRandomization(params={"ahu_fan_efficiency": Uniform(0.7, 0.95), "max_electricity_rate": Choice([1.0, 2.0, 3.0, 4.0, 5.0])},
                            seed=99)
  seen = set()
  for n in range(2000):
    v = er.values(n % 50, n // 50)
    assert 0.7 <= v["ahu_fan_efficiency"] <= 0.95
    seen.add(v["max_electricity_rate"])
    f = er.fields[1]
    c0 = host_inputs._philox_block(((n % 50), 0, n // 50, host_inputs.RANDOMIZATION_TAG | f.ident(None)), (99, 0))[0]
    assert 0 <= (c0 * 5) >> 32 < 5
  assert seen == {1.0, 2.0, 3.0, 4.0, 5.0}
  # other fields, another order: the draw of a field stays
  more = EpisodeRandomization(params=[("boiler_reheat_water_setpoint", Uniform(330.0, 360.0)),
                                      ("max_electricity_rate", Choice([1.0, 2.0, 3.0, 4.0, 5.0])),
                                      ("comfort_temp_window", Uniform((293.0, 296.5), (295.0, 299.0))),
                                      ("ahu_fan_efficiency", Uniform(0.7, 0.95))],
                              materials={"convection_coefficient": Uniform(6.0, 25.0)}, seed=99)
  for b, e in ((0, 0), (3, 1), (17, 40)):
    a, m = er.values(b, e), more.values(b, e, n_slots=3)
    assert a["ahu_fan_efficiency"] == m["ahu_fan_efficiency"] and a["max_electricity_rate"] == m["max_electricity_rate"]
  # a shard draws what the whole batch drew
  assert er.rows(3).values(2, 4) == er.values(5, 4)
  assert er.digest() != more.digest() and er.digest() == EpisodeRandomization(
      params={"max_electricity_rate": Choice([1.0, 2.0, 3.0, 4.0, 5.0]), "ahu_fan_efficiency": Uniform(0.7, 0.95)}, seed=99).digest()


def test_the_tag_collides_with_no_other_generator():
  assert host_inputs.RANDOMIZATION_TAG == _ffi.SB_RANDOMIZATION_TAG and host_inputs.RAND_MATERIAL == _ffi.SB_RAND_MATERIAL
  text = open(os.path.join(ROOT, "include", "sbsim_amd.h")).read()
  assert f"#define SB_RANDOMIZATION_TAG 0x{_ffi.SB_RANDOMIZATION_TAG:08X}u" in text
  lo, hi = _ffi.SB_RANDOMIZATION_TAG, _ffi.SB_RANDOMIZATION_TAG | (_ffi.SB_RAND_MATERIAL + 3 * 255)
  assert not lo <= _ffi.SB_INITIAL_CONDITIONS_TAG <= hi      # the start temperatures' one word
  assert lo > (0x80000000 | 0xFFFF) and lo > 1 << 21          # the convection shuffles' rooms and grid cells
  assert lo // 8 > 400_000_000                                # the occupancy generator: query * 8 + block
  assert set(_ffi.RANDOMIZATION_ENTRIES) <= set(_ffi.EXPORTS)


REFUSED = [   # (params, materials, extra arguments, what the message names)
    ({"ahu_fan_efficiencyy": Uniform(0.7, 0.9)}, None, {}, "ahu_fan_efficiencyy"),
    ({"time_step_sec": Uniform(100.0, 300.0)}, None, {}, "time_step_sec"),
    ([("ahu_fan_efficiency", Uniform(0.7, 0.9)), ("ahu_fan_efficiency", Uniform(0.7, 0.8))], None, {}, "ahu_fan_efficiency"),
    (None, {"conductivity": [(0, Uniform(1.0, 2.0)), (0, Uniform(1.0, 3.0))]}, {}, "conductivity[0]"),
    (None, {"thickness": {0: Uniform(1.0, 2.0)}}, {}, "thickness"),
    ({"ahu_fan_efficiency": Uniform(0.9, 0.7)}, None, {}, "ahu_fan_efficiency"),
    ({"ahu_fan_efficiency": Uniform(0.7, float("inf"))}, None, {}, "ahu_fan_efficiency"),
    ({"ahu_fan_efficiency": Uniform(float("nan"), 0.9)}, None, {}, "ahu_fan_efficiency"),
    ({"ahu_fan_efficiency": Choice([0.7, float("nan")])}, None, {}, "ahu_fan_efficiency"),
    ({"ahu_fan_efficiency": Choice([])}, None, {}, "ahu_fan_efficiency"),
    ({"ahu_fan_efficiency": Choice(np.linspace(0.5, 0.9, 65537))}, None, {}, "ahu_fan_efficiency"),
    ({"comfort_temp_window": Uniform(293.0, 295.0)}, None, {}, "comfort_temp_window"),
    ({"ahu_fan_efficiency": Uniform(0.7, 0.9)}, None, dict(seed=1 << 64), "seed"),
    ({"ahu_fan_efficiency": Uniform(0.7, 0.9)}, None, dict(seed=-1), "seed"),
    ({"ahu_fan_efficiency": Uniform(0.7, 0.9)}, None, dict(first_building=-1), "first_building"),
    (None, None, {}, "at least one field"),
]


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_a_randomisation_that_cannot_be_is_refused_naming_the_field(case):
  params, materials, kw, names = REFUSED[case]
  with pytest.raises(ValueError, match=names.replace("[", r"\[").replace("]", r"\]")):
    EpisodeRandomization(params=params, materials=materials, **kw)


def _nothing_is_created(monkeypatch):
  def boom(*a, **k):
    raise AssertionError("a simulator was created")
  monkeypatch.setattr(environment.BatchedSimulator, "__init__", boom)


B = 5
CHECKED = [   # (params, materials, environment arguments, the field, the building or None)
    (None, {"conductivity": {0: Uniform(1.0, 2.0)}}, {}, "conductivity[0]", None),                           # no materials handle
    (None, {"convection_coefficient": Uniform(6.0, 25.0)}, dict(solver="jacobi_fp32"), "convection_coefficient", None),
    (None, {"density": {3: Uniform(1.0, 2.0)}}, dict(materials=True), "density[3]", None),                   # the plan has 3 slots
    ({"ahu_fan_efficiency": Uniform(0.0, 0.9)}, None, {}, "ahu_fan_efficiency", 0),                           # a positive field at 0
    ({"vav_max_air_flow_rate": Uniform(-1.0, 1.0, scale=True)}, None, {}, "vav_max_air_flow_rate", 0),
    (None, {"heat_capacity": {1: Choice([1.0, 0.0])}}, dict(materials=True), "heat_capacity[1]", 0),
    (None, {"convection_coefficient": Uniform(-0.5, 5.0)}, dict(materials=True), "convection_coefficient", 0),
    ({"ahu_heating_air_temp_setpoint": Uniform(285.0, 299.0)}, None, {}, "ahu_heating_air_temp_setpoint", 0),  # the cooling setpoint: 298
    ({"ahu_cooling_air_temp_setpoint": Uniform(0.99, 1.1, scale=True)}, None, dict(cool=True), "ahu_cooling_air_temp_setpoint", 3),
    ({"comfort_temp_window": Uniform((293.0, 294.0), (295.0, 299.0))}, None, {}, "comfort_temp_window", 0),
    ({"eco_temp_window": (Uniform(280.0, 400.0), Uniform(1.0, 1.0, scale=True))}, None, {}, "eco_temp_window", 0),
    ({"productivity_weight": Uniform(-3.0, 1.0)}, None, {}, "productivity_weight", 0),
    ({"max_electricity_rate": Uniform(1e308, 1.7e308, scale=True)}, None, {}, "max_electricity_rate", 0),     # not finite
]


def _env(params, materials, extra, plan=None):
  plan = plan or rc.plan_small()
  kw = {k: v for k, v in extra.items() if k not in ("materials", "cool")}
  if extra.get("materials"):
    kw["building_materials"] = rc.building_materials(plan, B)
  if extra.get("cool"):   # building 3's heating setpoint sits above its own cooling setpoint's lowest draw
    kw["building_params"] = BuildingParams(ahu_cooling_air_temp_setpoint=np.array([298.0, 298.0, 298.0, 285.5, 298.0]),
                                           ahu_heating_air_temp_setpoint=np.full(B, 285.0))
  er = EpisodeRandomization(params=params, materials=materials, seed=3)
  return BatchedEnvironment(plan, B, episode_randomization=er, **kw)


@pytest.mark.parametrize("case", range(len(CHECKED)))
def test_what_the_batch_refuses_raises_before_anything_is_created(case, monkeypatch):
  params, materials, extra, field, building = CHECKED[case]
  _nothing_is_created(monkeypatch)
  with pytest.raises(ValueError) as e:
    _env(params, materials, extra)
  msg = str(e.value)
  assert field in msg, msg
  assert building is None or f"building {building}:" in msg, msg


def test_the_worst_case_of_the_setpoint_pair(monkeypatch):
  """ahu_heating_air_temp_setpoint = Uniform(285, 299) against the SimConfig's cooling setpoint of 298 is refused,
  Uniform(285, 297.9) is accepted (the check passes: the simulator's constructor is reached)."""
  assert rc.config().ahu_cooling_air_temp_setpoint == 298.0
  _nothing_is_created(monkeypatch)
  with pytest.raises(ValueError, match="ahu_heating_air_temp_setpoint"):
    _env({"ahu_heating_air_temp_setpoint": Uniform(285.0, 299.0)}, None, {})
  with pytest.raises(AssertionError, match="a simulator was created"):
    _env({"ahu_heating_air_temp_setpoint": Uniform(285.0, 297.9)}, None, {})
  EpisodeRandomization(params={"ahu_heating_air_temp_setpoint": Uniform(285.0, 297.9)}).check(B, rc.base_rows(B), None)


def test_an_argument_of_the_wrong_type_is_refused(monkeypatch):
  _nothing_is_created(monkeypatch)
  with pytest.raises(ValueError, match="EpisodeRandomization"):
    BatchedEnvironment(rc.plan_small(), B, episode_randomization={"ahu_fan_efficiency": Uniform(0.7, 0.9)})
