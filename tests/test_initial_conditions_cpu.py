"""Start temperatures per building without a GPU: what host_inputs.InitialConditions refuses, its host restatement
`start_temps` against a line-by-line spelling, the draw (range, streams per building and episode, shards), Philox's known
answers, the symbols of the library -- and the reference's own FloorPlanBasedBuilding(reset_temp_values=grid) rollout
(tests/golden/reset_temp_values.npz, tools/gen_golden_reset_temps.py) against the oracle twin, bit for bit, with the
margins that make equal sweep counts a legitimate demand."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from oracle.occupancy_oracle import philox4x32_10
from sbsim_amd import _ffi, build, host_inputs
from sbsim_amd.host_inputs import Choice, EpisodeRandomization, EpisodeStarts, InitialConditions, Uniform, UniformInt
from tests import initial_conditions_cases as icc
from tests.golden_util import load
from tests.twins import oracle_twin

H, W, B = 5, 7, 6
GRID = 290.0 + np.arange(H * W, dtype=np.float64).reshape(H, W) * 0.125
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulp32(a, b):
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_field_and_the_building():
  bad = GRID.copy()
  bad[2, 3] = np.inf
  per = np.full(B, 294.0)
  nan_b = per.copy()
  nan_b[4] = np.nan
  cases = [
      (dict(reset_temp_values=np.zeros((0, H, W))), r"reset_temp_values: K == 0"),
      (dict(reset_temp_values=np.zeros(H * W)), r"reset_temp_values must have shape \[H, W\] or \[K, H, W\]"),
      (dict(reset_temp_values=np.stack([GRID, GRID])), r"2 grids: grid_of must say"),
      (dict(reset_temp_values=np.stack([GRID, GRID]), grid_of=[0, 1, 2, 0, 1, 0]), r"building 2: grid_of 2 is outside the 2 grids"),
      (dict(reset_temp_values=GRID, grid_of=[0, -1, 0, 0, 0, 0]), r"building 1: grid_of -1 is outside"),
      (dict(reset_temp_values=GRID, grid_of=[0.0] * B), r"grid_of must be an integer array"),
      (dict(grid_of=[0] * B), r"grid_of needs reset_temp_values"),
      (dict(reset_temp_values=GRID, initial_temp=per), r"initial_temp and reset_temp_values are two bases"),
      (dict(reset_temp_values=bad), r"reset_temp_values: grid 0 cell \(2, 3\) is not finite"),
      (dict(initial_temp=nan_b), r"building 4: initial_temp is not finite"),
      (dict(reset_temp_values=GRID, offset=nan_b), r"building 4: offset is not finite"),
      (dict(initial_temp=per.reshape(2, 3)), r"initial_temp must have shape \[B\]"),
      (dict(jitter=(1.0, 0.5, 3)), r"jitter: lo 1.0 > hi 0.5"),
      (dict(jitter=(0.0, np.inf, 3)), r"jitter: lo and hi must be finite"),
      (dict(jitter=(0.0, 1.0, 1 << 64)), r"jitter: seed must be an integer in \[0, 2\^64\)"),
      (dict(jitter=(0.0, 1.0, -1)), r"jitter: seed must be an integer"),
      (dict(jitter=(0.0, 1.0, 2.5)), r"jitter: seed must be an integer"),
      (dict(jitter=(0.0, 1.0)), r"jitter must be \(lo, hi, seed\)"),
      (dict(initial_temp=per, offset=np.zeros(B + 1)), r"different lengths: initial_temp 6, offset 7"),
      (dict(initial_temp=per, first_building=-1), r"first_building must be an integer >= 0"),
      (dict(), r"needs at least one field"),
  ]
  for kw, msg in cases:
    with pytest.raises(ValueError, match=msg):
      InitialConditions(**kw)
  # what needs the batch: the plan's shape and the batch's length
  with pytest.raises(ValueError, match=r"reset_temp_values: grids of shape \(5, 7\), the floor plan is \(7, 5\)"):
    InitialConditions(reset_temp_values=GRID).check(B, (W, H))
  with pytest.raises(ValueError, match=r"offset has 6 rows, the batch 7 buildings"):
    InitialConditions(offset=np.zeros(B)).check(B + 1, (H, W))
  with pytest.raises(ValueError, match=r"grid_of has 6 rows, the batch 5 buildings"):
    InitialConditions(reset_temp_values=GRID, grid_of=[0] * B).check(B - 1, (H, W))
  InitialConditions(reset_temp_values=GRID, jitter=(0.0, 1.0, (1 << 64) - 1)).check(1234, (H, W))   # no [B] array: any batch


def test_the_arrays_are_copies_and_read_only():
  g = GRID.copy()
  ic = InitialConditions(reset_temp_values=g, offset=np.zeros(B))
  g[0, 0] = 0.0
  assert ic.reset_temp_values.shape == (1, H, W) and ic.reset_temp_values[0, 0, 0] == GRID[0, 0]
  with pytest.raises(ValueError):
    ic.offset[0] = 1.0
  assert ic.n_grids == 1 and ic.n_buildings == B and ic.has_base
  assert not InitialConditions(jitter=(0.0, 1.0, 1)).has_base and InitialConditions(jitter=(0.0, 1.0, 1)).n_buildings is None


# ---------------------------------------------------------------- the formula
def _spelled(ic, b, e, initial_temp, shape):
  """The issue's formula, cell by cell, on Python floats; the draw through the oracle's Philox."""
  Hh, Ww = shape
  out = np.empty(shape)
  u = None
  if ic.jitter is not None:
    lo, hi, seed = ic.jitter
    gb = ic.first_building + b
    c = philox4x32_10(gb & 0xFFFFFFFF, gb >> 32, e & 0xFFFFFFFF, _ffi.SB_INITIAL_CONDITIONS_TAG, seed & 0xFFFFFFFF, seed >> 32)
    r = (int(c[1]) << 32) | int(c[0])
    u = lo + (hi - lo) * ((r >> 11) * 2.0 ** -53)
  for y in range(Hh):
    for x in range(Ww):
      if ic.reset_temp_values is not None:
        v = float(ic.reset_temp_values[0 if ic.grid_of is None else ic.grid_of[b], y, x])
      elif ic.initial_temp is not None:
        v = float(ic.initial_temp[b])
      else:
        v = float(initial_temp)
      if ic.offset is not None:
        v = v + float(ic.offset[b])
      if u is not None:
        v = v + u
      out[y, x] = v
  return out


@pytest.mark.parametrize("variant", icc.VARIANTS + ("offset-only", "one-grid"))
def test_start_temps_is_the_formula_line_by_line(variant):
  shape = (17, 29)
  if variant == "offset-only":
    ic = InitialConditions(offset=icc.offsets(), first_building=3)
  elif variant == "one-grid":
    ic = InitialConditions(reset_temp_values=icc.grids(shape)[1], jitter=(0.25, 0.25, 9), first_building=(1 << 32) + 5)
  else:
    ic = icc.conditions(variant, shape, first_building=11)
  for b in (0, 1, 63, 64, 66):
    for e in (0, 1, 7, (1 << 31) + 3):
      got = ic.start_temps(b, e, initial_temp=icc.INITIAL_TEMP, shape=shape)
      want = _spelled(ic, b, e, icc.INITIAL_TEMP, shape)
      assert got.shape == shape and got.dtype == np.float64
      assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (variant, b, e)
  if variant == "jitter":
    with pytest.raises(ValueError, match="needs the plan's shape"):
      ic.start_temps(0, 0, initial_temp=294.0)
    with pytest.raises(ValueError, match="needs the reset call's initial_temp"):
      ic.start_temps(0, 0, shape=shape)


def test_nothing_is_added_for_an_absent_field():
  g = GRID.copy()
  g[1, 1] = -0.0   # v + 0.0 would make it +0.0
  ic = InitialConditions(reset_temp_values=g)
  assert np.array_equal(ic.start_temps(0, 0).view(np.uint64), g.view(np.uint64))
  ic = InitialConditions(reset_temp_values=g, offset=np.zeros(2))
  assert np.signbit(g[1, 1]) and not np.signbit(ic.start_temps(0, 0)[1, 1])   # (a given field IS added)


# ---------------------------------------------------------------- the draw
def test_the_draw_lies_in_the_interval_and_a_point_interval_gives_the_point():
  ic = InitialConditions(jitter=(-0.75, 0.5, icc.SEED))
  u = np.array([[ic.draw(b, e) for e in range(40)] for b in range(200)])
  assert (u >= -0.75).all() and (u < 0.5).all()
  assert abs(u.mean() - (-0.125)) < 0.02 and u.min() < -0.74 and u.max() > 0.49   # (8000 uniform draws: sigma 0.004)
  for lo in (0.0, -3.25, 294.0, 1e-300):
    ic = InitialConditions(jitter=(lo, lo, 5))
    assert all(ic.draw(b, e) == lo for b in range(5) for e in range(5))


def test_the_draw_differs_per_building_and_per_episode():
  ic = InitialConditions(jitter=(0.0, 1.0, 42))
  u = np.array([[ic.draw(b, e) for e in range(16)] for b in range(67)])
  assert len(set(u.reshape(-1).tolist())) == u.size
  other = InitialConditions(jitter=(0.0, 1.0, 43))
  assert other.draw(0, 0) != ic.draw(0, 0)
  big = InitialConditions(jitter=(0.0, 1.0, 42), first_building=1 << 32)   # the high word of the global building counts
  assert big.draw(0, 0) != ic.draw(0, 0)


def test_the_draw_does_not_depend_on_the_sharding():
  shape = (17, 29)
  whole = icc.conditions("grids", shape, first_building=1000)
  for cuts in ((0, 67), (0, 1, 67), (0, 22, 45, 67), (0, 64, 66, 67)):
    for lo, hi in zip(cuts[:-1], cuts[1:]):
      shard = whole.rows(lo, hi)
      assert shard.first_building == 1000 + lo and shard.n_buildings == hi - lo
      for i in (0, hi - lo - 1):
        for e in (0, 3):
          assert np.array_equal(shard.start_temps(i, e), whole.start_temps(lo + i, e)), (lo, hi, i, e)
  with pytest.raises(ValueError, match="outside the conditions' 67 buildings"):
    whole.rows(60, 68)


# ---------------------------------------------------------------- Philox
def test_philox_known_answers():
  """Random123's known-answer vectors of philox4x32-10, through the oracle's restatement and the product's."""
  kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
  for ctr, key, want in kat:
    assert tuple(int(x) for x in philox4x32_10(*ctr, *key)) == want
    assert host_inputs._philox_block(ctr, key) == want
  rs = np.random.RandomState(1)
  for _ in range(50):
    ctr = tuple(int(x) for x in rs.randint(0, 1 << 32, size=4, dtype=np.uint64))
    key = tuple(int(x) for x in rs.randint(0, 1 << 32, size=2, dtype=np.uint64))
    assert host_inputs._philox_block(ctr, key) == tuple(int(x) for x in philox4x32_10(*ctr, *key))


def test_the_tag_keeps_the_counters_apart():
  """The other generators' last counter word under the same seed (generators.hip): the occupancy's query * 8 + block,
  the convection shuffle's grid cell (below 2^21) or 0x80000000 | 2 * room (+ 1)."""
  tag = _ffi.SB_INITIAL_CONDITIONS_TAG
  assert tag == host_inputs.INITIAL_CONDITIONS_TAG == 0xC1C00000
  assert tag >= 1 << 21 and not (0x80000000 <= tag < 0x80000000 + (1 << 17))
  assert tag // 8 > 400_000_000   # occupancy queries of one handle before its counters reach the tag
  text = open(os.path.join(ROOT, "include", "sbsim_amd.h")).read()
  assert "#define SB_INITIAL_CONDITIONS_TAG 0xC1C00000u" in text


# ---------------------------------------------------------------- the device's draw, built for the host
# stdin: one draw per line -- seed gb e lo hi; stdout: the bits of csrc/episode_draw.h's initial_conditions_draw
DRAW_PROGRAM = textwrap.dedent("""
    #include <cinttypes>
    #include <cstdio>
    #include <cstring>
    #include "episode_draw.h"
    int main() {
      unsigned long long seed, gb;
      unsigned e;
      double lo, hi;
      while (std::scanf("%llu %llu %u %la %la", &seed, &gb, &e, &lo, &hi) == 5) {
        const double u = sb::initial_conditions_draw(lo, hi, seed, gb, e);
        uint64_t bits;
        std::memcpy(&bits, &u, 8);
        std::printf("%016" PRIx64 "\\n", bits);
      }
      return 0;
    }
""")


def test_the_host_build_of_the_draw_equals_the_restatement_and_the_oracles_philox(tmp_path):
  """The one draw of the three that k_reset_ic / k_reset_jacobi_ic call, compiled by a plain C++ compiler with one
  rounding per operation, against ``InitialConditions.draw`` and against the formula on the oracle's Philox, bit for bit."""
  src, exe = os.path.join(tmp_path, "draw.cpp"), os.path.join(tmp_path, "draw")
  open(src, "w").write(DRAW_PROGRAM)
  subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "sbsim_amd", "csrc"),
                  "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
  seeds = (0, 1, 2 ** 32 - 1, 2 ** 32, 0x9E3779B97F4A7C15, 2 ** 63 + 5, 2 ** 64 - 1)
  buildings = (0, 1, 69, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 17)
  episodes = (0, 1, 2, 1000, 2 ** 31, 2 ** 32 - 1)
  intervals = ((-0.5, 0.5), (0.25, 0.25), (-3.0, -1.0 / 3.0), (288.15, 301.0))   # lo == hi; a negative lo
  cases = [(s, gb, e, lo, hi) for s in seeds for gb in buildings for e in episodes for lo, hi in intervals]
  text = "".join(f"{s} {gb} {e} {float(lo).hex()} {float(hi).hex()}\n" for s, gb, e, lo, hi in cases)
  out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
  assert len(out) == len(cases)
  for (seed, gb, e, lo, hi), bits in zip(cases, out):
    got = np.array([int(bits, 16)], dtype=np.uint64).view(np.float64)[0]
    restated = InitialConditions(jitter=(lo, hi, seed), first_building=gb).draw(0, e)
    c = philox4x32_10(gb & 0xFFFFFFFF, gb >> 32, e & 0xFFFFFFFF, _ffi.SB_INITIAL_CONDITIONS_TAG, seed & 0xFFFFFFFF, seed >> 32)
    r = (int(c[1]) << 32) | int(c[0])
    spelled = lo + (hi - lo) * ((r >> 11) * 2.0 ** -53)
    assert float(got).hex() == float(restated).hex() == float(spelled).hex(), (seed, gb, e, lo, hi)
    assert lo <= got <= hi


# ---------------------------------------------------------------- the digests snapshots compare
def test_the_digests_of_the_three_attachments_are_those_of_the_commit_before_their_shared_core():
  """``digest()`` goes into ``BatchedSimulator.state_fingerprint``: a snapshot taken before the three classes shared one
  parsed distribution must still load.  The strings were recorded by running that commit's classes on these inputs."""
  grids = np.arange(24, dtype=np.float64).reshape(2, 3, 4) * 0.125 + 290.0
  cases = {
      "ic_grids_jitter": InitialConditions(reset_temp_values=grids, grid_of=np.array([1, 0, 1], dtype=np.int32),
                                           offset=np.array([-0.5, 0.0, 1.25]), jitter=(-0.5, 0.25, 2 ** 63 + 5), first_building=3),
      "ic_base_jitter": InitialConditions(initial_temp=np.array([291.0, 294.5]), jitter=(0.0, 0.0, 7)),
      "er_mixed": EpisodeRandomization(
          params={"ahu_fan_efficiency": Uniform(0.7, 0.95), "vav_max_air_flow_rate": Uniform(0.8, 1.2, scale=True),
                  "comfort_temp_window": Uniform((293.0, 296.5), (295.0, 299.0)),
                  "boiler_reheat_water_setpoint": Choice([340.0, 350.0, 360.5])},
          materials={"conductivity": {0: Choice([0.5, 1.0, 2.0], scale=True)}, "convection_coefficient": Uniform(6.0, 25.0)},
          seed=2 ** 64 - 3, first_building=2 ** 32 + 1),
      "er_pair": EpisodeRandomization(params={"eco_temp_window": (Choice([285.0, 287.0]), Uniform(300.0, 303.0))}, seed=7),
      "es_int_step": EpisodeStarts(offsets=UniformInt(0, 364 * 288, step=288), weather_low=Uniform(268.0, 285.0),
                                   weather_high=Choice([286.0, 290.5, 305.0]), seed=11),
      "es_choice_relative": EpisodeStarts(offsets=Choice([0, 12, 288]), relative=True, weather_shift=Uniform(-3600.0, 7200.0),
                                          seed=2 ** 40 + 17, first_building=69),
  }
  recorded = {
      "ic_grids_jitter": "59f3c0f2f57640967ee912f8b19485e2fcb19e6c6df396e1ff89726c61da0190",
      "ic_base_jitter": "b9cb79a576f628f69f22bac0ee77933d38a15a25748c8c8572c2acc2412b786e",
      "er_mixed": "61a6f46bac90e706314705fb4571a099245a3141a8df619e866a740db2b3ddd1",
      "er_pair": "38078404a1df9322ef39187a0bba05844f02c4826a4cb841c90925e3b35dd7ee",
      "es_int_step": "d1dff216a04774e1b152256520e750e623a3126293b5f32e033eb9122bd38683",
      "es_choice_relative": "b1d1653bada6c70dbcf3bc9b4d4ee4eb9e092b5b47092511e48446788c6ee6f2",
  }
  assert {name: a.digest() for name, a in cases.items()} == recorded


# ---------------------------------------------------------------- the library, without a device
def test_the_entries_are_exported_and_refuse_null_handles():
  lib = C.CDLL(build.build())
  for name in _ffi.INITIAL_CONDITIONS_ENTRIES:
    assert hasattr(lib, name), name
  assert set(_ffi.INITIAL_CONDITIONS_ENTRIES) <= set(_ffi.EXPORTS)
  L = _ffi.load()
  assert _ffi.initial_conditions_entry("sb_initial_conditions_attach")(None, None) == -1
  assert b"sb_initial_conditions_attach: null argument" in L.sb_last_error()
  assert _ffi.initial_conditions_entry("sb_initial_conditions_detach")(None) == -1
  assert _ffi.initial_conditions_entry("sb_initial_conditions_episodes_get")(None, None, None) == -1
  assert _ffi.initial_conditions_entry("sb_initial_conditions_episodes_set")(None, None, None) == -1
  assert C.sizeof(_ffi.InitialConditionsDesc) == 72


def test_the_descriptor_matches_the_header():
  import subprocess, tempfile, textwrap
  src = textwrap.dedent("""
      #include <stddef.h>
      #include <stdio.h>
      #include "sbsim_amd.h"
      int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(sb_initial_conditions), offsetof(sb_initial_conditions, grid_of),
                       offsetof(sb_initial_conditions, jitter_lo), offsetof(sb_initial_conditions, seed),
                       offsetof(sb_initial_conditions, first_building)); return 0; }
  """)
  with tempfile.TemporaryDirectory() as d:
    c = os.path.join(d, "p.c")
    open(c, "w").write(src)
    exe = os.path.join(d, "p")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
  D = _ffi.InitialConditionsDesc
  assert got == [C.sizeof(D), D.grid_of.offset, D.jitter_lo.offset, D.seed.offset, D.first_building.offset]


# ---------------------------------------------------------------- the reference's own reset_temp_values
def _fixture_twin_run():
  """Both episodes of the fixture on ONE oracle twin: [(episode prefix, [step results with max_delta], grid after step 1)]."""
  g = load("reset_temp_values.npz")
  from sbsim_amd.environment import SimConfig
  fp, cfg = icc.fixture_plan(g), SimConfig.sb1()
  grid = g["reset_temp_values"]
  assert fp.shape == grid.shape == (23, 12)
  ob = oracle_twin(fp, cfg, grid.reshape(-1))
  runs = []
  for ep in ("e1_", "e2_"):
    ob.reset()
    ob.observe_boiler(float(g[ep + "ts_seconds"][0]))   # Environment.reset()'s observation
    outs, grid_1 = [], None
    for t in range(len(g[ep + "n_sweeps"])):
      outs.append(ob.step(
          now_ts=float(g[ep + "ts_seconds"][t]), t_amb_now=float(g[ep + "t_amb_now"][t]), h_conv=float(g["h_conv"]),
          t_amb_next=float(g[ep + "t_amb_next"][t]), comfort_now=bool(g[ep + "comfort_now"][t]),
          comfort_prev=g[ep + "comfort_prev"][t] == 1, comfort_next=bool(g[ep + "comfort_next"][t]),
          occupancy=float(g[ep + "occupancy"][t]), e_price=float(g[ep + "e_price"][t]), e_carbon=float(g[ep + "e_carbon"][t]),
          g_price=float(g[ep + "g_price"][t]), g_carbon=float(g[ep + "g_carbon"][t]), action=g[ep + "action_native"][t],
          observe=True, trace=True))
      if t == 0:
        grid_1 = ob.grid().copy()
    runs.append((ep, outs, grid_1, ob.grid().copy()))
  return g, cfg, runs


def test_oracle_twin_restates_the_reference_reset_temp_values_rollout():
  """The bars of tests/test_oracle_golden.py: sweep counts, zone temperatures and grids EQUAL (float64, bit for bit);
  the float32 rates within one unit in the last place (the gas rate holds an np.log)."""
  g, cfg, runs = _fixture_twin_run()
  assert len(g["e1_n_sweeps"]) == len(g["e2_n_sweeps"]) == 12 and g["e1_n_sweeps"].max() > 20
  for ep, outs, grid_1, final in runs:
    for t, o in enumerate(outs):
      assert o["n_sweeps"] == int(g[ep + "n_sweeps"][t]), (ep, t, o["n_sweeps"])
      assert np.array_equal(o["zone_temp_post"], g[ep + "zone_temp_post"][t]), (ep, t)
      assert np.array_equal(o["zone_temp_pre"], g[ep + "zone_temp_pre"][t]), (ep, t)
      rates = np.array([o["blower_rate"], o["ac_rate"], o["gas_rate"], o["pump_rate"]], np.float32)
      assert _ulp32(rates, g[ep + "rates"][t]).max() <= 1, (ep, t, rates, g[ep + "rates"][t])
    assert np.array_equal(grid_1, g[ep + "grid_1"]), ep
    assert np.array_equal(final, g[ep + "final_grid"]), ep


def test_the_second_episode_of_the_reference_equals_the_first():
  """reset() copies the grid back: the same actions from the same grid."""
  g = load("reset_temp_values.npz")
  for k in ("n_sweeps", "zone_temp_post", "zone_temp_pre", "grid_1", "final_grid", "actions_norm"):
    assert np.array_equal(g["e1_" + k], g["e2_" + k]), k
  assert np.array_equal(g["e1_rates"][1:], g["e2_rates"][1:])   # (step 0's gas rate sees the boiler's action age: it survives a reset)
  assert not np.array_equal(g["e1_grid_1"], g["reset_temp_values"])


def test_no_stopping_decision_of_the_fixture_or_the_twins_sits_on_its_edge():
  """Conditions on the inputs: should one fail, change the seed of the grid or of the actions, never the margin."""
  g, cfg, runs = _fixture_twin_run()
  thr = cfg.convergence_threshold
  for ep, outs, _, _ in runs:
    for t, o in enumerate(outs):
      md = o["max_delta"]
      assert len(md) == o["n_sweeps"] and (np.abs(md - thr) >= 1e-9 * thr).all(), (ep, t)
  for t, row in enumerate(icc.twin_rollout()):
    for b, o in enumerate(row):
      md = o["max_delta"]
      assert len(md) == o["n_sweeps"] and (np.abs(md - thr) >= 1e-9 * thr).all(), (t, b)


def test_no_decision_of_the_crossed_case_sits_on_its_edge():
  """tests/test_crossed_batches_cpu.py's conditions on the crossed case's twins: the stopping decisions, the
  thermostat's thresholds, the productivity's branches -- and that the program restarts buildings at all."""
  sc, ic, out, episodes = icc.crossing()
  thr = sc.config.convergence_threshold
  assert sc.case["materials"] == "building_materials" and sc.case["time"] == "calendars" and sc.per_building
  assert episodes.min() >= 2 and episodes.max() >= 4   # every building restarted, some three times
  for op, res in out[1:-1]:
    for b, r in enumerate(res):
      if r is None or op.kind != "step":
        continue
      lo, hi = r["window_now"]
      for edge in (lo, hi, 0.5 * (hi - lo) + lo):
        assert np.abs(r["zone_temp_pre"] - edge).min() >= 1e-6, (op.row, b, edge)
      md = r["max_delta"]
      assert len(md) == r["n_sweeps"] and (np.abs(md - thr) > 1e-9 * thr).all(), (op.row, b)
      lo, hi = r["window_next"]
      t32 = r["zone_temp_post"].astype(np.float32).astype(np.float64)
      for edge in (float(np.float32(lo)), float(np.float32(hi))):
        assert np.abs(t32 - edge).min() >= 1e-4, (op.row, b, edge)
