"""CPU-only checks of the second reward function (sb_set_reward_function, host_inputs.SetpointEnergyCarbonReward): the
struct layout, the refusals that need no device, and a float64 NumPy restatement of
reward/setpoint_energy_carbon_reward.py:127-190 held to every row of tests/golden/reward_sec_kat.json
(tools/gen_golden_reward.py).  tests/test_reward_function_gpu.py holds k_post to the same restatement."""
import ctypes as C
import os
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest

from sbsim_amd import _ffi, build, host_inputs
from tests.reward_cases import F32_ULP, SET_FIELDS, fixture, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def restate_named(doc, row) -> dict:
  c = doc["named"]["config"]
  per_w_s = lambda per_kwh: per_kwh / 3600.0 / 1000.0
  prices = (per_w_s(c["electricity_usd_per_kwh"]), per_w_s(c["electricity_kg_per_kwh"]), per_w_s(c["gas_usd_per_kwh"]),
            per_w_s(c["gas_kg_per_kwh"]))
  return restate(c, c["heating_setpoint"], c["cooling_setpoint"], [row["zone_air_temperature"]] * c["n_zones"],
                 [row["average_occupancy"]] * c["n_zones"], [(row["blower"], row["air_conditioning"])] * c["n_ahu"],
                 [(row["natural_gas"], row["pump"])] * c["n_boiler"], prices, c["dt_sec"], real_cost_models=False)


def restate_random(row) -> dict:
  return restate(row, row["heating_setpoint"], row["cooling_setpoint"], row["zone_air_temperature"], row["average_occupancy"],
                 [(row["blower"], row["air_conditioning"])], [(row["natural_gas"], row["pump"])],
                 (row["e_price"], row["e_carbon"], row["g_price"], row["g_carbon"]), row["dt_sec"])


def test_reward_config_layout_matches_header():
  names = [n for n, _ in _ffi.RewardConfig._fields_]
  assert names == ["kind", "energy_cost_weight", "carbon_cost_weight", "carbon_cost_factor", "normalizer_shift",
                   "normalizer_scale"]
  offs = ", ".join(f"offsetof(sb_reward_config, {n})" for n in names)
  src = textwrap.dedent("""
      #include <stdio.h>
      #include <stddef.h>
      #include "sbsim_amd.h"
      int main(void) { size_t v[] = {sizeof(sb_reward_config), %s};
                       for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%zu ", v[i]);
                       printf("%%d %%d %%d %%zu\\n", SB_REWARD_REGRET, SB_REWARD_SETPOINT_ENERGY_CARBON, SB_ABI_VERSION,
                              sizeof(sb_params));
                       return 0; }
  """ % offs)
  with tempfile.TemporaryDirectory() as d:
    c = os.path.join(d, "p.c")
    open(c, "w").write(src)
    exe = os.path.join(d, "p")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    vals = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
  assert vals == ([C.sizeof(_ffi.RewardConfig)] + [getattr(_ffi.RewardConfig, n).offset for n in names]
                  + [_ffi.SB_REWARD_REGRET, _ffi.SB_REWARD_SETPOINT_ENERGY_CARBON, 8, C.sizeof(_ffi.Params)])
  assert _ffi.SB_ABI_VERSION == 8   # the entry is bound when present: the ABI version and sb_params stay


def test_the_entry_refuses_a_null_handle_without_a_device():
  build.build()
  L = _ffi.load()
  cfg = _ffi.RewardConfig(1, 1.0, 1.0, 0.2, 0.0, 1.0)
  assert L.sb_set_reward_function(None, C.byref(cfg)) == -1
  assert b"null handle" in L.sb_last_error()


def test_a_library_without_the_entry_asks_for_a_rebuild(monkeypatch):
  class Old:   # a library of the same ABI version built before sb_set_reward_function
    pass
  monkeypatch.setattr(_ffi, "_lib", Old())
  with pytest.raises(_ffi.SbsimError, match="rebuild"):
    _ffi.reward_entry("sb_set_reward_function")


def test_setpoint_energy_carbon_reward_validates_its_arguments():
  r = host_inputs.SetpointEnergyCarbonReward(1.0, 2, 0.2)
  assert r.as_tuple() == (1, 1.0, 2.0, 0.2, 0.0, 1.0)
  assert r == host_inputs.SetpointEnergyCarbonReward(1.0, 2.0, 0.2, 0.0, 1.0)
  assert r != host_inputs.SetpointEnergyCarbonReward(1.0, 2.0, 0.2, 0.0, 2.0)
  assert host_inputs.SetpointEnergyCarbonReward(0.0, -1.0, 0.0, -3.0, -2.0).reward_normalizer_scale == -2.0
  with pytest.raises(ValueError, match="reward_normalizer_scale must not be 0"):
    host_inputs.SetpointEnergyCarbonReward(1.0, 1.0, 0.2, 0.0, 0.0)
  for bad in (float("nan"), float("inf"), -float("inf")):
    for pos in range(5):
      args = [1.0, 1.0, 0.2, 0.0, 1.0]
      args[pos] = bad
      with pytest.raises(ValueError, match="not finite"):
        host_inputs.SetpointEnergyCarbonReward(*args)
  for bad in (None, "1.0", True, [1.0]):
    with pytest.raises(ValueError, match="must be a number"):
      host_inputs.SetpointEnergyCarbonReward(bad, 1.0, 0.2)
  with pytest.raises(TypeError):
    host_inputs.SetpointEnergyCarbonReward(1.0, 1.0)   # the three weights have no default, as in the reference


def test_the_fixture_covers_what_it_is_meant_to():
  doc = fixture()
  assert [r["name"] for r in doc["named"]["rows"]] == [
      "occupied_in_setpoint", "not_occupied_in_setpoint", "occupied_below_setpoint", "occupied_above_setpoint",
      "occupied_in_setpoint_no_energy"]
  rows = doc["random"]
  assert len(rows) >= 36 and {len(r["zone_air_temperature"]) for r in rows} == {1, 2, 3}
  where = set()
  for r in rows:
    for t in r["zone_air_temperature"]:
      where.add("below" if t < r["heating_setpoint"] else "above" if t > r["cooling_setpoint"] else "inside")
  assert where == {"below", "inside", "above"}
  occ = [o for r in rows for o in r["average_occupancy"]]
  assert min(occ) == 0.0 and max(occ) > 0.0
  assert any(r["air_conditioning"] < 0 for r in rows) and any(r["air_conditioning"] > 0 for r in rows)
  sb1_max_gas = 400000.0   # SimConfig.sb1().max_natural_gas_rate: the regret function's cap
  assert any(r["natural_gas"] < 0 for r in rows) and any(r["natural_gas"] > sb1_max_gas for r in rows)
  assert all(r["reward_normalizer_shift"] != 0.0 and r["reward_normalizer_scale"] != 1.0 for r in rows)
  for r in rows + doc["named"]["rows"]:   # the fields the reference leaves alone are the proto's default
    assert all(v == 0.0 for k, v in r["response"].items() if k not in SET_FIELDS), r["name"]


def test_the_restatement_reproduces_the_named_cases():
  doc = fixture()
  for row in doc["named"]["rows"]:
    got = restate_named(doc, row)
    # the reference's test states these to four decimals (assertAlmostEqual places=4)
    for key, want in (("agent_reward_value", "expected_reward"), ("productivity_reward", "expected_productivity"),
                      ("electricity_energy_cost", "expected_electricity_cost"),
                      ("natural_gas_energy_cost", "expected_natural_gas_cost"),
                      ("carbon_emitted", "expected_carbon_emitted"), ("carbon_cost", "expected_carbon_cost")):
      assert float(got[key]) == pytest.approx(row[want], abs=5e-5), (row["name"], key)
    for key in SET_FIELDS:   # and what the reference function returned: its float32 fields
      assert float(np.float32(got[key])) == pytest.approx(row["response"][key], rel=F32_ULP, abs=0.0), (row["name"], key)


def test_the_restatement_reproduces_every_random_row():
  for row in fixture()["random"]:
    got = restate_random(row)
    for key in SET_FIELDS:
      assert float(np.float32(got[key])) == pytest.approx(row["response"][key], rel=F32_ULP, abs=0.0), (row["name"], key)


def test_a_capped_gas_rate_would_show():
  """The rows beyond SB1's max_natural_gas_rate: with the regret function's cap the gas cost misses the fixture."""
  rows = [r for r in fixture()["random"] if r["natural_gas"] > 400000.0]
  assert rows
  for row in rows:
    capped = restate_random(dict(row, natural_gas=400000.0))
    assert float(capped["natural_gas_energy_cost"]) != pytest.approx(row["response"]["natural_gas_energy_cost"], rel=1e-3)
