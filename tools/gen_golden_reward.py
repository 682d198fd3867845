"""Generates tests/golden/reward_sec_kat.json from the reference's own SetpointEnergyCarbonRewardFunction
(reward/setpoint_energy_carbon_reward.py), imported through oracle/refshim.  Run it where the reference tree exists
(``python tools/gen_golden_reward.py``); tests never run it and never read the reference.  The file holds data only.

  named   the named cases of reward/setpoint_energy_carbon_reward_test.py:31-107, built by that test's own
          _get_test_reward_info / _get_test_reward_function (two zones, two air handlers, two boilers, the test's
          fixed-price TestEnergyCost): the inputs, the values the test asserts (to four decimals), and what the
          reference function returned here.  The rates recorded per row are those of ONE device; ``n_ahu`` /
          ``n_boiler`` say how many identical ones the RewardInfo holds.
  random  seeded random RewardInfo rows through the reference function with the reference's ElectricityEnergyCost and
          NaturalGasEnergyCost: 1-3 zones with their own temperatures (below, inside, above the window) and
          occupancies (0 and positive), one air handler (air conditioning of either sign), one boiler (a gas rate
          that is negative, ordinary, or beyond SB1's max_natural_gas_rate), shift != 0 and scale != 1.  Every
          RewardResponse field is recorded as the proto holds it (float32, printed exactly); ``e_price``, ``e_carbon``,
          ``g_price``, ``g_carbon`` are the cost models' USD and kg per W per s at the row's start time.  Every float
          input is a float32 value.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reward_sec_kat.json")
RESPONSE_FIELDS = ("agent_reward_value", "productivity_reward", "electricity_energy_cost", "natural_gas_energy_cost",
                   "carbon_emitted", "carbon_cost", "productivity_weight", "energy_cost_weight", "carbon_emission_weight",
                   "person_productivity", "total_occupancy", "reward_scale", "reward_shift", "productivity_regret",
                   "normalized_productivity_regret", "normalized_energy_cost", "normalized_carbon_emission")
N_RANDOM = 40
MAX_GAS_SB1 = 400000.0   # SB1's max_natural_gas_rate: what the regret function would cap the gas rate at


def f32(x) -> float:
  return float(np.float32(x))


def response_dict(resp) -> dict:
  return {name: float(getattr(resp, name)) for name in RESPONSE_FIELDS}


_NAMED = {}   # test method name -> the tuples its @parameterized.named_parameters decorator was given


def _record_named_parameters(params):
  """Stand-in for absl's decorator (the shim's drops the tuples): keeps them, leaves the method alone."""
  def deco(fn):
    _NAMED[fn.__name__] = [tuple(p) for p in params]
    return fn
  return deco


def named_cases(test_mod) -> dict:
  cls = test_mod.SetpointEnergyCarbonRewardTest
  t = cls.__new__(cls)
  rows = _NAMED["test_compute_reward"]   # the test's own @parameterized.named_parameters tuples, in its order
  fn = t._get_test_reward_function()
  out = []
  for (name, temp, occ, blower, ac, gas, pump, e_reward, e_prod, e_elec, e_gas, e_carbon, e_ccost) in rows:
    info = t._get_test_reward_info(temp, occ, blower, ac, gas, pump)
    resp = fn.compute_reward(info)
    got = response_dict(resp)
    for key, want in (("agent_reward_value", e_reward), ("productivity_reward", e_prod), ("electricity_energy_cost", e_elec),
                      ("natural_gas_energy_cost", e_gas), ("carbon_emitted", e_carbon), ("carbon_cost", e_ccost)):
      assert abs(got[key] - want) < 5e-5, (name, key, got[key], want)   # the reference test's own assertion
    out.append(dict(name=name, zone_air_temperature=temp, average_occupancy=occ, blower=blower, air_conditioning=ac,
                    natural_gas=gas, pump=pump, expected_reward=e_reward, expected_productivity=e_prod,
                    expected_electricity_cost=e_elec, expected_natural_gas_cost=e_gas, expected_carbon_emitted=e_carbon,
                    expected_carbon_cost=e_ccost, response=got))
  zones = info.zone_reward_infos
  z0 = zones[sorted(zones)[0]]
  config = dict(max_productivity_personhour_usd=fn._max_productivity_personhour_usd,
                productivity_midpoint_delta=fn._productivity_midpoint_delta,
                productivity_decay_stiffness=fn._productivity_decay_stiffness,
                energy_cost_weight=fn._energy_cost_weight, carbon_cost_weight=fn._carbon_cost_weight,
                carbon_cost_factor=fn._carbon_cost_factor, reward_normalizer_shift=fn._reward_normalizer_shift,
                reward_normalizer_scale=fn._reward_normalizer_scale,
                electricity_usd_per_kwh=0.19, electricity_kg_per_kwh=0.01, gas_usd_per_kwh=0.03, gas_kg_per_kwh=0.188,
                heating_setpoint=float(z0.heating_setpoint_temperature), cooling_setpoint=float(z0.cooling_setpoint_temperature),
                n_zones=len(zones), n_ahu=len(info.air_handler_reward_infos), n_boiler=len(info.boiler_reward_infos),
                dt_sec=float(info.end_timestamp.seconds - info.start_timestamp.seconds))
  return dict(config=config, rows=out)


def random_rows(m) -> list:
  pb = m["pb"]
  conv = m["conversion_utils"]
  elec, gas_model = m["electricity_energy_cost"].ElectricityEnergyCost(), m["natural_gas_energy_cost"].NaturalGasEnergyCost()
  rs = np.random.RandomState(20261017)
  rows = []
  for i in range(N_RANDOM):
    n_zones = 1 + i % 3
    dt_sec = (300.0, 600.0, 120.0)[i % 3]   # one step length per zone count: a test needs one handle per pair
    start = pd.Timestamp("2021-05-03 00:10:00+00:00") + pd.Timedelta(hours=int(rs.randint(0, 24 * 300)), minutes=5 * int(rs.randint(0, 12)))
    heat = f32(rs.uniform(288.0, 294.5))
    cool = f32(heat + rs.uniform(1.0, 6.0))
    where = [(i + z) % 3 for z in range(n_zones)]   # 0 below / 1 inside / 2 above the window, every row mixes them
    temps = [f32({0: heat - rs.uniform(0.05, 4.0), 1: rs.uniform(heat, cool), 2: cool + rs.uniform(0.05, 4.0)}[w]) for w in where]
    if i % 10 == 0:
      temps[0] = heat    # on the window's edges: full productivity (the comparisons are strict)
    if i % 10 == 5:
      temps[0] = cool
    occs = [0.0 if (i + 2 * z) % 4 == 0 else f32(rs.uniform(0.1, 25.0)) for z in range(n_zones)]
    blower = f32(rs.uniform(0.0, 30000.0))
    ac = f32(rs.uniform(-90000.0, 90000.0))      # negative: cooling
    pump = f32(rs.uniform(0.0, 2000.0))
    gas = f32({0: rs.uniform(-5000.0, -1.0), 1: rs.uniform(0.0, 300000.0), 2: rs.uniform(1.05, 2.0) * MAX_GAS_SB1}[i % 3])
    fn_cfg = dict(max_productivity_personhour_usd=f32(rs.uniform(50.0, 600.0)), productivity_midpoint_delta=f32(rs.uniform(0.25, 2.5)),
                  productivity_decay_stiffness=f32(rs.uniform(1.0, 6.0)), energy_cost_weight=f32(rs.uniform(0.1, 5.0)),
                  carbon_cost_weight=f32(rs.uniform(0.1, 5.0)), carbon_cost_factor=f32(rs.uniform(0.05, 3.0)),
                  reward_normalizer_shift=f32(rs.uniform(-400.0, 400.0)), reward_normalizer_scale=f32(rs.choice([-1, 1]) * rs.uniform(2.0, 900.0)))
    fn = m["setpoint_energy_carbon_reward"].SetpointEnergyCarbonRewardFunction(
        fn_cfg["max_productivity_personhour_usd"], fn_cfg["productivity_midpoint_delta"], fn_cfg["productivity_decay_stiffness"],
        elec, gas_model, fn_cfg["energy_cost_weight"], fn_cfg["carbon_cost_weight"], fn_cfg["carbon_cost_factor"],
        fn_cfg["reward_normalizer_shift"], fn_cfg["reward_normalizer_scale"])
    info = pb.RewardInfo()
    info.start_timestamp.CopyFrom(conv.pandas_to_proto_timestamp(start))
    info.end_timestamp.CopyFrom(conv.pandas_to_proto_timestamp(start + pd.Timedelta(seconds=dt_sec)))
    for z in range(n_zones):
      zi = info.zone_reward_infos["zone_%d" % z]   # (a map: the reference iterates it in insertion order)
      zi.heating_setpoint_temperature, zi.cooling_setpoint_temperature = heat, cool
      zi.zone_air_temperature, zi.average_occupancy = temps[z], occs[z]
    ah = info.air_handler_reward_infos["air_handler_id"]
    ah.blower_electrical_energy_rate, ah.air_conditioning_electrical_energy_rate = blower, ac
    bl = info.boiler_reward_infos["boiler_id"]
    bl.natural_gas_heating_energy_rate, bl.pump_electrical_energy_rate = gas, pump
    resp = fn.compute_reward(info)
    # the cost models' rates at the row's start time, as the reward function's calls see it
    t0 = conv.proto_to_pandas_timestamp(info.start_timestamp)
    price_tab = elec._weekday_energy_prices if conv.is_work_day(t0) else elec._weekend_energy_prices
    rates = dict(e_price=float(getattr(price_tab[t0.hour], "magnitude", price_tab[t0.hour])),
                 e_carbon=float(getattr(elec._carbon_emission_rates[t0.hour], "magnitude", elec._carbon_emission_rates[t0.hour])),
                 g_price=float(gas_model._month_gas_price[t0.month - 1]), g_carbon=float(gas_model._carbon_rate))
    got = response_dict(resp)
    raw = got["agent_reward_value"] * fn_cfg["reward_normalizer_scale"]
    assert abs(raw) > 0.02 * max(abs(fn_cfg["reward_normalizer_shift"]), 1.0), (i, raw)   # no reward that is all cancellation
    rows.append(dict(name="random_%02d" % i, start=str(start), dt_sec=dt_sec, heating_setpoint=heat, cooling_setpoint=cool,
                     zone_air_temperature=temps, average_occupancy=occs, blower=blower, air_conditioning=ac,
                     natural_gas=gas, pump=pump, **fn_cfg, **rates, response=got))
  return rows


def main() -> None:
  if not refshim.available():
    raise SystemExit("the reference tree is not here: nothing written")
  refshim.install()
  sys.modules["absl.testing.parameterized"].named_parameters = _record_named_parameters
  m = {name.split(".")[-1]: refshim.ref(name) for name in (
      "reward.setpoint_energy_carbon_reward", "reward.setpoint_energy_carbon_reward_test",
      "reward.electricity_energy_cost", "reward.natural_gas_energy_cost", "utils.conversion_utils")}
  m["pb"] = refshim.ref("proto.smart_control_reward_pb2")
  doc = dict(source="reward/setpoint_energy_carbon_reward.py:127-190 through tools/gen_golden_reward.py",
             numpy=np.__version__, response_fields=list(RESPONSE_FIELDS),
             named=named_cases(m["setpoint_energy_carbon_reward_test"]), random=random_rows(m))
  with open(OUT, "w") as fh:
    json.dump(doc, fh, indent=1)
    fh.write("\n")
  print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
  main()
