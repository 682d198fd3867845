"""The second reward function (host_inputs.SetpointEnergyCarbonReward) restated in float64 NumPy, and its fixture
(tests/golden/reward_sec_kat.json, tools/gen_golden_reward.py): tests/test_reward_function_cpu.py holds the restatement to
the fixture, tests/test_reward_function_gpu.py and tests/crossed_batches.py hold k_post to the restatement."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reward_sec_kat.json")
# the RewardResponse fields SetpointEnergyCarbonRewardFunction sets (:168-188); every other field stays 0
SET_FIELDS = ("agent_reward_value", "productivity_reward", "electricity_energy_cost", "natural_gas_energy_cost",
              "carbon_emitted", "carbon_cost")
F32_ULP = 2.0 ** -23   # a float32 rounding of the float64 result is within half of this, relatively


def fixture() -> dict:
  with open(GOLDEN) as fh:
    return json.load(fh)


def restate(cfg, heating_setpoint, cooling_setpoint, zone_temps, occupancies, ahus, boilers, prices, dt,
            real_cost_models=True) -> dict:
  """SetpointEnergyCarbonRewardFunction.compute_reward in float64, operation by operation, on the float32 values a
  RewardInfo holds.  cfg: the constructor's arguments by name; ahus: [(blower, air conditioning)] and boilers:
  [(gas, pump)] in W; prices: (e_price, e_carbon, g_price, g_carbon) per W per s.  real_cost_models: the reference's
  ElectricityEnergyCost (|rate|) and NaturalGasEnergyCost (a negative rate reads as 0); False: its test's TestEnergyCost
  (price * rate * dt).  Returns the RewardResponse fields it sets, as float64 before the proto's float32 store -- except
  carbon_cost, which the reference reads back from the proto (float32) before it enters the reward."""
  f = lambda x: np.float64(np.float32(x))
  max_prod, delta, stiff = (np.float64(cfg[k]) for k in ("max_productivity_personhour_usd", "productivity_midpoint_delta",
                                                          "productivity_decay_stiffness"))
  heat, cool, dt = f(heating_setpoint), f(cooling_setpoint), np.float64(dt)
  productivity = np.float64(0.0)
  for t, occ in zip(zone_temps, occupancies):   # base_setpoint_energy_carbon_reward.py:54-123
    t, occ = f(t), f(occ)
    if t < heat:
      prod = max_prod / (1.0 + np.exp(-stiff * (t - (heat - delta))))
    elif t > cool:
      prod = max_prod * (1.0 - 1.0 / (1.0 + np.exp(-stiff * (t - (cool + delta)))))
    else:
      prod = max_prod
    productivity += prod * occ * dt / 3600.0
  elec = np.float64(0.0)   # :137-159
  for blower, ac in ahus:
    elec += f(blower) + np.abs(f(ac))
  for _, pump in boilers:
    elec += f(pump)
  gas = np.float64(0.0)    # :161-172
  for g, _ in boilers:
    gas += f(g)
  e_price, e_carbon, g_price, g_carbon = (np.float64(p) for p in prices)
  if real_cost_models:
    gas = np.float64(0.0) if gas < 0.0 else gas
    elec_cost, elec_carbon = e_price * np.abs(elec) * dt, e_carbon * np.abs(elec) * dt
    gas_cost, gas_carbon = g_price * (gas * dt), g_carbon * (gas * dt)
  else:
    elec_cost, elec_carbon = e_price * elec * dt, e_carbon * elec * dt
    gas_cost, gas_carbon = g_price * gas * dt, g_carbon * gas * dt
  carbon = elec_carbon + gas_carbon
  carbon_cost = f(carbon * np.float64(cfg["carbon_cost_factor"]))
  raw = (productivity - np.float64(cfg["energy_cost_weight"]) * (elec_cost + gas_cost)
         - np.float64(cfg["carbon_cost_weight"]) * carbon_cost)
  reward = (raw - np.float64(cfg["reward_normalizer_shift"])) / np.float64(cfg["reward_normalizer_scale"])
  return dict(agent_reward_value=reward, productivity_reward=productivity, electricity_energy_cost=elec_cost,
              natural_gas_energy_cost=gas_cost, carbon_emitted=carbon, carbon_cost=carbon_cost)
