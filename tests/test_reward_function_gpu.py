"""The second reward function (sb_set_reward_function, SetpointEnergyCarbonReward) on the GPU: the reference's known
answers and the fixture's random rows through sb_tap_post with the energy rates PRODUCED by k_post from device state
(as tests/test_gpu_kats.py does for the regret function), whole steps against the float64 restatement of
tests/test_reward_function_cpu.py, and what the option must leave alone: the state, the default reward, the
per-building rows, rejection, mixed batches, snapshots."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, EnvSnapshot, MixedBatchedEnvironment, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from sbsim_amd.host_inputs import BuildingParams, SetpointEnergyCarbonReward  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import need_gpu  # noqa: E402
from tests.reward_cases import SET_FIELDS, fixture, restate  # noqa: E402
from tests.twins import plan_from_npz  # noqa: E402

C_AIR = 1006.0   # utils/constants.py:21
SB1 = SimConfig.sb1()
REWARD = SetpointEnergyCarbonReward(1.5, 0.75, 0.2, reward_normalizer_shift=-3.0, reward_normalizer_scale=50.0)
INFO_COLUMNS = dict(zip(SET_FIELDS, range(7, 13)))   # RewardResponse field -> info column


def _small():
  return plan_from_npz(load("plan_small_test.npz"))


def _row_plan(zones):
  return FloorPlan.from_file_input(rectangular_floor_plan((1, zones), (8, 8)), Materials.sb1(), 10.0, 300.0)


class Tap:
  """A handle of two buildings whose building 1 is driven through sb_tap_post: the row's energy rates are produced by
  k_post (blower = flow * dp with full recirculation, air conditioning = flow * c_air * (setpoint - mixed), gas = the
  tank's dissipation, pump = flow * rho g head); what differs from row to row is the building's row of a per-building
  table and the handle's reward function."""
  FLOW, WFLOW, MIXED, T_OUT = 2.0, 0.5, 290.0, 280.0

  def __init__(self, zones, dt_sec):
    self.cfg = dataclasses.replace(SB1, time_step_sec=float(dt_sec), ahu_recirculation=1.0, ahu_fan_efficiency=1.0,
                                   boiler_water_pump_efficiency=1.0)
    self.sim = BatchedSimulator(_row_plan(zones), self.cfg, 2, 100.0)
    assert self.sim.Z == zones
    c = self.cfg
    r2 = c.boiler_tank_radius + c.boiler_insulation_thickness   # boiler.py:275-320: watts per kelvin
    self.k_diss = c.boiler_tank_length * 2.0 * math.pi / (
        math.log(r2 / c.boiler_tank_radius) / c.boiler_insulation_conductivity + 1.0 / c.boiler_convection_coefficient / r2)

  def post(self, reward_function, window, productivity, zone_temps, occupancies, blower, ac, gas, pump, prices):
    """reward, info of building 1.  productivity: (max_productivity_personhour_usd, midpoint_delta, decay_stiffness)."""
    sim = self.sim
    rows = {"comfort_temp_window": np.array([SB1.comfort_temp_window, window], dtype=np.float64),
            "max_productivity_personhour_usd": np.array([SB1.max_productivity_personhour_usd, productivity[0]]),
            "productivity_midpoint_delta": np.array([SB1.productivity_midpoint_delta, productivity[1]]),
            "productivity_decay_stiffness": np.array([SB1.productivity_decay_stiffness, productivity[2]]),
            "ahu_fan_differential_pressure": np.array([SB1.ahu_fan_differential_pressure, blower / self.FLOW]),
            "boiler_water_pump_differential_head": np.array([SB1.boiler_water_pump_differential_head,
                                                             pump / (1000.0 * 9.8 * self.WFLOW)])}
    sim.set_building_params(BuildingParams(rows))
    sim.set_reward_function(reward_function)
    d_ac = ac / (self.FLOW * C_AIR)
    supply_w = self.T_OUT + gas / self.k_diss
    bld = _ffi.TapBld()
    bld.t_now = bld.t_next = self.T_OUT
    bld.t_sa = 285.0
    bld.heat_sp = self.MIXED + d_ac if d_ac >= 0 else 200.0
    bld.cool_sp = self.MIXED + d_ac if d_ac < 0 else 400.0
    bld.ahu_flow, bld.blr_flow = self.FLOW, self.WFLOW
    bld.blr_sp = bld.blr_return = supply_w
    si = _ffi.StepIn()
    si.t_amb_now = si.t_amb_next = self.T_OUT
    si.comfort_now = si.comfort_prev = si.comfort_next = 1
    occ = torch.tensor(np.asarray(occupancies, dtype=np.float64), device="cuda")
    si.occupancy_dev = occ.data_ptr()
    si.e_price, si.e_carbon, si.g_price, si.g_carbon = prices
    zt = np.ascontiguousarray(zone_temps, dtype=np.float64)
    rew = C.c_float(0.0)
    info = np.zeros(_ffi.SB_INFO_STRIDE, dtype=np.float32)
    torch.cuda.synchronize()
    _ffi.check(sim._lib.sb_tap_post(sim._h, 1, C.byref(bld), zt.ctypes.data_as(C.POINTER(C.c_double)), self.MIXED, 1,
                                    C.byref(si), C.byref(rew), info.ctypes.data_as(C.POINTER(C.c_float))), "sb_tap_post")
    return float(rew.value), info.astype(np.float64)

  def close(self):
    self.sim.close()


def _check_rates(info, blower, ac, gas, pump, name):   # (the tolerances of test_reward_known_answers_through_k_post)
  assert info[0] == pytest.approx(blower, rel=1e-6, abs=1e-4), name
  assert info[1] == pytest.approx(ac, rel=1e-6, abs=1e-3), name
  assert info[2] == pytest.approx(gas, rel=1e-6, abs=1e-3), name
  assert info[3] == pytest.approx(pump, rel=1e-6, abs=1e-4), name


def test_named_known_answers_through_k_post():
  """setpoint_energy_carbon_reward_test.py:31-148: the values that test asserts, to its four decimals.  Its RewardInfo
  holds two air handlers and two boilers; the building here has one of each with their summed rates."""
  need_gpu()
  doc = fixture()
  c = doc["named"]["config"]
  per_w_s = lambda per_kwh: per_kwh / 3600.0 / 1000.0
  prices = (per_w_s(c["electricity_usd_per_kwh"]), per_w_s(c["electricity_kg_per_kwh"]), per_w_s(c["gas_usd_per_kwh"]),
            per_w_s(c["gas_kg_per_kwh"]))
  fn = SetpointEnergyCarbonReward(c["energy_cost_weight"], c["carbon_cost_weight"], c["carbon_cost_factor"],
                                  c["reward_normalizer_shift"], c["reward_normalizer_scale"])
  tap = Tap(c["n_zones"], c["dt_sec"])
  for row in doc["named"]["rows"]:
    blower, ac = c["n_ahu"] * row["blower"], c["n_ahu"] * row["air_conditioning"]
    gas, pump = c["n_boiler"] * row["natural_gas"], c["n_boiler"] * row["pump"]
    reward, info = tap.post(fn, (c["heating_setpoint"], c["cooling_setpoint"]),
                            (c["max_productivity_personhour_usd"], c["productivity_midpoint_delta"], c["productivity_decay_stiffness"]),
                            [row["zone_air_temperature"]] * c["n_zones"], [row["average_occupancy"]] * c["n_zones"],
                            blower, ac, gas, pump, prices)
    name = row["name"]
    print(name, reward, info[7:13])
    _check_rates(info, blower, ac, gas, pump, name)
    assert reward == pytest.approx(row["expected_reward"], abs=5e-5), name
    assert info[7] == reward, name
    assert info[8] == pytest.approx(row["expected_productivity"], rel=1e-6, abs=5e-5), name
    assert info[9] == pytest.approx(row["expected_electricity_cost"], abs=5e-5), name
    assert info[10] == pytest.approx(row["expected_natural_gas_cost"], abs=5e-5), name
    assert info[11] == pytest.approx(row["expected_carbon_emitted"], abs=5e-5), name
    assert info[12] == pytest.approx(row["expected_carbon_cost"], abs=5e-5), name
    assert not info[13:].any(), name   # the fields the reference leaves at the proto's default (scale and shift too)
  tap.close()


def test_random_rows_through_k_post():
  """Every RewardResponse field of the fixture's seeded rows (the reference function with its own cost models), to
  float32 rounding: 1-3 zones on either side of the window, empty zones, cooling, a gas rate the regret function
  would cap, shift and scale."""
  need_gpu()
  rows = fixture()["random"]
  taps = {}
  for row in rows:
    key = (len(row["zone_air_temperature"]), row["dt_sec"])
    if key not in taps:
      taps[key] = Tap(*key)
    fn = SetpointEnergyCarbonReward(row["energy_cost_weight"], row["carbon_cost_weight"], row["carbon_cost_factor"],
                                    row["reward_normalizer_shift"], row["reward_normalizer_scale"])
    reward, info = taps[key].post(
        fn, (row["heating_setpoint"], row["cooling_setpoint"]),
        (row["max_productivity_personhour_usd"], row["productivity_midpoint_delta"], row["productivity_decay_stiffness"]),
        row["zone_air_temperature"], row["average_occupancy"], row["blower"], row["air_conditioning"],
        row["natural_gas"], row["pump"], (row["e_price"], row["e_carbon"], row["g_price"], row["g_carbon"]))
    name = row["name"]
    print(name, reward, info[7:13], [row["response"][k] for k in SET_FIELDS])
    _check_rates(info, row["blower"], row["air_conditioning"], row["natural_gas"], row["pump"], name)
    assert info[7] == reward, name
    for field, col in INFO_COLUMNS.items():
      assert info[col] == pytest.approx(row["response"][field], rel=1e-6, abs=0.0), (name, field)
    assert not info[13:].any(), name
  assert len(taps) == 3
  for t in taps.values():
    t.close()


# ---- whole steps ----
def _actions(T, B, seed):
  gen = torch.Generator(device="cuda")
  gen.manual_seed(seed)
  return torch.rand((T, B, 2), generator=gen, device="cuda") * 2 - 1


def _start(env, seed=5):
  """reset(), then grids that put zones below, inside and above the comfort window."""
  env.reset()
  rs = np.random.RandomState(seed)
  H, W = env.sim.H, env.sim.W
  base = np.array([292.0, 295.5, 299.0, 295.0])[np.arange(env.batch_size) % 4, None]
  init = np.clip(base + 1.5 * rs.randn(env.batch_size, H * W), 285.0, 306.0)
  env.sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))


def _run(env, acts, rejected=None):
  """Per step: observation, reward, info, temperatures (clones), and what the restatement needs of the step."""
  out = []
  for t in range(acts.shape[0]):
    si = env.make_step_in(env.current_simulation_timestamp)   # (stateless host models: asking twice changes nothing)
    ts = env.step(acts[t], rejected=rejected)
    out.append(dict(obs=ts.observation.clone(), reward=ts.reward.clone(), info=env.info.clone(), temps=env.sim.temps(),
                    zone_temps=env.sim.zone_temps().cpu().numpy(), occupancy=si.occupancy, comfort=bool(si.comfort_next),
                    prices=(si.e_price, si.e_carbon, si.g_price, si.g_carbon)))
  return out


def _restated_rewards(env, step, reward_function):
  """The restatement on every building's info[0:4], zone temperatures, occupancy and rates of one step."""
  bp = env.building_params()
  r = reward_function
  info = step["info"].cpu().numpy().astype(np.float64)
  want = []
  for b in range(env.batch_size):
    cfg = dict(max_productivity_personhour_usd=bp["max_productivity_personhour_usd"][b],
               productivity_midpoint_delta=bp["productivity_midpoint_delta"][b],
               productivity_decay_stiffness=bp["productivity_decay_stiffness"][b],
               energy_cost_weight=r.energy_cost_weight, carbon_cost_weight=r.carbon_cost_weight,
               carbon_cost_factor=r.carbon_cost_factor, reward_normalizer_shift=r.reward_normalizer_shift,
               reward_normalizer_scale=r.reward_normalizer_scale)
    lo, hi = bp["comfort_temp_window" if step["comfort"] else "eco_temp_window"][b]
    want.append(restate(cfg, lo, hi, step["zone_temps"][b], [step["occupancy"]] * env.sim.Z, [(info[b, 0], info[b, 1])],
                        [(info[b, 2], info[b, 3])], step["prices"], env.config.time_step_sec))
  return want


@pytest.mark.parametrize("solver", ["gauss_seidel", "jacobi_fp32"])
def test_whole_steps_equal_the_restatement_and_change_nothing_but_the_reward(solver):
  need_gpu()
  B, T = 4, 3
  acts = _actions(T, B, 31)
  plain = BatchedEnvironment(_small(), B, collect_info=True, solver=solver)
  other = BatchedEnvironment(_small(), B, collect_info=True, solver=solver, reward_function=REWARD)
  assert other.sim.reward_function == REWARD and plain.sim.reward_function is None
  _start(plain)
  _start(other)
  x, y = _run(plain, acts), _run(other, acts)
  for t in range(T):
    for k in ("obs", "temps"):
      assert torch.equal(x[t][k], y[t][k]), (t, k)
    assert torch.equal(x[t]["info"][:, 0:7], y[t]["info"][:, 0:7]), t
    assert not torch.equal(x[t]["reward"], y[t]["reward"]), t
    reward = y[t]["reward"].cpu().numpy().astype(np.float64)
    info = y[t]["info"].cpu().numpy().astype(np.float64)
    for b, want in enumerate(_restated_rewards(other, y[t], REWARD)):
      print(solver, t, b, reward[b], float(want["agent_reward_value"]))
      assert reward[b] == pytest.approx(float(want["agent_reward_value"]), rel=2e-6, abs=0.0), (t, b)
      assert info[b, 7] == reward[b], (t, b)
      for field, col in INFO_COLUMNS.items():
        assert info[b, col] == pytest.approx(float(want[field]), rel=2e-6, abs=0.0), (t, b, field)
      assert not info[b, 13:].any(), (t, b)
  zt = np.concatenate([s["zone_temps"].reshape(-1) for s in y])
  lo, hi = SB1.comfort_temp_window
  assert (zt < lo).any() and (zt > hi).any() and ((zt >= lo) & (zt <= hi)).any()   # every branch of the productivity
  plain.close()
  other.close()


def test_the_default_is_untouched_by_a_kind_set_in_between():
  need_gpu()
  B, T = 4, 3
  acts = _actions(T, B, 32)
  never = BatchedEnvironment(_small(), B, collect_info=True)
  between = BatchedEnvironment(_small(), B, collect_info=True, reward_function=REWARD)
  _start(never)
  _start(between)
  x = _run(never, acts)
  y = _run(between, acts[:1])            # one step under the other reward (it does not touch the state) ...
  between.set_reward_function(None)      # ... then the default again
  assert between.sim.reward_function is None
  y += _run(between, acts[1:])
  assert not torch.equal(x[0]["reward"], y[0]["reward"])
  for t in range(1, T):
    for k in ("obs", "reward", "info", "temps"):
      assert torch.equal(x[t][k], y[t][k]), (t, k)
  assert between.sim.state_fingerprint() == never.sim.state_fingerprint()
  never.close()
  between.close()


def test_per_building_rows_keep_applying():
  need_gpu()
  B, T = 4, 2
  acts = _actions(T, B, 33)[:, :1].expand(T, B, 2).contiguous()   # the same actions for every building
  rows = {"max_productivity_personhour_usd": np.array([300.0, 450.0, 300.0, 120.0])}
  weights = dict(rows, productivity_weight=np.array([0.2, 0.9, 0.05, 0.5]))
  a = BatchedEnvironment(_small(), B, collect_info=True, reward_function=REWARD, building_params=BuildingParams(rows))
  b = BatchedEnvironment(_small(), B, collect_info=True, reward_function=REWARD, building_params=BuildingParams(weights))
  for env in (a, b):   # every building from the same grid
    env.reset()
    env.sim.reset(temps=torch.full((B, env.sim.H * env.sim.W), 292.5, dtype=torch.float64, device="cuda"))
  x, y = _run(a, acts), _run(b, acts)
  for t in range(T):
    reward = x[t]["reward"].cpu().numpy().astype(np.float64)
    assert reward[0] == reward[2] and len({reward[0], reward[1], reward[3]}) == 3, (t, reward)
    for i, want in enumerate(_restated_rewards(a, x[t], REWARD)):
      assert reward[i] == pytest.approx(float(want["agent_reward_value"]), rel=2e-6, abs=0.0), (t, i)
    for k in ("obs", "reward", "info", "temps"):   # the regret's weight is not this reward's
      assert torch.equal(x[t][k], y[t][k]), (t, k)
  a.close()
  b.close()


def test_a_rejected_building_gets_minus_infinity():
  need_gpu()
  B = 4
  env = BatchedEnvironment(_small(), B, collect_info=True, reward_function=REWARD)
  _start(env)
  rejected = torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device="cuda")
  step = _run(env, _actions(1, B, 34), rejected=rejected)[0]
  reward = step["reward"].cpu().numpy()
  assert np.isneginf(reward[[1, 3]]).all() and np.isfinite(reward[[0, 2]]).all(), reward
  env.close()


def test_mixed_classes_with_a_reward_function_each():
  need_gpu()
  plans = [_small(), _row_plan(3)]
  rewards = [None, REWARD]
  T = 3
  mixed = MixedBatchedEnvironment([(p, 2) for p in plans], collect_info=True, reward_function=rewards)
  singles = [BatchedEnvironment(p, 2, collect_info=True, reward_function=r) for p, r in zip(plans, rewards)]
  acts = _actions(T, mixed.batch_size, 35)
  mixed.reset()
  for s in singles:
    s.reset()
  for t in range(T):
    ts = mixed.step(acts[t])
    for k, (s, (a, b)) in enumerate(zip(singles, mixed.slices)):
      tk = s.step(acts[t, a:b].contiguous())
      assert torch.equal(ts.observation[a:b, :mixed.observation_widths[k]], tk.observation), (t, k)
      assert torch.equal(ts.reward[a:b], tk.reward), (t, k)
      assert torch.equal(mixed.envs[k].info, s.info), (t, k)
  assert float(mixed.envs[0].info[0, 18]) == 1.0 and not mixed.envs[1].info[:, 13:].any()   # regret / the other reward
  mixed.set_reward_function(REWARD)   # one for all
  assert [e.sim.reward_function for e in mixed.envs] == [REWARD, REWARD]
  with pytest.raises(ValueError, match="one per class"):
    mixed.set_reward_function([REWARD])
  with pytest.raises(ValueError, match="one per class"):
    MixedBatchedEnvironment([(p, 2) for p in plans], reward_function=[REWARD, None, None])
  mixed.close()
  for s in singles:
    s.close()


def test_snapshots_carry_the_reward_function():
  need_gpu()
  B = 4
  acts = _actions(5, B, 36)
  plain = BatchedEnvironment(_small(), B, collect_info=True)
  other = BatchedEnvironment(_small(), B, collect_info=True, reward_function=REWARD)
  scaled = BatchedEnvironment(_small(), B, collect_info=True,
                              reward_function=SetpointEnergyCarbonReward(1.5, 0.75, 0.2, -3.0, 51.0))
  for env in (plain, other, scaled):
    _start(env)
  assert len(plain.sim.state_fingerprint()) == 5   # the default's is what it was: earlier checkpoints still load
  assert other.sim.state_fingerprint()[:5] == plain.sim.state_fingerprint()
  assert other.sim.state_fingerprint()[5] == ("reward_function",) + REWARD.as_tuple()
  _run(plain, acts[:2])
  _run(other, acts[:2])
  snap_plain, snap = plain.snapshot(), other.snapshot()
  for env, s in ((other, snap_plain), (plain, snap), (scaled, snap)):   # across kinds, and across constants
    with pytest.raises(ValueError, match="another floor plan, configuration"):
      env.restore(s)
  first = _run(other, acts[2:])
  other.restore(EnvSnapshot.from_state_dict(snap.state_dict(), "cuda"))   # (through the form a checkpoint file holds)
  again = _run(other, acts[2:])
  for t, (u, v) in enumerate(zip(first, again)):
    for k in ("obs", "reward", "info", "temps"):
      assert torch.equal(u[k], v[k]), (t, k)
  other.set_reward_function(None)   # ... and a handle back on the default takes the default's snapshot
  other.restore(snap_plain)
  for env in (plain, other, scaled):
    env.close()


def test_refusals():
  need_gpu()
  sim = BatchedSimulator(_small(), SB1, 2, 12.0)
  fn = _ffi.reward_entry("sb_set_reward_function")
  good = (1, 1.0, 1.0, 0.2, 0.0, 1.0)
  for bad, word in (((1, 1.0, 1.0, 0.2, 0.0, 0.0), b"normalizer_scale must not be 0"),
                    ((1, float("nan"), 1.0, 0.2, 0.0, 1.0), b"energy_cost_weight is not finite"),
                    ((1, 1.0, 1.0, float("inf"), 0.0, 1.0), b"carbon_cost_factor is not finite"),
                    ((7, 1.0, 1.0, 0.2, 0.0, 1.0), b"unknown kind 7")):
    assert fn(sim._h, C.byref(_ffi.RewardConfig(*bad))) == -1, bad   # SB_ERR_INVALID
    assert word in sim._lib.sb_last_error(), (bad, sim._lib.sb_last_error())
  assert fn(sim._h, C.byref(_ffi.RewardConfig(*good))) == 0
  assert fn(sim._h, C.byref(_ffi.RewardConfig(0, float("nan"), 0.0, 0.0, 0.0, 0.0))) == 0   # the default reads no field
  assert fn(sim._h, None) == 0
  late = SetpointEnergyCarbonReward(1.0, 1.0, 0.2)
  late.reward_normalizer_scale = 0.0   # past the constructor's check: the library's refusal is a ValueError
  with pytest.raises(ValueError, match="normalizer_scale"):
    sim.set_reward_function(late)
  assert sim.reward_function is None
  with pytest.raises(ValueError, match="SetpointEnergyCarbonReward"):
    sim.set_reward_function("regret")
  sim.close()
