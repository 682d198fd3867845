"""The configurable action set (boiler / air-handler heating + cooling setpoints / VAV damper
command) and the action-rejection path, against a rollout of the reference itself
(tests/golden/h2_sb1_r9_actions.npz from oracle/gen_golden_actions.py: SimulatorBuilding +
the reward function in Environment._step's order; at some steps request_action is never
reached -- RejectionSimulatorBuilding -- and at others the damper command leaves [0, 1]).

CPU: the oracle's restatement of those paths is bit-exact.  GPU (-m gpu): the HIP path through
the C ABI (sb_params.act_kind / sb_step_in.reject_dev) within the usual tolerances, and the
reward is -inf exactly where the reference's Environment returns ACTION_REJECTION_REWARD."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.golden_util import load, oracle_params, oracle_plan
from tests.twins import (T_TOL, native_value, oracle_params_of, oracle_plan_of, plan_from_npz, rates_match, step_in,
                         step_kwargs)


def _ulp32(a, b):
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _damper_cmd(g, t, Z):
  cmd = np.full(Z, np.nan)
  cmd[int(g["action_zone"][3])] = float(g["action_native_all"][t][3])
  return cmd


def test_oracle_restates_rejections_and_the_extra_actions():
  g = load("h2_sb1_r9_actions.npz")
  plan = oracle_plan(load("plan_r9_sb1.npz"))
  prm = oracle_params(g["params_json"])
  ob = orc.OracleBuilding(plan, prm, float(g["initial_temp"]))
  T, Z = len(g["n_sweeps"]), len(plan.zones)
  assert g["rejected"].sum() == 6 and (g["action_accepted"] == 0).sum() == 9
  for t in range(T):
    nat = g["action_native_all"][t]
    out = ob.step(
        now_ts=float(g["ts_seconds"][t]), t_amb_now=float(g["t_amb_now"][t]), h_conv=float(g["h_conv"]),
        t_amb_next=float(g["t_amb_next"][t]), comfort_now=bool(g["comfort_now"][t]),
        comfort_prev=g["comfort_prev"][t] == 1, comfort_next=bool(g["comfort_next"][t]),
        occupancy=float(g["occupancy"][t]), e_price=float(g["e_price"][t]), e_carbon=float(g["e_carbon"][t]),
        g_price=float(g["g_price"][t]), g_carbon=float(g["g_carbon"][t]), action=nat[:2], observe=True,
        reject=bool(g["rejected"][t]), cool_sp=float(nat[2]), damper_cmd=_damper_cmd(g, t, Z))
    assert out["action_accepted"] == bool(g["action_accepted"][t]), t
    assert out["n_sweeps"] == int(g["n_sweeps"][t]), t
    assert np.array_equal(out["zone_temp_post"], g["zone_temp_post"][t]), t
    assert np.array_equal(out["mode"], g["mode"][t]) and np.array_equal(out["damper"], g["damper"][t]), t
    assert out["blr_tank_temp"] == g["blr_tank_temp"][t] and out["t_supply_air"] == g["t_supply_air"][t], t
    rates = np.array([out["blower_rate"], out["ac_rate"], out["gas_rate"], out["pump_rate"]], np.float32)
    assert _ulp32(rates, g["rates"][t]).max() <= 1, (t, rates, g["rates"][t])
    assert _ulp32(out["reward"], g["reward"][t]) <= 2, t
  assert np.array_equal(ob.grid(), g["final_grid"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["reg", "lds"])
def test_hip_action_set_and_rejections_against_reference_golden(path, monkeypatch):
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  from sbsim_amd import _ffi
  from sbsim_amd.environment import ACTION_REJECTION_REWARD, BatchedSimulator, SimConfig, observation_field_names
  from tests.parity import step_buffers
  if path == "lds":
    monkeypatch.setenv("SBSIM_FORCE_LDS_PATH", "1")
  g = load("h2_sb1_r9_actions.npz")
  cfg = SimConfig.sb1()
  cfg.action_names = tuple(str(n) for n in g["action_names"])
  cfg.action_zones = tuple(int(z) for z in g["action_zone"])
  cfg.action_ranges = tuple((float(lo), float(hi)) for lo, hi in g["action_ranges"])
  B = 6
  sim = BatchedSimulator(plan_from_npz(load("plan_r9_sb1.npz")), cfg, B, float(g["h_conv"]))
  assert sim.n_actions == 4 and sim.launch_info["path"] == (1 if path == "reg" else 0)
  sim.reset()
  obs, rew, info = step_buffers(sim)
  col_aux = observation_field_names([str(z) for z in g["zone_names"]], True)[4]
  T = len(g["n_sweeps"])
  # buildings 0..3 follow the golden (its rejections included); 4 and 5 are never rejected and
  # must differ from it after the first rejected step (the mask is per building)
  for t in range(T):
    act = torch.tensor(np.tile(g["actions_norm"][t], (B, 1)), dtype=torch.float32, device="cuda")
    rej = torch.zeros((B,), dtype=torch.uint8, device="cuda")
    rej[:4] = int(g["rejected"][t])
    si = step_in(g, t)
    si.reject_dev = rej.data_ptr()
    sim.step(act, si, obs, rew, info)
    i = info.cpu().numpy().astype(np.float64)
    zt = sim.zone_temps().cpu().numpy()
    assert (i[:4, 4] == g["n_sweeps"][t]).all(), (t, i[:, 4], g["n_sweeps"][t])
    assert np.abs(zt[:4] - g["zone_temp_post"][t]).max() < T_TOL, t
    assert np.array_equal(sim.modes().cpu().numpy()[:4], np.tile(g["mode"][t], (4, 1))), t
    assert rates_match(i[:4, :4], g["rates"][t].astype(np.float64)), t
    r = rew.cpu().numpy().astype(np.float64)
    if g["action_accepted"][t]:
      assert np.abs(r[:4] - float(g["reward"][t])).max() < 1e-6, t
    else:   # environment.py:1301-1302
      assert (r[:4] == ACTION_REJECTION_REWARD).all(), (t, r)
      assert np.abs(i[:4, 7] - float(g["reward"][t])).max() < 1e-6   # what compute_reward returned
    if g["rejected"][t]:
      assert np.isfinite(r[4:]).all() or not g["action_accepted"][t]
    o = obs.cpu().numpy()
    assert np.allclose(o[:4, :col_aux], g["obs"][t], rtol=1e-6, atol=1e-6), t
  grid = sim.temps().cpu().numpy()
  assert np.abs(grid[:4] - g["final_grid"]).max() < T_TOL
  assert np.abs(grid[4:] - g["final_grid"]).max() > 1e-3   # the never-rejected buildings went another way
  sc = sim.scalars().cpu().numpy()
  assert np.allclose(sc[:4, 8], g["blr_tank_temp"][-1], atol=1e-9)
  sim.close()


@pytest.mark.gpu
def test_hip_simulator_building_replays_the_reference_rollout():
  """``HipSimulatorBuilding`` -- BaseBuilding's request / response interface
  (simulator_building.py:151-315) on the HIP library -- driven exactly like the harness that made
  tests/golden/h2_sb1_r9_random.npz drove the reference's SimulatorBuilding: request_action ->
  wait_time -> request_observations -> reward_info, one simulated day."""
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  import datetime as dt
  from sbsim_amd import building_adapter as ba
  g = load("h2_sb1_r9_random.npz")
  start = dt.datetime.fromisoformat(str(g["start_timestamp"]))
  b = ba.HipSimulatorBuilding(plan_from_npz(load("plan_r9_sb1.npz")), start_timestamp=start, holiday_calendar=None)
  assert b.time_step_sec == 300.0 and b.current_timestamp == start and len(b.zones) == 9 and len(b.devices) == 11
  req = b.observation_request_for_all_fields()
  names = [f"{r.device_id}/{r.measurement_name}" for r in req.single_observation_requests]
  assert [n.split("/")[1] for n in names] == [str(n).split("/")[-1] for n in g["obs_names"]]
  first = b.request_observations(req)
  assert np.allclose([r.continuous_value for r in first.single_observation_responses], g["obs_reset"], rtol=1e-6, atol=1e-6)
  T = len(g["n_sweeps"])
  for t in range(T):
    assert int(b.current_timestamp.replace(tzinfo=dt.timezone.utc).timestamp()) == int(g["ts_seconds"][t])
    areq = ba.ActionRequest(timestamp=b.current_timestamp, single_action_requests=[
        ba.SingleActionRequest("boiler_id", "supply_water_setpoint", float(g["action_native"][t][0])),
        ba.SingleActionRequest("air_handler_id", "supply_air_heating_temperature_setpoint", float(g["action_native"][t][1]))])
    resp = b.request_action(areq)
    assert all(r.response_type == ba.ActionResponseType.ACCEPTED for r in resp.single_action_responses)
    b.wait_time()
    obs = b.request_observations(req)
    vals = np.array([r.continuous_value for r in obs.single_observation_responses])
    assert all(r.observation_valid for r in obs.single_observation_responses)
    assert np.allclose(vals, g["obs"][t], rtol=1e-6, atol=1e-6), t
    ri = b.reward_info
    zt = np.array([z.zone_air_temperature for z in ri.zone_reward_infos.values()])
    assert np.abs(zt - g["ri_zone_temp"][t]).max() <= 4e-5, t   # fp32 fields of temperatures within 1e-8 K
    assert np.allclose([z.heating_setpoint_temperature for z in ri.zone_reward_infos.values()], g["ri_heat_sp"][t])
    assert np.allclose([z.cooling_setpoint_temperature for z in ri.zone_reward_infos.values()], g["ri_cool_sp"][t])
    assert np.allclose([z.average_occupancy for z in ri.zone_reward_infos.values()], g["ri_occ"][t])
    ah, bl = ri.air_handler_reward_infos["air_handler_id"], ri.boiler_reward_infos["boiler_id"]
    rates = [ah.blower_electrical_energy_rate, ah.air_conditioning_electrical_energy_rate,
             bl.natural_gas_heating_energy_rate, bl.pump_electrical_energy_rate]
    assert rates_match(rates, g["rates"][t].astype(np.float64)), t
    assert abs(b.last_reward - float(g["reward"][t])) < 1e-6, t
    assert b.num_occupants == int(g["num_occupants"][t]), t
  # an unknown device, a field that is not settable, a damper command the handle does not drive
  resp = b.request_action(ba.ActionRequest(single_action_requests=[
      ba.SingleActionRequest("no_such_device", "supply_water_setpoint", 340.0),
      ba.SingleActionRequest("boiler_id", "supply_water_temperature_sensor", 340.0),
      ba.SingleActionRequest(b.devices[2].device_id, "supply_air_damper_percentage_command", 0.5)]))
  assert [r.response_type for r in resp.single_action_responses] == [
      ba.ActionResponseType.REJECTED_INVALID_DEVICE, ba.ActionResponseType.REJECTED_NOT_ENABLED_OR_AVAILABLE,
      ba.ActionResponseType.REJECTED_NOT_ENABLED_OR_AVAILABLE]
  bad = b.request_observations(ba.ObservationRequest(single_observation_requests=[ba.SingleObservationRequest("boiler_id", "nope")]))
  assert not bad.single_observation_responses[0].observation_valid
  b.close()


@pytest.mark.gpu
def test_hip_simulator_building_rejections_and_damper_commands():
  """The same interface on the four-column action set of h2_sb1_r9_actions.npz: a step whose request
  the building rejected is ``wait_time`` without ``request_action``; a damper command outside [0, 1]
  comes back REJECTED_NOT_ENABLED_OR_AVAILABLE while the other setpoints apply."""
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  import datetime as dt
  from sbsim_amd import building_adapter as ba
  from sbsim_amd.environment import SimConfig
  g = load("h2_sb1_r9_actions.npz")
  cfg = SimConfig.sb1()
  cfg.action_names = tuple(str(n) for n in g["action_names"])
  cfg.action_zones = tuple(int(z) for z in g["action_zone"])
  cfg.action_ranges = tuple((float(lo), float(hi)) for lo, hi in g["action_ranges"])
  b = ba.HipSimulatorBuilding(plan_from_npz(load("plan_r9_sb1.npz")), config=cfg, holiday_calendar=None,
                              start_timestamp=dt.datetime.fromisoformat(str(g["start_timestamp"])))
  vav = b.devices[2 + int(g["action_zone"][3])].device_id
  for t in range(len(g["n_sweeps"])):
    nat = [float(x) for x in g["action_native_all"][t]]
    if not g["rejected"][t]:
      resp = b.request_action(ba.ActionRequest(timestamp=b.current_timestamp, single_action_requests=[
          ba.SingleActionRequest("boiler_id", "supply_water_setpoint", nat[0]),
          ba.SingleActionRequest("air_handler_id", "supply_air_heating_temperature_setpoint", nat[1]),
          ba.SingleActionRequest("air_handler_id", "supply_air_cooling_temperature_setpoint", nat[2]),
          ba.SingleActionRequest(vav, "supply_air_damper_percentage_command", nat[3])]))
      ok = all(r.response_type == ba.ActionResponseType.ACCEPTED for r in resp.single_action_responses)
      assert ok == bool(g["action_accepted"][t]), t
      assert [r.response_type for r in resp.single_action_responses[:3]] == [ba.ActionResponseType.ACCEPTED] * 3
    b.wait_time()
    assert int(b._info_row[4]) == int(g["n_sweeps"][t]), t
    zt = b.env.sim.zone_temps()[0].cpu().numpy()
    assert np.abs(zt - g["zone_temp_post"][t]).max() < T_TOL, t
    assert abs(b.last_reward - float(g["reward"][t])) < 1e-6, t
  # a damper command of -inf: the host says REJECTED and the device must reject the step too (reward -inf,
  # environment.py:1301-1302) -- the raw value would read as "field not mentioned" there (<= SB_ACTION_KEEP)
  resp = b.request_action(ba.ActionRequest(timestamp=b.current_timestamp, single_action_requests=[
      ba.SingleActionRequest("boiler_id", "supply_water_setpoint", 340.0),
      ba.SingleActionRequest(vav, "supply_air_damper_percentage_command", float("-inf"))]))
  assert resp.single_action_responses[1].response_type == ba.ActionResponseType.REJECTED_NOT_ENABLED_OR_AVAILABLE
  b.wait_time()
  assert float(b.env._reward[0]) == float("-inf")
  b.close()


@pytest.mark.gpu
def test_hip_simulator_building_on_a_four_wavefront_plan(monkeypatch):
  """The single-building adapter on a 205 x 89 / 40-zone plan (step_band.hip, four wavefronts per building; one
  building = one workgroup): request_action -> wait_time -> request_observations -> reward_info, against a second
  adapter on the LDS-grid kernel (SBSIM_NO_BAND_PATH=1) given the same requests: sweep counts EQUAL, observations and
  rewards equal to float32 rounding, grids within 1e-9 K."""
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  from sbsim_amd import building_adapter as ba
  from sbsim_amd.environment import SimConfig
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  plan = FloorPlan.from_file_input(rectangular_floor_plan((10, 4), (19, 20)), Materials.sb1(), 10.0, 300.0)
  cfg = SimConfig.sb1()
  b = ba.HipSimulatorBuilding(plan, cfg, holiday_calendar=None)
  monkeypatch.setenv("SBSIM_NO_BAND_PATH", "1")
  ref = ba.HipSimulatorBuilding(plan, cfg, holiday_calendar=None)
  monkeypatch.delenv("SBSIM_NO_BAND_PATH")
  assert b.env.sim.launch_info["kernel"] == 5 and b.env.sim.launch_info["waves_per_building"] == 4
  assert ref.env.sim.launch_info["kernel"] == 0 and len(b.zones) == 40
  rs = np.random.RandomState(5)
  for t in range(6):
    sw, sa = float(rs.uniform(310.0, 350.0)), float(rs.uniform(285.0, 295.0))
    out = []
    for bld in (b, ref):
      resp = bld.request_action(ba.ActionRequest(timestamp=bld.current_timestamp, single_action_requests=[
          ba.SingleActionRequest("boiler_id", "supply_water_setpoint", sw),
          ba.SingleActionRequest("air_handler_id", "supply_air_heating_temperature_setpoint", sa)]))
      assert all(r.response_type == ba.ActionResponseType.ACCEPTED for r in resp.single_action_responses)
      bld.wait_time()
      obs = bld.request_observations(bld.observation_request_for_all_fields())
      out.append((np.array([r.continuous_value for r in obs.single_observation_responses]), bld.last_reward, bld._info_row[4]))
    assert out[0][2] == out[1][2] >= 1                       # Gauss-Seidel sweeps of the step
    assert np.allclose(out[0][0], out[1][0], rtol=1e-6, atol=1e-6) and abs(out[0][1] - out[1][1]) < 1e-6
  assert np.abs(b.env.sim.temps().cpu().numpy() - ref.env.sim.temps().cpu().numpy()).max() < 1e-9
  b.close()
  ref.close()


@pytest.mark.gpu
def test_action_vector_as_wide_as_the_building_has_setpoints():
  """ABI 8: one action column per settable field (environment/environment.py:591-653 admits every device setpoint with a
  normaliser): the boiler's, the air handler's two and one damper command per VAV of a 126-zone plan -- a 129-column
  vector (the 16-column limit of ABI <= 7 did not hold an SB1 agent that drives its dampers, vav.py:66-70).  Against
  oracle twins (their `damper_cmd` path, sb_oracle.c: vav.py:125-129): some columns left out of a request
  (SB_ACTION_KEEP), some commands outside [0, 1] (that action is rejected, the others apply, the reward is -inf)."""
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  from oracle import oracle as orc   # checker only
  from sbsim_amd import _ffi
  from sbsim_amd.environment import ACTION_REJECTION_REWARD, BatchedSimulator, SimConfig
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  from tests.parity import step_buffers
  plan = FloorPlan.from_file_input(rectangular_floor_plan((14, 9), (8, 7)), Materials.sb1(), 10.0, 300.0)
  Z = len(plan.zone_cell_lists())
  assert Z == 126
  cfg = SimConfig.sb1()
  cfg.action_names = ("supply_water_setpoint", "supply_air_heating_temperature_setpoint",
                      "supply_air_cooling_temperature_setpoint") + ("supply_air_damper_percentage_command",) * Z
  # the dampers are listed in reverse zone order: a column is not its zone's index
  cfg.action_zones = (0, 0, 0) + tuple(range(Z - 1, -1, -1))
  cfg.action_ranges = ((310.0, 355.0), (285.0, 295.0), (296.0, 305.0)) + ((-0.001, 1.001),) * Z   # a normaliser that can overshoot [0, 1] (one damper in 500)
  g = load("h2_sb1_r9_random.npz")
  B, T = 6, 8
  sim = BatchedSimulator(plan, cfg, B, float(g["h_conv"]))
  assert sim.n_actions == 3 + Z
  rs = np.random.RandomState(5)
  H, W = plan.shape
  init = np.clip(294.0 + rs.randn(B, 1) + np.zeros((B, H * W)), 285.0, 305.0)
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  oplan, oprm = oracle_plan_of(plan), oracle_params_of(cfg)
  twins = [orc.OracleBuilding(oplan, oprm, 0.0, reset_temps=init[b]) for b in range(B)]
  obs, rew, info = step_buffers(sim)
  n_rejected = 0
  for t in range(T):
    norm = rs.uniform(-1, 1, size=(B, 3 + Z)).astype(np.float32)
    native = np.empty((B, 3 + Z), dtype=np.float32)
    for i, (lo, hi) in enumerate(cfg.action_ranges):
      native[:, i] = [native_value(a, lo, hi) for a in norm[:, i]]
    keep = rs.rand(B, 3 + Z) < 0.3                      # the request does not mention these fields
    keep[:, :2] = False                                 # (the twins' interface always carries the two SB1 setpoints)
    if t % 2 == 0:                                      # every other step in native units with left-out columns
      act = native.copy()
      act[keep] = _ffi.SB_ACTION_KEEP
    else:
      act, keep = norm, np.zeros_like(keep)
    si = step_in(g, t + 100)
    si.actions_native = int(t % 2 == 0)
    sim.step(torch.tensor(act, device="cuda"), si, obs, rew, info)
    i_ = info.cpu().numpy().astype(np.float64)
    zt, r = sim.zone_temps().cpu().numpy(), rew.cpu().numpy()
    dm = sim._get(sim._lib.sb_get_zone_power, (B, Z), torch.float64).cpu().numpy()
    for b in range(B):
      cmd = np.full(Z, np.nan)
      for col in range(3, 3 + Z):
        if not keep[b, col]:
          cmd[cfg.action_zones[col]] = float(native[b, col])
      o = twins[b].step(**step_kwargs(g, t + 100, t, cfg, norm[b, :2]),   # (the first two columns: native[b, :2])
                        cool_sp=None if keep[b, 2] else float(native[b, 2]), damper_cmd=cmd)
      assert i_[b, 4] == o["n_sweeps"], (t, b, i_[b, 4], o["n_sweeps"])
      assert np.abs(zt[b] - o["zone_temp_post"]).max() < T_TOL, (t, b)
      assert np.allclose(dm[b], o["q_zone"], rtol=1e-12, atol=1e-9), (t, b)     # every zone's VAV power: every damper landed
      if o["action_accepted"]:
        assert abs(float(r[b]) - o["reward"]) < 1e-6, (t, b)
      else:
        n_rejected += 1
        assert r[b] == ACTION_REJECTION_REWARD and abs(i_[b, 7] - o["reward"]) < 1e-6, (t, b)
  assert 0 < n_rejected < B * T          # the overshooting normaliser rejected some steps, not all
  sim.close()


@pytest.mark.gpu
def test_damper_commands_of_exactly_zero_keep_the_grid_finite():
  """A normalised command of -1 under a (0, 1) range is a damper of exactly 0, which vav.py:125-129 accepts and vav.py:177
  asserts on.  Stated departure (sb_step's header comment): such a zone gets no air -- q_zone = 0 (the reference's own
  guard, vav.py:207-208), no air demand, the air handler's supply temperature in the return-water average -- and its
  reheat demand still counts.  The 129-column test's plan; some dampers held at -1 for every step, against oracle twins
  at the rollouts' tolerances, the sweep counts EQUAL and every stored value finite."""
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("no GPU")
  from oracle import oracle as orc   # checker only
  from sbsim_amd.environment import BatchedSimulator, SimConfig
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  from tests.parity import step_buffers
  from tests.twins import REWARD_TOL
  plan = FloorPlan.from_file_input(rectangular_floor_plan((14, 9), (8, 7)), Materials.sb1(), 10.0, 300.0)
  Z = len(plan.zone_cell_lists())
  assert Z == 126
  cfg = SimConfig.sb1()
  cfg.action_names = ("supply_water_setpoint", "supply_air_heating_temperature_setpoint",
                      "supply_air_cooling_temperature_setpoint") + ("supply_air_damper_percentage_command",) * Z
  cfg.action_zones = (0, 0, 0) + tuple(range(Z - 1, -1, -1))
  cfg.action_ranges = ((310.0, 355.0), (285.0, 295.0), (296.0, 305.0)) + ((0.0, 1.0),) * Z
  g = load("h2_sb1_r9_random.npz")
  B, T = 6, 5
  sim = BatchedSimulator(plan, cfg, B, float(g["h_conv"]))
  rs = np.random.RandomState(11)
  H, W = plan.shape
  init = np.clip(292.0 + 2.0 * rs.randn(B, 1) + np.zeros((B, H * W)), 285.0, 305.0)   # some buildings heat: valves open
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  oplan, oprm = oracle_plan_of(plan), oracle_params_of(cfg)
  twins = [orc.OracleBuilding(oplan, oprm, 0.0, reset_temps=init[b]) for b in range(B)]
  obs, rew, info = step_buffers(sim)
  shut = rs.rand(B, Z) < 0.3            # these zones' dampers are held at 0; building 5: every one of them
  shut[5] = True
  shut[0] = False
  n_heating_without_air = 0
  for t in range(T):
    norm = rs.uniform(-1, 1, size=(B, 3 + Z)).astype(np.float32)
    for b in range(B):
      for z in np.nonzero(shut[b])[0]:
        norm[b, 3 + (Z - 1 - z)] = np.float32(-1.0)
    sim.step(torch.tensor(norm, device="cuda"), step_in(g, t + 100), obs, rew, info)
    i_ = info.cpu().numpy().astype(np.float64)
    zt, r = sim.zone_temps().cpu().numpy(), rew.cpu().numpy()
    dm = sim.zone_power().cpu().numpy()
    sc = sim.scalars().cpu().numpy()
    assert np.isfinite(dm).all() and np.isfinite(sc).all() and np.isfinite(i_).all() and np.isfinite(r).all(), t
    assert np.isfinite(sim.temps().cpu().numpy()).all(), t
    for b in range(B):
      cmd = np.array([float(native_value(norm[b, 3 + (Z - 1 - z)], 0.0, 1.0)) for z in range(Z)])
      assert (cmd[shut[b]] == 0.0).all()
      o = twins[b].step(**step_kwargs(g, t + 100, t, cfg, norm[b, :2]), cool_sp=float(native_value(norm[b, 2], 296.0, 305.0)),
                        damper_cmd=cmd)
      assert o["action_accepted"] and i_[b, 4] == o["n_sweeps"], (t, b, i_[b, 4], o["n_sweeps"])
      assert np.abs(zt[b] - o["zone_temp_post"]).max() < T_TOL, (t, b)
      assert np.allclose(dm[b], o["q_zone"], rtol=1e-12, atol=1e-9) and not dm[b][shut[b]].any(), (t, b)
      assert rates_match(i_[b, :4], np.array([o["blower_rate"], o["ac_rate"], o["gas_rate"], o["pump_rate"]], np.float64)), (t, b)
      assert abs(float(r[b]) - o["reward"]) < REWARD_TOL, (t, b)
      assert sc[b, 3] == o["ahu_count"] == int((~shut[b]).sum()) and sc[b, 6] == o["blr_count"], (t, b)
      assert sc[b, 7] == pytest.approx(o["blr_return_temp"], rel=1e-12), (t, b)
      n_heating_without_air += int(((o["valve"] == 1) & shut[b]).sum())
  assert n_heating_without_air > 0      # the 0/0 of the unguarded formula: a shut damper on an open reheat valve
  assert np.abs(sim.temps().cpu().numpy().reshape(B, -1) - np.stack([tw.temp for tw in twins])).max() < T_TOL
  sim.close()
