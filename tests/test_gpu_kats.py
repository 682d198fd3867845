"""The reference's own known answers asked of the HIP path itself: k_pre and k_post -- the kernels
sb_step launches around the sweep -- run on prescribed state of one building through the C ABI's
known-answer taps (sb_tap_pre / sb_tap_post).  tests/test_device_kats.py and
tests/test_oracle_golden.py ask the same vectors of the CPU oracle.

  reward vectors        reward/setpoint_energy_carbon_regret_test.py:30-167 (tests/golden/reward_kat.json)
  boiler                simulator/boiler_test.py:131-176 (thermal rates), :431-439 (dissipation), :399-416
                        (pump), :197-230 (tank lag)
  air handler           simulator/air_handler_test.py:110-175 (mixed / supply temperature), :335-420 (powers)
  VAV                   simulator/vav_test.py:198-262 (zone supply temperature, energy), :150-174 (settings)
  thermostat            simulator/thermostat_test.py:47-135
"""
import ctypes as C
import dataclasses
import datetime as dt
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan  # noqa: E402
from tests.parity import need_gpu  # noqa: E402

C_AIR, C_WATER = 1006.0, 4180.0   # utils/constants.py:21-24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _plan2():
  return FloorPlan.from_file_input(rectangular_floor_plan((1, 2), (8, 8)), Materials.sb1(), 10.0, 300.0)


class Taps:
  """A two-zone handle whose building 0 is driven through the taps."""

  def __init__(self, **cfg):
    self.cfg = dataclasses.replace(SimConfig.sb1(), **cfg)
    self.sim = BatchedSimulator(_plan2(), self.cfg, 2, 100.0)
    self.Z = self.sim.Z
    assert self.Z == 2
    self.lib = self.sim._lib

  def close(self):
    self.sim.close()

  @staticmethod
  def step_in(t_now=280.0, t_next=280.0, comfort_now=1, comfort_prev=1, comfort_next=1, has_action=0,
              occupancy=0.0, e_price=0.0, e_carbon=0.0, g_price=0.0, g_carbon=0.0):
    si = _ffi.StepIn()
    si.t_amb_now, si.t_amb_next = t_now, t_next
    si.comfort_now, si.comfort_prev, si.comfort_next, si.has_action = comfort_now, comfort_prev, comfort_next, has_action
    si.occupancy = occupancy
    si.e_price, si.e_carbon, si.g_price, si.g_carbon = e_price, e_carbon, g_price, g_carbon
    return si

  def scalars(self, **over):
    c = self.cfg
    s = np.zeros(16)
    s[0], s[1], s[4] = c.ahu_heating_air_temp_setpoint, c.ahu_cooling_air_temp_setpoint, c.boiler_reheat_water_setpoint
    s[8] = c.boiler_reheat_water_setpoint
    s[11] = 290.0
    names = dict(heat_sp=0, cool_sp=1, blr_sp=4, tank=8, tank_change=9, duration=10, recirc=11)
    for k, v in over.items():
      s[names[k]] = v
    return s

  def pre(self, zone_temps, modes=None, scalars=None, actions=None, si=None):
    zt = np.ascontiguousarray(zone_temps, dtype=np.float64)
    md = None if modes is None else np.ascontiguousarray(modes, dtype=np.int32)
    sc = None if scalars is None else np.ascontiguousarray(scalars, dtype=np.float64)
    ac = None if actions is None else np.ascontiguousarray(actions, dtype=np.float32)
    bld = _ffi.TapBld()
    q, dmp, mo = np.zeros(self.Z), np.zeros(self.Z), np.zeros(self.Z, dtype=np.int32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    _ffi.check(self.lib.sb_tap_pre(self.sim._h, 0, p(zt, C.c_double), p(md, C.c_int32), p(sc, C.c_double),
                                   p(ac, C.c_float), C.byref(si or self.step_in()), C.byref(bld),
                                   p(q, C.c_double), p(dmp, C.c_double), p(mo, C.c_int32)), "sb_tap_pre")
    return bld, q, dmp, mo

  def post(self, bld, zone_temps, grid_mean, si):
    zt = np.ascontiguousarray(zone_temps, dtype=np.float64)
    rew = C.c_float(0.0)
    info = np.zeros(_ffi.SB_INFO_STRIDE, dtype=np.float32)
    _ffi.check(self.lib.sb_tap_post(self.sim._h, 0, C.byref(bld), zt.ctypes.data_as(C.POINTER(C.c_double)),
                                    float(grid_mean), 1, C.byref(si), C.byref(rew),
                                    info.ctypes.data_as(C.POINTER(C.c_float))), "sb_tap_post")
    return float(rew.value), info.astype(np.float64)


def _bld(**kw):
  b = _ffi.TapBld()
  b.t_now = b.t_next = 280.0
  b.heat_sp, b.cool_sp, b.blr_sp, b.t_sa = 285.0, 298.0, 360.0, 285.0
  for k, v in kw.items():
    setattr(b, k, v)
  return b


def test_reward_known_answers_through_k_post():
  """setpoint_energy_carbon_regret_test.py:30-167: every row's energy rates are PRODUCED by k_post from
  device state chosen for it (blower = flow * dp with full recirculation, air conditioning =
  flow * c_air * (setpoint - mixed), gas = the tank's dissipation, pump = flow * rho g head)."""
  need_gpu()
  with open(os.path.join(GOLDEN, "reward_kat.json")) as fh:
    kat = json.load(fh)
  c = kat["config"]
  price, carbon = c["usd_per_kwh"] / 3600.0 / 1000.0, c["kg_per_kwh"] / 3600.0 / 1000.0
  base = SimConfig.sb1()
  r2 = base.boiler_tank_radius + base.boiler_insulation_thickness   # boiler.py:275-320: watts per kelvin
  k_diss = base.boiler_tank_length * 2.0 * math.pi / (
      math.log(r2 / base.boiler_tank_radius) / base.boiler_insulation_conductivity + 1.0 / base.boiler_convection_coefficient / r2)
  for row in kat["rows"]:
    flow, wflow = 2.0, 0.5
    t = Taps(max_productivity_personhour_usd=c["max_productivity_personhour_usd"],
             min_productivity_personhour_usd=c["min_productivity_personhour_usd"],
             productivity_decay_stiffness=c["productivity_decay_stiffness"],
             productivity_midpoint_delta=c["productivity_midpoint_delta"],
             max_electricity_rate=c["max_electricity_rate"], max_natural_gas_rate=c["max_natural_gas_rate"],
             productivity_weight=row["productivity_weight"], energy_cost_weight=row["energy_cost_weight"],
             carbon_emission_weight=row["carbon_emission_weight"],
             comfort_temp_window=(c["heating_setpoint"], c["cooling_setpoint"]), time_step_sec=c["dt_sec"],
             ahu_recirculation=1.0, ahu_fan_efficiency=1.0, ahu_fan_differential_pressure=max(row["blower"], 0.0) / flow,
             boiler_water_pump_efficiency=1.0,
             boiler_water_pump_differential_head=row["pump"] / (1000.0 * 9.8 * wflow))
    mixed = 290.0
    d_ac = row["air_conditioning"] / (flow * C_AIR)
    t_out = 280.0
    supply_w = t_out + row["natural_gas"] / k_diss
    bld = _bld(t_next=t_out, ahu_flow=flow, blr_flow=wflow, blr_sp=supply_w, blr_return=supply_w, duration=0.0,
               heat_sp=mixed + d_ac if d_ac >= 0 else 200.0, cool_sp=mixed + d_ac if d_ac < 0 else 400.0)
    si = t.step_in(t_next=t_out, comfort_next=1, occupancy=row["average_occupancy"], e_price=price, e_carbon=carbon,
                   g_price=price, g_carbon=carbon)
    reward, info = t.post(bld, [row["zone_air_temperature"]] * 2, mixed, si)
    t.close()
    assert info[0] == pytest.approx(row["blower"], rel=1e-6, abs=1e-4), row["name"]
    assert info[1] == pytest.approx(row["air_conditioning"], rel=1e-6, abs=1e-3), row["name"]
    assert info[2] == pytest.approx(row["natural_gas"], rel=1e-6, abs=1e-3), row["name"]
    assert info[3] == pytest.approx(row["pump"], rel=1e-6, abs=1e-4), row["name"]
    assert reward == pytest.approx(row["expected_reward"], abs=5e-5), row["name"]
    assert info[8] == pytest.approx(row["expected_productivity"], rel=1e-6, abs=5e-5), row["name"]
    # the reference's test states these to four decimals (assertAlmostEqual places=4)
    assert info[9] == pytest.approx(row["expected_electricity_cost"], abs=5e-5), row["name"]
    assert info[10] == pytest.approx(row["expected_natural_gas_cost"], abs=5e-5), row["name"]
    assert info[11] == pytest.approx(row["expected_carbon_emitted"], abs=5e-5), row["name"]


def test_boiler_known_answers_through_k_post():
  """boiler_test.py:131-176 (500.066862, 562.57521, 100695.0501, 125.0167, 0), :431-439 (312.5418), pump."""
  need_gpu()
  t = Taps(boiler_water_pump_differential_head=3.0, boiler_water_pump_efficiency=0.6)
  si = t.step_in()
  for setpoint, flow, ret, outside, want in ((360.0, 0.0, 300.0, 280.0, 500.066862), (370.0, 0.0, 300.0, 280.0, 562.57521),
                                             (340.0, 0.6, 300.0, 280.0, 100695.0501), (300.0, 0.6, 300.0, 280.0, 125.0167),
                                             (300.0, 0.01, 300.0, 280.0, 125.0167), (300.0, 0.01, 300.0, 300.0, 0.0),
                                             (340.0, 0.0, 290.0, 290.0, 312.5418), (290.0, 0.0, 290.0, 290.0, 0.0)):
    _, info = t.post(_bld(blr_sp=setpoint, blr_flow=flow, blr_return=ret, t_next=outside, duration=0.0), [293.0, 293.0], 293.0,
                     t.step_in(t_next=outside))
    assert info[2] == pytest.approx(want, rel=2e-7, abs=2e-3), (setpoint, flow, ret, outside)
  _, info = t.post(_bld(blr_flow=0.6, blr_sp=300.0, blr_return=300.0), [293.0, 293.0], 293.0, si)
  assert info[3] == pytest.approx(0.6 * 1000.0 * 9.8 * 3.0 / 0.6, rel=1e-7)
  t.close()


def test_boiler_tank_lag_known_answers_through_k_pre():
  """boiler_test.py:197-230 _adjust_temperature, reached through _set_current_temperature (both rates
  positive there: the rate that the row does not use is given a dummy value)."""
  need_gpu()
  for sp, actual, secs, h, c_, want in ((330.0, 290.0, 60, 2.0, 0.5, 292.0), (300.0, 290.0, 600, 2.0, 0.5, 300.0),
                                        (320.0, 330.0, 60, 2.0, 0.5, 329.5), (320.0, 330.0, 600, 0.7, 2.0, 320.0),
                                        (330.0, 330.0, 60, 2.0, 0.5, 330.0)):
    t = Taps(time_step_sec=float(secs), boiler_heating_rate=h, boiler_cooling_rate=c_,
             action_ranges=((200.0, 400.0), (285.0, 300.0)))
    act = [(sp - 200.0) / 200.0 * 2.0 - 1.0, 0.0]
    bld, *_ = t.pre([293.0, 293.0], scalars=t.scalars(tank=actual, blr_sp=actual), actions=act, si=t.step_in(has_action=1))
    t.close()
    assert bld.blr_sp == pytest.approx(sp, abs=2e-5) and bld.duration == float(secs)
    assert bld.tank == pytest.approx(want, abs=2e-5), (sp, actual, secs)
    assert bld.tank_change == pytest.approx(want - actual, abs=2e-5)


def test_air_handler_known_answers():
  """air_handler_test.py:110-175 through k_pre (mixed / supply air temperature, setpoints 270 / 288) and
  :335-420 through k_post (thermal rate, fan powers: intake all the air, exhaust the fresh share)."""
  need_gpu()
  for r, recirc, amb, want in ((0.3, 280, 240, 270), (0.6, 244, 270, 270), (0.1, 210, 316, 288), (0.4, 250, 316, 288),
                               (0.4, 286, 266, 0.4 * 286 + 0.6 * 266), (0.12, 198, 290, 0.12 * 198 + 0.88 * 290)):
    t = Taps(ahu_recirculation=r, ahu_heating_air_temp_setpoint=270.0, ahu_cooling_air_temp_setpoint=288.0)
    bld, *_ = t.pre([293.0, 293.0], scalars=t.scalars(recirc=float(recirc)), si=t.step_in(t_now=float(amb)))
    t.close()
    assert bld.t_sa == want, (r, recirc, amb)
  t = Taps(ahu_recirculation=0.3, ahu_heating_air_temp_setpoint=270.0, ahu_cooling_air_temp_setpoint=288.0,
           ahu_fan_differential_pressure=20000.0, ahu_fan_efficiency=0.8)
  for flow, amb, recirc in ((100.0, 250.0, 210.0), (0.5, 280.0, 320.0), (1000.0, 155.0, 134.0), (2.0, 246.0, 290.0), (900.0, 50.0, 270.0)):
    mixed = 0.3 * recirc + (1 - 0.3) * amb
    supply = min(max(mixed, 270.0), 288.0)
    _, info = t.post(_bld(ahu_flow=flow, heat_sp=270.0, cool_sp=288.0, t_next=amb), [293.0, 293.0], recirc, t.step_in(t_next=amb))
    assert info[1] == pytest.approx(flow * C_AIR * (supply - mixed), rel=2e-7, abs=1e-6), (flow, amb, recirc)
  _, info = t.post(_bld(ahu_flow=5.0, heat_sp=270.0, cool_sp=288.0), [293.0, 293.0], 280.0, t.step_in())
  assert info[0] == pytest.approx(5.0 * 20000.0 / 0.8 + (5.0 * (1.0 - 0.3)) * 20000.0 / 0.8, rel=1e-7)
  t.close()


def test_vav_known_answers_through_k_pre():
  """vav_test.py:198-262: zone supply temperature and the energy applied to the zone.  The formulas see
  only valve * max_water_flow and damper * max_air_flow: the reheat valve is opened by the thermostat
  (HEAT: 1, COOL: 0), the damper by the agent's supply_air_damper_percentage_command."""
  need_gpu()
  for valve, max_w, damper, max_a, t_sa, t_w in ((0.5, 0.8, 0.3, 0.3, 270, 360), (0.1, 0.1, 0.4, 0.4, 210, 32),
                                                 (0, 0.2, 0.2, 0.9, 260, 270), (0.9, 0.4, 0.1, 0.6, 270, 430)):
    reheat, air = valve * max_w, damper * max_a
    t = Taps(vav_reheat_max_water_flow_rate=max(reheat, 1e-9) if valve else 0.2, vav_max_air_flow_rate=max_a,
             ahu_recirculation=1.0, ahu_heating_air_temp_setpoint=100.0, ahu_cooling_air_temp_setpoint=500.0,
             action_names=("supply_air_damper_percentage_command", "supply_air_damper_percentage_command"),
             action_zones=(0, 1), action_ranges=((0.0, 1.0), (0.0, 1.0)),
             comfort_temp_window=(292.0, 295.0))
    tz = 291.0 if valve else 296.0            # below the window: HEAT (valve 1); above: COOL (valve 0)
    dn = np.float32(damper) * 2.0 - 1.0
    bld, q, dmp, modes = t.pre([tz, tz], modes=[0, 0], scalars=t.scalars(recirc=float(t_sa), blr_sp=float(t_w), heat_sp=100.0, cool_sp=500.0),
                               actions=[dn, dn], si=t.step_in(has_action=1))
    t.close()
    d32 = float(np.float32((float(dn) + 1.0) / 2.0))
    air = d32 * max_a
    want = (t_sa * (C_AIR * air - C_WATER * reheat) + t_w * C_WATER * reheat) / air / C_AIR   # vav_test.py:55-75
    assert bld.t_sa == float(t_sa) and list(modes) == ([1, 1] if valve else [2, 2])
    assert dmp[0] == pytest.approx(damper, rel=1e-6)
    assert q[0] == pytest.approx(air * C_AIR * (want - tz), rel=1e-12, abs=1e-9), (valve, max_w, damper, max_a)
    assert bld.blr_return == pytest.approx(want if valve else 0.0, rel=1e-6)


@pytest.mark.parametrize("ts,zone_temp,damper,valve", [
    ("2021-05-09 14:00", 293, 0.1, 0.0), ("2021-05-10 09:00", 296, 1.0, 0.0), ("2021-05-12 09:00", 291, 1.0, 1.0),
    ("2021-05-12 17:59", 291, 1.0, 1.0), ("2021-05-11 03:00", 288, 1.0, 1.0), ("2021-05-11 03:00", 291, 0.1, 0.0),
    ("2021-05-11 22:00", 298, 1.0, 0.0), ("2021-05-11 22:00", 297, 0.1, 0.0)])
def test_vav_update_settings_table_through_k_pre(ts, zone_temp, damper, valve):
  """vav_test.py:150-174: thermostat 9-18 h, comfort (292, 295), eco (290, 297), previous update one
  hour earlier; the host schedule supplies the mode flags, k_pre does the control."""
  need_gpu()
  now = dt.datetime.fromisoformat(ts)
  sched = host_inputs.SetpointSchedule(9, 18, (292, 295), (290, 297), holidays=set())
  t = Taps(comfort_temp_window=(292.0, 295.0), eco_temp_window=(290.0, 297.0), morning_start_hour=9, evening_start_hour=18)
  si = t.step_in(comfort_now=int(sched.is_comfort_mode(now)),
                 comfort_prev=int(sched.is_comfort_mode(now - dt.timedelta(minutes=60))))
  bld, q, dmp, modes = t.pre([float(zone_temp)] * 2, modes=[0, 0], si=si)
  t.close()
  assert dmp[0] == damper and (modes[0] == 1) == (valve == 1.0)
  assert bld.blr_count == (2 if valve else 0)          # the reheat valve opens: one heating request per VAV


def test_thermostat_state_machine_through_k_pre():
  """thermostat_test.py:47-135 with its schedule (9-18 h, comfort (292, 295), eco (290, 297)).
  Modes: 0 OFF, 1 HEAT, 2 COOL, 3 PASSIVE_COOL."""
  need_gpu()
  t = Taps(comfort_temp_window=(292.0, 295.0), eco_temp_window=(290.0, 297.0))
  low, high = 292.0, 295.0
  mid = (low + high) / 2
  mode, seq = [0, 0], []
  for tz in (low - 1, mid - 1, high + 1, mid + 1, mid - 1, mid + 1):      # test_update_comfort_mode / _default_control
    _, _, _, mode = t.pre([tz, tz], modes=mode, si=t.step_in(comfort_now=1, comfort_prev=1))
    seq.append(int(mode[0]))
  assert seq == [1, 1, 2, 2, 0, 0]
  _, _, _, m = t.pre([0.0, 0.0], modes=[0, 0], si=t.step_in(comfort_now=1, comfort_prev=-1))   # test_eco_transition
  _, _, dmp, m = t.pre([0.0, 0.0], modes=m, si=t.step_in(comfort_now=0, comfort_prev=1))
  assert list(m) == [3, 3] and dmp[0] == 0.1
  _, _, _, m = t.pre([(290.0 + 297.0) / 2] * 2, modes=m, si=t.step_in(comfort_now=0, comfort_prev=0))   # test_eco_mode
  assert list(m) == [3, 3]
  _, _, _, m = t.pre([0.0, 0.0], modes=m, si=t.step_in(comfort_now=0, comfort_prev=0))
  assert list(m) == [1, 1]
  t.close()
