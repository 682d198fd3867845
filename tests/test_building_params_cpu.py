"""CPU checks of the per-building parameter table (sb_set_building_params, host_inputs.BuildingParams): the host
type's refusals, the name -> sb_building_param mapping against sb_params and the header, the mixed batch's global-row
slicing, and the C entry's null-handle refusal."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from sbsim_amd import _ffi, distributed
from sbsim_amd.environment import SimConfig
from sbsim_amd.host_inputs import (BUILDING_PARAM_NAMES, PER_BATCH_CONFIG_FIELDS, BuildingParams,
                                   effective_building_params)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mapping_covers_the_32_double_fields_of_sb_params_in_order():
  doubles = [n for n, t in _ffi.PARAM_FIELDS if t is C.c_double]
  expected = doubles[doubles.index("vav_max_air_flow"):doubles.index("w_carbon") + 1]
  assert len(expected) == 32 == _ffi.SB_NUM_BUILDING_PARAMS
  assert list(_ffi.BUILDING_PARAM_FIELDS) == expected
  assert [f for fields in BUILDING_PARAM_NAMES.values() for f in fields] == expected
  # ... and the header's enum, value by value
  text = open(os.path.join(ROOT, "include", "sbsim_amd.h")).read()
  body = re.search(r"typedef enum sb_building_param \{(.*?)\} sb_building_param;", text, re.S).group(1)
  body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
  enum = [n.split("=")[0].strip() for n in body.split(",") if n.strip()]
  assert enum == ["SB_BP_" + f.upper() for f in expected] + ["SB_NUM_BUILDING_PARAMS"]
  # what SimConfig.to_params() writes for each name is the field it maps to
  cfg, prm = SimConfig.sb1(), SimConfig.sb1().to_params()
  for name, fields in BUILDING_PARAM_NAMES.items():
    v = np.atleast_1d(getattr(cfg, name))
    assert [getattr(prm, f) for f in fields] == list(v), name


def test_every_simconfig_field_is_per_building_or_per_batch():
  names = {f.name for f in dataclasses.fields(SimConfig)}
  assert names == set(BUILDING_PARAM_NAMES) | set(PER_BATCH_CONFIG_FIELDS)
  assert not set(BUILDING_PARAM_NAMES) & set(PER_BATCH_CONFIG_FIELDS)


def test_unknown_name_lists_the_allowed_ones():
  with pytest.raises(ValueError, match="unknown per-building parameter 'fan_power'.*ahu_fan_efficiency.*carbon_emission_weight"):
    BuildingParams({"fan_power": [1.0]})


@pytest.mark.parametrize("name", PER_BATCH_CONFIG_FIELDS)
def test_per_batch_fields_are_refused(name):
  with pytest.raises(ValueError, match=f"{name}.*per batch"):
    BuildingParams({name: [1.0, 2.0]})


@pytest.mark.parametrize("values,match", [
    ({"ahu_fan_efficiency": [[0.9, 0.8]]}, r"ahu_fan_efficiency must have shape \[B\]"),
    ({"ahu_fan_efficiency": 0.9}, r"must have shape \[B\]"),
    ({"ahu_fan_efficiency": []}, r"must have shape \[B\]"),
    ({"comfort_temp_window": [294.0, 297.0]}, r"comfort_temp_window must have shape \[B\] x 2"),
    ({"eco_temp_window": [[289.0, 298.0, 1.0]]}, r"eco_temp_window must have shape \[B\] x 2"),
    ({"ahu_fan_efficiency": [0.9, 0.8], "boiler_heating_rate": [0.5]}, "one row per building"),
    ({}, "at least one field"),
])
def test_wrong_shapes_are_refused(values, match):
  with pytest.raises(ValueError, match=match):
    BuildingParams(values)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_values_are_refused(bad):
  with pytest.raises(ValueError, match="building 1: boiler_heating_rate is not finite"):
    BuildingParams({"boiler_heating_rate": [0.5, bad, 0.5]})
  with pytest.raises(ValueError, match="building 0: comfort_temp_window is not finite"):
    BuildingParams({"comfort_temp_window": [[294.0, bad]]})


@pytest.mark.parametrize("name", ["vav_max_air_flow_rate", "ahu_fan_efficiency", "ahu_max_air_flow_rate",
                                  "boiler_water_pump_efficiency", "boiler_convection_coefficient", "boiler_tank_length",
                                  "boiler_tank_radius", "boiler_insulation_conductivity", "boiler_insulation_thickness"])
@pytest.mark.parametrize("bad", [0.0, -1.0])
def test_divisors_must_be_positive(name, bad):
  with pytest.raises(ValueError, match=f"building 2: {name} must be positive"):
    BuildingParams({name: [1.0, 1.0, bad]})


def test_windows_keep_the_reference_order_and_messages():
  with pytest.raises(ValueError, match=r"building 1: comfort_temp_window\[0\] must be less than comfort_temp_window\[1\]"):
    BuildingParams({"comfort_temp_window": [[294.0, 297.0], [298.0, 297.0]]})
  with pytest.raises(ValueError, match=r"building 0: eco_temp_window\[0\] must be less than eco_temp_window\[1\]"):
    BuildingParams({"eco_temp_window": [[299.0, 298.0]]})
  BuildingParams({"comfort_temp_window": [[296.0, 296.0]]}).validate(SimConfig.sb1())   # equal ends: allowed, as there


def test_air_handler_setpoints_are_checked_against_the_config():
  cfg = SimConfig.sb1()   # heating 285, cooling 298
  msg = "cooling_air_temp_setpoint must greater than heating_air_temp_setpoint"
  with pytest.raises(ValueError, match=f"building 1: {msg}"):
    BuildingParams({"ahu_heating_air_temp_setpoint": [285.0, 298.0]}).validate(cfg)
  with pytest.raises(ValueError, match=f"building 0: {msg}"):
    BuildingParams({"ahu_cooling_air_temp_setpoint": [280.0, 299.0]}).validate(cfg)
  with pytest.raises(ValueError, match=f"building 2: {msg}"):
    BuildingParams({"ahu_heating_air_temp_setpoint": [285.0, 285.0, 290.0],
                    "ahu_cooling_air_temp_setpoint": [298.0, 286.0, 289.0]}).validate(cfg)
  BuildingParams({"ahu_heating_air_temp_setpoint": [290.0, 297.0]}).validate(cfg)


def test_reward_weights_must_not_sum_to_zero():
  bp = BuildingParams({"productivity_weight": [0.2, 0.0], "energy_cost_weight": [0.4, 0.0],
                       "carbon_emission_weight": [0.4, 0.0]})
  with pytest.raises(ValueError, match="building 1: productivity_weight \\+ energy_cost_weight"):
    bp.validate(SimConfig.sb1())
  BuildingParams({"carbon_emission_weight": [0.0, 0.0]}).validate(SimConfig.sb1())   # one weight 0: fine


def test_c_table_and_effective_values():
  cfg = SimConfig.sb1()
  bp = BuildingParams({"eco_temp_window": [[288.0, 299.0], [287.0, 300.0]], "ahu_fan_efficiency": [0.7, 0.8]})
  fields, values = bp.c_table()
  names = [_ffi.BUILDING_PARAM_FIELDS[k] for k in fields]
  assert names == ["eco_lo", "eco_hi", "ahu_eff"]
  assert values.shape == (3, 2) and values.flags.c_contiguous and values.dtype == np.float64
  np.testing.assert_array_equal(values, [[288.0, 287.0], [299.0, 300.0], [0.7, 0.8]])
  eff = bp.effective(cfg)
  assert set(eff) == set(BUILDING_PARAM_NAMES)
  np.testing.assert_array_equal(eff["ahu_fan_efficiency"], [0.7, 0.8])
  np.testing.assert_array_equal(eff["comfort_temp_window"], [cfg.comfort_temp_window] * 2)
  np.testing.assert_array_equal(eff["boiler_tank_length"], [cfg.boiler_tank_length] * 2)
  none = effective_building_params(None, cfg, 3)
  assert none["eco_temp_window"].shape == (3, 2) and none["vav_max_air_flow_rate"].shape == (3,)
  sub = bp.rows(1, 2)
  assert sub.n_buildings == 1 and sub.fields["ahu_fan_efficiency"][0] == 0.8
  with pytest.raises(ValueError, match="outside"):
    bp.rows(1, 3)


@pytest.mark.parametrize("world", [1, 2, 8])
def test_global_rows_give_every_building_exactly_one_row(world):
  totals = [8, 13, 21]
  hits = np.zeros(sum(totals), dtype=np.int64)
  for rank in range(world):
    rows = distributed.class_global_rows(totals, rank, world)
    ranges = distributed.class_shard_ranges(totals, rank, world)
    for k, ((glo, ghi), (lo, hi)) in enumerate(zip(rows, ranges)):
      assert ghi - glo == hi - lo            # as many rows as the class has buildings on this rank
      assert glo == sum(totals[:k]) + lo     # the generators' first_building (MixedBatchedEnvironment)
      assert sum(totals[:k]) <= glo < ghi <= sum(totals[:k + 1])   # inside the class's block
      hits[glo:ghi] += 1
  assert (hits == 1).all()


def test_c_entry_refuses_a_null_handle():
  lib = _ffi.load()
  fields = np.array([6], dtype=np.int32)
  values = np.array([0.9], dtype=np.float64)
  rc = _ffi.entry("sb_set_building_params")(None, 1, fields.ctypes.data_as(C.c_void_p),
                                            values.ctypes.data_as(C.c_void_p), None)
  assert rc == -1   # SB_ERR_INVALID
  assert b"null handle" in lib.sb_last_error()
  assert _ffi.entry("sb_set_building_params")(None, 0, None, None, None) == -1


def test_a_stale_library_gets_the_rebuild_message():
  with pytest.raises(_ffi.SbsimError, match="rebuild"):
    _ffi.entry("sb_no_such_entry")
  assert _ffi.has_experimental_kernels() in (True, False)
