"""Per-building parameter tables (host_inputs.BuildingParams) drawn around SB1, and a building's row by the oracle's
names: tests/test_building_params_gpu.py and tests/crossed_batches.py."""
import numpy as np

from sbsim_amd.host_inputs import BUILDING_PARAM_NAMES, BuildingParams

# temperatures move by kelvins around SB1's, everything else by a factor in [0.7, 1.3]
TEMPS_K = {"ahu_heating_air_temp_setpoint": 4.0, "ahu_cooling_air_temp_setpoint": 4.0,
           "boiler_reheat_water_setpoint": 10.0}


def random_params(B, seed, keep_default=(0,)) -> BuildingParams:
  """Every per-building field of every building drawn around SB1 (buildings in keep_default: SB1's own values), the
  windows and the air handler's setpoint order kept valid."""
  from sbsim_amd.environment import SimConfig
  SB1 = SimConfig.sb1()
  rs = np.random.RandomState(seed)
  out = {}
  for name in BUILDING_PARAM_NAMES:
    v = np.asarray(getattr(SB1, name), dtype=np.float64)
    if name in TEMPS_K:
      a = v + rs.uniform(-TEMPS_K[name], TEMPS_K[name], size=B)
    elif v.ndim == 1:   # a window: its lower end +- 2 K, its width * [0.7, 1.3]
      lo = v[0] + rs.uniform(-2.0, 2.0, size=B)
      a = np.stack([lo, lo + (v[1] - v[0]) * rs.uniform(0.7, 1.3, size=B)], axis=1)
    else:
      a = v * rs.uniform(0.7, 1.3, size=B)
    a[list(keep_default)] = v
    out[name] = a
  return BuildingParams(out)


def c_row(bp: BuildingParams, b: int) -> dict:
  """Building b's parameters by sb_params field name (the oracle's OracleParams names)."""
  row = {}
  for name, a in bp.fields.items():
    for j, f in enumerate(BUILDING_PARAM_NAMES[name]):
      row[f] = float(a[b] if a.ndim == 1 else a[b, j])
  return row
