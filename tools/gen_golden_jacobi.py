"""Generates the Jacobi-solver fixtures tests/golden/jacobi_*.npz from the reference's own TFSimulator
(simulator/tf_simulator.py), run on a NumPy float32 stand-in for ``tensorflow``.  Run it where the reference tree
exists (``python tools/gen_golden_jacobi.py``); tests never run it and never read the reference.

The stand-in and its fidelity.  tf_simulator.py uses these TF ops, all elementwise or data movement on float32
tensors: add, multiply, divide, subtract, abs, scalar_mul, pad, boolean_mask, fill, where, convert_to_tensor, constant
and count_nonzero.  TF on a CPU evaluates each one as one kernel per op, every element one correctly rounded IEEE
binary32 operation (no fusion, no reassociation, no FMA contraction across ops).  NumPy's float32 ufuncs are correctly
rounded binary32 operations too, and scalars combine with float32 arrays in float32 (NumPy >= 2, NEP 50), so each op
gives TF's bits.  pad / boolean_mask / fill / where / convert_to_tensor / constant only move or round values (float64
-> float32 round-to-nearest-even, as TF's cast).  count_nonzero only feeds a log line.  The recorded NumPy version is
part of every fixture: the float32 comparison ``max_delta <= threshold`` of simulator.py:362 depends on NEP 50.

Fixtures:
  jacobi_tensors.npz  (a) per plan: classify_cv's type per CV, u / v, the oriented k / h tensors, den and the exterior
                      mask -- the reference test plans, SB1's R9 and the 10 x 9 plan of tf_simulator_test.py (with its
                      floor-plan arrays, prefix tf10x9_plan_)
  jacobi_fd.npz       (b) finite_differences_timestep on seeded random grids, input_q and T_inf, iteration limits 100
                      and 2: grid, iterations, converged
  jacobi_h1_r9_test.npz, jacobi_h2_sb1_r9_random.npz
                      (c) a 288-step thermostat-only rollout on r9_test and a seeded random-action rollout on SB1 R9
                      (oracle/gen_golden.py's harnesses with TFSimulator in place of SimulatorFlexibleGeometries)
  jacobi_fd_large.npz (``--large``: writes this fixture alone) finite_differences_timestep on the 155 x 155 plan
                      rectangular_floor_plan((6, 5), (24, 29)) with SB1's materials, beyond what k_sweep_jacobi holds in
                      LDS: per seeded case and iteration limit the grid, iterations, converged.  The plan, Tprev, the
                      zone powers and T_inf are not stored: large_case() regenerates them from the stored seeds.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402
from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
f32 = np.float32


class _Tensor(np.ndarray):
  """An eager tensor: a float32 / bool array with .numpy()."""

  def numpy(self):
    return np.asarray(self)


def _t(x, dtype=None):
  return np.asarray(x, dtype=dtype).view(_Tensor)


class _Recorder:
  last_divide = None


def _divide(a, b):
  out = _t(np.divide(a, b))
  _Recorder.last_divide = (np.asarray(a).copy(), np.asarray(b).copy())
  return out


def _tf_standin() -> types.ModuleType:
  tf = types.ModuleType("tensorflow")
  tf.float32 = np.float32
  tf.Tensor = _Tensor
  math = types.ModuleType("tensorflow.math")
  math.add = lambda a, b: _t(np.add(a, b))
  math.multiply = lambda a, b: _t(np.multiply(a, b))
  math.divide = _divide
  math.subtract = lambda a, b: _t(np.subtract(a, b))
  math.abs = lambda a: _t(np.abs(a))
  math.scalar_mul = lambda s, x: _t(np.multiply(s, x))
  math.count_nonzero = lambda x: int(np.count_nonzero(x))
  tf.math = math
  tf.scalar_mul = math.scalar_mul
  tf.convert_to_tensor = lambda x, dtype=None: _t(x, dtype)
  tf.constant = lambda v, dtype=None: np.asarray(v, dtype=dtype)[()]
  tf.pad = lambda x, paddings, constant_values=0: _t(np.pad(np.asarray(x), paddings, constant_values=constant_values))
  tf.boolean_mask = lambda x, mask, axis=0: _t(np.compress(np.asarray(mask), np.asarray(x), axis=axis))
  tf.fill = lambda shape, value: _t(np.full(shape, value, dtype=np.asarray(value).dtype))
  tf.where = lambda c, a, b: _t(np.where(c, a, b))
  return tf


def load_tf_simulator():
  """refshim's modules, the stand-in as ``tensorflow``, and the reference's real tf_simulator.py in place of refshim's
  inert stub."""
  refshim.install()
  sys.modules["tensorflow"] = _tf_standin()
  name = "smart_buildings.smart_control.simulator.tf_simulator"
  path = os.path.join(refshim.REFERENCE_ROOT, "smart_control", "simulator", "tf_simulator.py")
  spec = importlib.util.spec_from_file_location(name, path)
  mod = importlib.util.module_from_spec(spec)
  sys.modules[name] = mod
  spec.loader.exec_module(mod)
  sys.modules["smart_buildings.smart_control.simulator"].tf_simulator = mod
  return mod



def type_code(tfs, cv):
  if cv.position == tfs.CVPositionType.EXTERIOR:
    return 0
  if cv.position == tfs.CVPositionType.INTERIOR:
    return 1
  if cv.boundary == tfs.CVBoundaryType.CORNER:
    return 2 + list(tfs.CVCornerOrientationType).index(cv.corner)
  return 6 + list(tfs.CVEdgeOrientationType).index(cv.edge)


def tensors_of(tfs, sim, b, h, t_amb):
  """(a): the reference's own tensors of one simulator."""
  nb = b.neighbors
  H, W = b.temp.shape
  codes = np.zeros((H, W), np.int64)
  for i in range(H):
    for j in range(W):
      codes[i, j] = type_code(tfs, tfs.classify_cv((i, j), nb))
  bmap = tfs.get_cv_mapping(nb, position_criterion=tfs.CVPositionType.BOUNDARY)
  u, v = tfs.get_cv_dimension_tensors(b.cv_size_cm / 100.0, bmap, b.temp.shape)
  kL, kR, kT, kB = tfs.get_oriented_conductivity_tensors(b.conductivity, bmap)
  hL, hR, hT, hB = tfs.get_oriented_convection_coefficient_tensors(h, b.temp.shape, bmap)
  sim.update_temperature_estimates(b.temp.copy(), ambient_temperature=t_amb, convection_coefficient=h)
  den = _Recorder.last_divide[1]
  return dict(type=codes, u=u.numpy(), v=v.numpy(), kL=kL.numpy(), kR=kR.numpy(), kT=kT.numpy(), kB=kB.numpy(),
              hL=hL.numpy(), hR=hR.numpy(), hT=hT.numpy(), hB=hB.numpy(), den=np.asarray(den, f32),
              exterior=np.asarray(sim._t_exerior_temps_mask, bool))


LARGE_ROOMS, LARGE_ROOM_SHAPE = (6, 5), (24, 29)   # 155 x 155 = 24,025 CVs, 30 zones
LARGE_SEEDS, LARGE_LIMITS = (20261016, 20261017), (100, 2)


def large_case(seed: int, shape, n_zones: int):
  """(Tprev float32, zone powers, T_inf) of one seeded case of jacobi_fd_large.npz (tests/test_jacobi_large_*.py draw
  the same)."""
  rs = np.random.RandomState(seed)
  prev = (285.0 + 12.0 * rs.rand(*shape)).astype(f32)
  qz = rs.uniform(-4000.0, 4000.0, n_zones)
  return prev, qz, float(rs.uniform(265.0, 305.0))


def main_large() -> None:
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  from tests import jacobi_restatement as jr
  tfs = load_tf_simulator()
  m = gg._mods()
  tfm = dict(m, simulator_flexible_floor_plan=types.SimpleNamespace(SimulatorFlexibleGeometries=tfs.TFSimulator))
  file_plan = rectangular_floor_plan(LARGE_ROOMS, LARGE_ROOM_SHAPE)
  sim, b, *_ = gg.build_sb1(tfm, np.asarray(file_plan), pd.Timestamp("2012-12-21"))
  fp = FloorPlan.from_file_input(file_plan, Materials.sb1(), gg.SB1["cv_size_cm"], gg.SB1["floor_height_cm"])
  H, W = b.temp.shape
  assert (H, W) == fp.shape
  out = {"numpy_version": np.array(np.__version__), "h": 100.0, "dt": 300.0, "thr": 0.1,
         "rooms": np.array(LARGE_ROOMS), "room_shape": np.array(LARGE_ROOM_SHAPE), "seeds": np.array(LARGE_SEEDS),
         "limits": np.array(LARGE_LIMITS), "cv_size_cm": gg.SB1["cv_size_cm"], "floor_height_cm": gg.SB1["floor_height_cm"]}
  for seed in LARGE_SEEDS:
    prev, qz, t_amb = large_case(seed, (H, W), fp.n_zones)
    for limit in LARGE_LIMITS:
      sim._iteration_limit = limit
      b.temp = prev.astype(np.float64)
      b.input_q = np.zeros((H, W))
      for z, name in enumerate(fp.zone_names):
        b.apply_thermal_power_zone(name, float(qz[z]))
      # what a test regenerates is what the reference saw
      assert np.array_equal(jr.input_q(fp, qz), b.input_q.astype(f32))
      counter = gg.SweepCounter(sim)
      conv = sim.finite_differences_timestep(ambient_temperature=t_amb, convection_coefficient=100.0)
      key = f"{seed}_{limit}"
      out[key + "_grid"] = np.asarray(b.temp, f32)
      out[key + "_iterations"] = counter.take()
      out[key + "_converged"] = bool(conv)
      print(f"  {key}: {out[key + '_iterations']} iterations, converged={conv}")
  np.savez_compressed(os.path.join(OUT, "jacobi_fd_large.npz"), **out)


def main() -> None:
  if not refshim.available():
    print("reference tree not present; nothing to do")
    return
  if "--large" in sys.argv[1:]:
    main_large()
    return
  tfs = load_tf_simulator()
  m = gg._mods()
  ft = m["simulator_flexible_floor_plan_test"].FlexibleFloorplanSimulatorTest()
  wc = m["weather_controller"]
  tfm = dict(m, simulator_flexible_floor_plan=types.SimpleNamespace(SimulatorFlexibleGeometries=tfs.TFSimulator))
  meta = dict(generated_by="tools/gen_golden_jacobi.py", numpy=np.__version__)
  start = pd.Timestamp("2012-12-21")

  def tf_sim(b, limit=100, t_amb=280.0):
    hv = ft._create_scenario_hvac(zone_identifier=list(b._room_dict.keys()))
    return tfs.TFSimulator(b, hv, wc.WeatherController(t_amb, t_amb), 300.0, 0.1, limit, 1000, start)

  # the 10 x 9 plan of tf_simulator_test.py:36-139 (building_py.FloorPlanBasedBuilding with its materials)
  bp = m["building"]
  plan10 = np.array([[2] * 9, [2, 1, 1, 2, 2, 2, 1, 1, 2], [2, 1, 0, 1, 2, 1, 0, 1, 2], [2, 1, 0, 0, 1, 0, 0, 1, 2],
                     [2, 1, 0, 0, 1, 0, 0, 1, 2], [2, 1, 1, 1, 1, 1, 1, 1, 2], [2, 1, 0, 0, 1, 0, 0, 1, 2],
                     [2, 1, 0, 0, 1, 0, 0, 1, 2], [2, 1, 1, 1, 1, 1, 1, 1, 2], [2] * 9])
  b10 = bp.FloorPlanBasedBuilding(
      cv_size_cm=20.0, floor_height_cm=300.0, initial_temp=292.0,
      inside_air_properties=bp.MaterialProperties(conductivity=50.0, heat_capacity=700.0, density=1.0),
      inside_wall_properties=bp.MaterialProperties(conductivity=2.0, heat_capacity=1000.0, density=1800.0),
      building_exterior_properties=bp.MaterialProperties(conductivity=0.05, heat_capacity=1000.0, density=3000.0),
      floor_plan=plan10, floor_plan_filepath=None, zone_map=plan10.copy(), zone_map_filepath=None,
      buffer_from_walls=0)
  sb1_sim, b_sb1, *_ = gg.build_sb1(tfm, np.asarray(ft._create_scenario_floor_plan()), start)
  buildings = {
      "r9_test": ft._create_scenario_building(initial_temp=292.0, match_old_diffusers=True),
      "small_test": ft._create_small_building(initial_temp=293.0),
      "weird_test": ft._create_weirdly_shaped_building(initial_temp=293.0),
      "tf10x9": b10,
  }

  # ---- (a) tensors ----
  print("(a) tensors")
  out = {"numpy_version": np.array(np.__version__), "h": 100.0, "dt": 300.0}
  sims = {name: tf_sim(b) for name, b in buildings.items()}
  sims["r9_sb1"] = sb1_sim
  buildings["r9_sb1"] = b_sb1
  for name, sim in sims.items():
    b = buildings[name]
    for k, v in tensors_of(tfs, sim, b, 100.0, 280.0).items():
      out[f"{name}_{k}"] = v
    print(f"  {name}: {b.temp.shape}")
  for k, v in gg.dump_building(b10, plan10).items():
    out[f"tf10x9_plan_{k}"] = v
  np.savez_compressed(os.path.join(OUT, "jacobi_tensors.npz"), **out)

  # ---- (b) FD time steps ----
  print("(b) FD time steps")
  rs = np.random.RandomState(20261015)
  out = {"numpy_version": np.array(np.__version__), "h": 100.0, "dt": 300.0, "thr": 0.1}
  for name, b in buildings.items():
    H, W = b.temp.shape
    zones = [z for z in b._room_dict.keys() if z.startswith("room")]
    for case in range(2):
      prev = (285.0 + 12.0 * rs.rand(H, W)).astype(f32).astype(np.float64)
      qz = rs.uniform(-4000.0, 4000.0, len(zones))
      t_amb = float(rs.uniform(265.0, 305.0))
      for limit in (100, 2):
        sim = sb1_sim if name == "r9_sb1" else tf_sim(b, limit)
        sim._iteration_limit = limit
        b.temp = prev.copy()
        b.input_q = np.zeros((H, W))
        for z, q in zip(zones, qz):
          b.apply_thermal_power_zone(z, float(q))
        counter = gg.SweepCounter(sim)
        conv = sim.finite_differences_timestep(ambient_temperature=t_amb, convection_coefficient=100.0)
        key = f"{name}_{case}_{limit}"
        out[key + "_prev"] = prev
        out[key + "_input_q"] = b.input_q.copy()
        out[key + "_t_amb"] = t_amb
        out[key + "_grid"] = np.asarray(b.temp, f32)
        out[key + "_iterations"] = counter.take()
        out[key + "_converged"] = bool(conv)
        print(f"  {key}: {out[key + '_iterations']} iterations, converged={conv}")
    sb1_sim._iteration_limit = gg.SB1["iteration_limit"]
  np.savez_compressed(os.path.join(OUT, "jacobi_fd.npz"), **out)

  # ---- (c) rollouts ----
  print("(c) rollouts")
  b = ft._create_scenario_building(initial_temp=292.0, match_old_diffusers=True)
  hv = ft._create_scenario_hvac(zone_identifier=list(b._room_dict.keys()))
  sim = tfs.TFSimulator(b, hv, wc.WeatherController(296.0, 296.0), 300.0, 0.1, 100, 10, start)
  out = gg.rollout_h1(m, sim, b, hv, 288, "r9_test thermostat-only (TFSimulator)")
  out["params_json"] = np.array(json.dumps(gg.hvac_params_of(hv, sim)))
  out["t_amb"], out["h_conv"], out["initial_temp"] = 296.0, 12.0, 292.0
  ts = [start + pd.Timedelta(300 * i, unit="s") for i in range(289)]
  sch = next(iter(hv.vavs.values())).thermostat.get_setpoint_schedule()
  out["comfort"] = np.array([sch.is_comfort_mode(t) for t in ts], dtype=np.int64)
  out["numpy_version"] = np.array(np.__version__)
  np.savez_compressed(os.path.join(OUT, "jacobi_h1_r9_test.npz"), **out)

  start2 = pd.Timestamp("2023-07-06 07:00:00")
  rnd = np.random.RandomState(4321).uniform(-1.0, 1.0, size=(288, 2)).astype(np.float32)
  sim, building, hvac, weather, schedule = gg.build_sb1(tfm, np.asarray(ft._create_scenario_floor_plan()), start2)
  out = gg.rollout_h2(m, sim, building, hvac, weather, schedule, 288, rnd, (1, 144), "sb1_r9 random (TFSimulator)")
  out["h_conv"] = gg.SB1["weather"]["convection_coefficient"]
  out["initial_temp"] = gg.SB1["initial_temp"]
  out["start_timestamp"] = np.array(str(start2))
  out["numpy_version"] = np.array(np.__version__)
  np.savez_compressed(os.path.join(OUT, "jacobi_h2_sb1_r9_random.npz"), **out)
  print(json.dumps(meta))


if __name__ == "__main__":
  main()
