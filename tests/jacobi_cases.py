"""Plans and seeded inputs of the float32 Jacobi solver's tests (tests/test_jacobi_cpu.py, test_jacobi_gpu.py and the
two test_jacobi_large modules)."""
import numpy as np

from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
from tests.golden_util import load
from tests.twins import plan_from_npz

GOLDEN_PLANS = {"r9_test": "plan_r9_test.npz", "small_test": "plan_small_test.npz", "weird_test": "plan_weird_test.npz",
                "r9_sb1": "plan_r9_sb1.npz", "tf10x9": None}


def golden_plan(name):
  """The FloorPlan of a fixture plan: the shipped plan dumps, or the 10 x 9 plan of tf_simulator_test.py stored with
  the tensors."""
  if GOLDEN_PLANS[name] is not None:
    return plan_from_npz(load(GOLDEN_PLANS[name]))
  t = load("jacobi_tensors.npz")
  return plan_from_npz({k[len("tf10x9_plan_"):]: t[k] for k in t.files if k.startswith("tf10x9_plan_")})


PLAN_155 = ((6, 5), (24, 29))      # 155 x 155 = 24,025 CVs: the first size class beyond the LDS limit
PLAN_SB1 = ((14, 9), (20, 43))     # 299 x 401 = 119,899 CVs, 126 zones: the benchmark's SB1 stand-in


def large_plan(rooms, room_shape):
  return FloorPlan.from_file_input(rectangular_floor_plan(rooms, room_shape), Materials.sb1(), 10.0, 300.0)


def large_case(seed, shape, n_zones):
  """tools/gen_golden_jacobi.py's large_case: (Tprev float32, zone powers, T_inf) of a stored seed."""
  rs = np.random.RandomState(seed)
  prev = (285.0 + 12.0 * rs.rand(*shape)).astype(np.float32)
  qz = rs.uniform(-4000.0, 4000.0, n_zones)
  return prev, qz, float(rs.uniform(265.0, 305.0))
