"""Plans and material sets of the per-building-materials tests (tests/test_building_materials_cpu.py and _gpu.py) and of
the tables that substitute a building's materials into a plan (tests/regimes.py, tests/crossed_batches.py)."""
import dataclasses

import numpy as np

from sbsim_amd.floorplan import FloorPlan
from tests import irregular_plans as ip
from tests.golden_util import load
from tests.twins import plan_from_npz


def golden_plan(name: str) -> FloorPlan:
  return plan_from_npz(load(name + ".npz"))


def fourth_material_plan() -> FloorPlan:
  """plan_r9_test with one cell near the bottom left given a material of its own: row-major raster order meets the
  interior wall before that cell, column-major order after it, so the plan and its transpose number the slots
  differently."""
  plan = golden_plan("plan_r9_test")
  H, _ = plan.shape
  grids = {f: getattr(plan, f).copy() for f in ("conductivity", "heat_capacity", "density")}
  for f, factor in (("conductivity", 3.0), ("heat_capacity", 0.5), ("density", 1.7)):
    grids[f][H - 4, 3] *= factor
  return dataclasses.replace(plan, **grids)


def the_plan(name: str) -> FloorPlan:
  if name == "r9-fourth-material":
    return fourth_material_plan()
  return golden_plan(name) if name.startswith("plan_") else ip.plan(name)


def random_sets(table: np.ndarray, n: int, seed: int):
  """n material sets around the slot table [M, 3]: every value log-uniform within a factor of 10 of the plan's,
  h_conv uniform in [0, 200]; the last set has two slots made equal (when there are two).  Returns ([n, M, 3], [n])."""
  rs = np.random.RandomState(seed)
  sets = table[None] * 10.0 ** rs.uniform(-1.0, 1.0, size=(n,) + table.shape)
  if len(table) > 1:
    sets[-1, 1] = sets[-1, 0]
  return sets, rs.uniform(0.0, 200.0, size=n)


def substituted(plan: FloorPlan, ids: np.ndarray, mats: np.ndarray) -> FloorPlan:
  """`plan` with slot s's material replaced by mats[s] = (conductivity, heat_capacity, density)."""
  return dataclasses.replace(plan, conductivity=np.ascontiguousarray(mats[ids, 0]),
                             heat_capacity=np.ascontiguousarray(mats[ids, 1]), density=np.ascontiguousarray(mats[ids, 2]))
