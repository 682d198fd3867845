"""Per-building materials without a GPU: the structural compile (classes keyed by what a cell is) with the NumPy
restatement of the coefficient arithmetic, bitwise against FloorPlan.compile() on the plan with the materials
substituted; material_slots(); every refusal of host_inputs.BuildingMaterials."""
import dataclasses

import numpy as np
import pytest

from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan, structural_class_coef
from sbsim_amd.host_inputs import BuildingMaterials, effective_building_materials
from tests import irregular_plans as ip
from tests.materials_cases import fourth_material_plan, random_sets, substituted, the_plan

DT = 300.0
GOLDEN_PLANS = ("plan_small_test", "plan_weird_test", "plan_r9_test", "plan_r9_sb1")
IRREGULAR = ("L", "roll66-48sets")
N_SETS = 5


def _check_against_compile(plan: FloorPlan, seed: int):
  ids, table = plan.material_slots()
  sp = plan.compile_structural(DT)
  assert sp.n_slots == len(table) and sp.class_desc.shape == (sp.n_classes, 4)
  sets, hs = random_sets(table, N_SETS, seed)
  cases = [(table, 12.0)] + list(zip(sets, hs))
  merged = False
  for mats, h in cases:
    cp = substituted(plan, ids, mats).compile(DT, float(h))
    coef = structural_class_coef(sp, mats[:, 0], mats[:, 1], mats[:, 2], float(h), DT, sp.dx, sp.zh)
    assert coef.shape == (sp.n_classes, 8)
    got, want = coef[sp.cell_class], cp.class_coef[cp.cell_class]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.argwhere(got != want)[:4]
    assert np.array_equal(sp.class_zone[sp.cell_class], cp.class_zone[cp.cell_class])
    assert np.array_equal(sp.zone_off, cp.zone_off) and np.array_equal(sp.zone_cells, cp.zone_cells)
    merged = merged or cp.n_classes < sp.n_classes
  return sp, merged


@pytest.mark.parametrize("name", GOLDEN_PLANS + IRREGULAR)
def test_structural_compile_equals_compile_bitwise(name):
  plan = the_plan(name)
  sp, merged = _check_against_compile(plan, seed=5)
  spt, _ = _check_against_compile(plan.transposed(), seed=6)
  assert spt.n_classes == sp.n_classes and spt.n_slots == sp.n_slots
  # the set with two equal slots makes value-keyed compile() merge classes the structural map keeps apart
  if sp.n_slots > 1:
    assert merged


def test_structural_classes_do_not_depend_on_the_values():
  plan = the_plan("plan_small_test")
  ids, table = plan.material_slots()
  sets, _ = random_sets(table, 2, seed=1)
  a, b = plan.compile_structural(DT), substituted(plan, ids, sets[0]).compile_structural(DT)
  assert np.array_equal(a.cell_class, b.cell_class) and np.array_equal(a.class_desc, b.class_desc)


@pytest.mark.parametrize("name", GOLDEN_PLANS + IRREGULAR)
def test_material_slots_round_trip(name):
  plan = the_plan(name)
  ids, table = plan.material_slots()
  assert ids.dtype == np.uint8 and ids.shape == plan.shape and table.shape == (int(ids.max()) + 1, 3)
  assert np.array_equal(table[ids, 0], plan.conductivity)
  assert np.array_equal(table[ids, 1], plan.heat_capacity)
  assert np.array_equal(table[ids, 2], plan.density)
  assert len({tuple(r) for r in table}) == len(table)
  first = [int(np.flatnonzero(ids.reshape(-1) == s)[0]) for s in range(len(table))]
  assert first == sorted(first)   # slots in order of first raster occurrence
  idt, tt = plan.transposed().material_slots()
  assert np.array_equal(tt[idt].transpose(1, 0, 2), table[ids])


def test_transposed_compile_keeps_the_callers_slot_numbering():
  """A table's columns follow the caller's plan.material_slots(), whichever orientation the device runs: the transposed
  plan compiled with the caller's slots has the caller's slot table, and its coefficients for a material set given in
  that numbering equal compile() on the transposed substituted plan."""
  plan = fourth_material_plan()
  ids, table = plan.material_slots()
  pt = plan.transposed()
  assert len(table) == 4 and not np.array_equal(pt.material_slots()[1], table)   # the first-occurrence orders do differ
  assert not np.array_equal(pt.compile_structural(DT).slot_table, table)
  spt = pt.compile_structural(DT, slots=(ids.T, table))
  assert np.array_equal(spt.slot_table, table) and spt.n_classes == pt.compile_structural(DT).n_classes
  sets, hs = random_sets(table, 3, seed=11)
  for mats, h in zip(sets, hs):
    cp = substituted(plan, ids, mats).transposed().compile(DT, float(h))
    coef = structural_class_coef(spt, mats[:, 0], mats[:, 1], mats[:, 2], float(h), DT, spt.dx, spt.zh)
    got, want = coef[spt.cell_class], cp.class_coef[cp.cell_class]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.argwhere(got != want)[:4]
  with pytest.raises(ValueError, match="slots must be"):
    pt.compile_structural(DT, slots=(ids, table))
  with pytest.raises(ValueError, match="slots must be"):
    pt.compile_structural(DT, slots=(ids.T, table[::-1]))
  with pytest.raises(ValueError, match="slots must be"):   # an id beyond the table
    pt.compile_structural(DT, slots=(ids.T, table[:3]))


def test_from_file_input_plan_has_three_slots():
  plan = FloorPlan.from_file_input(rectangular_floor_plan((2, 2), (6, 7)), Materials.sb1(), 10.0, 300.0)
  ids, table = plan.material_slots()
  m = Materials.sb1()
  assert len(table) == 3
  assert {tuple(r) for r in table} == {(x.conductivity, x.heat_capacity, x.density)
                                       for x in (m.air, m.interior_wall, m.exterior_wall)}


def test_more_than_255_structural_classes_is_the_existing_error():
  plan = ip.u_ladder(220)
  d = plan.diffusers.copy()   # every diffuser a weight of its own: far more than 255 classes
  cells = np.flatnonzero(d.reshape(-1) > 0)
  d.reshape(-1)[cells] = 1.0 + np.arange(len(cells)) * 1e-3
  assert len(cells) > 255
  with pytest.raises(ValueError, match="cell classes; the device format holds 255"):
    dataclasses.replace(plan, diffusers=d).compile_structural(DT)


def test_building_materials_refusals():
  ok = np.ones((4, 3))
  with pytest.raises(ValueError, match="at least one field"):
    BuildingMaterials()
  with pytest.raises(ValueError, match=r"conductivity must have shape \[B, M\]"):
    BuildingMaterials(conductivity=np.ones(4))
  with pytest.raises(ValueError, match=r"convection_coefficient must have shape \[B\]"):
    BuildingMaterials(convection_coefficient=np.ones((4, 1)))
  with pytest.raises(ValueError, match=r"density must have shape"):
    BuildingMaterials(density=np.ones((0, 3)))
  with pytest.raises(ValueError, match="heat_capacity has 5 rows, the other fields 4"):
    BuildingMaterials(conductivity=ok, heat_capacity=np.ones((5, 3)))
  with pytest.raises(ValueError, match="density has 2 material slots, the other fields 3"):
    BuildingMaterials(conductivity=ok, density=np.ones((4, 2)))
  with pytest.raises(ValueError, match="convection_coefficient has 3 rows"):
    BuildingMaterials(conductivity=ok, convection_coefficient=np.ones(3))
  for name in ("conductivity", "heat_capacity", "density"):
    for bad, what in ((np.nan, "is not finite"), (np.inf, "is not finite"), (0.0, "must be positive"),
                      (-1.0, "must be positive")):
      a = ok.copy()
      a[2, 1] = bad
      with pytest.raises(ValueError, match=f"building 2: {name} {what}"):
        BuildingMaterials(**{name: a})
  h = np.array([1.0, 0.0, 5.0, 7.0])
  BuildingMaterials(convection_coefficient=h)   # 0 is allowed
  for bad, what in ((np.nan, "is not finite"), (-0.5, "must not be negative")):
    a = h.copy()
    a[3] = bad
    with pytest.raises(ValueError, match=f"building 3: convection_coefficient {what}"):
      BuildingMaterials(convection_coefficient=a)
  bm = BuildingMaterials(conductivity=ok, convection_coefficient=h)
  with pytest.raises(ValueError, match="4 rows, the simulator 5 buildings"):
    bm.check_plan(5, 3)
  with pytest.raises(ValueError, match="3 material slots, the floor plan 2"):
    bm.check_plan(4, 2)
  with pytest.raises(ValueError, match="outside the table's 4 buildings"):
    bm.rows(2, 5)
  assert bm.rows(1, 3).n_buildings == 2 and bm.rows(1, 3).fields["convection_coefficient"].tolist() == [0.0, 5.0]


def test_c_table_and_effective_values():
  k = np.arange(1.0, 7.0).reshape(2, 3)
  bm = BuildingMaterials(conductivity=k, convection_coefficient=[3.0, 4.0])
  fields, values = bm.c_table(3)
  assert fields.tolist() == [0, 1, 2, 9] and values.shape == (4, 2)
  assert np.array_equal(values[:3].T, k) and values[3].tolist() == [3.0, 4.0]
  table = np.array([[50.0, 700.0, 1.0], [0.05, 700.0, 1.0], [50.0, 1.0, 700.0]])
  eff = effective_building_materials(bm, table, 12.0, 2)
  assert np.array_equal(eff["conductivity"], k) and eff["convection_coefficient"].tolist() == [3.0, 4.0]
  assert np.array_equal(eff["density"], np.tile(table[:, 2], (2, 1)))
  none = effective_building_materials(None, table, 12.0, 2)
  assert np.array_equal(none["heat_capacity"], np.tile(table[:, 1], (2, 1))) and none["convection_coefficient"].tolist() == [12.0, 12.0]
