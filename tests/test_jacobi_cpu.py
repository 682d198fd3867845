"""CPU checks of the Jacobi solver's host side (FloorPlan.compile_jacobi, the NumPy restatement, the division route of
k_sweep_jacobi, the Python switch's refusals) -- no device needed."""
import numpy as np
import pytest

from sbsim_amd import _ffi
from sbsim_amd.floorplan import JACOBI_FIELDS, FloorPlan, Materials, jacobi_cv_tensors, rectangular_floor_plan
from tests import jacobi_restatement as jr
from tests.golden_util import load
from tests.jacobi_cases import GOLDEN_PLANS, golden_plan
from tests.twins import plan_from_npz

f32 = np.float32
PLANS = ("plan_r9_sb1.npz", "plan_r9_test.npz", "plan_small_test.npz", "plan_weird_test.npz")


def _box(H=6, W=7):
  """A solid H x W block inside a ring of exterior space: every corner and edge orientation once."""
  ext = np.ones((H + 2, W + 2), bool)
  ext[1:-1, 1:-1] = False
  shape = ext.shape
  label = np.full(shape, -1, np.int16)
  label[2:-2, 2:-2] = 0
  diff = np.zeros(shape)
  diff[3, 3] = 1.0
  return FloorPlan(conductivity=np.full(shape, 2.0), heat_capacity=np.full(shape, 500.0), density=np.full(shape, 1800.0),
                   exterior_space=ext, zone_label=label, diffusers=diff, cv_size_cm=20.0, floor_height_cm=300.0)


@pytest.mark.parametrize("name", PLANS)
def test_compile_jacobi_tables_expand_to_the_cv_tensors(name):
  fp = plan_from_npz(load(name))
  jp = fp.compile_jacobi(300.0, 100.0)
  t = jacobi_cv_tensors(fp, 300.0, 100.0)
  e = jp.expand()
  for f in JACOBI_FIELDS[:-1]:
    assert e[f].dtype == np.float32 and np.array_equal(e[f].view(np.uint32), t[f].view(np.uint32)), f
  assert np.array_equal(e["exterior"], t["exterior"])
  assert jp.n_classes <= 255 and jp.cell_class.shape == (fp.shape[0] * fp.shape[1],)
  # q's weight and zone: the diffusers of the zones' CVs, nowhere else
  on = e["diffuser"] > 0
  assert np.array_equal(e["diffuser"][on], fp.diffusers[on]) and (fp.zone_label[on] == e["zone"][on]).all()


def test_boundary_orientations_follow_the_reference():
  """tf_simulator.py:180-456: a missing neighbour above -> TOP (v halved, k_top = 0, h_top = h), left (j-1) -> LEFT
  (u halved, k_left = 0, h_left = h), corners both; 0-1 neighbours -> exterior."""
  fp = _box()
  t = jacobi_cv_tensors(fp, 300.0, 12.5)
  cv, h = f32(0.2), f32(12.5)
  half = f32(0.2 * 0.5)
  # top-left corner (1, 1): neighbours below and right
  assert t["u"][1, 1] == half and t["v"][1, 1] == half
  assert t["hT"][1, 1] == h and t["hL"][1, 1] == h and t["hB"][1, 1] == 0 and t["hR"][1, 1] == 0
  assert t["kT"][1, 1] == 0 and t["kL"][1, 1] == 0 and t["kB"][1, 1] == f32(2.0)
  # left edge (3, 1): u halved, left side outside
  assert t["u"][3, 1] == half and t["v"][3, 1] == cv and t["hL"][3, 1] == h and t["kL"][3, 1] == 0
  assert t["k1u"][3, 1] == 0 and t["k3u"][3, 1] == f32(2.0) / half
  # bottom edge (6, 3): v halved, bottom outside
  assert t["v"][6, 3] == half and t["hB"][6, 3] == h and t["k2v"][6, 3] == 0
  # interior and exterior
  assert t["u"][3, 3] == cv and t["v"][3, 3] == cv and not t["exterior"][3, 3]
  assert t["exterior"][0, 0] and t["exterior"][0, 4]
  # den and M in the reference's op order (the heat capacity twice)
  z = f32(3.0)
  M = (z * (((f32(1800.0) * half) * half) * f32(500.0))) * f32(500.0)
  assert t["M"][1, 1] == M


def test_opposite_neighbours_raise_value_error():
  fp = _box(5, 5)
  ext = fp.exterior_space.copy()
  ext[1:-1, 3] = True        # cut the block: a single solid column (up and down neighbours only) next to it
  ext[1:-1, 1] = True
  fp2 = FloorPlan(conductivity=fp.conductivity, heat_capacity=fp.heat_capacity, density=fp.density, exterior_space=ext,
                  zone_label=fp.zone_label, diffusers=fp.diffusers, cv_size_cm=fp.cv_size_cm,
                  floor_height_cm=fp.floor_height_cm)
  with pytest.raises(ValueError, match="corner"):
    fp2.compile_jacobi(300.0, 100.0)


def test_horizontal_neighbours_are_swapped_as_in_the_reference():
  """TL = T[i][j+1] goes with k_left / u and TR = T[i][j-1] with k_right / u: a LEFT-edge CV conducts with the cell
  on its exterior side (j - 1), not with its interior neighbour (j + 1).  The vertical pair is not swapped."""
  fp = _box()
  tt = jr.tensors(fp, 300.0, 100.0)
  rs = np.random.RandomState(1)
  T = (290.0 + rs.rand(*fp.shape)).astype(f32)
  q = np.zeros(fp.shape, f32)
  base, _ = jr.update(tt, T, T, q, 280.0, 300.0)
  i, j = 3, 1                                   # left edge
  for dj, moves in ((-1, True), (+1, False)):
    T2 = T.copy()
    T2[i, j + dj] += f32(5.0)
    new, _ = jr.update(tt, T2, T, q, 280.0, 300.0)
    assert (new[i, j] != base[i, j]) == moves, dj
  i, j = 1, 3                                   # top edge: no conduction with the row above
  for di, moves in ((-1, False), (+1, True)):
    T2 = T.copy()
    T2[i + di, j] += f32(5.0)
    new, _ = jr.update(tt, T2, T, q, 280.0, 300.0)
    assert (new[i, j] != base[i, j]) == moves, di
  # the compiled tables agree: a left edge has k1u == 0 and k3u > 0
  e = fp.compile_jacobi(300.0, 100.0).expand()
  assert e["k1u"][3, 1] == 0 and e["k3u"][3, 1] > 0


def _f32_quotient_via_f64(num, den):
  return (num.astype(np.float64) * (1.0 / den.astype(np.float64))).astype(f32)


@pytest.mark.parametrize("name", PLANS)
def test_division_route_is_correctly_rounded_on_the_plans_denominators(name):
  """k_sweep_jacobi computes num / den as float((double)num * (1.0 / (double)den)).  Over every denominator of the
  plan: random numerators across binades, and numerators next to the midpoints of the binary32 quotients."""
  fp = plan_from_npz(load(name))
  dens = np.unique(fp.compile_jacobi(300.0, 100.0).class_f32[:, 6])
  rs = np.random.RandomState(7)
  for den in dens:
    d = np.full(20000, den, f32)
    num = (rs.uniform(1.0, 2.0, 20000) * 2.0 ** rs.randint(-20, 40, 20000)).astype(f32)
    assert np.array_equal(_f32_quotient_via_f64(num, d), num / d), den
    # numerators whose exact quotient sits right next to a rounding midpoint: num ~ den * (m + 1/2 ulp)
    qf = (rs.uniform(250.0, 320.0, 20000)).astype(f32)
    mid = qf.astype(np.float64) + np.spacing(qf).astype(np.float64) / 2
    near = (mid * float(den)).astype(f32)
    for nn in (near, np.nextafter(near, f32(np.inf)), np.nextafter(near, f32(0))):
      assert np.array_equal(_f32_quotient_via_f64(nn, d), nn / d), den


def test_restatement_stops_at_the_float32_threshold():
  fp = _box()
  tt = jr.tensors(fp, 300.0, 100.0)
  T = np.full(fp.shape, 293.0, f32)
  q = jr.input_q(fp, np.array([500.0]))
  g1, n1, c1 = jr.fd_timestep(tt, T, q, 283.0, 300.0, 0.1, 100)
  g2, n2, c2 = jr.fd_timestep(tt, T, q, 283.0, 300.0, 0.1, 2)
  assert c1 and 1 <= n1 <= 100 and g1.dtype == np.float32
  assert n2 == min(n1, 2) and c2 == (n1 <= 2)


def test_missing_jacobi_entries_ask_for_a_rebuild(monkeypatch):
  class Old:   # a library of the same ABI version built before the Jacobi solver
    pass
  monkeypatch.setattr(_ffi, "_lib", Old())
  with pytest.raises(_ffi.SbsimError, match="rebuild"):
    _ffi.jacobi_entry("sb_create_jacobi")


def test_solver_switch_refuses_what_it_cannot_do_without_a_gpu():
  from sbsim_amd.environment import SOLVERS, BatchedSimulator, SimConfig
  assert SOLVERS == ("gauss_seidel", "jacobi_fp32")
  fp = FloorPlan.from_file_input(rectangular_floor_plan((1, 1), (4, 4)), Materials.sb1(), 20.0, 300.0)
  with pytest.raises(ValueError, match="orientation"):
    BatchedSimulator(fp, SimConfig.sb1(), 1, 100.0, solver="jacobi_fp32", orientation="columns")
  with pytest.raises(ValueError, match="solver"):
    BatchedSimulator(fp, SimConfig.sb1(), 1, 100.0, solver="tf")


# ---- against the reference's own TFSimulator (tests/golden/jacobi_*.npz, tools/gen_golden_jacobi.py) ----
@pytest.mark.parametrize("name", sorted(GOLDEN_PLANS))
def test_cv_tensors_equal_the_reference_bitwise(name):
  """(a): u, v, the oriented k and h tensors, den and the exterior mask of TFSimulator equal jacobi_cv_tensors and the
  expanded compile_jacobi tables bit for bit; the reference's CV types agree with the sides found outside."""
  g = load("jacobi_tensors.npz")
  assert str(g["numpy_version"]).split(".")[0] >= "2"
  fp = golden_plan(name)
  h, dt = float(g["h"]), float(g["dt"])
  t = jacobi_cv_tensors(fp, dt, h)
  e = fp.compile_jacobi(dt, h).expand()
  for k in ("u", "v", "kL", "kR", "kT", "kB", "hL", "hR", "hT", "hB", "den"):
    ref = g[f"{name}_{k}"]
    assert ref.dtype == np.float32 and np.array_equal(t[k].view(np.uint32), ref.view(np.uint32)), k
    if k in e:
      assert np.array_equal(e[k].view(np.uint32), ref.view(np.uint32)), k
  assert np.array_equal(t["exterior"], g[f"{name}_exterior"]) and np.array_equal(e["exterior"], g[f"{name}_exterior"])
  # classify_cv's types (0 exterior, 1 interior, 2-5 corners, 6-9 edges): corners have both axes halved, edges one
  codes = g[f"{name}_type"]
  assert np.array_equal(codes == 0, t["exterior"])
  half = f32(fp.cv_size_cm / 100.0 * 0.5)
  n_half = (t["u"] == half).astype(int) + (t["v"] == half).astype(int)
  assert np.array_equal(n_half == 2, (codes >= 2) & (codes < 6)) and np.array_equal(n_half == 1, codes >= 6)


@pytest.mark.parametrize("name", sorted(GOLDEN_PLANS))
def test_restatement_equals_the_reference_fd_timestep_bitwise(name):
  """(b): grid, iteration count and converged flag of finite_differences_timestep, limits 100 and 2."""
  g = load("jacobi_fd.npz")
  fp = golden_plan(name)
  tt = jr.tensors(fp, float(g["dt"]), float(g["h"]))
  for case in range(2):
    for limit in (100, 2):
      key = f"{name}_{case}_{limit}"
      grid, n, conv = jr.fd_timestep(tt, g[key + "_prev"], g[key + "_input_q"].astype(f32), float(g[key + "_t_amb"]),
                                     float(g["dt"]), float(g["thr"]), limit)
      assert (n, conv) == (int(g[key + "_iterations"]), bool(g[key + "_converged"])), key
      assert np.array_equal(grid.view(np.uint32), g[key + "_grid"].view(np.uint32)), key
