"""CPU checks for the Jacobi solver on floor plans beyond one CU's LDS (k_sweep_jacobi_g): sb_create_jacobi's size
rule, and the NumPy restatement against the reference's finite_differences_timestep on the 155 x 155 plan
(tests/golden/jacobi_fd_large.npz, tools/gen_golden_jacobi.py --large) -- no device needed."""
import contextlib
import re

import numpy as np
import pytest

from sbsim_amd import _ffi
from sbsim_amd.environment import BatchedSimulator, SimConfig
from sbsim_amd.floorplan import FloorPlan
from tests import jacobi_restatement as jr
from tests.golden_util import load
from tests.jacobi_cases import PLAN_155, PLAN_SB1, large_case, large_plan

f32 = np.float32
SB_ERR_NO_DEVICE, SB_ERR_TOO_LARGE = -2, -4


def _create_code(fp, monkeypatch):
  """The code sb_create_jacobi answers for one building of this plan (0 with a device).  Without a device
  BatchedSimulator would stop before it calls the library, so its two uses of torch.cuda are stood in for."""
  from sbsim_amd import environment
  if not environment.torch.cuda.is_available():
    monkeypatch.setattr(environment.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(environment.torch.cuda, "device", lambda _: contextlib.nullcontext())
  try:
    BatchedSimulator(fp, SimConfig.sb1(), 1, 100.0, solver="jacobi_fp32").close()
  except _ffi.SbsimError as e:
    m = re.search(r"sb_create_jacobi failed \((-?\d+)\)", str(e))
    assert m, f"not sb_create_jacobi's answer: {e}"
    return int(m.group(1)), str(e)
  return 0, ""


@pytest.mark.parametrize("rooms,room_shape,shape", [(*PLAN_155, (155, 155)), (*PLAN_SB1, (299, 401))])
def test_plans_beyond_lds_are_not_too_large(rooms, room_shape, shape, monkeypatch):
  fp = large_plan(rooms, room_shape)
  assert fp.shape == shape and shape[0] * shape[1] > 20480
  assert fp.compile_jacobi(300.0, 100.0).n_classes <= 255
  code, msg = _create_code(fp, monkeypatch)
  # the size check comes before the device check: a box without a GPU answers SB_ERR_NO_DEVICE
  assert code in (0, SB_ERR_NO_DEVICE), (code, msg)


def test_a_plan_beyond_the_global_kernels_limit_is_too_large_and_says_the_limit(monkeypatch):
  """1,025 x 1,024 CVs > 2^20: a solid block in a ring of exterior space (few classes)."""
  H, W = 1025, 1024
  ext = np.ones((H, W), bool)
  ext[1:-1, 1:-1] = False
  label = np.full((H, W), -1, np.int16)
  label[2:-2, 2:-2] = 0
  diff = np.zeros((H, W))
  diff[3, 3] = 1.0
  fp = FloorPlan(conductivity=np.full((H, W), 2.0), heat_capacity=np.full((H, W), 500.0), density=np.full((H, W), 1800.0),
                 exterior_space=ext, zone_label=label, diffusers=diff, cv_size_cm=20.0, floor_height_cm=300.0)
  code, msg = _create_code(fp, monkeypatch)
  assert code == SB_ERR_TOO_LARGE, (code, msg)
  assert str(1 << 20) in msg, msg


def test_restatement_equals_the_reference_fd_timestep_on_the_155_plan_bitwise():
  g = load("jacobi_fd_large.npz")
  assert int(str(g["numpy_version"]).split(".")[0]) >= 2
  fp = large_plan(tuple(int(v) for v in g["rooms"]), tuple(int(v) for v in g["room_shape"]))
  assert fp.shape == (155, 155)
  tt = jr.tensors(fp, float(g["dt"]), float(g["h"]))
  seen = []
  for seed in g["seeds"]:
    prev, qz, tinf = large_case(int(seed), fp.shape, fp.n_zones)
    for limit in g["limits"]:
      key = f"{int(seed)}_{int(limit)}"
      grid, n, conv = jr.fd_timestep(tt, prev, jr.input_q(fp, qz), tinf, float(g["dt"]), float(g["thr"]), int(limit))
      assert (n, conv) == (int(g[key + "_iterations"]), bool(g[key + "_converged"])), key
      assert np.array_equal(grid.view(np.uint32), g[key + "_grid"].view(np.uint32)), key
      seen.append(conv)
  assert True in seen and False in seen   # both ways out of the loop
