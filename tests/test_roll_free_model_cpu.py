"""k_sweep_roll's free periods on the CPU: the NumPy replay of the schedule (tests/roll_free_model.py) against the plain
rolling schedule (tests/kernel_model.py) and the oracle -- grids bit-identical to the plain schedule's, sweep counts equal
to the oracle's, and the accumulator hygiene the kernel relies on (asserted inside the model: a measuring period behind a
free one yields its sweep's true max|delta| high word; the proof at a period's top reads only the sweep in progress; a
free period is never the step's last sweep)."""
import numpy as np
import pytest

from oracle import oracle as orc
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
from tests.roll_free_model import RollFreeModel
from tests.twins import oracle_plan_of

PLANS = [((3, 3), (20, 30), 3),   # R9: 66 x 96, two tail rows
         ((2, 3), (30, 30), 3),   # 65 x 94: one tail row
         ((2, 3), (20, 30), 1)]   # 43 x 94: pad lanes


def _case(rooms, shape, seed=5):
  fp = FloorPlan.from_file_input(rectangular_floor_plan(rooms, shape), Materials.sb1(), 10.0, 300.0)
  cp = fp.compile(300.0, 100.0)
  rs = np.random.RandomState(seed)
  H, W = fp.shape
  prev = np.clip(293.0 + 1.5 * rs.randn(H, W), 285.0, 300.0)
  qz = rs.uniform(-400.0, 900.0, size=cp.Z)
  q = np.zeros((H, W))
  for z, cells in enumerate(fp.zone_cell_lists()):
    q.reshape(-1)[cells] = qz[z] * fp.diffusers.reshape(-1)[cells]
  plan = oracle_plan_of(fp)
  return cp, plan, prev, qz, q


@pytest.mark.parametrize("rooms,shape,mode", PLANS)
def test_free_periods_change_neither_grid_nor_sweep_count(rooms, shape, mode):
  cp, plan, prev, qz, q = _case(rooms, shape)
  m = RollFreeModel(cp)
  assert m.mode == mode
  ref, n_ref, _ = orc.fd_timestep(plan, prev, q, 279.5, 100.0, 300.0, 0.05, 40)
  plain, n_plain = m.fd_timestep(prev, 279.5, qz, 0.05, 40, schedule="rolling")
  meas, n_meas, log_m = m.fd_timestep_free(prev, 279.5, qz, 0.05, 40, free=False)
  got, n_got, log = m.fd_timestep_free(prev, 279.5, qz, 0.05, 40, free=True)
  assert n_got == n_meas == n_plain == n_ref and n_ref >= 3
  assert np.array_equal(got, plain) and np.array_equal(meas, plain)
  assert np.abs(got - ref).max() < 1e-10
  kinds = [k for k, _, _ in log]
  assert kinds[-1] == "measuring" and kinds.count("free") >= 1 and all(k == "measuring" for k, _, _ in log_m)
  # the two schedules see the same proofs and the same sweeps
  assert [(t, md) for _, t, md in log] == [(t, md) for _, t, md in log_m]
  # every sweep but the last is above the threshold here; those whose triangle alone shows it ran free
  assert kinds.count("free") == sum(1 for _, t, _ in log[:-1] if t > int(np.float64(0.05).view(np.uint64) >> np.uint64(32)))


@pytest.mark.parametrize("limit", [1, 2, 3])
def test_the_sweep_that_reaches_the_iteration_limit_measures(limit):
  """The limit ends a step whatever max|delta| is: its last period keeps the copies that undo the started sweep."""
  cp, plan, prev, qz, q = _case((3, 3), (20, 30), seed=11)
  m = RollFreeModel(cp)
  ref, n_ref, _ = orc.fd_timestep(plan, prev, q, 279.5, 100.0, 300.0, 1e-9, limit)
  plain, _ = m.fd_timestep(prev, 279.5, qz, 1e-9, limit, schedule="rolling")
  got, n_got, log = m.fd_timestep_free(prev, 279.5, qz, 1e-9, limit)
  assert n_got == n_ref == limit
  assert np.array_equal(got, plain) and np.abs(got - ref).max() < 1e-10
  assert [k for k, _, _ in log] == ["free"] * (limit - 1) + ["measuring"]
