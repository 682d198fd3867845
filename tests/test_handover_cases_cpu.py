"""CPU: the divergent batches of tests/handover_cases.py are what tests/test_handover_gpu.py needs them to be.

On the oracle twins alone, every case has a step at which one building needs at most two sweeps, one ends at the
iteration limit unconverged, one converges strictly between the two, and the batch holds at least five distinct sweep
counts -- so that workgroups meet predecessors that ended in every way.  sb_plan_info (host only) gives the kernel, the
wavefront count and, with SBSIM_DEBUG_CUS=1, the buildings handed out by index: every batch is four hand-overs deep,
and the switch changes nothing the planner chooses."""
import numpy as np
import pytest

from tests import handover_cases as hc


def test_every_case_of_the_issue_is_there():
  kernels = {c.kernel for c in hc.CASES.values()} | {c.kernel for c in hc.JACOBI_CASES.values()}
  assert kernels == {hc.LDS, hc.REG, hc.REG_PAIR, hc.ROLL, hc.TWO, hc.BAND, hc.STREAM, hc.JACOBI}
  assert {c.waves for c in hc.CASES.values() if c.kernel == hc.BAND} == {2, 3, 4}
  assert {c.waves for c in hc.CASES.values() if c.kernel == hc.STREAM} == {1, 2, 3, 4, 5}
  assert set(hc.NATURAL) <= set(hc.CASES)


def test_the_ladder_and_the_shuffle():
  init, acts, kind = hc.batch(500, 19, 4, 31)
  assert init.shape == (19, 500) and acts.shape == (4, 19, 2) and acts.dtype == np.float32
  assert sorted(np.bincount(kind).tolist()) == [6, 6, 7] and not (kind == np.arange(19) % 3).all()   # shuffled
  span = init.max(axis=1) - init.min(axis=1)
  assert (span[kind == 0] == 0.0).all()                                   # exactly isothermal
  assert (span[kind == 1] > 0.0).all() and (span[kind == 1] < 0.1).all()  # noise of 0.01 K
  assert (span[kind == 2] > 10.0).all()                                   # noise of 3 K
  assert init.min() >= 285.0 and init.max() <= 305.0
  again = hc.batch(500, 19, 4, 31)
  assert all(np.array_equal(a, b) for a, b in zip((init, acts, kind), again))


@pytest.mark.parametrize("name", list(hc.CASES))
def test_pins_depth_and_that_the_switch_only_changes_the_geometry(name):
  case = hc.CASES[name]
  one, three, free = (hc.plan_info(case, case.B, cus) for cus in (1, 3, None))
  assert (free["kernel"], free["waves_per_building"], free["path"]) == (case.kernel, case.waves, case.path), free
  assert free["sweep_steps"] == case.steps, free
  for capped in (one, three):
    assert all(capped[k] == free[k] for k in hc.PINNED), (capped, free)
  assert case.B >= hc.DEPTH * hc.static_count(one) + 3, (case.B, one)
  assert three["workgroups"] == 3 * one["workgroups"] and free["workgroups"] >= three["workgroups"]
  big = hc.plan_info(case, 1 << 20)
  assert big["workgroups"] == hc.NATURAL_CUS * hc.plan_info(case, 1 << 20, 1)["workgroups"]


@pytest.mark.parametrize("name", list(hc.CASES))
def test_spread_of_sweep_counts_on_the_oracle(name):
  case = hc.CASES[name]
  n, conv = hc.oracle_rollout(case)
  t = hc.spread(n, conv, case.limit)
  assert t is not None, [sorted(row.tolist()) for row in n]
  print(f"{name}: step {t}: sweeps {sorted(n[t].tolist())}")


@pytest.mark.parametrize("name", list(hc.NATURAL))
def test_spread_among_the_checked_buildings_of_the_natural_batches(name):
  """The batch of the device's own geometry (static count + 7 buildings): the spread holds already among the buildings
  that get a twin and the 48 before the drawn ones (the whole batch is thousands of buildings)."""
  case = hc.natural_case(name)
  static = hc.natural_static(case)
  B = static + hc.NATURAL_EXTRA
  some = sorted(set(hc.natural_checked(static)) | set(range(static - 48, static)))
  n, conv = hc.oracle_rollout(case, some, B)
  assert hc.spread(n, conv, case.limit) is not None, [sorted(row.tolist()) for row in n]
