"""The parity harness itself (tests/twins.py, tests/parity.py and the case tables), without a GPU: the bars of
assert_step_matches are the ones the suite claims, the oracle side imports without torch, and no module borrows from a
test module."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sbsim_amd.environment import SimConfig
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
from tests import twins
from tests.golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def step():
  """One oracle step on the 15 x 23 plan and the device rows that match it exactly: (info row, zone temperatures,
  reward, the oracle's result)."""
  fp = FloorPlan.from_file_input(rectangular_floor_plan((2, 2), (5, 9)), Materials.sb1(), 10.0, 300.0)
  assert (fp.shape[0] - 2, fp.shape[1] - 2) == (15, 23)
  cfg = SimConfig.sb1()
  g = load("h2_sb1_r9_random.npz")
  rs = np.random.RandomState(11)
  init = np.clip(294.0 + 2.0 * rs.randn(1) + 0.2 * rs.randn(fp.shape[0] * fp.shape[1]), 285.0, 305.0)
  o = twins.oracle_twin(fp, cfg, init).step(**twins.step_kwargs(g, 96, 0, cfg, rs.uniform(-1, 1, size=2).astype(np.float32)))
  info = np.zeros(8)
  info[:4], info[4], info[5] = twins.oracle_rates(o), o["n_sweeps"], o["converged"]
  return info, np.array(o["zone_temp_post"], np.float64), float(o["reward"]), o


def test_the_bars_are_the_ones_the_suite_claims():
  assert (twins.T_TOL, twins.RATE_RTOL, twins.RATE_ATOL, twins.REWARD_TOL) == (1e-8, 2e-6, 1e-6, 2e-6)


def test_a_step_inside_half_of_every_tolerance_matches(step):
  info, zt, reward, o = step
  assert o["n_sweeps"] >= 1 and np.abs(info[:4]).max() > 1.0    # (a real step: sweeps ran, the plant drew power)
  twins.assert_step_matches(info, zt, reward, o, "exact")
  for sign in (1.0, -1.0):
    near = info.copy()
    near[:4] += sign * 0.5 * (twins.RATE_ATOL + twins.RATE_RTOL * np.abs(info[:4]))
    twins.assert_step_matches(near, zt + sign * 0.5 * twins.T_TOL, reward + sign * 0.5 * twins.REWARD_TOL, o, "half")


def _changes(info, zt, reward):
  k = int(np.abs(info[:4]).argmax())   # a rate of more than 1 W: 1e-5 of it is beyond atol + rtol * |rate|

  def edit(i=None, v=None, z=None, r=0.0):
    row, zone = info.copy(), zt.copy()
    if i is not None:
      row[i] = v
    if z is not None:
      zone[z] += 2e-8
    return row, zone, reward + r

  return {
      "n_sweeps + 1": edit(4, info[4] + 1), "n_sweeps - 1": edit(4, info[4] - 1), "converged flipped": edit(5, 1.0 - info[5]),
      "one zone temperature + 2e-8 K": edit(z=len(zt) - 1), "one rate * (1 + 1e-5)": edit(k, info[k] * (1.0 + 1e-5)),
      "reward + 1e-5": edit(r=1e-5),
  }


@pytest.mark.parametrize("change", ["n_sweeps + 1", "n_sweeps - 1", "converged flipped", "one zone temperature + 2e-8 K",
                                    "one rate * (1 + 1e-5)", "reward + 1e-5"])
def test_each_change_alone_fails_the_step(step, change):
  info, zt, reward, o = step
  row, zone, rew = _changes(info, zt, reward)[change]
  with pytest.raises(AssertionError, match="somewhere"):
    twins.assert_step_matches(row, zone, rew, o, "somewhere")


def _support_modules():
  names = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "tests", "*cases.py")))
  return ["twins"] + names + ["regimes", "zone_ladder", "irregular_plans", "crossed_batches"]


def test_the_cpu_support_modules_import_without_torch():
  mods = _support_modules()
  assert {"threshold_cases", "handover_cases", "materials_cases", "reward_cases", "params_cases", "jacobi_cases"} <= set(mods)
  code = ("import sys; sys.modules['torch'] = None\n"
          "import importlib\n"
          f"for m in {mods!r}: importlib.import_module('tests.' + m)\n"
          "assert sys.modules['torch'] is None\n")
  r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr[-3000:]


def test_no_module_imports_from_a_test_module():
  pat = re.compile(r"from tests\.test_|import tests\.test_")
  files = [p for d in ("tests", "tools", "oracle") for p in glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)]
  assert len(files) > 100
  hits = [os.path.relpath(p, ROOT) for p in files if pat.search(open(p).read())]
  assert not hits, hits
