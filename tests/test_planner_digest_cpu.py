"""CPU: every table and launch scalar the planner (sbsim_amd/csrc/planner.cpp) hands a sweep kernel, pinned by digest.

The sweep kernels trust cmapS, amapS, zmapS, cell_state, tcls, tcset, tmul and the LDS offsets without checking, and
sb_plan_info reports the launch geometry alone.  sb_debug_plan_digest hashes all of it; tests/golden/plan_digests.json
holds status, refusal text, sb_launch_info and digest of every entry of tests/planner_digest_cases.py's corpus, written by
the planner as it was before it became a unit of its own (tools/README.md)."""
import json

import pytest

from tests import planner_digest_cases as pc

LDS, STREAM, TOO_LARGE = 0, 6, -4                  # sb_sweep_kernel, sb_status (include/sbsim_amd.h)
INFO = ("waves_per_workgroup", "workgroups", "lds_bytes_per_workgroup", "sweep_steps", "algorithmic_bytes_per_env_step",
        "state_bytes_per_env_step", "path", "waves_per_building", "kernel", "reserved")   # sb_launch_info, in order


@pytest.fixture(scope="module")
def measured():
  return pc.measure_all()


@pytest.fixture(scope="module")
def golden():
  with open(pc.GOLDEN) as f:
    return json.load(f)


def test_every_entry_equals_the_golden(measured, golden):
  assert sorted(measured) == sorted(golden)
  wrong = {k: (v, golden[k]) for k, v in measured.items() if v != golden[k]}
  assert not wrong, (len(wrong), sorted(wrong)[:20], next(iter(wrong.values())))


def test_corpus_reaches_every_kernel_and_shape_of_plan(measured):
  """On the corpus itself, from sb_plan_info: every sweep kernel, one to four wavefronts per building, both orientations, a
  refusal.  (A condition that fails: extend the corpus.)"""
  from sbsim_amd import _ffi
  assert tuple(f[0] for f in _ffi.LaunchInfo._fields_) == INFO
  infos = [dict(zip(INFO, v[2])) for v in measured.values() if v[0] == 0]
  assert {i["kernel"] for i in infos} >= set(range(LDS, STREAM + 1))
  assert {i["waves_per_building"] for i in infos} >= {1, 2, 3, 4}
  columns = {args[2] for _, args, _, _ in pc.corpus()}
  assert columns == {False, True}
  refused = [v for v in measured.values() if v[0] == TOO_LARGE]
  assert refused and all(v[1] and v[3] == "0" * 16 for v in refused)
  assert any(per_building and measured[k][0] == 0 for k, _, _, per_building in pc.corpus())
