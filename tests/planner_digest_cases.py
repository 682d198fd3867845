"""The corpus of tests/test_planner_digest_cpu.py and the generator of its golden (host only).

An entry is a compiled floor plan in one orientation under one setting of the planner's switches; what is recorded for it is
sb_plan_info's status, sb_last_error()'s text on a refusal, the whole sb_launch_info and sb_debug_plan_digest's hash of
every table and launch scalar the planner hands the chosen sweep kernel.  tests/golden/plan_digests.json holds these for
the planner as it was BEFORE it moved into planner.cpp (tools/README.md has the commands); regenerate it only when a
change means to alter a table:  python -m tests.planner_digest_cases --write"""
import ctypes as C
import functools
import json
import os
import sys
from typing import Dict, Iterator, List, Tuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digests.json")

# every switch the planner reads: set by an entry or absent, never inherited
PLANNER_SWITCHES = ("SBSIM_FORCE_STREAM_PATH", "SBSIM_FORCE_LDS_PATH", "SBSIM_BAND_PATH", "SBSIM_NO_TWO_ROW_PATH",
                    "SBSIM_NO_BAND_PATH", "SBSIM_NO_TWO_64", "SBSIM_NO_ROLL_64", "SBSIM_NO_ROLL_SMALL", "SBSIM_TWO_GENERAL",
                    "SBSIM_TWO_MAX_LEVEL", "SBSIM_DEBUG_LDS_PAD", "SBSIM_STREAM_MS", "SBSIM_STREAM_ROLL", "SBSIM_DEBUG_CUS")

# the settings every plan of the seeded family appears under
FAMILY_SETTINGS: Tuple[Tuple[str, Tuple[Tuple[str, str], ...]], ...] = (
    ("default", ()),
    ("force-lds", (("SBSIM_FORCE_LDS_PATH", "1"),)),
    ("force-stream", (("SBSIM_FORCE_STREAM_PATH", "1"),)),
    ("band-path", (("SBSIM_BAND_PATH", "1"),)),
    ("no-two", (("SBSIM_NO_TWO_ROW_PATH", "1"),)),
    ("no-two-no-band", (("SBSIM_NO_TWO_ROW_PATH", "1"), ("SBSIM_NO_BAND_PATH", "1"))),
    ("no-roll-small", (("SBSIM_NO_ROLL_SMALL", "1"),)),
    ("no-roll-64", (("SBSIM_NO_ROLL_64", "1"),)),
    ("no-two-64", (("SBSIM_NO_TWO_64", "1"),)),
    ("two-general", (("SBSIM_TWO_GENERAL", "1"),)),
    ("two-max-level-0", (("SBSIM_TWO_MAX_LEVEL", "0"),)),
    ("two-max-level-1", (("SBSIM_TWO_MAX_LEVEL", "1"),)),
    ("lds-pad", (("SBSIM_DEBUG_LDS_PAD", "30000"),)),
)
FAMILY_N, FAMILY_SEED = (16, 8), 7


class _Switches:
  """The planner's switches for a block: `pairs` set, every other one absent; restored afterwards."""

  def __init__(self, pairs):
    self.pairs = dict(pairs)

  def __enter__(self):
    self.old = {k: os.environ.pop(k, None) for k in set(PLANNER_SWITCHES) | set(self.pairs)}
    os.environ.update(self.pairs)

  def __exit__(self, *exc):
    for k, v in self.old.items():
      os.environ.pop(k, None)
      if v is not None:
        os.environ[k] = v


def _rect(rooms, shape):
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  return FloorPlan.from_file_input(rectangular_floor_plan(rooms, shape), Materials.sb1(), 10.0, 300.0)


def family() -> List[Tuple[Tuple[int, int], Tuple[int, int]]]:
  """(rooms, room shape) drawn as tools/fuzz_planner.py draws them: FAMILY_N[0] within its limits (262 rows x 110 columns:
  the register kernels' range), FAMILY_N[1] up to 300 rows x 420 columns."""
  rs = np.random.RandomState(FAMILY_SEED)
  out = []
  for n, (rooms0, rooms1, w_hi, rows_hi, cols_hi, zones_hi) in zip(FAMILY_N, ((8, 6, 45, 262, 110, 60), (15, 10, 60, 300, 420, 126))):
    while n > 0:
      r0, r1 = int(rs.randint(1, rooms0)), int(rs.randint(1, rooms1))
      h, w = int(rs.randint(4, 60)), int(rs.randint(4, w_hi))
      rows, cols = r0 * (h + 1) + 3, r1 * (w + 1) + 3
      if 12 <= rows <= rows_hi and 12 <= cols <= cols_hi and r0 * r1 <= zones_hi:
        out.append(((r0, r1), (h, w)))
        n -= 1
  # the family's own corners: one room of 4 x 4, and the 300 x 420 limit itself
  return out + [((1, 1), (4, 4)), ((9, 9), (32, 45))]


# the plans of tests/test_abi_cpu.py's plan-info tests: (name, rooms, room shape, settings)
_ABI = (
    ("r9", (3, 3), (20, 30), ((),)), ("sb1", (14, 9), (8, 7), ((),)), ("small", (1, 2), (6, 8), ((),)),
    ("wide", (2, 3), (20, 30), ((),)), ("narrow", (4, 5), (10, 8), ((),)), ("mid80", (2, 3), (20, 24), ((),)),
    ("mid84", (2, 3), (30, 24), ((),)), ("big", (14, 9), (20, 43), ((),)), ("tall", (1, 1), (1119, 20), ((),)),
    ("huge", (1, 1), (514, 1094), ((),)), ("sb2", (8, 5), (12, 14), ((), (("SBSIM_BAND_PATH", "1"),))),
    ("p4", (10, 4), (19, 20), ((), (("SBSIM_NO_BAND_PATH", "1"),))), ("i3", (10, 4), (18, 20), ((),)),
    ("i96", (10, 4), (19, 22), ((),)), ("i3b", (9, 4), (16, 17), ((),)), ("wide153", (6, 6), (24, 24), ((),)),
    ("w2", (6, 4), (17, 21), ((), (("SBSIM_NO_BAND_PATH", "1"),))),
    ("two64", (8, 5), (12, 10), ((), (("SBSIM_NO_TWO_64", "1"),))), ("band68", (9, 4), (16, 15), ((),)),
    ("band72", (12, 3), (20, 22), ((),)),
)


@functools.lru_cache(maxsize=None)
def _compiled(source: str, name, columns: bool, h_conv: float):
  """The compiled plan of a source ("abi", "family", "irregular", "handover", "threshold", "convection") by name."""
  if source in ("abi", "family"):
    fp = _rect(*name)
  elif source == "irregular":
    from tests import irregular_plans as ip
    fp = ip.plan(name)
  elif source == "handover":
    from tests import handover_cases as hc
    fp = hc.floor_plan(hc.Case("", name, "rows", 1, 0, 1, 0, 1, 1))
  elif source == "threshold":
    from tests import threshold_cases as tc
    fp = tc.floor_plan(name)
  else:
    from tests import convection_cases as cc
    fp = cc._plan(name)
  return (fp.transposed() if columns else fp).compile(300.0, h_conv)


def corpus() -> Iterator[Tuple[str, tuple, Tuple[Tuple[str, str], ...], bool]]:
  """(key, arguments of _compiled, switches, per-building tables) of every entry; keys are unique."""
  from tests import convection_cases as cc
  from tests import handover_cases as hc
  from tests import irregular_plans as ip
  from tests import threshold_cases as tc
  tag = lambda env: ",".join(f"{k[6:]}={v}" for k, v in env) or "default"
  for name, c in ip.CASES.items():
    yield f"irregular/{name}", ("irregular", name, c.orientation == "columns", 12.0), tuple(c.env), False
  for name, c in hc.CASES.items():
    yield (f"handover/{name}", ("handover", c.plan, c.orientation == "columns", 100.0),
           tuple(sorted(hc.case_env(c).items())), False)
  for name in tc.PLANS:
    for columns in (False, True):
      yield f"threshold/{name}/{'columns' if columns else 'rows'}", ("threshold", name, columns, 100.0), (), False
  seen = set()
  for name, c in cc.CASES.items():   # (many cases share a plan, an orientation and switches: one entry each)
    env = tuple(sorted((k, v) for k, v in cc.case_env(c).items() if k in PLANNER_SWITCHES))
    what = (c.plan, c.orientation, env)
    if what not in seen:
      seen.add(what)
      yield f"convection/{name}", ("convection", c.plan, c.orientation == "columns", 100.0), env, False
  for name, rooms, shape, settings in _ABI:
    for columns in (False, True):
      for env in settings:
        yield f"abi/{name}/{'columns' if columns else 'rows'}/{tag(env)}", ("abi", (rooms, shape), columns, 12.0), env, False
  for i, spec in enumerate(family()):
    for columns in (False, True):
      where = f"family/{i}-{spec[0][0]}x{spec[0][1]}-{spec[1][0]}x{spec[1][1]}/{'columns' if columns else 'rows'}"
      for sname, env in FAMILY_SETTINGS:
        yield f"{where}/{sname}", ("family", spec, columns, 12.0), env, False
      yield f"{where}/per-building-tables", ("family", spec, columns, 12.0), (), True


def measure(args: tuple, env, per_building: bool) -> list:
  """[status, sb_last_error() on a refusal, sb_launch_info's fields in order, the digest in hex]."""
  from sbsim_amd import _ffi
  cp = _compiled(*args)
  keep = [np.ascontiguousarray(x) for x in (cp.cell_class, cp.class_coef, cp.class_zone, cp.zone_off, cp.zone_cells)]
  desc = _ffi.PlanDesc(cp.H, cp.W, cp.Z, cp.n_classes, keep[0].ctypes.data_as(C.POINTER(C.c_uint8)),
                       keep[1].ctypes.data_as(_ffi._dp), keep[2].ctypes.data_as(_ffi._ip),
                       keep[3].ctypes.data_as(_ffi._ip), keep[4].ctypes.data_as(_ffi._ip))
  L = _ffi.load()
  info, digest = _ffi.LaunchInfo(), C.c_uint64(0)
  plan_info = _ffi.entry("sb_plan_info_materials") if per_building else L.sb_plan_info
  with _Switches(env):
    rc = plan_info(C.byref(desc), 3 * cp.Z + 19, 1024, C.byref(info))
    err = L.sb_last_error().decode() if rc != 0 else ""
    rc2 = _ffi.entry("sb_debug_plan_digest")(C.byref(desc), 1 if per_building else 0, C.byref(digest))
    err2 = L.sb_last_error().decode() if rc2 != 0 else ""
  assert (rc2, err2) == (rc, err), (rc, err, rc2, err2)   # the digest entry answers as the plan-info entry does
  fields = [getattr(info, f[0]) for f in _ffi.LaunchInfo._fields_] if rc == 0 else []
  return [rc, err, fields, f"{digest.value:016x}"]


def measure_all() -> Dict[str, list]:
  out = {}
  for key, args, env, per_building in corpus():
    assert key not in out, key
    out[key] = measure(args, env, per_building)
  return out


if __name__ == "__main__":
  if sys.argv[1:] != ["--write"]:
    sys.exit("usage: python -m tests.planner_digest_cases --write")
  with open(GOLDEN, "w") as f:
    json.dump(measure_all(), f, indent=0, sort_keys=True, separators=(",", ":"))
    f.write("\n")
  print("wrote", GOLDEN)
