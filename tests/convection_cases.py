"""Cases for the device convection shuffle on its own (test utility, no GPU).

`k_convect<Q>` and `k_convect_all` (sbsim_amd/csrc/generators.hip) are checked against their restatement
(oracle/convection_oracle.py) inside a rollout at one geometry only: R9, nine equal 600-cell rectangles, B = 4 -- every
workgroup runs one building, Q is 3, every `i < n` guard sees one n.  The table here pins what that leaves out:

  hand-over   a tiny plan under SBSIM_DEBUG_CUS=1 with so many buildings that every workgroup runs at least DEPTH of them
              and the last round is partly empty (the early draw of the next building, the val/oth hand-over, the re-arm
              of head[], `more` ending at different times; k_convect_all's b += gridDim.x loop);
  q           every instantiation 1 .. 8 through SBSIM_DEBUG_CONV_Q on rooms of unequal sizes, and the natural sizes at
              the boundaries: 256, 257, 600 and 2047 cells (the rank field, the 16-bit packing and the partner table at
              their limits);
  shapes      rooms of 1, 2, 3, 64, 65 and 600 cells in one plan; an L-shaped room, a room with a one-cell-wide corridor
              whose zone also owns two distant closets (partner lists of 1, 2 and 3 cells inside a large zone);
              tests/irregular_plans.py's zone_quirks -- each under the offset table (distance 5), the box branch (20),
              the by-rank branch (-1 with p < 1) and the whole-room shuffle (-1 with p = 1);
  layout      one case per state layout the planner can choose (ConvCell.sidx comes from h_state_index), pinned with
              sb_plan_info / launch_info as tests/handover_cases.py does, table and wide window;
  calls       three launches in a row, and first_building at the end of the 32-bit range.

The input of every case has distinct values, cell g of building b holds float(b * N + g), so the permutation is
identified exactly; exterior-space cells hold AMBIENT (see tests/test_convection_cases_gpu.py for why).
tests/test_convection_cases_cpu.py proves on the restatement alone that every case reaches what it names;
tests/test_convection_cases_gpu.py compares the device with the restatement bit for bit.

Hand-over depth: sb_launch_convection launches min(B, cus * per_cu) workgroups of k_convect, per_cu from the runtime's
occupancy query.  A CU holds at most 32 wavefronts, the tiny plan's workgroup is one wavefront, so per_cu <= 32 and
B = DEPTH * 32 + 3 is deep enough whatever the query answers; k_convect_all launches cus * 8 workgroups."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle.convection_oracle import ConvectionOracle
from tests import handover_cases as hc
from tests import irregular_plans as ip

SWITCH, Q_SWITCH = hc.SWITCH, "SBSIM_DEBUG_CONV_Q"
DEPTH = 4
MAX_RESIDENT = 32                 # single-wavefront workgroups a CU holds at most
ALL_PER_CU = 8                    # k_convect_all: workgroups per CU (sb_launch_convection)
B_HANDOVER = DEPTH * MAX_RESIDENT + 3
AMBIENT = 0.0
MAX_ROOM = 2047                   # kConvMaxRoom
TABLE, RANK, BOX, ALL = "table", "by-rank", "box", "whole-room"
TINY = ((2, 2), (5, 9))


@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  group: str                       # "handover", "q", "shapes", "layout", "calls"
  plan: object                     # (rooms, room shape) of rectangular_floor_plan, a name of PLANS, or a plan of handover_cases
  p: float
  distance: int
  branches: Tuple[str, ...]        # the partner branches the case's rooms take, sorted
  hits: str                        # what the case is built to hit
  q: Optional[int]                 # the k_convect instantiation that runs (None: k_convect_all)
  B: int = 3
  seed: int = 4242
  first_building: int = 1000
  force_q: bool = False            # q through SBSIM_DEBUG_CONV_Q, not from the largest room
  calls: int = 1
  cus: Optional[int] = None        # SBSIM_DEBUG_CUS
  orientation: str = "rows"
  env: Tuple[Tuple[str, str], ...] = ()
  pin: Optional[Tuple[int, int, int]] = None   # launch_info's (kernel, path, waves_per_building)


# ---------------------------------------------------------------- plans
def _sizes():
  """Rooms of 600, 64, 65, 1, 2 and 3 cells (zones in raster order of their first cell: 600, 64, 65, 1, 2, 3)."""
  s = ip.Sketch(26, 50)
  s.air(2, 22, 2, 32).air(2, 10, 34, 42).air(12, 17, 34, 47)
  s.air(19, 20, 34, 35).air(19, 20, 37, 39).air(21, 22, 34, 37)
  return s.plan()


def _q256():
  """Rooms of 256 (16 x 16), 77, 15 and 2 cells."""
  return ip.Sketch(20, 36).air(2, 18, 2, 18).air(2, 9, 20, 31).air(11, 14, 20, 25).air(16, 17, 20, 22).plan()


def _q257():
  """A 16 x 16 room with one notch cell on its right side (257 cells), and a room of 24."""
  return ip.Sketch(20, 28).air(2, 18, 2, 18).air(10, 11, 18, 19).air(2, 6, 21, 27).plan()


def _one(rows: int, cols: int):
  return ip.Sketch(rows + 4, cols + 4).air(2, 2 + rows, 2, 2 + cols).plan()


def _shapes():
  """An L-shaped room (120 cells); a room of a 6 x 16 block, a one-cell-wide corridor down from it and along a bend
  (116 cells) whose zone also owns a one-cell and a two-cell closet at the other end of the plan; a plain room."""
  s = ip.Sketch(30, 40)
  s.air(2, 14, 2, 8).air(10, 14, 8, 20)                        # the L
  s.air(2, 8, 22, 38).air(8, 20, 27, 28).air(19, 20, 28, 36)   # block, corridor, bend
  s.air(24, 25, 4, 5).air(24, 25, 8, 10)                       # the closets
  s.air(17, 28, 12, 24)
  fp = s.plan()
  zl, d = fp.zone_label.copy(), fp.diffusers.copy()
  at = lambda r, c: zl[1 + r, 1 + c]
  room = at(3, 30)
  for closet in (at(24, 4), at(24, 8)):
    assert closet >= 0 and closet != room
    zl[zl == closet] = room
  total = d[zl == room].sum()
  if total > 0:
    d[zl == room] /= total
  return ip.relabel(fp, zl, d)


PLANS = {"sizes": _sizes, "q256": _q256, "q257": _q257, "one2047": lambda: _one(23, 89), "one2048": lambda: _one(32, 64),
         "shapes": _shapes, "quirks": ip.zone_quirks}


@functools.lru_cache(maxsize=None)
def _plan(spec):
  if isinstance(spec, str) and spec in PLANS:
    return PLANS[spec]()
  return hc.floor_plan(hc.Case("", spec, "rows", 1, 0, 1, 0, 1, 1))


def floor_plan(case: Case):
  """The case's plan in the caller's orientation."""
  return _plan(case.plan)


def zones(fp) -> List[np.ndarray]:
  return [np.asarray(c, dtype=np.int64) for c in fp.zone_cell_lists()]


# ---------------------------------------------------------------- what a case must reach
def natural_q(fp) -> int:
  """sb_launch_convection: cells per lane for workgroups of about 256 lanes."""
  return max(1, (max(len(c) for c in zones(fp)) + 255) // 256)


def threads(fp, q: int) -> int:
  """The workgroup of k_convect<q>: ceil(largest room / q) lanes, rounded up to a wavefront (512 at the most)."""
  return ((max(len(c) for c in zones(fp)) + q - 1) // q + 63) // 64 * 64


def branch(n: int, p: float, distance: int) -> str:
  """The partner branch a room of n cells takes."""
  if distance == -1 and p == 1.0:
    return ALL
  d = 1000 if distance == -1 else distance
  if d <= 19:
    return TABLE
  R = int(np.floor(np.sqrt(d)))
  return RANK if n < (2 * R + 1) ** 2 else BOX


def branches(fp, p: float, distance: int) -> Tuple[str, ...]:
  """(k_convect_all skips rooms of one cell; every other branch runs for every room.)"""
  return tuple(sorted({branch(len(c), p, distance) for c in zones(fp)}))


def partner_counts(fp, distance: int) -> List[np.ndarray]:
  """Length of every cell's partner list under the offset table, zone by zone."""
  H, W = fp.shape
  o = ConvectionOracle(zones(fp), H, W, 1.0, distance, seed=0)
  out = []
  for z, cells in enumerate(o.zones):
    n = np.zeros(len(cells), dtype=np.int64)
    for i, g in enumerate(cells):
      x, y = divmod(int(g), W)
      for dx, dy in o.off:
        xx, yy = x + dx, y + dy
        n[i] += 0 <= xx < H and 0 <= yy < W and o.room[xx * W + yy] == z
    out.append(n)
  return out


def chase(n: int, seq) -> Tuple[int, int, bool]:
  """Of a room's swap sequence: (the most swaps that chose one cell, the most successive swaps that moved one value,
  whether a cell that starts no swap is chosen by one) -- a list link followed, a chase of several hops, a head[]
  entry without a record of its own."""
  chosen = np.zeros(n, dtype=np.int64)
  starts = np.zeros(n, dtype=bool)
  hops = np.zeros(n, dtype=np.int64)      # by value (= the cell it started in)
  at = np.arange(n)                       # the value in every cell
  for i, o in seq:
    chosen[o] += 1
    starts[i] = True
    hops[at[i]] += 1
    hops[at[o]] += 1
    at[i], at[o] = at[o], at[i]
  return int(chosen.max(initial=0)), int(hops.max(initial=0)), bool(((chosen > 0) & ~starts).any())


# ---------------------------------------------------------------- inputs and the restatement's answer
def input_grids(fp, B: int) -> np.ndarray:
  """[B, H, W]: cell g of building b holds float(b * N + g); exterior space holds AMBIENT."""
  H, W = fp.shape
  g = np.arange(B * H * W, dtype=np.float64).reshape(B, H, W)
  g[:, np.asarray(fp.exterior_space, dtype=bool)] = AMBIENT
  return g


def oracle(case: Case, first_building: Optional[int] = None) -> ConvectionOracle:
  fp = floor_plan(case)
  return ConvectionOracle(zones(fp), fp.shape[0], fp.shape[1], case.p, case.distance, seed=case.seed,
                          first_building=case.first_building if first_building is None else first_building)


@functools.lru_cache(maxsize=None)
def _expected(name: str) -> Tuple[np.ndarray, ...]:
  case = _cases()[name]
  o = oracle(case)
  g = input_grids(floor_plan(case), case.B)
  out = []
  for _ in range(case.calls):
    o.apply(g)
    out.append(g.copy())
    out[-1].setflags(write=False)
  return tuple(out)


def expected(case: Case) -> Tuple[np.ndarray, ...]:
  """The grids after every call, [calls] x [B, H, W] (computed once per case, read-only)."""
  return _expected(case.name)


def case_env(case: Case) -> Dict[str, str]:
  """The case's switches; SBSIM_DEBUG_CUS and SBSIM_DEBUG_CONV_Q are set or absent, never inherited."""
  env = dict(case.env)
  if case.pin is not None and case.pin[1] == 0:
    env["SBSIM_FORCE_LDS_PATH"] = "1"
  if case.cus is not None:
    env[SWITCH] = str(case.cus)
  if case.force_q:
    env[Q_SWITCH] = str(case.q)
  return env


def plan_info(case: Case) -> dict:
  """sb_plan_info (host only) of a layout case."""
  kernel, path, waves = case.pin
  return hc.plan_info(hc.Case(case.name, case.plan, case.orientation, path, kernel, waves, 0, case.B, 10, env=case.env),
                      case.B)


# ---------------------------------------------------------------- the table
SETTINGS = (("d5", 1.0, 5), ("d20", 0.7, 20), ("d1000", 0.5, -1), ("all", 1.0, -1))

# e. layouts: (plan, orientation, env, (kernel, path, waves))
LAYOUTS = (
    ("reg", TINY, "rows", (), (hc.REG, 1, 1)),
    ("pair", ((2, 5), (30, 12)), "columns", hc.PAIR_ENV, (hc.REG_PAIR, 1, 2)),
    ("roll", "R9", "rows", (), (hc.ROLL, 1, 1)),
    ("two", hc.SB2, "rows", (), (hc.TWO, 1, 1)),
    # (SB1-synth's 14 x 9 rooms of 8 x 7 are 129 rows: two wavefronts of k_sweep_band, and only with the two-row kernel
    # switched off; three wavefronts take 131 .. 194 rows: the 9 x 4 rooms of 16 x 17 of tests/test_convection.py)
    ("band2", hc.SB1, "rows", (("SBSIM_NO_TWO_ROW_PATH", "1"),), (hc.BAND, 1, 2)),
    ("band3", ((9, 4), (16, 17)), "rows", (), (hc.BAND, 1, 3)),
    ("band4", "260x80", "rows", (), (hc.BAND, 1, 4)),
    ("lds-rows", "R9", "rows", (), (hc.LDS, 0, 1)),
    ("lds-columns", "R9", "columns", (), (hc.LDS, 0, 1)),
)


@functools.lru_cache(maxsize=None)
def _cases() -> Dict[str, Case]:
  """The table.  A case's branches and its q come from its plan, and preprocessing a plan loads the library: the table is
  built when it is first asked for (`CASES`, below), not when this module is imported."""
  cases: Dict[str, Case] = {}

  def _add(name: str, group: str, plan, p: float, distance: int, hits: str, **kw) -> None:
    assert name not in cases
    fp = _plan(plan)
    br = branches(fp, p, distance)
    if "q" not in kw:
      kw["q"] = None if br == (ALL,) else natural_q(fp)
    cases[name] = Case(name, group, plan, p, distance, br, hits, **kw)

  # a. hand-over: every workgroup DEPTH buildings deep, the last round partly empty
  _add("handover-d5", "handover", TINY, 1.0, 5, "early draw, val/oth hand-over, head[] re-arm: every cell starts a swap",
       B=B_HANDOVER, cus=1, seed=11)
  _add("handover-d5-p0.5", "handover", TINY, 0.5, 5, "the same with cells that start no swap (word 0)", B=B_HANDOVER, cus=1, seed=12)
  _add("handover-d20", "handover", TINY, 0.7, 20, "the wide draw issued early for the next building", B=B_HANDOVER, cus=1, seed=13)
  _add("handover-all", "handover", TINY, 1.0, -1, "k_convect_all's b += gridDim.x loop", B=B_HANDOVER, cus=1, seed=14)

  # c. every Q
  for _q in range(1, 9):
    _add(f"q{_q}-forced", "q", "q256", 0.75, 5, f"k_convect<{_q}> on rooms of 256, 77, 15 and 2 cells", q=_q, force_q=True,
         seed=20 + _q)
  _add("q1-256cells", "q", "q256", 1.0, 5, "256 cells: the last size of k_convect<1>, four full wavefronts", seed=31)
  _add("q2-257cells", "q", "q257", 1.0, 5, "257 cells: the first size of k_convect<2>, 192 lanes", seed=32)
  _add("q3-600cells", "q", "sizes", 1.0, 5, "600 cells on k_convect<3>, the other zones far smaller", seed=33)
  _add("q4-600cells", "q", "sizes", 0.75, 20, "600 cells on 192 lanes (k_convect<4>): the last q partly filled", q=4, force_q=True,
       seed=34)
  _add("q8-2047cells", "q", "one2047", 1.0, 5, "2047 cells: the 11-bit rank, other | next << 16 and the partner table at their limits",
       B=2, seed=35)
  _add("q8-2047cells-rank", "q", "one2047", 0.5, -1, "2047 cells drawn by rank (by_rank[] and list indices up to 2046)", B=2, seed=36)
  _add("all-2047cells", "q", "one2047", 1.0, -1, "k_convect_all with all eight cells per lane in use", B=2, seed=37)

  # d. room shapes
  for _plan_name, _what in (("sizes", "rooms of 600, 64, 65, 1, 2 and 3 cells"),
                            ("shapes", "an L, a corridor, closets of the corridor's zone"),
                            ("quirks", "a zone of two rooms, a one-cell zone, an unzoned corridor")):
    for _tag, _p, _d in SETTINGS:
      _add(f"{_plan_name}-{_tag}", "shapes", _plan_name, _p, _d, _what, seed=40 + len(cases))

  # e. layouts
  for _name, _spec, _orient, _env, _pin in LAYOUTS:
    _add(f"{_name}-d5", "layout", _spec, 1.0, 5, f"ConvCell.sidx of {_name}", B=2, orientation=_orient, env=_env, pin=_pin,
         seed=70 + len(cases))
    _add(f"{_name}-d20", "layout", _spec, 0.7, 20, f"the wide window on {_name}", B=2, orientation=_orient, env=_env, pin=_pin,
         seed=70 + len(cases))
  _add("pair-d1000", "layout", ((2, 5), (30, 12)), 0.5, -1, "the by-rank branch with the handle transposed (W0 = H)", B=2,
       orientation="columns", env=hc.PAIR_ENV, pin=(hc.REG_PAIR, 1, 2), seed=90)
  _add("lds-columns-all", "layout", "R9", 1.0, -1, "k_convect_all with the handle transposed", B=2, orientation="columns",
       pin=(hc.LDS, 0, 1), seed=91)

  # f. call number and first_building
  _add("calls3-d5", "calls", TINY, 0.5, 5, "calls 0, 1, 2 of the table path", calls=3, seed=101)
  _add("calls3-d20", "calls", TINY, 0.7, 20, "calls 0, 1, 2 of a wide window", calls=3, seed=102)
  _add("calls3-all", "calls", TINY, 1.0, -1, "calls 0, 1, 2 of the whole-room shuffle", calls=3, seed=103)
  _add("first-max-d5", "calls", TINY, 1.0, 5, "first_building + B = 2^32 exactly", B=5, first_building=2 ** 32 - 5, seed=104)
  _add("first-max-all", "calls", TINY, 1.0, -1, "first_building + B = 2^32 exactly (Philox counter)", B=5,
       first_building=2 ** 32 - 5, seed=105)
  return cases


def __getattr__(name):
  if name == "CASES":
    return _cases()
  raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# refusals (tests/test_convection_cases_gpu.py): a 2048-cell room at attach; a forced Q too small for the largest room at launch
REFUSED_ROOM = "one2048"
TOO_SMALL_Q = ("sizes", 1)      # 600 cells on one cell per lane: 640 lanes

# re-attach: (p, distance, seed) one after the other on one simulator of the tiny plan
REATTACH = ((1.0, 5, 7), (0.5, -1, 8), (1.0, -1, 9), (0.6, 3, 10))
