"""Irregular, mixed-material floor plans for the sweep kernels (test utility, no GPU).

Every plan the other parity tests use is `rectangular_floor_plan`: equal rooms, one material per wall kind, a one-CV
exterior ring.  Much of the planner (planner.cpp: plan_two's two-coefficient check, the tail rows' coefficient sets,
the zone-free tail rows of plan_band / k_sweep_roll, the class-table strides) only does something once a plan stops
being that.  The builders here draw file-format plans (exterior space / wall / interior) with notches, courtyards,
passages and wall stubs, pass them through `FloorPlan.from_file_input` (wall kinds and diffusers follow the
reference's rules), then give rooms and wall segments materials of their own and, where a case needs it, edit zones
and diffusers directly.  Diffusers always sum to 1 in every zone that has any.

Each `Case` pins what the planner does with the plan in the orientation it runs in (`sb_plan_info`): the sweep
kernel, wavefronts per building, the steps of one sweep, and the counts the plan is built to hit (cell classes,
distinct (bU, bD, bL, bR) sets, zones).  tests/test_irregular_plans_cpu.py checks the pins and runs the NumPy schedule
models on the plans; tests/test_irregular_plans_gpu.py runs every case against the CPU oracle.  All builders are
deterministic."""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Optional, Tuple

import numpy as np

from sbsim_amd.floorplan import EXTERIOR_SPACE, INTERIOR_SPACE, WALL, FloorPlan, Material, Materials

# sb_sweep_kernel (include/sbsim_amd.h)
LDS, REG, REG_PAIR, ROLL, TWO, BAND, STREAM = 0, 1, 2, 3, 4, 5, 6

DT, H_CONV = 300.0, 12.0    # what FloorPlan.compile gets for the class counts (the counts do not depend on them)


# ---------------------------------------------------------------- drawing
class Sketch:
  """A file-format plan of `rows` x `cols` cells inside a one-CV ring of exterior space, all wall to begin with.
  Coordinates are those inside the ring: (0, 0) is the first cell the sweep owns when nothing is trimmed."""

  def __init__(self, rows: int, cols: int):
    self.g = np.full((rows + 2, cols + 2), WALL, dtype=np.int8)
    self.g[0, :] = self.g[-1, :] = EXTERIOR_SPACE
    self.g[:, 0] = self.g[:, -1] = EXTERIOR_SPACE

  def air(self, r0: int, r1: int, c0: int, c1: int) -> "Sketch":
    self.g[1 + r0:1 + r1, 1 + c0:1 + c1] = INTERIOR_SPACE
    return self

  def out(self, r0: int, r1: int, c0: int, c1: int) -> "Sketch":
    self.g[1 + r0:1 + r1, 1 + c0:1 + c1] = EXTERIOR_SPACE
    return self

  def wall(self, r0: int, r1: int, c0: int, c1: int) -> "Sketch":
    self.g[1 + r0:1 + r1, 1 + c0:1 + c1] = WALL
    return self

  def rooms(self, r_edges, c_edges) -> "Sketch":
    """Rooms between consecutive edges (one-CV walls between them): r_edges = (a, b, c) gives rows a..b-2, b..c-1."""
    for i in range(len(r_edges) - 1):
      for j in range(len(c_edges) - 1):
        self.air(r_edges[i], r_edges[i + 1] - 1, c_edges[j], c_edges[j + 1] - 1)
    return self

  def plan(self, diffuser_spacing: int = 10) -> FloorPlan:
    return FloorPlan.from_file_input(self.g, Materials.sb1(), 10.0, 300.0, diffuser_spacing=diffuser_spacing)


def inner(fp: FloorPlan, r0: int, r1: int, c0: int, c1: int):
  """The index expression of a box given in inside-the-ring coordinates."""
  return slice(1 + r0, 1 + r1), slice(1 + c0, 1 + c1)


# ---------------------------------------------------------------- materials, zones, diffusers
def with_materials(fp: FloorPlan, mask: np.ndarray, m: Material) -> FloorPlan:
  """`fp` with material `m` on the cells of `mask`."""
  k, c, rho = fp.conductivity.copy(), fp.heat_capacity.copy(), fp.density.copy()
  k[mask], c[mask], rho[mask] = m.conductivity, m.heat_capacity, m.density
  return dataclasses.replace(fp, conductivity=k, heat_capacity=c, density=rho)


def air_material(i: int) -> Material:
  """The i-th air-like material (i = 0: SB1's air): thermal diffusivities that differ by a few per cent."""
  return Material(50.0 * (1.0 + 0.03 * i), 700.0 * (1.0 + 0.011 * i), 1.0 + 0.007 * i)


def wall_material(i: int) -> Material:
  """The i-th interior-wall-like material (i = 0: SB1's interior wall)."""
  return Material(50.0 * (1.0 - 0.02 * i), 1.0 + 0.05 * i, 700.0 * (1.0 + 0.013 * i))


def per_room_materials(fp: FloorPlan, n: int, first: int = 1) -> FloorPlan:
  """Rooms 0 .. n-1 get air materials first .. first + n - 1 (each a coefficient set and a class of its own)."""
  for z in range(n):
    fp = with_materials(fp, fp.zone_label == z, air_material(first + z))
  return fp


def split_diffusers(fp: FloorPlan, extra: int) -> FloorPlan:
  """Adds exactly `extra` cell classes without a new coefficient set: zones' diffuser weights are made unequal (a
  zone with n diffusers of equal weight is one class; n distinct weights, still summing to 1, are n classes)."""
  d = fp.diffusers.copy()
  for z in range(fp.n_zones):
    if extra <= 0:
      break
    cells = np.flatnonzero((fp.zone_label.reshape(-1) == z) & (d.reshape(-1) > 0))
    if len(cells) < 2:
      continue
    n = min(len(cells), extra + 1)
    w = 1.0 + 0.125 * np.arange(n)                 # n distinct weights on the first n diffusers ...
    rest = len(cells) - n
    w = np.concatenate([w, np.full(rest, w[0])])   # ... the others share the first one's
    d.reshape(-1)[cells] = w / w.sum()
    extra -= n - 1
  assert extra == 0, "not enough diffusers to split"
  return dataclasses.replace(fp, diffusers=d)


def relabel(fp: FloorPlan, zone_label: np.ndarray, diffusers: np.ndarray) -> FloorPlan:
  """`fp` with zones renumbered in raster order of their first cell (what from_file_input gives)."""
  zl = np.full(zone_label.shape, -1, dtype=np.int16)
  order = []
  for z in zone_label.reshape(-1):
    if z >= 0 and z not in order:
      order.append(int(z))
  for new, old in enumerate(order):
    zl[zone_label == old] = new
  return dataclasses.replace(fp, zone_label=zl, diffusers=np.where(zl >= 0, diffusers, 0.0),
                             zone_names=tuple(f"room_{i + 1}" for i in range(len(order))))


# ---------------------------------------------------------------- the plans
def l_shape() -> FloorPlan:
  """60 x 70 inside the ring, a 22 x 28 notch of exterior space at the top-right corner: ambient cells inside the trim
  box, edge and corner cells along the notch.  Six rooms, two of them of other air materials, one wall segment of
  another material."""
  s = Sketch(60, 70).out(0, 22, 42, 70)
  s.rooms((2, 21, 40, 58), (2, 20, 40))         # the left wing: three rows of two rooms
  s.rooms((24, 58), (42, 55, 68))               # the bottom-right wing: two rooms below the notch
  fp = s.plan()
  fp = per_room_materials(fp, 2, first=1)
  fp = with_materials(fp, _box(fp, 20, 21, 2, 40), wall_material(1))
  return fp


def _box(fp: FloorPlan, r0, r1, c0, c1) -> np.ndarray:
  m = np.zeros(fp.shape, bool)
  m[inner(fp, r0, r1, c0, c1)] = True
  return m


def roll_tail(rows: int) -> FloorPlan:
  """`rows` (65 / 66) x 70: rooms in rows 2..61, the bottom exterior wall (rows 62..rows-1) is where the trouble is: a
  notch of exterior space into the last row, a wall stub of another material and a pocket of unzoned air in the tail
  rows (rows 64.. lie beyond k_sweep_roll's wavefront).  No zone cell reaches a tail row."""
  s = Sketch(rows, 70)
  s.rooms((2, 32, 62), (2, 25, 47, 68))
  s.out(rows - 1, rows, 10, 17).out(rows - 1, rows, 40, 42).out(rows - 1, rows, 60, 63)   # gaps in the last row
  fp = s.plan()
  fp = per_room_materials(fp, 3, first=2)
  fp = with_materials(fp, _box(fp, 63, rows - 1, 25, 31), wall_material(2))   # the stub
  fp = with_materials(fp, _box(fp, 64, 65, 45, 52), air_material(0))          # air, no zone
  return fp


def roll_tail_many(rows: int, sets: bool) -> FloorPlan:
  """roll_tail with a material per room and wall segment: past 32 coefficient sets (`sets`), or past 31 classes with
  few sets (split diffuser weights)."""
  fp = roll_tail(rows)
  if sets:
    fp = per_room_materials(fp, 6, first=10)
    for i in range(28):
      fp = with_materials(fp, _box(fp, 31, 32, 2 + 2 * i, 4 + 2 * i), wall_material(3 + i))
    return fp
  return split_diffusers(fp, 31 - _classes(fp) + 1)


def u_shape() -> FloorPlan:
  """110 x 70, a U: a courtyard of exterior space open at the top (rows 0..69, columns 24..46), so edge cells with a
  one-sided neighbour sit inside the trim box.  The last row is mixed: a notch and a wall segment of another
  material.  Twelve rooms."""
  s = Sketch(110, 70).out(0, 70, 24, 46)
  s.rooms((2, 24, 46, 72, 90, 108), (2, 22))
  s.rooms((2, 24, 46, 72), (48, 68))
  s.rooms((72, 90, 108), (24, 46, 68))
  s.out(109, 110, 30, 36)
  fp = s.plan()
  fp = per_room_materials(fp, 4, first=1)
  fp = with_materials(fp, _box(fp, 108, 110, 50, 60), wall_material(1))
  return fp


def two_wings() -> FloorPlan:
  """100 x 66: two wings joined by nothing but the trim box: a passage of exterior space runs the full height
  (columns 30..34).  Every cell has bU == bD, but the passage's edge cells have bL != bR inside the box: plan_two's
  two-coefficient check fails on h_ok alone."""
  s = Sketch(100, 66).out(0, 100, 30, 34)
  s.rooms((2, 30, 60, 98), (2, 28))
  s.rooms((2, 50, 98), (36, 64))
  fp = s.plan()
  return per_room_materials(fp, 2, first=3)


def sym_tail_notch() -> FloorPlan:
  """129 x 75 (SB1-synth's size), rectangular rooms of a few materials, and a notch of exterior space in the last row
  only: the row above it (row 127) and the notch's neighbours are edge cells in k_sweep_two's tail rows (127, 128),
  looked up in its tail-set table."""
  s = Sketch(129, 75)
  s.rooms(tuple(range(2, 128, 18)) + (127,), (2, 26, 50, 73))
  s.out(128, 129, 20, 28).out(128, 129, 50, 51)
  fp = s.plan()
  fp = per_room_materials(fp, 3, first=5)
  return with_materials(fp, _box(fp, 127, 129, 60, 70), wall_material(4))


def zone_in_tail() -> FloorPlan:
  """130 x 70: the bottom-right room reaches the exterior ring (a glass front: its last rows are exterior wall but
  still the room's cells), so a zone cell sits in row 129.  plan_two refuses; plan_band takes a third wavefront."""
  s = Sketch(130, 70)
  s.rooms((2, 45, 88, 128), (2, 35, 68))
  s.air(88, 130, 36, 68)
  return per_room_materials(s.plan(), 2, first=2)


def courtyard(rows: int) -> FloorPlan:
  """`rows` (150..258) x 80: a courtyard of exterior space in the middle (rows 50..rows-50, columns 28..52), rooms
  whose zones cross the 64-row seams (the wings' rooms span rows 40..90, 90..140, 140..190, ...), mixed materials."""
  return per_room_materials(_courtyard_sketch(rows).plan(), 5, first=1)


def _courtyard_sketch(rows: int) -> Sketch:
  s = Sketch(rows, 80).out(50, rows - 50, 28, 52)
  edges = [2, 40, 90, 140, 190, 240, rows - 2]
  edges = sorted(set(e for e in edges if e <= rows - 2))
  if edges[-1] - edges[-2] < 6:
    edges.pop(-2)
  s.rooms(tuple(edges), (2, 26))
  s.rooms(tuple(edges), (54, 78))
  s.rooms((2, 48), (28, 52))
  s.rooms((rows - 48, rows - 2), (28, 52))
  return s


def zone_quirks() -> FloorPlan:
  """60 x 72, zones the room grid never produces: one zone of two rooms (one diffuser set, weights summing to 1), a
  one-CV zone (a closet), a zone without a diffuser, an unzoned corridor across the plan."""
  s = Sketch(60, 72)
  s.rooms((2, 26), (2, 20, 38, 56, 70))
  s.air(27, 31, 2, 70)                       # the corridor
  s.rooms((32, 58), (2, 30, 58, 70))
  s.wall(42, 47, 62, 67).air(44, 45, 64, 65)   # a one-CV room at (44, 64), walled in inside the last room
  fp = s.plan()
  zl, d = fp.zone_label.copy(), fp.diffusers.copy()
  corridor = _box(fp, 27, 31, 2, 70)
  d[corridor] = 0.0
  zl[corridor] = -1
  a, b = zl[inner(fp, 10, 11, 10, 11)][0, 0], zl[inner(fp, 40, 41, 40, 41)][0, 0]   # merge two distant rooms
  d[zl == a] *= 0.25
  d[zl == b] *= 0.75
  zl[zl == b] = a
  c = zl[inner(fp, 10, 11, 25, 26)][0, 0]    # a room without a diffuser
  d[zl == c] = 0.0
  fp = relabel(fp, zl, d)
  return per_room_materials(fp, 3, first=1)


def with_classes(fp: FloorPlan, n: int) -> FloorPlan:
  """`fp` with exactly n cell classes and no new coefficient set (split diffuser weights)."""
  return split_diffusers(fp, n - _classes(fp))


def _classes(fp: FloorPlan) -> int:
  return fp.compile(DT, H_CONV).n_classes


def u_ladder(n: int) -> FloorPlan:
  """The U-shape's footprint, SB1 materials, diffusers every 3 CVs, set to exactly n cell classes."""
  s = Sketch(110, 70).out(0, 70, 24, 46)
  s.rooms((2, 24, 46, 72, 90, 108), (2, 22))
  s.rooms((2, 24, 46, 72), (48, 68))
  s.rooms((72, 90, 108), (24, 46, 68))
  s.out(109, 110, 30, 36)
  return with_classes(s.plan(diffuser_spacing=3), n)


def courtyard_ladder(n: int) -> FloorPlan:
  """The 190-row courtyard's footprint, SB1 materials, diffusers every 3 CVs, set to exactly n cell classes."""
  return with_classes(_courtyard_sketch(190).plan(diffuser_spacing=3), n)


def roll_ladder(n: int) -> FloorPlan:
  """roll_tail(66) set to exactly n cell classes."""
  return with_classes(roll_tail(66), n)


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  build: Callable[[], FloorPlan]
  orientation: str                 # "rows" / "columns": the orientation the library runs it in
  kernel: int                      # sb_sweep_kernel the planner picks
  waves: int                       # waves_per_building
  steps: Optional[int] = None      # sweep_steps, where fixed
  env: Tuple[Tuple[str, str], ...] = ()
  n_classes: Optional[int] = None  # the counts the case is built to hit
  n_sets: Optional[int] = None
  n_zones: Optional[int] = None
  zone_in_last_row: bool = False
  tail_rows: int = 0               # rows past the wavefronts a scan finishes (k_sweep_roll / k_sweep_two / k_sweep_band)


def _plan_for(case: Case) -> FloorPlan:
  fp = case.build()
  return fp.transposed() if case.orientation == "columns" else fp


CASES: Dict[str, Case] = {}


def _add(*cases: Case) -> None:
  for c in cases:
    assert c.name not in CASES
    CASES[c.name] = c


def plan(name: str) -> FloorPlan:
  """The case's plan in the file's orientation (BatchedSimulator transposes it when the case says "columns")."""
  return CASES[name].build()


def device_plan(name: str) -> FloorPlan:
  """The case's plan as the sweep sees it (transposed for "columns")."""
  return _plan_for(CASES[name])


_add(
    # k_sweep_roll: one wavefront, ambient cells inside the trim box; then one / two mixed tail rows
    Case("L", l_shape, "rows", ROLL, 1, 72, n_classes=24, n_sets=16, n_zones=8),
    Case("roll65", lambda: roll_tail(65), "rows", ROLL, 1, 72 + 4, n_classes=24, n_sets=18, n_zones=6, tail_rows=1),
    Case("roll66", lambda: roll_tail(66), "rows", ROLL, 1, 72 + 8, n_classes=23, n_sets=17, n_zones=6, tail_rows=2),
    Case("roll66-31cls", lambda: roll_ladder(31), "rows", ROLL, 1, 72 + 8, n_classes=31, n_sets=17, n_zones=6,
         tail_rows=2),
    # ... past k_sweep_roll's 31 classes / 32 sets: no register kernel takes 66 rows any more -> the LDS-grid kernel
    Case("roll66-32cls", lambda: roll_ladder(32), "rows", LDS, 1, n_classes=32, n_sets=17, n_zones=6),
    Case("roll66-48sets", lambda: roll_tail_many(66, True), "rows", LDS, 1, n_classes=54, n_sets=48, n_zones=6),
    # k_sweep_two's four-coefficient variant by the library's own choice (v_ok and h_ok fail / h_ok alone fails)
    Case("U", u_shape, "rows", TWO, 1, 76 + 55 - 1, n_classes=35, n_sets=23, n_zones=12),
    Case("wings", two_wings, "rows", TWO, 1, 76 + 50 - 1, n_classes=18, n_sets=13, n_zones=5),
    # ... its two-coefficient variant with mixed tail rows (rows 127, 128 through the tail-set table)
    Case("sym-tail", sym_tail_notch, "rows", TWO, 1, 76 + 64 - 1 + 8, n_classes=40, n_sets=19, n_zones=21,
         tail_rows=2),
    # k_sweep_band
    Case("U-band", u_shape, "rows", BAND, 2, 72, env=(("SBSIM_BAND_PATH", "1"),), n_classes=35, n_sets=23,
         n_zones=12),
    Case("zone-tail", zone_in_tail, "rows", BAND, 3, 72, n_classes=19, n_sets=13, n_zones=6, zone_in_last_row=True),
    Case("court190", lambda: courtyard(190), "rows", BAND, 3, 80, n_classes=34, n_sets=24, n_zones=10),
    Case("court250", lambda: courtyard(250), "rows", BAND, 4, 80, n_classes=38, n_sets=24, n_zones=14),
    # transposed tables: the L drawn in the file, run lanes = its columns (70 rows x 60): k_sweep_two, general
    Case("L-columns", l_shape, "columns", TWO, 1, 64 + 35 - 1, n_classes=24, n_sets=16, n_zones=8),
    # forced kernels
    Case("L-lds", l_shape, "rows", LDS, 1, env=(("SBSIM_FORCE_LDS_PATH", "1"),), n_classes=24, n_sets=16, n_zones=8),
    Case("U-lds", u_shape, "rows", LDS, 1, env=(("SBSIM_FORCE_LDS_PATH", "1"),), n_classes=35, n_sets=23,
         n_zones=12),
    Case("L-stream", l_shape, "rows", STREAM, 1, env=(("SBSIM_FORCE_STREAM_PATH", "1"),), n_classes=24, n_sets=16,
         n_zones=8),
    Case("court190-stream", lambda: courtyard(190), "rows", STREAM, 3, env=(("SBSIM_FORCE_STREAM_PATH", "1"),),
         n_classes=34, n_sets=24, n_zones=10),
    # zone quirks: a two-room zone, a one-CV zone, a zone without a diffuser, an unzoned corridor
    Case("quirks", zone_quirks, "rows", ROLL, 1, 72, n_classes=21, n_sets=14, n_zones=7),
)
# class counts at both sides of every class-table stride (32 / 64 / 128 / 256), sets unchanged
for _n in (31, 32, 63, 64, 127, 128, 220):
  _add(Case(f"U-{_n}cls", lambda n=_n: u_ladder(n), "rows", TWO, 1, 76 + 55 - 1, n_classes=_n, n_sets=17, n_zones=12),
       Case(f"court190-{_n}cls", lambda n=_n: courtyard_ladder(n), "rows", BAND, 3, 80, n_classes=_n, n_sets=19,
            n_zones=10))
