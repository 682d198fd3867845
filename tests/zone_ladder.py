"""Floor plans that walk every kernel's zone reduce and per-zone passes over their edges (test utility, no GPU).

tests/irregular_plans.py is the ladder of the class tables; this is its twin for the zones.  Every other parity test
runs zones that are whole rooms (compact rectangles of 56..900 cells) at a few zone counts, while each kernel that
touches zones has a grouping, a scratch layout and a capacity check of its own: 16 zones per pass in k_pre and in the
register kernels' reduce, 8 per group in k_post, 4 per observation store, 64 per pass in k_sweep_two / k_sweep_band /
k_sweep_lds, a zone per wavefront in the Jacobi kernels, 512-cell index blocks in k_sweep_lds.  Zones here are labels on
the cells of ONE room inside a one-CV wall ring, so the zone count and the zones' shapes are free:

  "bands"    row stripes: a zone touches few lanes (few slots of the compact scratch of k_sweep_two / k_sweep_band)
  "columns"  column stripes: every lane touches every zone
  "cells"    cell (r, c) of the room belongs to zone (stride * r + c) mod Z: the most slots
  "sized"    an explicit list of zone sizes laid down in raster order (k_sweep_lds' 512-cell blocks); the cells that
             are left over stay unzoned air

Diffusers always sum to 1 in a zone that has any; a zone without one is legal.  Each `Case` pins what the planner does
with the plan (sb_plan_info): kernel, wavefronts per building, the steps of one sweep, the zone count.
tests/test_zone_ladder_cpu.py checks the pins and the conditions on the inputs, tests/test_zone_ladder_gpu.py runs
every case against the CPU oracle.  All builders are deterministic."""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from sbsim_amd.floorplan import FloorPlan
from tests.irregular_plans import BAND, LDS, REG, ROLL, STREAM, TWO, Case, Sketch, relabel

LAYOUTS = ("bands", "columns", "cells", "sized")
B, T = 5, 6               # buildings and steps of the GPU test
SEED = 41
PHASE, BUILDING_SHIFT = 0.70, 0.0125   # of the zones' offsets: building 0's, and from one building to the next


# ---------------------------------------------------------------- the builder
def zoned(rows: int, cols: int, Z: int, layout: str, n_diffusers: int, *, stride: int = 3,
          sizes: Optional[Sequence[int]] = None, doubles: int = 0) -> FloorPlan:
  """One room of (rows - 2) x (cols - 2) air cells inside a one-CV wall ring, its cells labelled with Z zones in
  `layout`.  `n_diffusers` zones, spread evenly over the zone numbers, get a diffuser in their middle cell; the first
  `doubles` of them get two of unequal weight (5/8 and 3/8) instead: a cell class each."""
  assert layout in LAYOUTS
  fp = Sketch(rows, cols).air(1, rows - 1, 1, cols - 1).plan()
  R, C = rows - 2, cols - 2
  r, c = np.mgrid[0:R, 0:C]
  if layout == "bands":
    assert Z <= R
    z = r * Z // R
  elif layout == "columns":
    assert Z <= C
    z = c * Z // C
  elif layout == "cells":
    assert Z <= R * C
    z = (stride * r + c) % Z
  else:
    assert sizes is not None and len(sizes) == Z and sum(sizes) <= R * C and min(sizes) >= 1
    z = np.repeat(np.arange(Z + 1), list(sizes) + [R * C - sum(sizes)]).reshape(R, C)
    z = np.where(z == Z, -1, z)
  zl = np.full(fp.shape, -1, dtype=np.int64)
  zl[2:2 + R, 2:2 + C] = z
  assert ((zl >= 0) <= (fp.zone_label >= 0)).all()      # zone cells are the room's air cells
  assert n_diffusers <= Z and doubles <= n_diffusers
  d = np.zeros(fp.shape)
  flat = zl.reshape(-1)
  for i, zone in enumerate(np.arange(n_diffusers) * Z // max(n_diffusers, 1)):
    cells = np.flatnonzero(flat == zone)
    if i < doubles and len(cells) >= 2:
      d.reshape(-1)[cells[len(cells) // 3]] = 0.625
      d.reshape(-1)[cells[len(cells) // 3 + max(1, len(cells) // 3)]] = 0.375
    else:
      d.reshape(-1)[cells[len(cells) // 2]] = 1.0
  return relabel(fp, zl, d)


def initial_grids(fp: FloorPlan, n_buildings: int = B, seed: int = SEED) -> np.ndarray:
  """[n_buildings, H * W]: every zone its own offset, 294 - 5 + 11 * frac(0.618 * (z + 1) + PHASE + BUILDING_SHIFT * b), plus 0.2 K of
  noise; cells outside a zone 294 K plus the noise.  The golden-ratio steps put OFF, HEAT and COOL among the zones of
  step 0 and keep two zones' means apart, so two zones swapped by a reduce change a thermostat."""
  rs = np.random.RandomState(seed)
  H, W = fp.shape
  zl = fp.zone_label.reshape(-1)
  init = np.empty((n_buildings, H * W))
  for b in range(n_buildings):
    off = 294.0 - 5.0 + 11.0 * np.modf(0.618 * (np.arange(fp.n_zones) + 1.0) + PHASE + BUILDING_SHIFT * b)[0]
    init[b] = np.where(zl >= 0, off[np.maximum(zl, 0)], 294.0) + 0.2 * rs.randn(H * W)
  return init


def actions(n_steps: int = T, n_buildings: int = B, seed: int = SEED) -> np.ndarray:
  return np.random.RandomState(seed + 1).uniform(-1, 1, size=(n_steps, n_buildings, 2)).astype(np.float32)


# ---------------------------------------------------------------- cases
CASES: Dict[str, Case] = {}
_BASE_CLASSES = 10        # the wall ring's and the plain air cells' classes of every plan here
_NO_ROLL = (("SBSIM_NO_ROLL_SMALL", "1"),)
_BAND = (("SBSIM_BAND_PATH", "1"),)
_LDS = (("SBSIM_FORCE_LDS_PATH", "1"),)
_STREAM = (("SBSIM_FORCE_STREAM_PATH", "1"),)


def _case(name: str, rows: int, cols: int, Z: int, layout: str, kernel: int, waves: int, steps: int, *,
          nd: Optional[int] = None, doubles: int = 0, env: Tuple[Tuple[str, str], ...] = (),
          orientation: str = "rows", classes: Optional[int] = None, **kw) -> None:
  """`rows` x `cols` is the plan as the file holds it; a "columns" case runs transposed (lanes = file columns)."""
  nd = min(Z, 12) if nd is None else nd
  assert name not in CASES
  CASES[name] = Case(name, lambda: zoned(rows, cols, Z, layout, nd, doubles=doubles, **kw), orientation, kernel, waves,
                     steps, env=env, n_classes=_BASE_CLASSES + nd + doubles if classes is None else classes, n_zones=Z)


def plan(name: str) -> FloorPlan:
  """The case's plan in the file's orientation (BatchedSimulator transposes it when the case says "columns")."""
  return CASES[name].build()


def device_plan(name: str) -> FloorPlan:
  """The case's plan as the sweep sees it (transposed for "columns")."""
  fp = plan(name)
  return fp.transposed() if CASES[name].orientation == "columns" else fp


# k_sweep_roll (40 x 30: one wavefront, the 64-slot instantiation).  [64][ZRS = (Z + 1) | 1] scratch, 16 zones x 4 row
# groups per pass of the reduce: one pass (Z + 1 <= 16), two passes, the largest Z; even and odd Z.  The class table
# holds 31, so at most 12 zones carry a diffuser.  Z = 32 falls off the kernel: the LDS-grid kernel takes it.
for _Z, _lay in ((1, "cells"), (15, "bands"), (16, "cells"), (17, "columns"), (30, "bands"), (31, "cells")):
  _case(f"roll-z{_Z}", 40, 30, _Z, _lay, ROLL, 1, 64)
_case("roll-z32-lds", 40, 30, 32, "cells", LDS, 1, 73)
_case("roll-z16-columns", 30, 40, 16, "columns", ROLL, 1, 64, orientation="columns")
# k_sweep_reg on the same plan: [Z + 1][ZRS] scratch aliasing A, 16 zone rows per pass of the reduce with the dump row
# Z among them (Z + 1 = 16, 17), and its capacity check (Z + 1) * ZRS <= RS * nl: 30 zones fit, 31 go to k_sweep_lds.
for _Z, _lay in ((1, "cells"), (15, "cells"), (16, "bands"), (17, "cells"), (30, "cells")):
  _case(f"reg-z{_Z}", 40, 30, _Z, _lay, REG, 1, 71, env=_NO_ROLL)
_case("reg-z31-lds", 40, 30, 31, "cells", LDS, 1, 73, env=_NO_ROLL)
_case("reg-z16-columns", 30, 40, 16, "columns", REG, 1, 71, env=_NO_ROLL, orientation="columns")
# 36 columns: k_sweep_reg by the library's own choice past k_sweep_roll's 31 zones; three 16-zone passes of k_pre
_case("reg-z33", 40, 36, 33, "cells", REG, 1, 105)
_case("lds-z33", 40, 36, 33, "cells", LDS, 1, 79, env=_LDS)

# k_sweep_two (100 x 72) and k_sweep_band on two (the same plan) and three (150 x 72) wavefronts: compact slots, a lane
# per zone, 64 zones per pass with the dump zone Z among them (Z + 1 = 64, 65, 66).  Most zones carry a diffuser, three
# of them two unequal ones.
for _lay in ("bands", "columns", "cells"):
  for _Z in (63, 64, 65):
    _case(f"two-{_lay}-z{_Z}", 100, 72, _Z, _lay, TWO, 1, 126, nd=_Z, doubles=3)
    _case(f"band2-{_lay}-z{_Z}", 100, 72, _Z, _lay, BAND, 2, 72, nd=_Z, doubles=3, env=_BAND)
    _case(f"band3-{_lay}-z{_Z}", 150, 72, _Z, _lay, BAND, 3, 72, nd=_Z, doubles=3)
# cell (r, c) -> zone (70 r + c) mod Z, the raster index: every lane touches most zones, the compact scratch outgrows A
_case("two-cells-z150", 100, 72, 150, "cells", TWO, 1, 126, nd=150, doubles=3, stride=70)
_case("band2-cells-z150", 100, 72, 150, "cells", BAND, 2, 72, nd=150, doubles=3, stride=70, env=_BAND)
# about 1,000 zones of six or seven cells each (the class table holds 255: 200 zones carry a diffuser)
_case("two-cells-z1000", 100, 72, 1000, "cells", TWO, 1, 126, nd=200, doubles=3, stride=70)
_case("band3-cells-z1000", 150, 72, 1000, "cells", BAND, 3, 72, nd=200, doubles=3, stride=70)
_case("two-z64-columns", 72, 100, 64, "bands", TWO, 1, 126, nd=64, doubles=3, orientation="columns")
_case("band2-z64-columns", 72, 100, 64, "bands", BAND, 2, 72, nd=64, doubles=3, env=_BAND, orientation="columns")
_case("band3-z65-columns", 72, 150, 65, "columns", BAND, 3, 72, nd=65, doubles=3, orientation="columns")

# k_sweep_lds (forced): `z = lane; z += 64` loops (Z = 64, 65), off_zscr / off_zmode rounded by the parity of Z (1, 2,
# 3), u16 index blocks of 512 cells walked six at a time.
for _Z in (1, 2, 3, 64, 65):
  _case(f"lds-z{_Z}", 40, 30, _Z, "cells", LDS, 1, 73, nd=_Z, doubles=min(_Z, 3) if _Z > 1 else 0, env=_LDS)
# zone sizes on both sides of a block: 1 + 1 + 1 + 2 + 2 = seven blocks (a second batch of one), 3 + 2 + 1 = six
_case("lds-sized-7blocks", 60, 50, 5, "sized", LDS, 1, 113, nd=5, doubles=4, env=_LDS, classes=_BASE_CLASSES + 5 + 3,
      sizes=(511, 1, 512, 513, 1024))   # (the one-cell zone cannot take two diffusers)
_case("lds-sized-6blocks", 60, 50, 3, "sized", LDS, 1, 113, nd=3, doubles=2, env=_LDS, sizes=(1025, 513, 1))
# 163,336 of the 163,840 bytes of LDS a workgroup may ask for
_case("lds-z1060-cap", 56, 36, 1060, "cells", LDS, 1, 95, nd=200, doubles=3, stride=34, env=_LDS)

# k_sweep_stream (forced): (Z + 1) * kZC scratch, u16 zone map
for _Z in (1, 64, 65):
  _case(f"stream-z{_Z}", 40, 30, _Z, "cells", STREAM, 1, 135, nd=_Z, doubles=min(_Z, 3) if _Z > 1 else 0, env=_STREAM)

# ---- the AHU's flow cap inside k_pre's second 16-zone pass (tests: CAP_CASES x the plan of reg-z33 / lds-z33)
CAP_CASES = ("reg-z33", "lds-z33")

# ---- solver="jacobi_fp32": a zone per wavefront, z += NW.  (kernel name, developer switch, NW, plan rows x columns)
JACOBI = {"lds": ((), 8), "global": ((("SBSIM_FORCE_JACOBI_GLOBAL", "1"),), 16)}


def jacobi_zone_counts(nw: int) -> Tuple[int, ...]:
  return (1, nw - 1, nw, nw + 1)


def jacobi_plan(Z: int) -> FloorPlan:
  return zoned(40, 30, Z, "cells", min(Z, 12))


# ---------------------------------------------------------------- step inputs and the oracle's rollout
AMBIENT = 295.0           # K at the first step, + 0.05 K per step
AHU_CAP = 0.5             # m3/s: ahu_max_air_flow_rate of the CAP_CASES (33 zones x 0.035 m3/s = 1.155 m3/s uncapped)


def step_rows() -> dict:
  """The step-input rows of h2_sb1_r9_random.npz (tests/parity.py's check_plan_against_oracle reads rows
  96 + t) with a mild ambient temperature inside the comfort window.  One room behind a one-CV wall follows the golden's
  winter morning (281 K) within a step, every zone then calls for heat and all zones look alike.  At 295 K the zones'
  own offsets and the thermostats' hysteresis keep two or three modes among the zones over the first steps."""
  from tests.golden_util import load
  g = dict(load("h2_sb1_r9_random.npz"))
  t = np.arange(len(g["t_amb_now"])) - 96
  g["t_amb_now"] = AMBIENT + 0.05 * t
  g["t_amb_next"] = AMBIENT + 0.05 * (t + 1)
  return g


_ROLLOUTS: Dict[Tuple[str, Optional[float]], list] = {}


def oracle_rollout(name: str, ahu_cap: Optional[float] = None) -> list:
  """[T][B] results of OracleBuilding.step on the case's plan, initial grids, actions and step rows (computed once)."""
  from sbsim_amd.environment import SimConfig
  from tests.twins import oracle_twin, step_kwargs
  key = (name, ahu_cap)
  if key not in _ROLLOUTS:
    cfg = SimConfig.sb1()
    if ahu_cap is not None:
      cfg = dataclasses.replace(cfg, ahu_max_air_flow_rate=ahu_cap)
    fp, g = plan(name), step_rows()
    init, acts = initial_grids(fp), actions()
    twins = [oracle_twin(fp, cfg, init[b]) for b in range(B)]
    _ROLLOUTS[key] = [[twins[b].step(**step_kwargs(g, 96 + t, t, cfg, acts[t, b])) for b in range(B)] for t in range(T)]
  return _ROLLOUTS[key]
