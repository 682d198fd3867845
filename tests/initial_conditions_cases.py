"""Start temperatures per building (host_inputs.InitialConditions): the cases the CPU and the GPU tests share (test
utility, no GPU, no torch).

The plan is tests/crossed_batches.py's 17 x 29 (493 cells, six zones, one zone over and several under 64 cells, odd row
length) with B = 67 buildings: one past a 64-building group, several buildings per wavefront of the reset launch.  Three
grids with non-uniform values in the exterior ring -- the register layout's ring extremes differ per grid -- mixed
irregularly over the buildings, an offset per building and a draw per building and episode.

`twin_rollout` runs every building's oracle twin from `start_temps(b, 0)` once (6 steps on the step-input rows of
h2_sb1_r9_random.npz, as tests/parity.py's check_plan_against_oracle feeds them); the CPU test asserts its margins, the
GPU test holds the device to it."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from sbsim_amd import host_inputs
from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
from tests import crossed_batches as cb
from tests.golden_util import load
from tests.twins import oracle_twin, step_kwargs

B = cb.B                 # 67
T_TWINS = 6
ROW0 = 96                # mid-morning rows of the golden's step inputs: occupied, comfort mode
SEED = 0x9E3779B97F4A7C15
JITTER = (-0.75, 0.5, SEED)
INITIAL_TEMP = 293.37    # the reset call's scalar where the conditions hold no base
VARIANTS = ("grids", "initial_temp", "jitter")


def plan() -> FloorPlan:
  return FloorPlan.from_file_input(rectangular_floor_plan(cb.ROOMS, cb.ROOM_SHAPE), Materials.sb1(), 10.0, 300.0)


def grids(shape) -> np.ndarray:
  """[3, H, W]: a smooth field per grid, and a ring of its own -- a ramp along the perimeter, another range per grid."""
  H, W = shape
  y, x = np.mgrid[0:H, 0:W].astype(np.float64)
  out = np.stack([292.5 + k + 1.1 * np.sin(0.37 * (k + 1) * y + 0.2 * k) * np.cos(0.23 * (k + 2) * x) + 0.03 * x - 0.02 * y
                  for k in range(3)])
  ring = np.zeros((H, W), bool)
  ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
  for k in range(3):
    out[k][ring] = 280.0 + 3.0 * k + 0.013 * (k + 1) * np.arange(int(ring.sum()))
  return out


def grid_of() -> np.ndarray:
  b = np.arange(B)
  return ((b * 7 + b // 5) % 3).astype(np.int32)


def offsets() -> np.ndarray:
  return np.random.RandomState(5).permutation(np.linspace(-1.5, 1.5, B))


def per_building_temps() -> np.ndarray:
  """bench.py's draw: clip(294 + N(0, 1), 285, 305)."""
  return np.clip(294.0 + np.random.RandomState(6).randn(B), 285.0, 305.0)


def conditions(variant: str, shape, first_building: int = 0) -> host_inputs.InitialConditions:
  if variant == "grids":
    return host_inputs.InitialConditions(reset_temp_values=grids(shape), grid_of=grid_of(), offset=offsets(), jitter=JITTER,
                                         first_building=first_building)
  if variant == "initial_temp":
    return host_inputs.InitialConditions(initial_temp=per_building_temps(), first_building=first_building)
  assert variant == "jitter"
  return host_inputs.InitialConditions(jitter=JITTER, first_building=first_building)


def materialised(ic: host_inputs.InitialConditions, episodes, shape, initial_temp: float = INITIAL_TEMP) -> np.ndarray:
  """float64 [B, H*W]: start_temps(b, episodes[b]) of every building, as reset(temps=...) takes it."""
  return np.stack([ic.start_temps(b, int(e), initial_temp=initial_temp, shape=shape).reshape(-1)
                   for b, e in enumerate(episodes)])


def actions(n: int, seed: int = 3) -> np.ndarray:
  return np.random.RandomState(seed).uniform(-1, 1, size=(n, B, 2)).astype(np.float32)


_ROLLOUT: Dict[str, list] = {}


def twin_config():
  from sbsim_amd.environment import SimConfig
  import dataclasses
  return dataclasses.replace(SimConfig.sb1(), initial_temp=INITIAL_TEMP)


def twin_rollout() -> List[List[dict]]:
  """[step][building]: OracleBuilding.step's result (with the sweeps' max|delta|) of every building's twin started from
  the "grids" variant's start_temps(b, 0)."""
  if "steps" not in _ROLLOUT:
    fp, cfg = plan(), twin_config()
    g = load("h2_sb1_r9_random.npz")
    ic = conditions("grids", fp.shape)
    acts = actions(T_TWINS)
    twins = [oracle_twin(fp, cfg, ic.start_temps(b, 0).reshape(-1)) for b in range(B)]
    _ROLLOUT["steps"] = [[twins[b].step(trace=True, **step_kwargs(g, ROW0 + t, t, cfg, acts[t, b])) for b in range(B)]
                         for t in range(T_TWINS)]
    _ROLLOUT["final"] = np.stack([tw.grid() for tw in twins])
  return _ROLLOUT["steps"]


def twin_final_grids() -> np.ndarray:
  twin_rollout()
  return _ROLLOUT["final"]


# ---------------------------------------------------------------- crossed with the other per-building features
CROSSING = "initial-conditions"


def _hook(tw, ic, b: int) -> None:
  """The twin's every reset -- reset(), reset_buildings, its own autoreset -- starts from start_temps(b, its own e)."""
  tw.ic_episode = 0
  plain = tw.reset

  def reset():
    tw.ob.reset_temps = np.ascontiguousarray(ic.start_temps(b, tw.ic_episode).reshape(-1))
    tw.ic_episode += 1
    return plain()

  tw.reset = reset


def crossing():
  """tests/crossed_batches.py's machinery on a case of its factors that is not in its table: building_materials,
  calendars and per_building_episodes together, with the "grids" conditions attached.  Returns (scenario, conditions,
  [(op, the twins' results)] as crossed_batches.expected gives them -- every step with its sweeps' max|delta| --, the
  twins' episode numbers at the end)."""
  if "crossing" not in _ROLLOUT:
    cb.CASES[CROSSING] = cb._case(time="calendars", episodes="per_building", materials="building_materials")
    try:   # (Scenario reads its case from the table: the entry is there for the constructor alone)
      sc = cb.Scenario(CROSSING)
    finally:
      del cb.CASES[CROSSING]
    ic = conditions("grids", sc.plan.shape)
    twins = sc.twins()
    for b, tw in enumerate(twins):
      _hook(tw, ic, b)
      tw.trace = True
    out = [(cb.Op("reset"), [tw.reset() for tw in twins])]
    for op in sc.program:
      assert op.kind in ("step", "reset_buildings"), op.kind
      if op.kind == "step":
        rej = op.rejected if op.rejected is not None else np.zeros(B, dtype=bool)
        out.append((op, [twins[b].step(sc.actions[op.row, b], bool(rej[b])) for b in range(B)]))
      else:
        out.append((op, [twins[b].reset() if op.mask[b] else None for b in range(B)]))
    out.append((cb.Op("final"), np.stack([tw.ob.temp.copy() for tw in twins])))
    _ROLLOUT["crossing"] = (sc, ic, out, np.array([tw.ic_episode for tw in twins]))
  return _ROLLOUT["crossing"]


def fixture_plan(g) -> FloorPlan:
  """The floor plan stored in tests/golden/reset_temp_values.npz (prefix plan_)."""
  from tests.twins import plan_from_npz
  return plan_from_npz({k[len("plan_"):]: g[k] for k in g.files if k.startswith("plan_")})
