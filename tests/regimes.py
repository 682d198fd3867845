"""Coefficient regimes for the sweep kernels (test utility, no GPU).

Every other parity test builds its class table from Materials.sb1() at dt = 300 s, 10 cm control volumes and
h_conv = 100 or 12: interior air with b = 0.24997 on all four sides, ap <= 0.104, row sums up to 0.999883,
sc <= 5.6e-4, air and interior wall of one diffusivity (20 classes on R9, not 21), sweep counts that decay smoothly.
What depends on the coefficients' values -- plan_two's exact equalities among (bU, bD, bL, bR), the class and set
counts, the static tail scan's products of bL, the measure-free periods' b >= 0 / row sum <= 1 condition, the high-word
stopping test, the sweep-count predictors, k_pre's g table, the float32 class tensors of solver="jacobi_fp32" -- has
only run there.  A `Regime` is another point: materials by role, time step, CV size, stopping threshold and limit,
h_conv, and the device flows that keep the zones inside the thermostats' range.  Each row's purpose:

  sb1        the control
  physical   air / gypsum / concrete: 21 classes against SB1's 20, sc a thousand times SB1's
  short      the same at 60 s: small b with ap near 1
  coarse     the same at 900 s and 50 cm CVs: smaller b still, steps of <= 2 sweeps
  stiff      stiff rooms behind heavy walls: row sums near 1 AND ap near 1 in one table; counts pinned at the limit
  hour       SB1 at 3600 s: row sums near 1 with ap near 0, a sweep count that falls by >= 40 in one step
  second     SB1 at 1 s: ap near 1 in the walls, b = 0.24 in the air; counts that rise
  contrast   conductivities from 500 to 1e-4: ap near 1 with b spanning six decades, steps of <= 2 sweeps

`apply(fp, regime)` puts a regime's materials on a plan built with SB1's (the extra air-like and wall-like materials
of tests/irregular_plans.py are scaled by their base material's ratios, so distinct classes and sets stay distinct)
and its CV size; `config(regime, plan)` is the SimConfig, its VAV flows sized to the plan's rooms.  `CASES` names the
smallest pinned plan of every sweep-kernel instantiation (tests/handover_cases.py, tests/threshold_cases.py) with the
case's own developer switches;
`oracle_rollout` runs the oracle twins of exactly the batch tests/test_regimes_gpu.py runs.
tests/test_regimes_cpu.py pins the oracle to the reference at every regime (tests/golden/regimes.npz, written by
oracle/gen_golden_regimes.py) and checks the conditions on these inputs on the oracle alone."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, Optional, Tuple

import numpy as np

from sbsim_amd.floorplan import FloorPlan, Material, Materials
from tests import handover_cases as hc
from tests import threshold_cases as tc
from tests.materials_cases import substituted
from tests.twins import oracle_twin, step_kwargs

B, T = 5, 6
GOLDEN = "regimes.npz"
GOLDEN_PLAN = ((2, 2), (5, 9))       # 15 x 23 inside the ring
GOLDEN_STEPS = 6

_PHYSICAL = Materials(Material(0.026, 1005.0, 1.2), Material(0.17, 1090.0, 800.0), Material(1.4, 880.0, 2300.0))


@dataclasses.dataclass(frozen=True)
class Regime:
  name: str
  materials: Materials
  time_step_sec: float
  cv_size_cm: float
  convergence_threshold: float
  iteration_limit: int
  h_conv: float
  overrides: Tuple[Tuple[str, float], ...] = ()   # SimConfig fields (the device flows)
  seed: int = 11                                  # of the batch's initial grids and actions
  spread: float = 2.0                             # K: sigma of the buildings' offsets around 294 K
  noise: float = 0.2                              # K: sigma of the cells around their building's offset


def _flows(scale: float) -> Tuple[Tuple[str, float], ...]:
  """SB1's VAV air and reheat-water flows scaled (physical air holds a thousandth of the heat SB1's does)."""
  return (("vav_max_air_flow_rate", 0.035 * scale), ("vav_reheat_max_water_flow_rate", 0.03 * scale))


REGIMES: Dict[str, Regime] = {r.name: r for r in (
    Regime("sb1", Materials.sb1(), 300.0, 10.0, 0.1, 100, 100.0),
    Regime("physical", _PHYSICAL, 300.0, 10.0, 0.1, 100, 12.0, _flows(0.02)),
    Regime("short", _PHYSICAL, 60.0, 10.0, 0.01, 100, 100.0, _flows(0.02)),
    Regime("coarse", _PHYSICAL, 900.0, 50.0, 0.1, 100, 500.0, _flows(0.5)),
    Regime("stiff", Materials(Material(2.0, 700.0, 1.0), Material(2.0, 500.0, 1800.0), Material(0.05, 500.0, 3000.0)),
           300.0, 10.0, 0.01, 100, 100.0, _flows(0.1)),
    Regime("hour", Materials.sb1(), 3600.0, 10.0, 0.1, 100, 100.0),
    Regime("second", Materials.sb1(), 1.0, 10.0, 0.001, 100, 0.0),
    Regime("contrast", Materials(Material(500.0, 700.0, 1.0), Material(1e-3, 2000.0, 3000.0),
                                 Material(1e-4, 2000.0, 3000.0)), 300.0, 10.0, 0.1, 100, 12.0),
)}


def _triple(m: Material) -> Tuple[float, float, float]:
  return (m.conductivity, m.heat_capacity, m.density)


def _role(k: float, c: float, rho: float) -> str:
  """The role of a material of a plan built from SB1's: exterior wall (k = 0.05), wall-like (the interior wall's heat sits in
  its density column: rho of about 700), air-like."""
  if k < 1.0:
    return "exterior_wall"
  return "interior_wall" if rho > 100.0 else "air"


def apply(fp: FloorPlan, regime: Regime) -> FloorPlan:
  """`fp` (built from Materials.sb1()) with the regime's materials by role and its CV size.  An SB1 triple becomes the
  regime's material exactly; any other material becomes its own triple times (regime's / SB1's) of its role."""
  sb1 = Materials.sb1()
  ids, table = fp.material_slots()
  new = np.empty_like(table)
  roles = set()
  for s, row in enumerate(table):
    role = _role(*row)
    base, to = np.array(_triple(getattr(sb1, role))), np.array(_triple(getattr(regime.materials, role)))
    new[s] = to if tuple(row) == tuple(base) else row * (to / base)
    roles.add(role)
  assert "air" in roles and "exterior_wall" in roles, roles
  assert len({tuple(r) for r in new}) == len(new)       # distinct materials stay distinct
  return dataclasses.replace(fp, conductivity=np.ascontiguousarray(new[ids, 0]),
                             heat_capacity=np.ascontiguousarray(new[ids, 1]),
                             density=np.ascontiguousarray(new[ids, 2]), cv_size_cm=float(regime.cv_size_cm))


R9_ROOM_CELLS = 600      # SB1's VAV flows serve R9's rooms of 20 x 30 CVs


def config(regime: Regime, fp: Optional[FloorPlan] = None, limit: Optional[int] = None):
  """The regime's SimConfig.  With a plan, the VAV flows are sized to its smallest zone (flows * cells / 600): the heat a
  VAV moves per cell and step is then R9's on every plan, where SB1's flows drive a 45-cell room far outside the
  thermostats' range within a step."""
  from sbsim_amd.environment import SimConfig
  sb1 = SimConfig.sb1()
  kw = dict(time_step_sec=regime.time_step_sec, convergence_threshold=regime.convergence_threshold,
            iteration_limit=regime.iteration_limit if limit is None else limit, cv_size_cm=regime.cv_size_cm,
            materials=regime.materials, vav_max_air_flow_rate=sb1.vav_max_air_flow_rate,
            vav_reheat_max_water_flow_rate=sb1.vav_reheat_max_water_flow_rate)
  kw.update(dict(regime.overrides))
  if fp is not None:
    size = min(len(z) for z in fp.zone_cell_lists()) / R9_ROOM_CELLS
    kw["vav_max_air_flow_rate"] *= size
    kw["vav_reheat_max_water_flow_rate"] *= size
  return dataclasses.replace(sb1, **kw)


# ---------------------------------------------------------------- the kernel cases
@dataclasses.dataclass(frozen=True)
class KernelCase:
  name: str
  plan: object                     # a tests/handover_cases.py plan spec, or "threshold:<name>" of tests/threshold_cases.py
  orientation: str
  path: int
  kernel: int
  waves: int
  steps: int                       # sb_plan_info's sweep_steps at SB1: with the kernel, the instantiation
  env: Tuple[Tuple[str, str], ...] = ()


def _from_handover(name: str, **kw) -> KernelCase:
  c = hc.CASES[name]
  return KernelCase(kw.pop("as_name", name), c.plan, c.orientation, c.path, c.kernel, c.waves, c.steps, tuple(c.env), **kw)


CASES: Dict[str, KernelCase] = {c.name: c for c in (
    _from_handover("reg32-15x23"), _from_handover("reg66-22x34"), _from_handover("pair-68x65"),
    _from_handover("roll-47x48"),                                                   # no tail row (see ROLL_CAPACITY)
    KernelCase("roll-45x96", "threshold:45x96", "rows", 1, hc.ROLL, 1, 96),          # no tail row, at every regime
    KernelCase("65x63", "threshold:65x63", "rows", 1, hc.ROLL, 1, 68),               # one tail row
    _from_handover("roll-R9"),                                                      # two tail rows: the static scan
    _from_handover("two-107x58"), _from_handover("two-SB2"), _from_handover("two-SB1"),
    KernelCase("U-shape", "threshold:U-shape", "rows", 1, hc.TWO, 1, 130),           # the general four-coefficient variant
    _from_handover("band2-SB2"), _from_handover("band3-193x87"), _from_handover("band4-260x80"),
    _from_handover("lds-R9"), _from_handover("lds-R9-columns"), _from_handover("lds-generic-64x12"),
    _from_handover("stream1-15x23"), _from_handover("stream2-R9"), _from_handover("stream4-203x85"),
)}

# roll-47x48 has 31 cell classes at SB1, all k_sweep_roll's class words hold.  A regime whose interior wall has a diffusivity
# other than the air's has one class more (the walls' interior cells), and the planner then hands the plan to k_sweep_lds as
# it does with tests/irregular_plans.py's roll66-32cls: on this one plan the kernel does depend on the materials, by the
# class count alone.  There the pair is pinned to that kernel; roll-45x96 runs k_sweep_roll without a tail row at every
# regime and 65x63 its 64-slot instantiation.
ROLL_CAPACITY = 31
ROLL_47x48_LDS = (hc.LDS, 1, 98, 0)        # kernel, wavefronts, sweep steps, path


def pin(c: KernelCase, regime: Regime) -> Tuple[int, int, int, int]:
  """(kernel, wavefronts per building, sweep steps, path) the planner must report for the pair: the case's SB1 pin."""
  if c.plan == CASES["roll-47x48"].plan and c.kernel == hc.ROLL and compiled(c, regime).n_classes > ROLL_CAPACITY:
    return ROLL_47x48_LDS
  return (c.kernel, c.waves, c.steps, c.path)


# the same plan and batch under further switches: (case name, base case, the extra switch)
VARIANTS: Dict[str, Tuple[str, Tuple[str, str]]] = {
    "roll-R9-exact": ("roll-R9", ("SBSIM_ROLL_EXACT", "1")),
    "roll-R9-redo3": ("roll-R9", ("SBSIM_DEBUG_FORCE_REDO", "3")),
    "roll-R9-nofree": ("roll-R9", ("SBSIM_ROLL_FREE", "0")),
    "two-SB1-overrun": ("two-SB1", ("SBSIM_DEBUG_PRED_SLACK", "-100")),
}


def case(name: str) -> KernelCase:
  if name in VARIANTS:
    base, switch = VARIANTS[name]
    return dataclasses.replace(CASES[base], name=name, env=CASES[base].env + (switch,))
  return CASES[name]


_PLANS: Dict[object, FloorPlan] = {}


def sb1_plan(c: KernelCase) -> FloorPlan:
  """The case's plan with SB1's materials, in the file's orientation (built once per plan)."""
  if c.plan not in _PLANS:
    if isinstance(c.plan, str) and c.plan.startswith("threshold:"):
      _PLANS[c.plan] = tc.floor_plan(c.plan[len("threshold:"):])
    else:
      _PLANS[c.plan] = hc.floor_plan(hc.Case("", c.plan, "rows", 1, 0, 1, 0, 1, 1))
  return _PLANS[c.plan]


def plan(c: KernelCase, regime: Regime) -> FloorPlan:
  return apply(sb1_plan(c), regime)


def case_env(c: KernelCase) -> Dict[str, str]:
  """The case's switches with what tests/parity.py's check_plan_against_oracle sets for the case's own path and orientation."""
  fp = sb1_plan(c)
  env = dict(c.env)
  if c.orientation == "generic":
    env["SBSIM_FORCE_GENERIC_SWEEP"] = "1"
  if c.path == 0:
    env["SBSIM_FORCE_LDS_PATH"] = "1"
  if c.path == 2 and fp.shape[0] * fp.shape[1] < 100000:
    env["SBSIM_FORCE_STREAM_PATH"] = "1"
  return env


# (regime, plan) -> iteration limit, where the regime's own does not serve.  "stiff": the largest sweep count of the plan's batch
# at a limit of 100 that, as the limit, leaves the batch a step ending (limit, unconverged), one ending (limit, converged)
# and one converging strictly between 2 sweeps and the limit (tests/test_regimes_cpu.py checks all three on the oracle).
_STIFF_LIMITS = {"reg32-15x23": 18, "reg66-22x34": 38, "pair-68x65": 87, "roll-47x48": 31, "roll-45x96": 96, "65x63": 18, "roll-R9": 26,
                 "two-107x58": 45, "two-SB2": 61, "two-SB1": 23, "U-shape": 99, "band3-193x87": 98, "band4-260x80": 98,
                 "lds-generic-64x12": 46, "stream4-203x85": 51}
LIMITS: Dict[Tuple[str, object], int] = {("stiff", CASES[n].plan): v for n, v in _STIFF_LIMITS.items()}


def case_config(c: KernelCase, regime: Regime):
  return config(regime, sb1_plan(c), LIMITS.get((regime.name, c.plan)))


def compiled(c: KernelCase, regime: Regime):
  """The class table the device gets: the regime's plan in the case's orientation at the regime's dt and h_conv."""
  fp = plan(c, regime)
  return (fp.transposed() if c.orientation == "columns" else fp).compile(regime.time_step_sec, regime.h_conv)


def plan_info_and_digest(c: KernelCase, regime: Regime, n_buildings: int = B) -> Tuple[dict, str]:
  """sb_plan_info's launch geometry and sb_debug_plan_digest's hash of every table the planner hands the kernel (host only),
  under the case's switches and no other planner switch."""
  from sbsim_amd import _ffi
  from tests.planner_digest_cases import _Switches
  cp = compiled(c, regime)
  keep = [np.ascontiguousarray(x) for x in (cp.cell_class, cp.class_coef, cp.class_zone, cp.zone_off, cp.zone_cells)]
  desc = _ffi.PlanDesc(cp.H, cp.W, cp.Z, cp.n_classes, keep[0].ctypes.data_as(C.POINTER(C.c_uint8)),
                       keep[1].ctypes.data_as(_ffi._dp), keep[2].ctypes.data_as(_ffi._ip),
                       keep[3].ctypes.data_as(_ffi._ip), keep[4].ctypes.data_as(_ffi._ip))
  info, digest = _ffi.LaunchInfo(), C.c_uint64(0)
  with _Switches(case_env(c)):
    rc = _ffi.load().sb_plan_info(C.byref(desc), 3 * cp.Z + 19, n_buildings, C.byref(info))
    assert rc == 0, (c.name, regime.name, rc, _ffi.load().sb_last_error())
    rc = _ffi.entry("sb_debug_plan_digest")(C.byref(desc), 0, C.byref(digest))
    assert rc == 0, (c.name, regime.name, rc)
  return {f[0]: getattr(info, f[0]) for f in _ffi.LaunchInfo._fields_}, f"{digest.value:016x}"


# ---------------------------------------------------------------- the batches and their oracle twins
def batch(n_cells: int, regime: Regime, n_buildings: int = B, n_steps: int = T) -> Tuple[np.ndarray, np.ndarray]:
  """(initial grids [B, n_cells], actions [T, B, 2]): check_plan_against_oracle's own draw (a rough grid around an offset per
  building, clipped to 285 .. 305 K) with the regime's seed and widths."""
  rs = np.random.RandomState(regime.seed)
  init = np.clip(294.0 + regime.spread * rs.randn(n_buildings, 1) + regime.noise * rs.randn(n_buildings, n_cells),
                 285.0, 305.0)
  acts = rs.uniform(-1, 1, size=(n_steps, n_buildings, 2)).astype(np.float32)
  return init, acts


_ROLLOUTS: Dict[Tuple[object, str], list] = {}


def oracle_rollout(c: KernelCase, regime: Regime) -> list:
  """[T][B] results of OracleBuilding.step(trace=True) on the twins of the case's batch at the regime (computed once per plan
  and regime: the cases that share a plan share the twins)."""
  key = (c.plan, regime.name)
  if key not in _ROLLOUTS:
    from tests.golden_util import load
    g = load("h2_sb1_r9_random.npz")
    fp = plan(c, regime)
    cfg = case_config(c, regime)
    init, acts = batch(fp.shape[0] * fp.shape[1], regime)
    twins = [oracle_twin(fp, cfg, init[b]) for b in range(B)]
    _ROLLOUTS[key] = [[twins[b].step(**step_kwargs(g, tc.TT0 + t, t, cfg, acts[t, b], h_conv=regime.h_conv,
                                                              step_sec=regime.time_step_sec), trace=True) for b in range(B)]
                      for t in range(T)]
  return _ROLLOUTS[key]


def setpoints(g, t: int, cfg) -> Tuple[float, float]:
  return cfg.comfort_temp_window if bool(g["comfort_now"][tc.TT0 + t]) else cfg.eco_temp_window


# ---------------------------------------------------------------- the per-building-materials batch
MIXED = ("sb1", "physical", "stiff", "contrast")    # regimes that share dt = 300 s and 10 cm CVs: building b carries MIXED[b % 4]
MIXED_B, MIXED_T = 8, 6


def mixed_batch():
  """One batch on the per-building-materials handle (sb_create_materials, k_sweep_lds<true>): R9, building b with the
  materials and h_conv of regime MIXED[b % 4] -- conductivities from 500 to 1e-4 in one launch.  The step's scalars are
  shared: SB1's threshold and limit, a twentieth of SB1's VAV flows (physical air holds a thousandth of the heat).
  Returns (plan, cfg, slot ids, materials [B, M, 3], h_conv [B], initial grids, actions)."""
  fp = tc.floor_plan("R9")
  ids, table = fp.material_slots()
  mats = np.stack([apply(fp, REGIMES[MIXED[b % len(MIXED)]]).material_slots()[1] for b in range(MIXED_B)])
  assert mats.shape == (MIXED_B,) + table.shape
  for b in range(MIXED_B):   # apply() keeps the slots' order: the substituted plan is the regime's plan
    assert np.array_equal(mats[b][ids, 0], apply(fp, REGIMES[MIXED[b % len(MIXED)]]).conductivity)
  hs = np.array([REGIMES[MIXED[b % len(MIXED)]].h_conv for b in range(MIXED_B)])
  cfg = config(dataclasses.replace(REGIMES["sb1"], overrides=_flows(0.05)))
  rs = np.random.RandomState(17)
  init = np.clip(294.0 + 2.0 * rs.randn(MIXED_B, 1) + 0.2 * rs.randn(MIXED_B, fp.shape[0] * fp.shape[1]), 285.0, 305.0)
  acts = rs.uniform(-1, 1, size=(MIXED_T, MIXED_B, 2)).astype(np.float32)
  return fp, cfg, ids, mats, hs, init, acts


def mixed_twins(fp, cfg, ids, mats, init) -> list:
  return [oracle_twin(substituted(fp, ids, mats[b]), cfg, init[b]) for b in range(len(mats))]


def golden_inputs(regime: Regime, shape: Tuple[int, int]) -> np.ndarray:
  """The seeded rough grid of the reference run of tests/golden/regimes.npz."""
  rs = np.random.RandomState(1000 + sorted(REGIMES).index(regime.name))
  return np.clip(294.0 + 3.0 * rs.randn(*shape), 285.0, 305.0)
