"""Divergent batches for the hand-over between buildings in the persistent sweep kernels (test utility, no GPU).

Every sweep kernel takes its first building by index and draws further ones from a device counter; what a workgroup or
wavefront keeps across buildings (k_sweep_band's ring of max|delta| parts and progress counters, k_sweep_stream's
misc[2..4], k_sweep_roll's early draw and "proven unfinished" state, ...) can only go wrong for a building that is not
the first one of its workgroup, and shows most when the predecessor ended in another way.  The batches here make
neighbouring buildings differ as much as the solver allows:

  * initial grids on a ladder, building b of kind b % 3: exactly isothermal, noise of 0.01 K, noise of 3 K, each around
    an offset of its own (294 K + 2 K * N(0, 1)), clipped to 285 .. 305 K;
  * random per-building actions at every step;
  * an iteration limit per case that bites for some buildings and not for others;
  * the order shuffled with a fixed seed, so that which workgroup meets which kind of predecessor is not regular.

`Case` pins the kernel the planner picks (as tests/irregular_plans.py does) and the batch size B.  With SBSIM_DEBUG_CUS=1
the launch hands `static_count(launch_info)` buildings out by index; B >= 4 * that + 3 makes every workgroup (wavefront,
for k_sweep_roll and k_sweep_lds) run at least four buildings and leaves the last round partly empty.  No batch is
smaller than 15 buildings, so that one step can hold the whole spread of sweep counts.
tests/test_handover_cases_cpu.py checks the pins, the depth and the spread of sweep counts on the oracle alone;
tests/test_handover_gpu.py runs every case against its oracle twins."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import irregular_plans as ip
from tests import threshold_cases as tc
from tests.twins import oracle_twin, step_kwargs

LDS, REG, REG_PAIR, ROLL, TWO, BAND, STREAM, JACOBI = 0, 1, 2, 3, 4, 5, 6, 7   # sb_sweep_kernel (include/sbsim_amd.h)
SWITCH = "SBSIM_DEBUG_CUS"
DEPTH = 4                 # buildings every workgroup / wavefront runs at least
KINDS = ("isothermal", "noise-0.01K", "noise-3K")
PAIR_ENV = (("SBSIM_NO_TWO_ROW_PATH", "1"), ("SBSIM_NO_BAND_PATH", "1"))   # tests/test_state_snapshot.py, SCHEDULES["reg-pair"]


@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  plan: object                     # (rooms, room shape) of rectangular_floor_plan, "R9", "260x80" or "irregular:<case>"
  orientation: str                 # BatchedSimulator's argument, "rows" or "columns" -- for SB1-synth and SB2-synth "rows" is
                                   # what "auto" picks; "generic": rows on k_sweep_lds's generic sweep
  path: int                        # launch_info["path"]
  kernel: int                      # launch_info["kernel"]
  waves: int                       # launch_info["waves_per_building"]
  steps: int                       # launch_info["sweep_steps"]: with the kernel it names the instantiation (k_sweep_reg<32,1>:
                                   # 32 + rows - 1; <66,1>: 66 + rows - 1; k_sweep_roll<64>: 64; ...).  Jacobi: 1
  B: int                           # >= DEPTH * static count under SBSIM_DEBUG_CUS=1, + 3
  limit: int                       # SimConfig.iteration_limit: bites for some buildings, not for others
  T: int = 8
  env: Tuple[Tuple[str, str], ...] = ()
  seed: int = 31
  solver: str = "gauss_seidel"


def floor_plan(case: Case):
  """The case's plan in the file's orientation."""
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  spec = case.plan
  if spec == "R9":
    return tc.floor_plan("R9")
  if spec == "260x80":   # test_band_kernel_four_wavefronts_tail_rows_and_overrun_blocks: 258 rows inside the ring, TWO tail rows
    fp = rectangular_floor_plan((12, 3), (20, 24))
    for _ in range(3):
      fp = np.insert(fp, fp.shape[0] - 2, fp[-2], axis=0)
    assert fp.shape == (260, 80)
    return FloorPlan.from_file_input(fp, Materials.sb1(), 10.0, 300.0)
  if isinstance(spec, str) and spec.startswith("irregular:"):
    return ip.plan(spec[len("irregular:"):])
  return FloorPlan.from_file_input(rectangular_floor_plan(*spec), Materials.sb1(), 10.0, 300.0)


def config(case: Case):
  from sbsim_amd.environment import SimConfig
  return dataclasses.replace(SimConfig.sb1(), iteration_limit=case.limit)


def batch(n_cells: int, B: int, T: int, seed: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
  """(initial grids [B, n_cells], actions [T, B, 2], kind of every building [B]) of a divergent batch."""
  rs = np.random.RandomState(seed)
  kind = np.arange(B) % len(KINDS)
  rs.shuffle(kind)
  offset = 294.0 + 2.0 * rs.randn(B, 1)
  noise = rs.randn(B, n_cells) * np.array([0.0, 0.01, 3.0])[kind][:, None]
  init = np.clip(offset + noise, 285.0, 305.0)
  acts = rs.uniform(-1, 1, size=(T, B, 2)).astype(np.float32)
  return init, acts, kind


def case_batch(case: Case, B: Optional[int] = None):
  fp = floor_plan(case)
  return batch(fp.shape[0] * fp.shape[1], case.B if B is None else B, case.T, case.seed)


def static_count(info: dict) -> int:
  """Buildings a launch hands out by index before the draws (sbsim_hip.hip, setup_state): one per workgroup; one per
  wavefront on k_sweep_roll and k_sweep_lds."""
  if info["kernel"] in (ROLL, LDS):
    return info["workgroups"] * info["waves_per_workgroup"]
  return info["workgroups"]


PINNED = ("kernel", "path", "waves_per_building", "waves_per_workgroup", "lds_bytes_per_workgroup", "sweep_steps")


class _Env:
  """Environment variables set for a block (the developer switches are read at every sb_plan_info / sb_create)."""

  def __init__(self, pairs):
    self.pairs, self.old = dict(pairs), {}

  def __enter__(self):
    for k, v in self.pairs.items():
      self.old[k] = os.environ.get(k)
      os.environ[k] = v

  def __exit__(self, *exc):
    for k, v in self.old.items():
      if v is None:
        os.environ.pop(k, None)
      else:
        os.environ[k] = v


def case_env(case: Case) -> Dict[str, str]:
  """The case's switches, with what tests/parity.py's check_plan_against_oracle sets for its path."""
  env = dict(case.env)
  if case.orientation == "generic":
    env["SBSIM_FORCE_GENERIC_SWEEP"] = "1"
  if case.path == 0 and case.solver == "gauss_seidel":
    env["SBSIM_FORCE_LDS_PATH"] = "1"
  fp = floor_plan(case)
  if case.path == 2 and case.solver == "gauss_seidel" and fp.shape[0] * fp.shape[1] < 100000:
    env["SBSIM_FORCE_STREAM_PATH"] = "1"
  return env


def plan_info(case: Case, n_buildings: int, cus: Optional[int] = None) -> dict:
  """sb_plan_info (host only) of the case in its orientation (every case names one: BatchedSimulator has nothing to
  choose), with SBSIM_DEBUG_CUS=cus."""
  from sbsim_amd import _ffi
  assert case.solver == "gauss_seidel"
  fp = floor_plan(case)
  cfg = config(case)
  n_obs = 3 * fp.n_zones + 19
  env = case_env(case)
  env.pop(SWITCH, None)
  if cus is not None:
    env[SWITCH] = str(cus)
  transposed = case.orientation == "columns"
  with _Env(env):
    cp = (fp.transposed() if transposed else fp).compile(cfg.time_step_sec, 100.0)
    keep = [np.ascontiguousarray(x) for x in (cp.cell_class, cp.class_coef, cp.class_zone, cp.zone_off, cp.zone_cells)]
    desc = _ffi.PlanDesc(cp.H, cp.W, cp.Z, cp.n_classes, keep[0].ctypes.data_as(C.POINTER(C.c_uint8)),
                         keep[1].ctypes.data_as(_ffi._dp), keep[2].ctypes.data_as(_ffi._ip),
                         keep[3].ctypes.data_as(_ffi._ip), keep[4].ctypes.data_as(_ffi._ip))
    info = _ffi.LaunchInfo()
    rc = _ffi.load().sb_plan_info(C.byref(desc), n_obs, n_buildings, C.byref(info))
  assert rc == 0, (case.name, rc)
  return {f[0]: getattr(info, f[0]) for f in _ffi.LaunchInfo._fields_}


def oracle_rollout(case: Case, buildings: Optional[List[int]] = None, B: Optional[int] = None):
  """The oracle twins of `buildings` (default: all) over the case's T steps: (sweeps [T, n], converged [T, n])."""
  from tests.golden_util import load
  g = load("h2_sb1_r9_random.npz")
  fp, cfg = floor_plan(case), config(case)
  init, acts, _ = case_batch(case, B)
  bs = list(range(init.shape[0])) if buildings is None else list(buildings)
  twins = [oracle_twin(fp, cfg, init[b]) for b in bs]
  n = np.zeros((case.T, len(bs)), dtype=np.int64)
  conv = np.zeros((case.T, len(bs)), dtype=np.int64)
  for t in range(case.T):
    for k, b in enumerate(bs):
      o = twins[k].step(**step_kwargs(g, tc.TT0 + t, t, cfg, acts[t, b]))
      n[t, k], conv[t, k] = o["n_sweeps"], o["converged"]
  return n, conv


def spread(n: np.ndarray, conv: np.ndarray, limit: int) -> Optional[int]:
  """The first step whose sweep counts have the spread that makes a hand-over test meaningful (None: no step has):
  a building with <= 2 sweeps, one that ends at the limit unconverged, one that converges strictly between the two,
  and at least 5 distinct sweep counts."""
  for t in range(n.shape[0]):
    quick = (n[t] <= 2).any()
    cut = ((n[t] == limit) & (conv[t] == 0)).any()
    between = ((n[t] > 2) & (n[t] < limit) & (conv[t] == 1)).any()
    if quick and cut and between and len(set(n[t].tolist())) >= 5:
      return t
  return None


R9, SB1, SB2 = "R9", ((14, 9), (8, 7)), ((8, 5), (12, 14))

CASES: Dict[str, Case] = {}


def _add(*cases: Case) -> None:
  for c in cases:
    assert c.name not in CASES
    CASES[c.name] = c


def _irregular(name: str, B: int, limit: int, steps: int, **kw) -> Case:
  c = ip.CASES[name]
  assert c.steps in (None, steps)
  return Case(name, f"irregular:{name}", c.orientation, {ip.LDS: 0, ip.STREAM: 2}.get(c.kernel, 1), c.kernel, c.waves, steps,
              B, limit, env=c.env, **kw)


_add(
    # k_sweep_reg<32,1>, <66,1> and the pair variant (wave 0 writes draw_slot for wave 1)
    Case("reg32-15x23", ((2, 2), (5, 9)), "rows", 1, REG, 1, steps=46, B=19, limit=10),
    Case("reg66-22x34", ((2, 3), (9, 10)), "rows", 1, REG, 1, steps=88, B=19, limit=8, env=(("SBSIM_NO_ROLL_SMALL", "1"),)),
    Case("pair-68x65", ((2, 5), (30, 12)), "columns", 1, REG_PAIR, 2, steps=144, B=19, limit=8, env=PAIR_ENV),
    # k_sweep_roll: R9 (two tail rows) as the library runs it, every third building through the redo list, without
    # the free periods; 47 x 48 on <64> (pad lanes, no tail)
    Case("roll-R9", R9, "rows", 1, ROLL, 1, steps=104, B=19, limit=8),
    Case("roll-R9-redo3", R9, "rows", 1, ROLL, 1, steps=104, B=19, limit=8, env=(("SBSIM_DEBUG_FORCE_REDO", "3"),)),
    Case("roll-R9-nofree", R9, "rows", 1, ROLL, 1, steps=104, B=19, limit=8, env=(("SBSIM_ROLL_FREE", "0"),)),
    Case("roll-47x48", ((4, 5), (10, 8)), "rows", 1, ROLL, 1, steps=64, B=19, limit=10),
    # k_sweep_two: 80 slots; 76 slots + tail row; 64 slots; every step overrunning; measurements placed far too late
    Case("two-SB2", SB2, "rows", 1, TWO, 1, steps=133, B=19, limit=12),
    Case("two-SB1", SB1, "rows", 1, TWO, 1, steps=147, B=19, limit=8),
    Case("two-107x58", ((8, 5), (12, 10)), "rows", 1, TWO, 1, steps=117, B=19, limit=15),
    Case("two-SB1-overrun", SB1, "rows", 1, TWO, 1, steps=147, B=19, limit=8, env=(("SBSIM_DEBUG_PRED_SLACK", "-100"),)),
    Case("two-SB1-kappa40", SB1, "rows", 1, TWO, 1, steps=147, B=19, limit=8, env=(("SBSIM_DEBUG_SKIP_KAPPA", "40"),)),
    # k_sweep_band: two wavefronts; three (tail row); four (two tail rows), also with every step overrunning
    Case("band2-SB2", SB2, "rows", 1, BAND, 2, steps=80, B=19, limit=12, env=(("SBSIM_BAND_PATH", "1"),)),
    Case("band3-193x87", ((10, 4), (18, 20)), "rows", 1, BAND, 3, steps=92, B=19, limit=8, T=6),
    Case("band4-260x80", "260x80", "rows", 1, BAND, 4, steps=88, B=19, limit=8, T=6),
    Case("band4-260x80-overrun", "260x80", "rows", 1, BAND, 4, steps=88, B=19, limit=8, T=6,
         env=(("SBSIM_DEBUG_PRED_SLACK", "-100"),)),
    # k_sweep_lds: rows, columns, the generic sweep
    Case("lds-R9", R9, "rows", 0, LDS, 1, steps=207, B=19, limit=8),
    Case("lds-R9-columns", R9, "columns", 0, LDS, 1, steps=181, B=19, limit=8),
    Case("lds-generic-64x12", ((5, 1), (12, 10)), "generic", 0, LDS, 1, steps=101, B=67, limit=8),
    # k_sweep_stream on 1, 2, 4 and (the library's own choice) 5 wavefronts
    Case("stream1-15x23", ((2, 2), (5, 9)), "rows", 2, STREAM, 1, steps=135, B=67, limit=8),
    Case("stream2-R9", R9, "rows", 2, STREAM, 2, steps=223, B=35, limit=8),
    Case("stream4-203x85", ((10, 2), (19, 40)), "rows", 2, STREAM, 4, steps=341, B=19, limit=8, T=6, seed=32),
    Case("stream5-299x401", ((14, 9), (20, 43)), "rows", 2, STREAM, 5, steps=719, B=15, limit=10, T=5),
    # irregular, mixed-material plans
    _irregular("L", 19, 8, steps=72),
    _irregular("U", 19, 8, steps=130),
    _irregular("zone-tail", 19, 8, steps=72),
    _irregular("court190", 19, 10, steps=80, T=6),
    _irregular("court190-stream", 23, 8, steps=271, T=6),
)

# k_sweep_jacobi (solver="jacobi_fp32": no oracle twin; bitwise against tests/jacobi_restatement.py).  512 threads per
# building on both plans; at most four workgroups fit a CU (32 wavefronts), so 35 buildings are four rounds and more.
JACOBI_CASES: Dict[str, Case] = {
    "jacobi-R9": Case("jacobi-R9", R9, "rows", 0, JACOBI, 8, steps=1, B=35, limit=12, T=8, solver="jacobi_fp32"),
    "jacobi-L": Case("jacobi-L", "irregular:L", "rows", 0, JACOBI, 8, steps=1, B=35, limit=12, T=8, solver="jacobi_fp32"),
}

# The device's own geometry (no switch): the kernels no other test runs a second building on.
NATURAL = ("band3-193x87", "band4-260x80", "stream2-R9", "reg66-22x34", "pair-68x65")
NATURAL_EXTRA = 7      # drawn buildings
NATURAL_CUS = 256      # an MI355X; sb_plan_info plans for it


def natural_case(name: str) -> Case:
  """The case as it runs on the device's own geometry: eight steps on every plan (the spread needs them there)."""
  return dataclasses.replace(CASES[name], T=8)


def natural_static(case: Case) -> int:
  """Buildings handed out by index on the whole device, from a probe sb_plan_info at a large batch."""
  return static_count(plan_info(case, 1 << 20))


def natural_checked(static: int) -> List[int]:
  """The buildings that get an oracle twin: a fixed sample of 8 of those handed out by index, and every drawn one."""
  sample = np.random.RandomState(5).choice(static, size=8, replace=False)
  return sorted(int(b) for b in sample) + list(range(static, static + NATURAL_EXTRA))
