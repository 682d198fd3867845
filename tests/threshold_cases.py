"""Boundary cases for the step's stopping rule (simulator.py:348-368: a step ends after the first Gauss-Seidel sweep whose
max|delta| is at or below `convergence_threshold`, or at `iteration_limit`).

From a (floor plan, initial state, step inputs) triple this builds convergence thresholds theta that sit delta = 1e-10 K
from the oracle's max|delta| m_k of a chosen sweep k of the first step after the reset, and the (sweep count, converged
flag) the reference gives for each.  Every sweep kernel decides these cases its own way (the high words of max|delta|
and the redo list of k_sweep_roll, the measure-free periods of k_sweep_two, the float32 predictions of k_sweep_band /
k_sweep_stream_ms): tests/test_threshold_boundary_gpu.py runs them against the oracle twins, and
tests/test_threshold_cases_cpu.py checks the placements themselves on the oracle.

Placements (m_1 >= m_2 >= ... is the series of the step run with a threshold of 0):
  above        theta = m_k + delta                      -> stops at k, converged
  below        theta = m_k - delta                      -> the first j > k with m_j <= theta
  limit-above  theta = m_k + delta, iteration_limit = k -> k, converged
  limit-below  theta = m_k - delta, iteration_limit = k -> k, not converged
A placement is refused unless the neighbouring sweeps are far from theta (|m_{k+-1} - theta| >= 1e-6 theta), theta has
the high 32 bits of m_k (so k_sweep_roll's fast instantiation cannot decide the sweep and hands the building to its
float64 instantiation), and, below m_k, m_k - theta <= 1e-9 (k_sweep_two's `thr_far` band)."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests.twins import oracle_twin, plan_from_npz, step_kwargs

DELTA = 1e-10          # K: theta's distance from m_k
THR_FAR = 1e-9         # K: step_two_impl.h's thr_far band above the threshold
B = 6                  # buildings per case
TARGETS = (1, 4, 5)    # the buildings that start from the target state
TT0 = 96               # step t reads row TT0 + t of h2_sb1_r9_random.npz (mid-morning: occupied, comfort mode), as
                       # tests/parity.py's check_plan_against_oracle gives the device
SEED = 23
KINDS = ("above", "below", "limit-above", "limit-below")


# The floor plans of the GPU cases: (rooms, room shape) of rectangular_floor_plan, a golden plan file, or
# "irregular:<case>" of tests/irregular_plans.py (the plan in the file's orientation).  Every
# placement on them is checked on the CPU by tests/test_threshold_cases_cpu.py.
PLANS = {
    "R9": "plan_r9_sb1.npz",             # 66 x 96 inside the exterior ring
    "45x96": ((2, 3), (20, 30)),
    "65x63": ((2, 2), (30, 29)),         # k_sweep_roll<64> + ONE tail row
    "47x48": ((4, 5), (10, 8)),
    "narrow": ((5, 1), (12, 10)),        # H > 64, narrow: the generic (all-LDS) sweep
    "SB2-synth": ((8, 5), (12, 14)),
    "SB1-synth": ((14, 9), (8, 7)),      # 131 x 78: the two-rows kernel's tail row
    "156x75": ((9, 4), (16, 17)),        # three wavefronts of k_sweep_band
    "203x87": ((10, 4), (19, 20)),       # four wavefronts of k_sweep_band
    "U-shape": "irregular:U",            # 110 x 70 around a courtyard: k_sweep_two's general variant, no switch
}


def floor_plan(name: str):
  from sbsim_amd.floorplan import FloorPlan, Materials, rectangular_floor_plan
  spec = PLANS[name]
  if isinstance(spec, str) and spec.startswith("irregular:"):
    from tests import irregular_plans
    return irregular_plans.plan(spec[len("irregular:"):])
  if isinstance(spec, str):
    from tests.golden_util import load
    return plan_from_npz(load(spec))
  return FloorPlan.from_file_input(rectangular_floor_plan(*spec), Materials.sb1(), 10.0, 300.0)


def hi32(x: float) -> int:
  """The high 32 bits of a float64 (sign, exponent, 20 mantissa bits): what k_sweep_roll's fast instantiation compares."""
  return int(np.array(x, dtype=np.float64).view(np.uint64)) >> 32


def case_inputs(n_cells: int, T: int = 3, seed: int = SEED) -> Tuple[np.ndarray, np.ndarray]:
  """(initial grids [B, n_cells], actions [T, B, 2]): buildings TARGETS share one state, the others are independent."""
  rs = np.random.RandomState(seed)
  init = np.clip(294.0 + 2.0 * rs.randn(B, 1) + 0.2 * rs.randn(B, n_cells), 285.0, 305.0)
  for b in TARGETS[1:]:
    init[b] = init[TARGETS[0]]
  acts = rs.uniform(-1, 1, size=(T, B, 2)).astype(np.float32)
  return init, acts


def series(plan, cfg, g, init_flat, a) -> np.ndarray:
  """m_1, m_2, ...: the max|delta| of every sweep of the first step after the reset, run to cfg's iteration limit."""
  tw = oracle_twin(plan, dataclasses.replace(cfg, convergence_threshold=0.0), init_flat)
  return tw.step(**step_kwargs(g, TT0, 0, cfg, a), trace=True)["max_delta"]


def expected(m: Sequence[float], theta: float, limit: int) -> Tuple[int, bool]:
  """simulator.py:348-368 on a known series: (sweeps, converged)."""
  for j in range(min(limit, len(m))):
    if m[j] <= theta:
      return j + 1, True
  assert limit <= len(m), "the series is shorter than the limit"
  return limit, False


@dataclasses.dataclass(frozen=True)
class Placement:
  kind: str
  k: int
  theta: float
  limit: int
  n: int
  converged: bool

  @property
  def id(self) -> str:
    return f"{self.kind}-k{self.k}"


def check(m: Sequence[float], p: Placement, delta: float = DELTA) -> Optional[str]:
  """None if placement p satisfies the invariants on the series m, else why not."""
  k, th = p.k, p.theta
  mk = float(m[k - 1])
  for j in (k - 1, k + 1):
    if 1 <= j <= len(m) and abs(float(m[j - 1]) - th) < 1e-6 * th:
      return f"m_{j} = {m[j - 1]!r} is within 1e-6 theta of theta"
  if hi32(th) != hi32(mk):
    return "theta and m_k differ in their high 32 bits"
  if p.kind.endswith("above") and not 0.0 < th - mk <= delta * 1.5:
    return "theta is not just above m_k"
  if p.kind.endswith("below") and not 0.0 < mk - th <= THR_FAR:
    return "theta is not within the thr_far band below m_k"
  if (p.n, p.converged) != expected(m, th, p.limit):
    return "the expected outcome does not follow from the series"
  return None


def place(m: Sequence[float], k: int, kind: str, limit: int, delta: float = DELTA) -> Optional[Placement]:
  """The placement of `kind` at sweep k, or None if it fails a check."""
  mk = float(m[k - 1])
  theta = mk + delta if kind.endswith("above") else mk - delta
  lim = k if kind.startswith("limit") else limit
  n, conv = expected(m, theta, lim)
  p = Placement(kind, k, theta, lim, n, conv)
  return p if check(m, p, delta) is None else None


def natural_stop(m: Sequence[float], threshold: float) -> int:
  return expected(m, threshold, len(m))[0]


def chosen_sweeps(m: Sequence[float], threshold: float) -> List[int]:
  """k = 1 (its max|delta| includes the exterior ring's first update), 2, the middle and the last sweep before the
  step's natural stop at `threshold`."""
  n0 = natural_stop(m, threshold)
  return sorted({k for k in (1, 2, max(1, n0 // 2), n0 - 1) if 1 <= k < len(m)})


def placements(m: Sequence[float], threshold: float, limit: int, kinds: Sequence[str] = KINDS,
               ks: Optional[Sequence[int]] = None) -> Dict[str, Placement]:
  out = {}
  for k in (chosen_sweeps(m, threshold) if ks is None else ks):
    for kind in kinds:
      p = place(m, k, kind, limit)
      if p is not None:
        out[p.id] = p
  return out


# ---- k_sweep_jacobi (float32 max|delta| <= float32(threshold), tests/jacobi_restatement.py) ----

JACOBI_KINDS = ("exact", "mid-up", "mid-down", "mid")
JACOBI_K = 6   # the iteration the thresholds sit at


def jacobi_tap():
  """Inputs of one sb_tap_jacobi call on R9 (float32 grids [4, H, W], float32 q, T_inf [4]): buildings 0 and 3 are the
  target (the same inputs), 1 and 2 independent.  Returns (plan, tprev, q, tinf)."""
  from tests import jacobi_restatement as jr
  fp = floor_plan("R9")
  rs = np.random.RandomState(5)
  n = 4
  tprev = (288.0 + 8.0 * rs.rand(n, *fp.shape)).astype(np.float32)
  q = np.stack([jr.input_q(fp, rs.uniform(-3000.0, 3000.0, fp.n_zones)) for _ in range(n)])
  tinf = rs.uniform(265.0, 305.0, n)
  tprev[3], q[3], tinf[3] = tprev[0], q[0], tinf[0]
  return fp, tprev, q, tinf


def jacobi_series(tt: dict, tprev, q, tinf: float, dt: float, n: int) -> np.ndarray:
  """d_1 .. d_n: the float32 max|delta| of the first n Jacobi iterations of the restatement's timestep."""
  from tests import jacobi_restatement as jr
  est, out = np.asarray(tprev, np.float32), []
  for _ in range(n):
    est, d = jr.update(tt, est, tprev, q, tinf, dt)
    out.append(d)
  return np.array(out, dtype=np.float32)


def jacobi_theta(d_k: np.float32, kind: str) -> float:
  """exact: float64(d_k).  With p the float32 below d_k and mid = (p + d_k) / 2 (exact in float64): mid-up, the double
  just above mid, rounds to d_k; mid-down, the double just below, rounds to p; mid rounds to the one with an even
  significand."""
  d_k = np.float32(d_k)
  if kind == "exact":
    return float(d_k)
  p = np.nextafter(d_k, np.float32(0))
  mid = (float(p) + float(d_k)) / 2.0
  assert mid - float(p) == float(d_k) - mid
  return {"mid": mid, "mid-up": float(np.nextafter(mid, np.inf)), "mid-down": float(np.nextafter(mid, -np.inf))}[kind]


def jacobi_expected(d: Sequence[np.float32], theta: float, limit: int) -> Tuple[int, bool]:
  """The restatement's stopping rule on a known float32 series: (iterations, converged)."""
  thr = np.float32(theta)
  for j in range(min(limit, len(d))):
    if d[j] <= thr:
      return j + 1, True
  assert limit <= len(d), "the series is shorter than the limit"
  return limit, False
