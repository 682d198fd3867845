"""GPU: every sweep kernel's stopping decision at the convergence threshold.

The oracle stops a step with one compare, max|delta| <= threshold (oracle/sb_oracle.c, sbo_fd_timestep); the sweep kernels
decide on high words (k_sweep_roll, with the float64 instantiation behind it through the redo list), behind
measure-free periods (k_sweep_two's thr_far / all_meas re-run), behind float32 predictions (k_sweep_band,
k_sweep_stream_ms) or in float32 (k_sweep_jacobi).  Random starts never land a sweep within 1e-7 K of the threshold; the
cases of tests/threshold_cases.py put the threshold 1e-10 K above or below the oracle's max|delta| of a chosen sweep of
the first step (buildings 1, 4, 5; the others start elsewhere), with and without an iteration limit at that sweep.  Per
building and step: sweep count and converged flag EQUAL to the oracle twin's, temperatures within 1e-8 K.

Calibration: a float64 kernel reassociates the update, so its own max|delta| is not the oracle's to the bit.  Its grids
after k - 1 and k sweeps are held within delta / 4 of the oracle's, which bounds its max|delta| of sweep k within
delta / 2 of the oracle's: a wrong sweep count here is a wrong decision, not rounding."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from tests import jacobi_restatement as jr  # noqa: E402
from tests import threshold_cases as tc  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import check_plan_against_oracle, need_experimental_kernels, need_gpu  # noqa: E402
from tests.twins import oracle_twin, step_kwargs  # noqa: E402

# id: (plan, orientation, path, environment, sb_sweep_kernel, wavefronts per building or None, experimental library)
KERNELS = {
    "roll-R9": ("R9", "auto", 1, {}, 3, None, False),
    "roll-45x96": ("45x96", "rows", 1, {}, 3, None, False),
    "roll-65x63-tail": ("65x63", "rows", 1, {}, 3, None, False),
    "reg": ("47x48", "rows", 1, {"SBSIM_NO_ROLL_SMALL": "1"}, 1, None, False),
    "reg-pair": ("R9", "columns", 1, {"SBSIM_NO_TWO_ROW_PATH": "1", "SBSIM_NO_BAND_PATH": "1"}, 2, 2, False),
    "lds": ("R9", "rows", 0, {}, 0, None, False),
    "lds-generic": ("narrow", "generic", 0, {}, 0, None, False),
    "two-SB2-k0.9": ("SB2-synth", "auto", 1, {"SBSIM_DEBUG_SKIP_KAPPA": "0.9"}, 4, None, False),
    "two-SB2-k2.5": ("SB2-synth", "auto", 1, {"SBSIM_DEBUG_SKIP_KAPPA": "2.5"}, 4, None, False),
    "two-SB2-k40": ("SB2-synth", "auto", 1, {"SBSIM_DEBUG_SKIP_KAPPA": "40"}, 4, None, False),
    "two-SB2-noskip": ("SB2-synth", "auto", 1, {"SBSIM_TWO_NO_SKIP": "1"}, 4, None, False),
    "two-SB1-k0.9": ("SB1-synth", "auto", 1, {"SBSIM_DEBUG_SKIP_KAPPA": "0.9"}, 4, None, False),
    "two-SB1-k2.5": ("SB1-synth", "auto", 1, {"SBSIM_DEBUG_SKIP_KAPPA": "2.5"}, 4, None, False),
    "two-SB1-k40": ("SB1-synth", "auto", 1, {"SBSIM_DEBUG_SKIP_KAPPA": "40"}, 4, None, False),
    "two-SB1-noskip": ("SB1-synth", "auto", 1, {"SBSIM_TWO_NO_SKIP": "1"}, 4, None, False),
    "two-general": ("SB2-synth", "auto", 1, {"SBSIM_TWO_GENERAL": "1"}, 4, None, False),
    "two-general-U": ("U-shape", "rows", 1, {}, 4, None, False),     # the general variant by the library's own choice
    "two-max-level-0": ("SB2-synth", "auto", 1, {"SBSIM_TWO_MAX_LEVEL": "0"}, 4, None, False),
    "band-2": ("SB2-synth", "auto", 1, {"SBSIM_BAND_PATH": "1"}, 5, 2, False),
    "band-3": ("156x75", "rows", 1, {}, 5, 3, False),
    "band-4": ("203x87", "rows", 1, {}, 5, 4, False),
    "stream": ("SB2-synth", "rows", 2, {}, 6, None, False),
    "stream-ms": ("SB2-synth", "rows", 2, {"SBSIM_STREAM_MS": "1"}, 6, None, True),
    "stream-roll": ("SB2-synth", "rows", 2, {"SBSIM_STREAM_ROLL": "1"}, 6, None, True),
}
T = 3   # the boundary step and two more with the same threshold


class _Case:
  """A kernel's floor plan, inputs and oracle series; runs one configuration against the oracle twins."""

  def __init__(self, kernel, monkeypatch):
    need_gpu()
    name, self.orientation, self.path, env, self.kern, self.waves, exp = KERNELS[kernel]
    self.mp = monkeypatch
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    need_experimental_kernels(exp, monkeypatch)
    self.g = load("h2_sb1_r9_random.npz")
    self.plan = tc.floor_plan(name)
    self.cfg = SimConfig.sb1()
    self.init, self.acts = tc.case_inputs(self.plan.shape[0] * self.plan.shape[1], T)
    t0 = tc.TARGETS[0]
    self.m = tc.series(self.plan, self.cfg, self.g, self.init[t0], self.acts[0, t0])
    self._grids = {0: self.init[t0]}
    self.worst_cal = 0.0

  def run(self, theta, limit, steps=T):
    cfg = dataclasses.replace(self.cfg, convergence_threshold=theta, iteration_limit=limit)
    return check_plan_against_oracle(self.plan, self.plan.n_zones, self.orientation, self.path, self.mp,
                                     expect_kernel=self.kern, expect_waves=self.waves, B=tc.B, T=steps,
                                     init=self.init, acts=self.acts, cfg=cfg)

  def oracle_grid(self, k):
    """g_k: the oracle's grid after k sweeps of the first step (no zone power yet)."""
    if k not in self._grids:
      tw = oracle_twin(self.plan, dataclasses.replace(self.cfg, convergence_threshold=0.0, iteration_limit=k),
                          self.init[tc.TARGETS[0]])
      tw.step(**step_kwargs(self.g, tc.TT0, 0, self.cfg, self.acts[0, tc.TARGETS[0]]))
      self._grids[k] = tw.temp.copy()
    return self._grids[k]

  def calibrate(self, k, grid):
    """The kernel's grid after exactly k sweeps of the targets' first step against g_k: within delta / 4."""
    for b in tc.TARGETS:
      d = float(np.abs(grid[b].reshape(-1) - self.oracle_grid(k)).max())
      self.worst_cal = max(self.worst_cal, d)
      assert d <= tc.DELTA / 4, (k, b, d)

  def boundary(self, p, steps=T):
    """Placement p: every building against its twin; the targets' first step ends where the placement says."""
    infos, grids = self.run(p.theta, p.limit, steps)
    for b in tc.TARGETS:
      assert (infos[0][b, 4], bool(infos[0][b, 5])) == (p.n, p.converged), (p, b, infos[0][b, 4:6])
    if p.kind == "limit-below":     # exactly k sweeps
      self.calibrate(p.k, grids[0])
    return grids

  def calibrate_before(self, k):
    if k > 1:
      _, grids = self.run(0.0, k - 1, steps=1)
      self.calibrate(k - 1, grids[0])


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_sweep_kernel_decides_like_the_oracle_at_the_threshold(kernel, monkeypatch):
  c = _Case(kernel, monkeypatch)
  pl = tc.placements(c.m, c.cfg.convergence_threshold, c.cfg.iteration_limit)
  ks = tc.chosen_sweeps(c.m, c.cfg.convergence_threshold)
  assert {p.k for p in pl.values()} == set(ks) and len(pl) >= 3 * len(ks)
  for k in ks:
    c.calibrate_before(k)
  for p in pl.values():
    c.boundary(p)
  print(f"\n[{kernel}] k = {ks}, {len(pl)} placements, max |grid - oracle| after k sweeps = {c.worst_cal:.2e} K")


@pytest.mark.parametrize("plan", ["R9", "45x96", "65x63-tail"])
def test_roll_kernel_redo_list_at_the_threshold(plan, monkeypatch):
  """k_sweep_roll's fast instantiation cannot decide a sweep whose max|delta| has the threshold's high word: the building
  goes to the float64 instantiation through the redo list (no debug hook).  The same placements on the float64
  instantiation alone (SBSIM_ROLL_EXACT=1).  Both share the update's arithmetic (step_roll.hip: EXACT changes only
  how max|delta| is kept), so their grids agree bit for bit."""
  grids = {}
  for exact in (False, True):
    with monkeypatch.context() as mp:
      if exact:
        mp.setenv("SBSIM_ROLL_EXACT", "1")
      c = _Case("roll-" + plan, mp)
      pl = tc.placements(c.m, c.cfg.convergence_threshold, c.cfg.iteration_limit, kinds=("above", "below"))
      for p in pl.values():
        assert tc.hi32(p.theta) == tc.hi32(c.m[p.k - 1])
        grids[exact, p.id] = c.boundary(p)
  for (exact, pid), gr in grids.items():
    if not exact:
      for t in range(T):
        assert np.array_equal(gr[t], grids[True, pid][t]), (pid, t)


@pytest.mark.parametrize("kappa", ["0.9", "2.5", "40"])
def test_two_rows_kernel_every_sweep_just_below_the_threshold(kappa, monkeypatch):
  """k_sweep_two measures max|delta| only in some periods; which sweep is measured behind a measure-free stretch
  depends on the schedule (kappa).  The threshold 1e-10 K below m_k for every k up to the step's natural stop puts each
  sweep in turn inside the thr_far band (a measured max|delta| there, behind unmeasured sweeps, makes the kernel run
  the block again with every period measuring): the step must still end at k + 1."""
  c = _Case("two-SB2-k" + kappa, monkeypatch)
  n0 = tc.natural_stop(c.m, c.cfg.convergence_threshold)
  pl = tc.placements(c.m, c.cfg.convergence_threshold, c.cfg.iteration_limit, kinds=("below",), ks=range(1, n0 + 1))
  assert len(pl) >= n0 - 2, sorted(pl)
  for p in pl.values():
    c.boundary(p, steps=1)


@pytest.mark.parametrize("at_limit", [False, True])
@pytest.mark.parametrize("kind", tc.JACOBI_KINDS)
def test_jacobi_stops_where_float32_rounding_puts_the_threshold(kind, at_limit):
  """k_sweep_jacobi compares the float32 max|delta| with float32(threshold) (NumPy 2 / TF): thresholds at d_k, just
  above and just below the midpoint between d_k and the float32 below it, and at the midpoint (ties to even), with and
  without an iteration limit at k.  Iterations, converged flag and grid bit for bit against the restatement."""
  need_gpu()
  fp, tprev, q, tinf = tc.jacobi_tap()
  cfg = SimConfig.sb1()
  tt = jr.tensors(fp, cfg.time_step_sec, 100.0)
  d = tc.jacobi_series(tt, tprev[0], q[0], tinf[0], cfg.time_step_sec, cfg.iteration_limit)
  k = tc.JACOBI_K
  theta = tc.jacobi_theta(d[k - 1], kind)
  limit = k if at_limit else cfg.iteration_limit
  cfg = dataclasses.replace(cfg, convergence_threshold=theta, iteration_limit=limit)
  sim = BatchedSimulator(fp, cfg, 4, 100.0, solver="jacobi_fp32")
  assert sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI
  grid, iters, conv = sim.tap_jacobi(tprev, q, tinf)
  for b in range(4):
    want, wi, wc = jr.fd_timestep(tt, tprev[b], q[b], tinf[b], cfg.time_step_sec, theta, limit)
    assert (iters[b], bool(conv[b])) == (wi, wc), (b, iters[b], conv[b], wi, wc)
    assert np.array_equal(grid[b].view(np.uint32), want.view(np.uint32)), b
  n, cv = tc.jacobi_expected(d, theta, limit)
  for b in (0, 3):
    assert (iters[b], bool(conv[b])) == (n, cv)
  sim.close()
