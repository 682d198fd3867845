"""GPU: the device convection shuffle on its own, bit for bit against its restatement (tests/convection_cases.py).

Route: phase 4 alone.  After `reset()`, `set_temps(grid)` puts the case's distinct values into the state, and
`step(..., phases=4)` launches sb_launch_convection and k_post only (runtime.hip, sb_step_phases) -- no k_pre, no sweep.
k_post (sb_device.h, post_building) reads and writes per-building scalars, zone means, reward, info and the observation
row; it does not touch the grid, and everything it reads was zeroed when the handle was created, so the phase is safe
after a reset.  One thing follows from it: k_post records the step's ambient temperature as the value of exterior space,
and without k_pre that is the 0.0 the handle was created with -- on the register layouts, which keep no exterior ring in
the state, `temps()` then reports 0.0 there.  So the inputs hold AMBIENT = 0.0 in exterior space (a stray write there
still shows on the LDS layouts, which do store those cells); every other cell, walls included, holds a value of its
own.  Then `temps()` must be np.array_equal to ConvectionOracle.apply of the input: every building, every call, no
tolerance.

The CPU companion tests/test_convection_cases_cpu.py proves that the cases reach the instantiations, branches, list
links and hops they name."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from tests import convection_cases as cc  # noqa: E402
from tests.parity import need_gpu  # noqa: E402


class _Shuffler:
  """A simulator of the case's plan whose every `shuffle()` is one launch of the device shuffle."""

  def __init__(self, case, monkeypatch, B=None, cus="case", attach=True, first_building=None):
    for k in (cc.SWITCH, cc.Q_SWITCH):
      monkeypatch.delenv(k, raising=False)
    env = cc.case_env(case)
    if cus != "case":
      env.pop(cc.SWITCH, None)
      if cus is not None:
        env[cc.SWITCH] = str(cus)
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    self.case, self.fp, self.B = case, cc.floor_plan(case), case.B if B is None else B
    self.sim = BatchedSimulator(self.fp, SimConfig.sb1(), self.B, 100.0, orientation=case.orientation)
    info = self.sim.launch_info
    if case.pin is not None:
      assert (info["kernel"], info["path"], info["waves_per_building"]) == case.pin, info
    assert self.sim.transposed == (case.orientation == "columns")
    self.sim.reset()
    if attach:
      self.sim.convection_attach(case.p, case.distance, seed=case.seed,
                                 first_building=case.first_building if first_building is None else first_building)
    self.obs = torch.zeros((self.B, self.sim.O), dtype=torch.float32, device="cuda")
    self.rew = torch.zeros((self.B,), dtype=torch.float32, device="cuda")
    self.si = _ffi.StepIn()
    self.si.has_action = 0

  def put(self, grids):
    """(the reset gives exterior space its AMBIENT on the register layouts, which sb_set_temps leaves alone there)"""
    t = torch.tensor(grids, dtype=torch.float64, device="cuda")
    self.sim.reset(temps=t.reshape(self.B, -1))
    self.sim.set_temps(t)
    assert np.array_equal(self.sim.temps().cpu().numpy(), grids)   # what goes in comes out

  def shuffle(self):
    self.sim.step(None, self.si, self.obs, self.rew, None, phases=4)
    return self.sim.temps().cpu().numpy()

  def close(self):
    self.sim.close()


def _assert_equal(got, want, what):
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    raise AssertionError(f"{what}: {len(bad)} cells differ in buildings {sorted(set(bad[:, 0].tolist()))[:12]}, "
                         f"first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


@pytest.mark.parametrize("name", list(cc.CASES))
def test_device_shuffle_is_the_restatements_permutation(name, monkeypatch):
  need_gpu()
  case = cc.CASES[name]
  s = _Shuffler(case, monkeypatch)
  start = cc.input_grids(s.fp, case.B)
  s.put(start)
  before = start
  for k, want in enumerate(cc.expected(case)):
    got = s.shuffle()
    _assert_equal(got, want, f"{name}, call {k}")
    assert not np.array_equal(got, before)
    before = got
  s.close()


@pytest.mark.parametrize("name", [n for n, c in cc.CASES.items() if c.group == "handover"])
def test_same_answer_whoever_runs_the_building(name, monkeypatch):
  """The hand-over batch on the whole device (one building per workgroup), and in two halves as simulators of their own
  with first_building moved to the half's start: bitwise the answer of the one-CU run, i.e. the restatement's."""
  need_gpu()
  case = cc.CASES[name]
  want = cc.expected(case)[0]
  start = cc.input_grids(cc.floor_plan(case), case.B)
  whole = _Shuffler(case, monkeypatch, cus=None)
  whole.put(start)
  _assert_equal(whole.shuffle(), want, f"{name}, whole device")
  whole.close()
  cut = case.B // 2
  for lo, hi in ((0, cut), (cut, case.B)):
    half = _Shuffler(case, monkeypatch, B=hi - lo, first_building=case.first_building + lo)
    half.put(start[lo:hi])
    _assert_equal(half.shuffle(), want[lo:hi], f"{name}, buildings {lo}..{hi - 1}")
    half.close()


def test_reattach_resets_the_call_number_and_replaces_the_tables(monkeypatch):
  """One simulator, attached four times in a row (offset table, by-rank window, whole room, a smaller table), two
  launches after each: every one equals a fresh restatement's calls 0 and 1."""
  need_gpu()
  base = cc.CASES["calls3-d5"]
  s = _Shuffler(base, monkeypatch, attach=False)
  grids = cc.input_grids(s.fp, base.B)
  s.put(grids)
  for p, distance, seed in cc.REATTACH:
    case = cc.dataclasses.replace(base, p=p, distance=distance, seed=seed)
    s.sim.convection_attach(p, distance, seed=seed, first_building=case.first_building)
    o = cc.oracle(case)
    for call in range(2):
      o.apply(grids)
      _assert_equal(s.shuffle(), grids, f"p = {p}, distance = {distance}, call {call}")
  s.close()


def test_refusals(monkeypatch):
  """A room of 2048 cells at attach; one building past 2^32 at attach; a forced Q too small for the largest room at the
  launch, which then does not happen: the grid stays."""
  need_gpu()
  big = cc.Case("refused", "q", cc.REFUSED_ROOM, 1.0, 5, (cc.TABLE,), "", 8, B=1)
  s = _Shuffler(big, monkeypatch, attach=False)
  for p, distance in ((1.0, 5), (0.5, -1), (1.0, -1)):
    with pytest.raises(_ffi.SbsimError, match="more than 2047 cells"):
      s.sim.convection_attach(p, distance, seed=1)
  s.close()
  edge = cc.CASES["first-max-d5"]
  s = _Shuffler(edge, monkeypatch, attach=False)
  with pytest.raises(_ffi.SbsimError, match="reaches beyond"):
    s.sim.convection_attach(edge.p, edge.distance, seed=edge.seed, first_building=edge.first_building + 1)
  s.close()
  plan, q = cc.TOO_SMALL_Q
  small = cc.dataclasses.replace(cc.CASES["q3-600cells"], q=q, force_q=True)
  assert small.plan == plan
  s = _Shuffler(small, monkeypatch)
  start = cc.input_grids(s.fp, small.B)
  s.put(start)
  with pytest.raises(_ffi.SbsimError, match="room too large for one workgroup"):
    s.shuffle()
  assert np.array_equal(s.sim.temps().cpu().numpy(), start)
  s.close()
