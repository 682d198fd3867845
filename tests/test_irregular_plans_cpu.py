"""CPU checks of the irregular, mixed-material plans of tests/irregular_plans.py: what the launch planner picks for
each (sb_plan_info, host only), the numbers each plan is built to hit, the refusals, and the NumPy schedule models of
tests/kernel_model.py against the oracle on the plans they fit."""

import numpy as np
import pytest

from oracle import oracle as orc
from sbsim_amd import _ffi
from sbsim_amd.floorplan import jacobi_cv_tensors
from tests import irregular_plans as ip
from tests.twins import oracle_plan_of, plan_info


def _sets(cp) -> int:
  return len({tuple(r[:4]) for r in cp.class_coef})


def _trim(cp):
  """The trim box (rows, columns) of a compiled plan: every cell that is not ambient."""
  coef = cp.class_coef
  amb = np.array([(coef[c, :5] == 0).all() and coef[c, 5] == 1.0 and coef[c, 6] == 0 for c in range(cp.n_classes)])
  inside = ~amb[cp.cell_class.reshape(cp.H, cp.W)]
  rows, cols = np.nonzero(inside.any(axis=1))[0], np.nonzero(inside.any(axis=0))[0]
  return slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1)


@pytest.mark.parametrize("name", list(ip.CASES))
def test_planner_picks_the_pinned_kernel(name, monkeypatch):
  c = ip.CASES[name]
  for k, v in c.env:
    monkeypatch.setenv(k, v)
  fp = ip.device_plan(name)
  cp = fp.compile(ip.DT, ip.H_CONV)
  assert (cp.n_classes, _sets(cp), cp.Z) == (c.n_classes, c.n_sets, c.n_zones)
  rc, info = plan_info(fp, n_obs=3 * cp.Z + 19)
  assert rc == 0, _ffi.load().sb_last_error()
  assert (info["kernel"], info["waves_per_building"]) == (c.kernel, c.waves)
  if c.steps is not None:
    assert info["sweep_steps"] == c.steps
  assert info["lds_bytes_per_workgroup"] <= 160 * 1024
  rs, cs = _trim(cp)
  zl = fp.zone_label[rs, cs]
  assert ((zl[-1] >= 0).any()) == c.zone_in_last_row
  if c.tail_rows:                     # the tail rows are mixed: more than one class, no zone cell
    Hs = zl.shape[0]
    tail = cp.cell_class.reshape(cp.H, cp.W)[rs, cs][Hs - c.tail_rows:]
    assert (zl[Hs - c.tail_rows:] < 0).all()
    for row in tail:
      assert len(set(row.tolist())) >= 3, row


def test_irregular_plans_reach_their_targets():
  """What the cases exist for.  The general k_sweep_two variant and the two-coefficient one are told apart by the
  sweep's steps: the two-coefficient variant shifts the rows by one (a pad row above row 0), so an even number of
  wavefront rows needs one more lane."""
  kernels = {(c.kernel, c.waves) for c in ip.CASES.values()}
  assert {(ip.TWO, 1), (ip.BAND, 2), (ip.BAND, 3), (ip.BAND, 4), (ip.ROLL, 1), (ip.LDS, 1), (ip.STREAM, 1),
          (ip.STREAM, 3)} <= kernels
  for name, rows in (("U", 110), ("wings", 100)):    # general: lane l owns rows 2l, 2l + 1
    assert ip.CASES[name].steps == 76 + (rows + 1) // 2 - 1
  assert ip.CASES["sym-tail"].steps == 76 + (127 + 2) // 2 - 1 + 4 * 2   # sym: 127 wavefront rows + two tail rows
  assert ip.CASES["roll65"].tail_rows == 1 and ip.CASES["roll66"].tail_rows == 2


def test_two_coefficient_check_fails_on_h_ok_alone():
  """two_wings: every cell inside the trim box has bU == bD (or sits in the first / last row), but the passage's
  edge cells have bL != bR away from the box's first and last column -- plan_two must fall back to the general
  variant because of h_ok alone."""
  cp = ip.two_wings().compile(ip.DT, ip.H_CONV)
  rs, cs = _trim(cp)
  cls = cp.cell_class.reshape(cp.H, cp.W)[rs, cs]
  b = cp.class_coef[cls][:, :, :4]
  Hs, Ws = cls.shape
  R, C = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
  v_ok = (b[..., 0] == b[..., 1]) | ((b[..., 0] == 0) & (R == 0)) | ((b[..., 1] == 0) & (R == Hs - 1))
  h_ok = (b[..., 2] == b[..., 3]) | ((b[..., 2] == 0) & (C == 0)) | ((b[..., 3] == 0) & (C == Ws - 1))
  assert v_ok.all() and not h_ok.all()
  assert ip.CASES["wings"].kernel == ip.TWO and ip.CASES["wings"].steps == 76 + 50 - 1


def test_zone_quirks_are_in_the_plan():
  fp = ip.zone_quirks()
  cells = fp.zone_cell_lists()
  d = fp.diffusers.reshape(-1)
  sizes = [len(c) for c in cells]
  assert min(sizes) == 1                                               # a one-CV zone
  assert any(d[c].sum() == 0.0 for c in cells)                         # a zone without a diffuser
  for c in cells:
    assert d[c].sum() == 0.0 or abs(d[c].sum() - 1.0) < 1e-12
  corridor = ip._box(fp, 27, 31, 10, 60)                              # unzoned interior air
  assert (fp.zone_label[corridor] < 0).all() and (fp.conductivity[corridor] == 50.0).all()
  assert (fp.diffusers[corridor] == 0.0).all()


def test_two_room_zone_is_two_components():
  fp = ip.zone_quirks()
  lab = fp.zone_label
  found = False
  for z in range(fp.n_zones):
    m = lab == z
    seen = np.zeros_like(m)
    xs, ys = np.nonzero(m)
    stack = [(xs[0], ys[0])]
    while stack:
      x, y = stack.pop()
      if not (0 <= x < m.shape[0] and 0 <= y < m.shape[1]) or not m[x, y] or seen[x, y]:
        continue
      seen[x, y] = True
      stack += [(x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)]
    found |= bool((m & ~seen).any())
  assert found


def test_plan_no_kernel_holds_is_refused_with_a_message():
  """A 1,100-row irregular plan: more than 1,024 rows in both orientations' streaming form is SB_ERR_TOO_LARGE with
  a message, never a crash; past 255 classes compile() raises ValueError."""
  s = ip.Sketch(1100, 1100).out(300, 800, 300, 800)
  s.rooms((2, 290, 810, 1098), (2, 290, 810, 1098))
  fp = s.plan()
  rc, _ = plan_info(fp, n_obs=22)
  assert rc == -4 and len(_ffi.load().sb_last_error()) > 20
  rc, _ = plan_info(fp.transposed(), n_obs=22)
  assert rc == -4 and len(_ffi.load().sb_last_error()) > 20
  assert ip.u_ladder(255).compile(ip.DT, ip.H_CONV).n_classes == 255
  with pytest.raises(ValueError, match="cell classes"):
    ip.u_ladder(256).compile(ip.DT, ip.H_CONV)


def _inputs(fp, seed):
  rs = np.random.RandomState(seed)
  H, W = fp.shape
  prev = np.clip(293.0 + 1.5 * rs.randn(H, W), 285.0, 300.0)
  qz = rs.uniform(-400.0, 900.0, size=fp.n_zones)
  q = np.zeros((H, W))
  for z, cells in enumerate(fp.zone_cell_lists()):
    q.reshape(-1)[cells] = qz[z] * fp.diffusers.reshape(-1)[cells]
  oplan = oracle_plan_of(fp)
  return prev, q, qz, oplan


@pytest.mark.parametrize("name", ["L", "roll65", "quirks", "wings", "sym-tail", "court190-220cls"])
def test_lds_grid_schedule_models_match_the_oracle(name):
  """model_fd_timestep and FastSweepModel (the LDS-grid kernel's schedule) on compile()'s tables, one step."""
  from tests.kernel_model import FastSweepModel, model_fd_timestep
  fp = ip.device_plan(name)
  dt, h = 300.0, 100.0
  cp = fp.compile(dt, h)
  prev, q, qz, oplan = _inputs(fp, 5)
  ref, n_ref, _ = orc.fd_timestep(oplan, prev, q, 279.5, h, dt, 0.05, 40)
  got, n_got = model_fd_timestep(cp, prev, 279.5, qz, 0.05, 40)
  assert n_got == n_ref and n_ref >= 3
  assert np.abs(got - ref).max() < 1e-10
  fm = FastSweepModel(cp)
  got2, n2 = fm.fd_timestep(prev, 279.5, qz, 0.05, 40)
  assert n2 == n_ref
  assert np.abs(got2 - ref).max() < 1e-10


@pytest.mark.parametrize("name", ["roll65", "roll66", "roll66-31cls", "L", "quirks"])
@pytest.mark.parametrize("schedule", ["tight", "rolling"])
def test_register_schedule_models_match_the_oracle(name, schedule):
  """RegSweepModel (k_sweep_roll's tail recurrence and overlapped sweeps) on the <= 66-row plans, mixed tail rows."""
  from tests.kernel_model import RegSweepModel
  fp = ip.device_plan(name)
  dt, h = 300.0, 100.0
  cp = fp.compile(dt, h)
  m = RegSweepModel(cp)
  assert m.mode == (3 if ip.CASES[name].tail_rows else 1) and m.T == ip.CASES[name].tail_rows
  prev, q, qz, oplan = _inputs(fp, 7)
  ref, n_ref, _ = orc.fd_timestep(oplan, prev, q, 279.5, h, dt, 0.05, 40)
  got, n_got = m.fd_timestep(prev, 279.5, qz, 0.05, 40, schedule=schedule)
  assert n_got == n_ref and n_ref >= 3
  assert np.abs(got - ref).max() < 1e-10


@pytest.mark.parametrize("name", ["L", "U", "court190"])
def test_jacobi_plans_qualify(name):
  """The plans the GPU test runs on k_sweep_jacobi have no two-neighbour CV whose neighbours face each other."""
  jacobi_cv_tensors(ip.plan(name), 300.0, 100.0)
