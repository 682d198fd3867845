"""GPU parity on the irregular, mixed-material plans of tests/irregular_plans.py: every case on the kernel the planner
picks for it (pinned), against the CPU oracle, which reads k, rho, c, the exterior mask, the zones and the diffusers
and never FloorPlan.compile()'s class tables -- so one comparison checks compile(), the planner's tables and the kernel
together.  Sweep counts and converged flags EQUAL, zone and grid temperatures within 1e-8 K, rates and reward at the
suite's tolerances (tests/twins.py).  With notches and courtyards the AC rate also checks the grid mean
behind the recirculation temperature: ambient cells inside the trim box count in it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import BatchedSimulator, SimConfig  # noqa: E402
from tests import irregular_plans as ip  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import check_plan_against_oracle, jacobi_tap_bitwise, need_gpu, step_buffers  # noqa: E402
from tests.twins import T_TOL, assert_step_matches, oracle_twin, step_in, step_kwargs  # noqa: E402

B, T = 4, 8


def _run(name, monkeypatch, **kw):
  c = ip.CASES[name]
  for k, v in c.env:
    monkeypatch.setenv(k, v)
  path = {ip.LDS: 0, ip.STREAM: 2}.get(c.kernel, 1)
  return check_plan_against_oracle(ip.plan(name), c.n_zones, c.orientation, path, monkeypatch, expect_steps=c.steps,
                                   expect_kernel=c.kernel, expect_waves=c.waves, B=B, T=T, **kw)


@pytest.mark.parametrize("name", list(ip.CASES))
def test_case_against_oracle(name, monkeypatch):
  _run(name, monkeypatch)


@pytest.mark.parametrize("name", ["roll65", "roll66", "roll66-31cls"])
@pytest.mark.parametrize("knob", ["SBSIM_ROLL_EXACT", "SBSIM_DEBUG_FORCE_REDO"])
def test_roll_mixed_tail_rows_exact_and_redo(name, knob, monkeypatch):
  """k_sweep_roll's mixed tail rows on its float64 instantiation alone, and with every building sent through the redo
  list (the float64 re-run of a step the fast instantiation could not decide)."""
  monkeypatch.setenv(knob, "1")
  _run(name, monkeypatch)


@pytest.mark.parametrize("name,limit", [("U", 2), ("U", 3), ("zone-tail", 3)])
def test_iteration_limit_on_irregular_plans(name, limit, monkeypatch):
  """A limit that bites on k_sweep_two's general variant and on k_sweep_band's three wavefronts."""
  infos, _ = _run(name, monkeypatch, iteration_limit=limit)
  assert any((i[:, 4] == limit).all() and (i[:, 5] == 0).any() for i in infos)


@pytest.mark.parametrize("name", ["L", "U", "court190", "U-lds"])
def test_set_temps_inside_a_courtyard_plan(name, monkeypatch):
  """Two steps, an edit of interior cells only that changes the grid's sum, two more steps, against oracle twins that
  get the same edit (tests/test_gpu_parity.py's R9 case has no exterior space inside its trim box)."""
  need_gpu()
  c = ip.CASES[name]
  for k, v in c.env:
    monkeypatch.setenv(k, v)
  g = load("h2_sb1_r9_random.npz")
  fp = ip.plan(name)
  H, W = fp.shape
  cfg = SimConfig.sb1()
  rs = np.random.RandomState(17)
  init = np.clip(294.0 + rs.randn(B, 1) + 0.3 * rs.randn(B, H * W), 285.0, 305.0)
  acts = rs.uniform(-1, 1, size=(4, B, 2)).astype(np.float32)
  sim = BatchedSimulator(fp, cfg, B, float(g["h_conv"]), orientation=c.orientation)
  assert (sim.launch_info["kernel"], sim.launch_info["waves_per_building"]) == (c.kernel, c.waves)
  sim.reset(temps=torch.tensor(init, dtype=torch.float64, device="cuda"))
  twins = [oracle_twin(fp, cfg, init[b]) for b in range(B)]
  obs, rew, info = step_buffers(sim)

  def both(t):
    tt = 96 + t
    sim.step(torch.tensor(acts[t], device="cuda"), step_in(g, tt), obs, rew, info)
    i = info.cpu().numpy().astype(np.float64)
    zt, r = sim.zone_temps().cpu().numpy(), rew.cpu().numpy()
    for b in range(B):
      o = twins[b].step(**step_kwargs(g, tt, t, cfg, acts[t, b]))
      assert_step_matches(i[b], zt[b], r[b], o, (t, b))

  both(0)
  both(1)
  grid = sim.temps().cpu().numpy().reshape(B, H, W)
  inside = ~fp.exterior_space
  edit = grid.copy()
  edit[:, inside] += 1.5 + 0.5 * rs.rand(B, int(inside.sum()))   # every interior cell warmer: the sum changes
  edit[:, 10:30, 5:25] -= 2.0 * inside[10:30, 5:25]
  sim.set_temps(torch.tensor(edit, dtype=torch.float64, device="cuda"))
  for b in range(B):
    twins[b].temp[:] = edit[b].reshape(-1)
  assert abs(float(sim.scalars().cpu().numpy()[0, 11]) - edit[0].mean()) < 1e-9
  both(2)
  both(3)
  final = sim.temps().cpu().numpy()
  for b in range(B):
    assert np.abs(final[b].reshape(-1) - twins[b].temp).max() < T_TOL, b
  sim.close()


@pytest.mark.parametrize("name", ["L", "U", "court190"])
@pytest.mark.parametrize("limit", [100, 2])
def test_jacobi_tap_on_irregular_plans_bitwise(name, limit):
  """solver="jacobi_fp32" on the L and courtyard plans: sb_tap_jacobi bitwise against tests/jacobi_restatement.py."""
  need_gpu()
  fp = ip.plan(name)
  cfg = SimConfig.sb1()
  cfg.iteration_limit = limit
  h = 100.0
  sim = BatchedSimulator(fp, cfg, B, h, solver="jacobi_fp32")
  assert sim.launch_info["kernel"] == _ffi.SB_KERNEL_JACOBI
  jacobi_tap_bitwise(sim, fp, cfg, h, seed=3, limit=limit)
  sim.close()
