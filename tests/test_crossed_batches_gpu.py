"""GPU: crossed batch features against per-building oracle twins (tests/crossed_batches.py).  One BatchedEnvironment per
case -- 67 buildings of 493 cells, reset() and 12 steps with the case's partial reset, snapshot / restore and fork in
between -- and after every call EVERY building is held to its own twin, which was computed on the CPU without the library's
clock tables: sweep counts, modes, dampers, request counts, step types, -inf rewards and histogram fractions equal; zone
temperatures and grids within 1e-8 K; energy rates, rewards and the dollars reward's info columns within the bounds of
tests/twins.py and tests/test_reward_function_gpu.py; observation columns equal where they are made of equal
quantities and within one float32 step of the native value and of the result where they are made of a temperature."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment  # noqa: E402
from tests import crossed_batches as cb  # noqa: E402
from tests.parity import need_gpu  # noqa: E402
from tests.reward_cases import SET_FIELDS  # noqa: E402
from tests.twins import RATE_RTOL, REWARD_TOL, T_TOL, rates_match  # noqa: E402

INFO_COLUMNS = dict(zip(SET_FIELDS, range(7, 13)))   # RewardResponse field -> info column (tests/test_reward_function_gpu.py)
B = cb.B


class Worst:
  """The largest difference seen per compared quantity, next to its bound (printed: pytest -s)."""

  def __init__(self):
    self.seen = {}

  def note(self, what, value, bound):
    v, _ = self.seen.get(what, (0.0, bound))
    self.seen[what] = (max(v, float(value)), bound)

  def __str__(self):
    return "; ".join(f"{k} {v:.3g} (bound {b})" for k, (v, b) in self.seen.items())


def _check_rows(layout, got, want, native, rows, what, worst):
  """Observation rows `rows` of got [B, O] against the twins' rows and the float32 native values they came from."""
  assert got.shape[1] == layout.O, (got.shape, layout.O)
  kind = np.array(layout.kind)
  src = np.array(layout.col_source)
  sigma = np.where(src >= 0, layout.sigma[np.maximum(src, 0)], 1.0)
  for b in rows:
    g, w = got[b], want[b]
    exact = kind != "temperature"
    if not np.array_equal(g[exact], w[exact]):
      j = int(np.flatnonzero(exact)[np.argmax(g[exact] != w[exact])])
      name = (layout.fields + layout.aux_names)[j]
      raise AssertionError(f"{what}: building {b}: column {j} ({name}) is {g[j]!r}, the twin's {w[j]!r}")
    t = ~exact
    if t.any():   # one float32 step of the native value through the normaliser, plus one of the result
      nat = native[b][t].astype(np.float32)
      tol = np.spacing(np.abs(nat)).astype(np.float64) / sigma[t] + np.spacing(np.abs(w[t])).astype(np.float64)
      diff = np.abs(g[t].astype(np.float64) - w[t].astype(np.float64))
      worst.note("observation (temperature columns, in float32 steps of the bound)", (diff / tol).max(), 1.0)
      if not (diff <= tol).all():
        j = int(np.flatnonzero(t)[np.argmax(diff / tol)])
        name = (layout.fields + layout.aux_names)[j]
        raise AssertionError(f"{what}: building {b}: column {j} ({name}) is {g[j]!r}, the twin's {w[j]!r}: "
                             f"off by {diff.max():.3g}, allowed {tol[np.argmax(diff / tol)]:.3g}")


def _check_state(env, res, what, worst, rows=None):
  """The device state after a call against every twin's: zone means, modes, dampers, request counts, and the duration
  since the boiler's last action that the last observation stamped."""
  rows = range(B) if rows is None else rows
  sim = env.sim
  zt, modes, sc = sim.zone_temps().cpu().numpy(), sim.modes().cpu().numpy(), sim.scalars().cpu().numpy()
  damper = sim.save_state().zone[:, 2].cpu().numpy()
  for b in rows:
    r = res[b]
    d = np.abs(zt[b] - r["zone_now"]).max()
    worst.note("zone temperature [K]", d, T_TOL)
    assert d < T_TOL, (what, b, d)
    assert np.array_equal(modes[b], r["mode_now"]), (what, b, modes[b], r["mode_now"])
    assert np.array_equal(damper[b], r["damper_now"]), (what, b, damper[b], r["damper_now"])
    assert (int(sc[b, 3]), int(sc[b, 6])) == r["counts_now"], (what, b, sc[b, 3], sc[b, 6], r["counts_now"])
    assert sc[b, 10] == r["duration_now"], (what, b, sc[b, 10], r["duration_now"])   # (whole multiples of the step)


def _check_step(env, sc, ts, res, what, worst):
  info = env.info.cpu().numpy().astype(np.float64)
  reward = ts.reward.cpu().numpy().astype(np.float64)
  step_type, discount = ts.step_type.cpu().numpy(), ts.discount.cpu().numpy()
  obs = ts.observation.cpu().numpy()
  final = env.final_observation.cpu().numpy() if env.final_observation is not None else None
  for b in range(B):
    r = res[b]
    assert (int(info[b, 4]), int(info[b, 5])) == (r["n_sweeps"], r["converged"]), (what, b, info[b, 4:6], r["n_sweeps"])
    assert rates_match(info[b, :4], r["rates"]), (what, b, info[b, :4], r["rates"])
    worst.note("energy rates (relative, above 1 W)", (np.abs(info[b, :4] - r["rates"]) / np.maximum(np.abs(r["rates"]), 1.0)).max(), RATE_RTOL)
    assert (int(step_type[b]), float(discount[b])) == (r["step_type"], r["discount"]), (what, b, step_type[b], discount[b])
    if np.isneginf(r["reward"]):
      assert np.isneginf(reward[b]), (what, b, reward[b])
    elif r["dollars"] is None:
      worst.note("regret reward", abs(reward[b] - r["reward"]), REWARD_TOL)
      assert abs(reward[b] - r["reward"]) < REWARD_TOL, (what, b, reward[b], r["reward"])
    else:
      assert reward[b] == pytest.approx(r["dollars"]["agent_reward_value"], rel=2e-6, abs=0.0), (what, b)
      worst.note("dollars reward (relative)", abs(reward[b] - r["dollars"]["agent_reward_value"]) / abs(r["dollars"]["agent_reward_value"]), 2e-6)
    if r["dollars"] is not None:   # the RewardResponse fields are written whatever became of the request
      for field, col in INFO_COLUMNS.items():
        assert info[b, col] == pytest.approx(r["dollars"][field], rel=2e-6, abs=0.0), (what, b, field)
      assert not info[b, 13:].any(), (what, b)
  _check_rows(sc.layout, obs, [r["obs"] for r in res], [r["obs_native"] for r in res], range(B), what, worst)
  ended = [b for b in range(B) if "final_obs" in res[b]]
  if ended:
    _check_rows(sc.layout, final, {b: res[b]["final_obs"] for b in ended}, {b: res[b]["final_obs_native"] for b in ended},
                ended, what + " (final_observation)", worst)
  _check_state(env, res, what, worst)


@pytest.mark.parametrize("name", list(cb.CASES))
def test_every_building_of_a_crossed_batch_is_its_twin(name, monkeypatch):
  need_gpu()
  t0 = time.time()
  sc = cb.scenario(name)
  want = cb.expected(name)
  monkeypatch.delenv("SBSIM_FORCE_LDS_PATH", raising=False)
  for k, v in sc.switches:
    monkeypatch.setenv(k, v)
  env = BatchedEnvironment(sc.plan, B, **sc.env_kwargs())
  for k, _ in sc.switches:
    monkeypatch.delenv(k)
  lds = sc.case["kernel"] == "lds"
  assert (env.sim.launch_info["kernel"] == 0) == lds and (env.sim.launch_info["path"] == 0) == lds, env.sim.launch_info
  assert env.sim.O == sc.layout.O and env.steps_per_episode == cb.N_EPISODE and env.batch_size == B
  assert [n.replace("/", "_", 1) for n in env.field_names] == sc.layout.fields + sc.layout.aux_names
  worst = Worst()
  acts = torch.tensor(sc.actions, device="cuda")
  # reset(): every building's first observation; then the buildings' own initial grids
  ts = env.reset()
  first = want[0][1]
  assert ts.step_type.tolist() == [cb.STEP_FIRST] * B and ts.reward.tolist() == [0.0] * B and ts.discount.tolist() == [1.0] * B
  _check_rows(sc.layout, ts.observation.cpu().numpy(), [r["obs"] for r in first], [r["obs_native"] for r in first],
              range(B), "reset()", worst)
  env.sim.reset(temps=torch.tensor(sc.init, dtype=torch.float64, device="cuda"))
  snap = None
  for i, (op, res) in enumerate(want[1:-1]):
    what = f"{name}: call {i} ({op.kind}{'' if op.row < 0 else ' ' + str(op.row)})"
    if op.kind == "step":
      rejected = None if op.rejected is None else torch.tensor(op.rejected, device="cuda")
      ts = env.step(acts[op.row], rejected=rejected)
      _check_step(env, sc, ts, res, what, worst)
    elif op.kind == "reset_buildings":
      before = (ts.step_type.clone(), ts.reward.clone(), ts.discount.clone(), ts.observation.clone())
      ts = env.reset_buildings(op.mask)
      rows = [b for b in range(B) if op.mask[b]]
      keep = torch.tensor(~op.mask, device="cuda")
      for got, old in zip((ts.step_type, ts.reward, ts.discount, ts.observation), before):
        assert torch.equal(got[keep], old[keep]), what
      m = torch.tensor(op.mask, device="cuda")
      assert ts.step_type[m].tolist() == [cb.STEP_FIRST] * len(rows) and ts.reward[m].tolist() == [0.0] * len(rows)
      assert ts.discount[m].tolist() == [1.0] * len(rows)
      _check_rows(sc.layout, ts.observation.cpu().numpy(), {b: res[b]["obs"] for b in rows},
                  {b: res[b]["obs_native"] for b in rows}, rows, what, worst)
      stamped = env.sim.scalars().cpu().numpy()[:, 10]   # the reset observation's boiler read: the rewound action age
      assert [stamped[b] for b in rows] == [res[b]["duration_now"] for b in rows], what
    elif op.kind == "snapshot":
      snap = env.snapshot()
    elif op.kind == "restore":
      env.restore(snap)
    elif op.kind == "fork":
      env.fork(torch.tensor(op.src, dtype=torch.int64, device="cuda"))
  grid = env.sim.temps().cpu().numpy().reshape(B, -1)
  d = np.abs(grid - want[-1][1]).max(axis=1)
  worst.note("final grid [K]", d.max(), T_TOL)
  assert (d < T_TOL).all(), (name, int(np.argmax(d)), d.max())
  env.close()
  print(f"\n[{name}] {time.time() - t0:.1f} s, the twins included; {worst}")


def _small_env(**kw):
  sc = cb.scenario("dollars-on-the-clock")
  return BatchedEnvironment(sc.plan, B, num_days_in_episode=(cb.N_EPISODE + 0.5) / 288, start_timestamp=cb.START, **kw)


def test_the_refused_pairs_raise_before_any_step():
  need_gpu()
  lengths = np.full(B, 5)
  device = lambda k: cb.scenario("histograms-per-building")._device_occupancy(k)
  (_, occ_msg), (_, cal_msg), (_, life_msg) = cb.REFUSED
  with pytest.raises(ValueError, match=occ_msg):
    _small_env(occupancy=device(0), episode_steps=lengths)
  calendars = [host_inputs.Calendar(occupancy=device(k)) for k in range(3)]
  with pytest.raises(ValueError, match=cal_msg):
    _small_env(calendars=calendars, calendar_of=np.arange(B) % 3, episode_steps=lengths)
  env = _small_env(episode_steps=lengths)
  env.reset()
  with pytest.raises(ValueError, match=r"snapshot\(\) " + life_msg):
    env.snapshot()
  with pytest.raises(ValueError, match=r"fork\(\) " + life_msg):
    env.fork(torch.arange(B, device="cuda"))
  env.close()
