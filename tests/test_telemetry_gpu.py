"""Buildings scored against recorded zone temperatures on the GPU (sb_telemetry_attach; BatchedEnvironment(telemetry=...)).

The scalar and per-zone tables, running and completed, are held EQUAL, bit for bit, to ``host_inputs.TelemetryTwin`` fed
with ``sim.zone_temps()``: the kernel and the twin do the same IEEE double operations in the same order, so there is no
tolerance.  Against the reference: its own recorded day (tests/golden/h2_sb1_r9_random.npz) is the "real building", at
the bar the parity test of that fixture asserts for zone temperatures.  Plans of a few hundred cells and R9, at most 24
steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi  # noqa: E402
from sbsim_amd.environment import (STEP_LAST, BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment,  # noqa: E402
                                   SimConfig)
from sbsim_amd.host_inputs import BuildingMaterials, Telemetry, TelemetryTwin  # noqa: E402
from tests import convection_cases as cc  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.materials_cases import substituted  # noqa: E402
from tests.parity import need_gpu, step_buffers  # noqa: E402
from tests.twins import T_TOL, oracle_twin, plan_from_npz, step_in, step_kwargs  # noqa: E402

NAMES = _ffi.TELEMETRY_SCORE_NAMES
COL = {n: i for i, n in enumerate(NAMES)}
F, ZF = _ffi.SB_TL_FIELDS, _ffi.SB_TL_ZONE_FIELDS
JACOBI = 7   # sb_sweep_kernel
PLANS = {"small": "plan_small_test.npz", "r9": "plan_r9_sb1.npz"}


def _plan(name):
  return plan_from_npz(load(PLANS[name]))


def _bits(x):
  x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
  return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(got, want):
  return np.array_equal(_bits(got), _bits(want))


def _telemetry(B, Z, seed, n_traces=3, n_rows=6, per_zone=True, A=2):
  """3 traces of 6 rows around room temperature with NaNs sprinkled, trace_of mixed, first_row in {0, 2, 5}, weights that
  include a 0 (where there is more than one zone), the recorded setpoints."""
  rs = np.random.RandomState(seed)
  traces = rs.uniform(288.0, 300.0, size=(n_traces, n_rows, Z))
  traces[rs.rand(*traces.shape) < 0.15] = np.nan
  weights = rs.uniform(0.5, 2.0, size=Z)
  if Z > 1:
    weights[Z // 2] = 0.0
  return Telemetry(traces, trace_of=rs.randint(0, n_traces, size=B), first_row=rs.choice([0, 2, 5], size=B), zone_weights=weights,
                   actions=rs.uniform(-1, 1, size=(n_traces, n_rows, A)).astype(np.float32), per_zone=per_zone)


def _env(plan, B, tel, steps=24, **kw):
  args = dict(num_days_in_episode=steps / 288, holiday_calendar=None, collect_info=True, telemetry=tel)
  args.update(kw)
  return BatchedEnvironment(plan, B, **args)


def _tables(env):
  sim = env.sim if hasattr(env, "sim") else env
  return (sim.telemetry_scores(), sim.completed_telemetry_scores(), sim.telemetry_zone_scores(), sim.completed_telemetry_zone_scores())


def _twin_tables(twin):
  return (twin.running, twin.completed, twin.zone_running, twin.zone_completed)


def _equal(env, twin):
  return all(_same(g, w) for g, w in zip(_tables(env), _twin_tables(twin)))


def _spy_zone_means(env, monkeypatch):
  """The zone means of a step, before a same-step masked reset overwrites them for the buildings that ended."""
  seen = {}
  reset_buildings = env.sim.reset_buildings

  def spy(mask, **kw):
    seen["zm"] = env.sim.zone_temps().clone()
    return reset_buildings(mask, **kw)

  monkeypatch.setattr(env.sim, "reset_buildings", spy)
  return seen


# ---------------------------------------------------------------- 1. the kernel against the twin
@pytest.mark.parametrize("plan_name,B", [("small", 7), ("small", 65), ("r9", 7), ("r9", 65)])
def test_every_table_equals_the_twin_after_every_step(plan_name, B, monkeypatch):
  """Z = 2 takes the 16-byte loads, Z = 9 the 8-byte ones; B = 65 crosses a wavefront and leaves a partial one.  Episodes
  of mixed lengths: buildings of one launch stand at different rows, some past the end of their trace, and the same-step
  autoreset closes some and not others.  The actions are the recording's own, from the device."""
  need_gpu()
  plan = _plan(plan_name)
  Z = plan.n_zones
  assert Z == {"small": 2, "r9": 9}[plan_name]
  tel = _telemetry(B, Z, seed=17 + B)
  steps = np.random.RandomState(B).randint(2, 10, size=B)
  env = _env(plan, B, tel, steps=12, episode_steps=steps)
  twin = TelemetryTwin(tel, B, Z)
  seen = _spy_zone_means(env, monkeypatch)
  env.reset()                                          # the first reset: steps == 0, nothing closes
  assert _equal(env, twin)
  overran = closed = 0
  for t in range(12):
    acts = env.telemetry_actions()
    assert np.array_equal(acts.cpu().numpy(), twin.actions()), t
    overran += int((twin.first_row + twin.running[:, 1] >= tel.n_rows).sum())
    seen.clear()
    ts = env.step(acts)
    last = (ts.step_type == STEP_LAST).cpu().numpy()
    twin.step((seen["zm"] if "zm" in seen else env.sim.zone_temps()).cpu().numpy())
    assert np.array_equal(twin.close(last), last)      # every building that ended had stepped
    closed += int(last.sum())
    assert _equal(env, twin), (t, plan_name, B)
  run = env.telemetry_scores().cpu().numpy()
  assert overran > 0 and closed >= B and (twin.completed[:, COL["missing"]] > 0).any() and (twin.completed[:, COL["samples"]] > 0).any()
  assert (run[:, COL["samples"]] + run[:, COL["missing"]] == run[:, COL["steps"]] * Z).all()
  assert (env.completed_telemetry_zone_scores()[:, :, 0].sum(dim=1).cpu().numpy() == twin.completed[:, COL["samples"]]).all()
  env.close()


# ---------------------------------------------------------------- 2. the latch
def test_the_latch(monkeypatch):
  need_gpu()
  B, Z = 7, 2
  tel = _telemetry(B, Z, seed=3)
  env = _env(_plan("small"), B, tel, steps=12, episode_steps=np.full(B, 12))
  twin = TelemetryTwin(tel, B, Z)
  fresh = [t.clone() for t in _tables(env)]
  env.reset()                                          # the first reset closes nothing
  assert all(torch.equal(a, b) for a, b in zip(_tables(env), fresh)) and _equal(env, twin)
  for t in range(3):
    env.step(env.telemetry_actions())
    twin.step(env.sim.zone_temps().cpu().numpy())
  mask = np.array([1, 0, 0, 1, 0, 1, 0], dtype=bool)
  before = [t.cpu().numpy() for t in _tables(env)]
  env.reset_buildings(mask)
  assert np.array_equal(twin.close(mask), mask) and _equal(env, twin)
  for got, was in zip(_tables(env), before):           # an unmasked building: every bit of its four tables
    assert _same(got.cpu().numpy()[~mask], was[~mask])
  assert (env.completed_telemetry_scores()[:, COL["steps"]].cpu().numpy() == 3 * mask).all()
  env.reset_buildings(mask)                            # right behind it: no step since, nothing closes
  assert not twin.close(mask).any() and _equal(env, twin)
  env.reset()                                          # the others close, the masked ones do not close again
  assert np.array_equal(twin.close(), ~mask) and _equal(env, twin)
  env.reset()                                          # two resets in a row close once
  assert _equal(env, twin) and (env.telemetry_scores()[:, COL["episode"]] == 1).all()
  env.close()


def test_a_shared_clock_latches_at_the_next_reset():
  need_gpu()
  B, Z = 5, 2
  tel = _telemetry(B, Z, seed=5)
  for collect_info in (True, False):
    env = _env(_plan("small"), B, tel, steps=3, collect_info=collect_info)
    twin = TelemetryTwin(tel, B, Z)
    env.reset()
    for t in range(4):                                 # 3 steps and the LAST one
      ts = env.step(env.telemetry_actions())
      twin.step(env.sim.zone_temps().cpu().numpy())
    assert (ts.step_type == STEP_LAST).all() and _equal(env, twin)
    assert (env.completed_telemetry_scores()[:, COL["episode"]] == -1).all()   # ended, not closed yet
    env.step(env.telemetry_actions())                  # the reset that follows closes it
    assert twin.close().all() and _equal(env, twin)
    assert (env.completed_telemetry_scores()[:, COL["steps"]] == 4).all() and (env.telemetry_scores()[:, COL["steps"]] == 0).all()
    env.close()


# ---------------------------------------------------------------- 3. checkpoint, detach, not state
def test_get_set_round_trip_detach_and_attach():
  need_gpu()
  B, Z = 7, 2
  tel = _telemetry(B, Z, seed=7)
  env, plain = _env(_plan("small"), B, tel, steps=12), _env(_plan("small"), B, None, steps=12)
  assert env.has_telemetry and not plain.has_telemetry and plain.sim.telemetry is None
  with pytest.raises(ValueError, match="without telemetry"):
    plain.telemetry_scores()
  sim = env.sim
  env.reset(), plain.reset()
  acts = torch.tensor(np.random.RandomState(1).uniform(-1, 1, size=(8, B, 2)).astype(np.float32), device="cuda")
  for t in range(3):
    env.step(acts[t]), plain.step(acts[t])
  env.reset(), plain.reset()
  env.step(acts[3]), plain.step(acts[3])
  saved = [t.clone() for t in _tables(env)]
  assert (saved[1][:, COL["steps"]] == 3).all() and (saved[0][:, COL["steps"]] == 1).all()
  sim.telemetry_attach(tel)                            # attaching again re-initialises
  fresh = TelemetryTwin(tel, B, Z)
  assert _equal(env, fresh)
  for k in range(4):                                   # one table at a time: the other pointer NULL
    args = [None] * 4
    args[k] = saved[k]
    sim.telemetry_set(*args)
    got = _tables(env)
    assert all(torch.equal(got[j], saved[j]) if j <= k else _same(got[j], _twin_tables(fresh)[j]) for j in range(4)), k
  sim.telemetry_set(*saved)
  assert all(torch.equal(a, b) for a, b in zip(_tables(env), saved))
  with pytest.raises(ValueError):
    sim.telemetry_set(saved[0][:, :5])
  with pytest.raises(ValueError):
    sim.telemetry_set()
  sim.telemetry_detach()
  with pytest.raises(ValueError, match="no telemetry"):
    sim.telemetry_scores()
  for t in range(4, 8):                                # detached: what an environment that never attached computes
    a, p = env.step(acts[t]), plain.step(acts[t])
    assert torch.equal(a.observation, p.observation) and torch.equal(a.reward, p.reward) and torch.equal(env.info, plain.info), t
  sim.telemetry_attach(tel)
  assert _equal(env, fresh)
  env.close(), plain.close()


def test_the_tables_are_not_state():
  need_gpu()
  B, Z = 5, 2
  tel = _telemetry(B, Z, seed=9)
  env, plain = _env(_plan("small"), B, tel, steps=12), _env(_plan("small"), B, None, steps=12)
  assert env.sim.state_fingerprint() == plain.sim.state_fingerprint()
  twin = TelemetryTwin(tel, B, Z)
  env.reset()
  env.step(env.telemetry_actions())
  twin.step(env.sim.zone_temps().cpu().numpy())
  snap = env.snapshot()
  for t in range(3):
    env.step(env.telemetry_actions())
    twin.step(env.sim.zone_temps().cpu().numpy())
  after = [t.clone() for t in _tables(env)]
  env.restore(snap)
  assert all(torch.equal(a, b) for a, b in zip(_tables(env), after)) and _equal(env, twin)
  assert (env.telemetry_scores()[:, COL["steps"]] == 4).all()
  env.close(), plain.close()


# ---------------------------------------------------------------- 4. the recorded setpoints
def test_actions_follow_every_buildings_own_row():
  need_gpu()
  B, Z = 65, 2
  tel = _telemetry(B, Z, seed=11)
  steps = np.random.RandomState(4).randint(2, 9, size=B)
  env = _env(_plan("small"), B, tel, steps=12, episode_steps=steps)
  first_row = tel.first_row.astype(np.int64)
  env.reset()
  out = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
  rows_seen = set()
  for t in range(9):
    n = env.telemetry_scores()[:, COL["steps"]].cpu().numpy().astype(np.int64)
    row = np.minimum(first_row + n, tel.n_rows - 1)
    rows_seen |= set(zip(row.tolist(), (first_row + n >= tel.n_rows).tolist()))
    got = env.telemetry_actions(out)
    assert got is out and np.array_equal(out.cpu().numpy(), tel.actions[tel.trace_of, row]), t
    env.step(out)
  assert {r for r, _ in rows_seen} == set(range(tel.n_rows)) and (tel.n_rows - 1, True) in rows_seen   # staggered, and past the end
  with pytest.raises(ValueError):
    env.telemetry_actions(torch.zeros((B, 3), dtype=torch.float32, device="cuda"))
  env.close()


# ---------------------------------------------------------------- 5. the C entries' refusals
def test_c_level_refusals_leave_the_attachment_in_force():
  need_gpu()
  B, Z = 7, 2
  lib = _ffi.load()
  sim = BatchedSimulator(_plan("small"), SimConfig.sb1(), B, 12.0)
  out = torch.zeros((B, F), dtype=torch.float64, device="cuda")
  zout = torch.zeros((B, Z, ZF), dtype=torch.float64, device="cuda")
  aout = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
  p, zp, ap = C.c_void_p(out.data_ptr()), C.c_void_p(zout.data_ptr()), C.c_void_p(aout.data_ptr())
  assert lib.sb_telemetry_get(sim._h, p, None, None) == -5 and b"sb_telemetry_attach" in lib.sb_last_error()
  assert lib.sb_telemetry_zone_get(sim._h, zp, None, None) == -5 and lib.sb_telemetry_actions(sim._h, ap, None) == -5
  assert lib.sb_telemetry_set(sim._h, p, None, None) == -5 and lib.sb_telemetry_detach(sim._h) == 0
  assert lib.sb_telemetry_attach(sim._h, None) == -1 and lib.sb_telemetry_attach(None, None) == -1
  assert lib.sb_telemetry_attach(sim._h, C.byref(_ffi.Telemetry())) == -1                   # no traces
  tel = _telemetry(B, Z, seed=13, per_zone=False)
  tel.actions = None
  sim.telemetry_attach(tel)
  assert lib.sb_telemetry_get(sim._h, None, None, None) == -1 and lib.sb_telemetry_actions(sim._h, None, None) == -1
  assert lib.sb_telemetry_zone_get(sim._h, zp, None, None) == -5 and b"per_zone" in lib.sb_last_error()
  assert lib.sb_telemetry_actions(sim._h, ap, None) == -5 and b"action table" in lib.sb_last_error()
  with pytest.raises(ValueError, match="per_zone"):
    sim.telemetry_zone_scores()
  # refused attaches: the one in force keeps accumulating as before
  twin = TelemetryTwin(tel, B, Z)
  obs, rew, info = step_buffers(sim)
  g = load("h2_sb1_r9_random.npz")
  acts = torch.tensor(np.random.RandomState(2).uniform(-1, 1, size=(B, 2)).astype(np.float32), device="cuda")
  sim.reset()
  sim.step(acts, step_in(g, 100), obs, rew, info)
  twin.step(sim.zone_temps().cpu().numpy())
  traces = np.ascontiguousarray(tel.zone_temps)
  bad_of = np.ascontiguousarray(tel.trace_of.copy())
  bad_of[4] = tel.n_traces
  bad_row = np.ascontiguousarray(tel.first_row.copy())
  bad_row[2] = -1
  inf_traces = traces.copy()
  inf_traces[1, 2, 1] = np.inf
  weights = np.array([1.0, -1.0])
  wrong_actions = np.zeros((tel.n_traces, tel.n_rows, 3), dtype=np.float32)

  def desc(traces=traces, trace_of=None, first_row=None, zone_weights=None, actions=None, n_actions=0):
    d = _ffi.Telemetry()
    d.traces, d.n_traces, d.n_rows, d.per_zone = traces.ctypes.data_as(_ffi._dp), tel.n_traces, tel.n_rows, 1
    if trace_of is not None:
      d.trace_of = trace_of.ctypes.data_as(_ffi._ip)
    if first_row is not None:
      d.first_row = first_row.ctypes.data_as(_ffi._ip)
    if zone_weights is not None:
      d.zone_weights = zone_weights.ctypes.data_as(_ffi._dp)
    if actions is not None:
      d.actions, d.n_actions = actions.ctypes.data_as(C.POINTER(C.c_float)), n_actions
    return d

  for d, text in ((desc(trace_of=bad_of), b"building 4: trace_of 3"), (desc(first_row=bad_row), b"building 2: first_row -1"),
                  (desc(traces=inf_traces), b"trace 1 row 2 zone 1 is infinite"), (desc(zone_weights=weights), b"zone_weights[1]"),
                  (desc(actions=wrong_actions, n_actions=3), b"n_actions is 3")):
    assert lib.sb_telemetry_attach(sim._h, C.byref(d)) == -1 and text in lib.sb_last_error(), (text, lib.sb_last_error())
  d = desc()
  d.n_rows = 0
  assert lib.sb_telemetry_attach(sim._h, C.byref(d)) == -1
  assert lib.sb_telemetry_zone_get(sim._h, zp, None, None) == -5                             # still the attachment without per_zone
  sim.step(acts, step_in(g, 101), obs, rew, info)
  twin.step(sim.zone_temps().cpu().numpy())
  assert _same(sim.telemetry_scores(), twin.running) and (sim.telemetry_scores()[:, COL["steps"]] == 2).all()
  sim.close()


# ---------------------------------------------------------------- 6. the reference as the real building
def test_the_reference_day_scores_at_the_parity_bound_and_other_materials_score_worse():
  """The R9 SB1 building driven as tests/test_gpu_parity.py's one-day rollout drives it (the fixture's own step inputs,
  its ``actions_norm`` through ``telemetry_actions()``), over the first 24 of that test's 288 steps, scored against the
  fixture's ``zone_temp_post``: max_abs_err below tests.twins.T_TOL, the bar that test asserts for zone temperatures.
  Building 1 has the conductivity of material slot 1 (the 0.05 W/m/K layer of the exterior walls) doubled.  Picked on the
  CPU oracle twin first: with that change the twin's zone temperatures leave the recording by 0.8505 K at the first step
  (the largest of the 24 steps; 0.33 K at the third), 8.5e7 times T_TOL; the unchanged twin reproduces the recording
  exactly.  The twin's figure is computed again here and printed."""
  need_gpu()
  g = load("h2_sb1_r9_random.npz")
  plan, cfg = plan_from_npz(load("plan_r9_sb1.npz")), SimConfig.sb1()
  T, B, Z = 24, 2, 9
  assert T <= len(g["n_sweeps"]) == 288 and g["zone_temp_post"].shape == (288, Z) and g["zone_temp_post"].dtype == np.float64
  ids, table = plan.material_slots()
  sets = np.stack([table, table])
  sets[1, 1, 0] *= 2.0
  H, W = plan.shape
  other = oracle_twin(substituted(plan, ids, sets[1]), cfg, np.full(H * W, cfg.initial_temp))
  twin_diff = max(float(np.abs(other.step(**step_kwargs(g, t, t, cfg, g["actions_norm"][t]))["zone_temp_post"] - g["zone_temp_post"][t]).max())
                  for t in range(T))
  print(f"oracle twin with slot 1's conductivity doubled: max |dT_zone| {twin_diff:.4e} K over {T} steps (T_TOL {T_TOL:g})")
  assert twin_diff > 1e6 * T_TOL
  bm = BuildingMaterials(conductivity=sets[:, :, 0], heat_capacity=sets[:, :, 1], density=sets[:, :, 2],
                         convection_coefficient=np.full(B, float(g["h_conv"])))
  sim = BatchedSimulator(plan, cfg, B, float(g["h_conv"]), building_materials=bm)
  sim.telemetry_attach(Telemetry(g["zone_temp_post"], actions=g["actions_norm"], per_zone=True))
  obs, rew, info = step_buffers(sim)
  sim.reset()
  for t in range(T):
    act = sim.telemetry_actions()
    assert np.array_equal(act.cpu().numpy(), np.tile(g["actions_norm"][t].astype(np.float32), (B, 1))), t
    sim.step(act, step_in(g, t), obs, rew, info)
  s = sim.telemetry_scores().cpu().numpy()
  ours, changed = dict(zip(NAMES, s[0])), dict(zip(NAMES, s[1]))
  print(f"ours: max_abs_err {ours['max_abs_err']:.3e} K (row {ours['max_abs_row']:g}, zone {ours['max_abs_zone']:g}), "
        f"MAE {ours['sum_abs_err'] / ours['samples']:.3e}, bias {ours['sum_err'] / ours['samples']:.3e}; "
        f"changed: max_abs_err {changed['max_abs_err']:.3e} K, MAE {changed['sum_abs_err'] / changed['samples']:.3e}")
  assert (s[:, COL["missing"]] == 0).all() and (s[:, COL["samples"]] == T * Z).all() and (s[:, COL["steps"]] == T).all()
  assert 0.0 <= ours["max_abs_err"] < T_TOL
  assert changed["sum_abs_err"] > ours["sum_abs_err"] and changed["max_abs_err"] > 1e6 * T_TOL
  assert abs(changed["max_abs_err"] - twin_diff) < T_TOL    # the device's changed building is the twin's
  zs = sim.telemetry_zone_scores().cpu().numpy()
  assert (zs[:, :, 0] == T).all() and np.allclose(zs[:, :, 2].sum(axis=1), s[:, COL["sum_abs_err"]], rtol=1e-12)
  sim.close()


# ---------------------------------------------------------------- 7. the other solver, the mixed batch
def test_a_jacobi_handle_keeps_the_same_tables():
  need_gpu()
  B = 5
  plan = cc._plan(cc.TINY)
  Z = plan.n_zones
  tel = _telemetry(B, Z, seed=19)
  env = _env(plan, B, tel, steps=12, solver="jacobi_fp32")
  assert env.sim.launch_info["kernel"] == JACOBI
  twin = TelemetryTwin(tel, B, Z)
  env.reset()
  for t in range(8):                                   # past the end of the six rows
    env.step(env.telemetry_actions())
    twin.step(env.sim.zone_temps().cpu().numpy())
    assert _equal(env, twin), t
  assert (env.telemetry_scores()[:, COL["missing"]] >= 2 * Z).all() and (env.telemetry_scores()[:, COL["samples"]] > 0).any()
  env.close()


def test_a_mixed_batch_concatenates_its_classes():
  need_gpu()
  plans = [cc._plan(cc.TINY), _plan("small")]
  counts = [3, 4]
  tels = [_telemetry(n, p.n_zones, seed=23 + n) for p, n in zip(plans, counts)]
  kw = dict(num_days_in_episode=3 / 288, collect_info=True)
  mixed = MixedBatchedEnvironment(list(zip(plans, counts)), telemetry=tels, **kw)
  twins = [TelemetryTwin(tel, n, p.n_zones) for tel, p, n in zip(tels, plans, counts)]
  assert mixed.has_telemetry and mixed.TELEMETRY_SCORE_NAMES is NAMES
  mixed.reset()
  for t in range(6):                                   # 4 steps, the shared reset, one more step
    acts = mixed.telemetry_actions()
    assert np.array_equal(acts.cpu().numpy(), np.concatenate([tw.actions() for tw in twins])), t
    mixed.step(acts)
    if t == 4:
      assert all(tw.close().all() for tw in twins)
    else:
      for tw, e in zip(twins, mixed.envs):
        tw.step(e.sim.zone_temps().cpu().numpy())
    assert _same(mixed.telemetry_scores(), np.concatenate([tw.running for tw in twins])), t
    assert _same(mixed.completed_telemetry_scores(), np.concatenate([tw.completed for tw in twins])), t
    zr, zc = mixed.telemetry_zone_scores(), mixed.completed_telemetry_zone_scores()
    assert [tuple(x.shape) for x in zr] == [(n, p.n_zones, ZF) for p, n in zip(plans, counts)]
    assert all(_same(a, tw.zone_running) and _same(b, tw.zone_completed) for a, b, tw in zip(zr, zc, twins)), t
  assert (mixed.completed_telemetry_scores()[:, COL["steps"]] == 4).all() and (mixed.telemetry_scores()[:, COL["steps"]] == 1).all()
  with pytest.raises(ValueError, match="one host_inputs.Telemetry or None per class"):
    MixedBatchedEnvironment(list(zip(plans, counts)), telemetry=tels[0], **kw)
  plain = MixedBatchedEnvironment(list(zip(plans, counts)), **kw)
  assert not plain.has_telemetry
  mixed.close(), plain.close()
