"""Episodes per building (BatchedEnvironment(per_building_episodes=True / episode_steps=...), sb_reset_buildings,
sb_observe_buildings) on the GPU.  The oracle is the library itself: a partial reset must be a global reset for the
masked buildings and nothing for the rest, and a building with an episode length of its own must live the life of a
building of a plain environment with that length -- both sides run the same arithmetic on inputs of the same bits, so
equality is bitwise (k_sweep_stream excepted: its zone sums use LDS atomics).

Seven buildings, plans of a few hundred cells where the kernel allows, episodes of at most 12 steps."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd.environment import (STEP_FIRST, STEP_LAST, STEP_MID, BatchedEnvironment, BatchedSimulator,  # noqa: E402
                                   GymVectorEnv, MixedBatchedEnvironment, SimConfig)
from sbsim_amd.host_inputs import BuildingMaterials, BuildingParams  # noqa: E402
from tests import handover_cases as hc  # noqa: E402
from tests.golden_util import load  # noqa: E402
from tests.parity import need_gpu  # noqa: E402
from tests.twins import RATE_ATOL, RATE_RTOL, T_TOL, plan_from_npz  # noqa: E402

B, N = 7, 12
DT = dt.timedelta(seconds=300)
SHORT = dict(num_days_in_episode=N / 288)
OFFSETS = np.array([3, 17, 1, 40, 9, 26, 5])          # distinct, non-zero
MASK = np.array([True, False, True, True, False, False, True])
START = dt.datetime(2023, 7, 6, 7, 0, 0)              # the environment's default: the night, eco mode throughout
# 05:30 US/Pacific: with offsets of up to 12 steps the buildings cross the 06:00 switch to comfort mode at different
# positions of their episodes (the previous thermostat update, scal[18], against the plain environment's row lookup)
START_SWITCH = dt.datetime(2023, 7, 6, 12, 30, 0)
REG, LDS, REG_PAIR, ROLL, BAND, STREAM, JACOBI = 1, 0, 2, 3, 5, 6, 7   # sb_sweep_kernel


def _small():
  return plan_from_npz(load("plan_small_test.npz"))


def _params():
  """Rows that a reset must read per building: the AHU and boiler setpoints it restores."""
  return BuildingParams(ahu_heating_air_temp_setpoint=np.linspace(283.0, 289.0, B),
                        boiler_reheat_water_setpoint=np.linspace(330.0, 360.0, B),
                        vav_max_air_flow_rate=np.linspace(0.03, 0.045, B))


def _materials(plan):
  table = plan.material_slots()[1]
  sets = np.stack([table * (np.array([0.2, 3.0, 2.0]) if i % 2 == 0 else np.array([4.0, 0.3, 0.5])) for i in range(B)])
  return BuildingMaterials(conductivity=sets[:, :, 0], heat_capacity=sets[:, :, 1], density=sets[:, :, 2],
                           convection_coefficient=np.linspace(5.0, 150.0, B))


# name -> (plan, environment switches, BatchedEnvironment arguments, kernel, launch_info["path"] or None, bitwise)
LAYOUTS = {
    "small": (_small, (), {}, REG, None, True),
    "small-lds": (_small, (("SBSIM_FORCE_LDS_PATH", "1"),), {}, LDS, None, True),
    "small-stream": (_small, (("SBSIM_FORCE_STREAM_PATH", "1"),), {}, STREAM, None, False),
    "small-jacobi": (_small, (), dict(solver="jacobi_fp32"), JACOBI, 0, True),
    "small-jacobi-global": (_small, (("SBSIM_FORCE_JACOBI_GLOBAL", "1"),), dict(solver="jacobi_fp32"), JACOBI, 2, True),
    "r9-roll": (lambda: plan_from_npz(load("plan_r9_sb1.npz")), (), {}, ROLL, None, True),
    "pair-68x65": (lambda: hc.floor_plan(hc.CASES["pair-68x65"]),
                   hc.CASES["pair-68x65"].env + (("SBSIM_ORIENTATION", "columns"),), {}, REG_PAIR, None, True),
    "band3-193x87": (lambda: hc.floor_plan(hc.CASES["band3-193x87"]), hc.CASES["band3-193x87"].env, {}, BAND, None, True),
    "small-materials": (_small, (), dict(building_materials=True), LDS, None, True),
}


def _make(layout, monkeypatch, n=1, start=START, **kw):
  """n environments of one layout that differ in nothing but **kw's per-environment values (a list per key)."""
  mk_plan, switches, extra, kernel, path, _ = LAYOUTS[layout]
  for k, v in switches:
    monkeypatch.setenv(k, v)
  plan = mk_plan()
  envs = []
  for i in range(n):
    args = dict(SHORT, start_timestamp=start, collect_info=True, holiday_calendar=None, **extra)
    if args.get("building_materials"):
      args["building_materials"] = _materials(plan)
    args.update({k: v[i] for k, v in kw.items()})
    env = BatchedEnvironment(plan, B, **args)
    assert env.sim.launch_info["kernel"] == kernel, (layout, env.sim.launch_info)
    assert path is None or env.sim.launch_info["path"] == path, (layout, env.sim.launch_info)
    envs.append(env)
  return envs


def _outputs(env, ts):
  sim = env.sim
  out = dict(observation=ts.observation, reward=ts.reward, info=env.info, temps=sim.temps(), zone_temps=sim.zone_temps(),
             scalars=sim.scalars(), modes=sim.modes())
  return {k: v.clone() for k, v in out.items()}


def _assert_rows(got, want, rows, bitwise, what):
  idx = torch.as_tensor(np.nonzero(rows)[0], device="cuda")
  for k in got:
    g, w = got[k][idx], want[k][idx]
    if bitwise or k == "modes":
      assert torch.equal(g, w), f"{what}: {k} differs"
    elif k in ("temps", "zone_temps"):
      assert torch.allclose(g, w, rtol=0.0, atol=T_TOL), f"{what}: {k} differs by {(g - w).abs().max().item()}"
    else:
      assert torch.allclose(g.double(), w.double(), rtol=RATE_RTOL, atol=RATE_ATOL), f"{what}: {k} differs"


def _actions(n, seed=3):
  """One action per (position of a building's own episode, building)."""
  return torch.tensor(np.random.RandomState(seed).uniform(-1, 1, size=(n, B, 2)).astype(np.float32), device="cuda")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_partial_reset_is_a_global_reset_for_the_masked_and_nothing_for_the_rest(layout, monkeypatch):
  """A (episodes per building), C and D (plain start_offsets environments) take 5 steps; A.reset_buildings(MASK),
  C.reset(), nothing for D; 6 more steps, every building acting by the position in its own episode: A's masked buildings
  are C's, the others D's, at the reset and after every step.  Then all three reset() and take 3 steps.

  In that last part A's masked buildings are still C's, but its unmasked buildings are D's, not C's: what survives a reset
  depends on the episode before it.  The thermostat modes (with their hysteresis) of a building that ran 11 steps are not
  those of one that was reset after 5 -- measured on the GPU: they differ on the small plan -- and by the feature's own
  rule the boiler's action age rewinds by the building's own 11 steps against C's 6, so the duration its reset
  observation stamps is -10 dt against -5 dt (asserted).  D is the building with A's unmasked buildings' history, and
  the comparison with it is bitwise in every field."""
  need_gpu()
  bitwise = LAYOUTS[layout][5]
  a, c, d = _make(layout, monkeypatch, 3, start_offsets=[OFFSETS] * 3, building_params=[_params()] * 3,
                  per_building_episodes=[True, False, False])
  acts = _actions(11)
  mask_t = torch.as_tensor(MASK, device="cuda")
  every = np.ones(B, dtype=bool)
  ta, tc, td = a.reset(), c.reset(), d.reset()
  _assert_rows(_outputs(a, ta), _outputs(c, tc), every, bitwise, "first reset")
  for t in range(5):
    ta, tc, td = a.step(acts[t]), c.step(acts[t]), d.step(acts[t])
    oa = _outputs(a, ta)
    _assert_rows(oa, _outputs(c, tc), every, bitwise, f"step {t}")
    _assert_rows(oa, _outputs(d, td), every, bitwise, f"step {t} (D)")
  assert a.episode_positions().tolist() == [5] * B
  ta, tc = a.reset_buildings(MASK), c.reset()
  oa, oc, od = _outputs(a, ta), _outputs(c, tc), _outputs(d, td)
  _assert_rows(oa, oc, MASK, bitwise, "partial reset, masked")
  _assert_rows(oa, od, ~MASK, bitwise, "partial reset, unmasked")
  assert ta.step_type.tolist() == [STEP_FIRST if m else STEP_MID for m in MASK]
  assert ta.discount.tolist() == [1.0] * B and torch.equal(ta.reward[mask_t], torch.zeros(int(MASK.sum()), device="cuda"))
  assert a.episode_positions().tolist() == [0 if m else 5 for m in MASK]
  stamps = a.current_simulation_timestamps()
  assert stamps == [START + (int(o) + (0 if m else 5)) * DT for o, m in zip(OFFSETS, MASK)]
  for k in range(6):
    mixed = torch.where(mask_t[:, None], acts[k], acts[5 + k])
    ta, tc, td = a.step(mixed), c.step(acts[k]), d.step(acts[5 + k])
    oa = _outputs(a, ta)
    _assert_rows(oa, _outputs(c, tc), MASK, bitwise, f"step {k} after the partial reset, masked")
    _assert_rows(oa, _outputs(d, td), ~MASK, bitwise, f"step {k} after the partial reset, unmasked")
    assert ta.step_type.tolist() == [STEP_MID] * B
  ta, tc, td = a.reset(), c.reset(), d.reset()
  oa, oc, od = _outputs(a, ta), _outputs(c, tc), _outputs(d, td)
  _assert_rows(oa, oc, MASK, bitwise, "second reset, masked")
  _assert_rows(oa, od, ~MASK, bitwise, "second reset, unmasked")
  # the action age rewound by every building's own steps: the duration the reset observation stamps is (1 - own steps) dt
  assert oa["scalars"][:, 10].tolist() == [(1.0 - (6.0 if m else 11.0)) * 300.0 for m in MASK]
  assert a.episode_positions().tolist() == [0] * B
  assert a.current_simulation_timestamps() == c.current_simulation_timestamps()
  for k in range(3):
    ta, tc, td = a.step(acts[k]), c.step(acts[k]), d.step(acts[k])
    oa = _outputs(a, ta)
    _assert_rows(oa, _outputs(c, tc), MASK, bitwise, f"step {k} after the second reset, masked")
    _assert_rows(oa, _outputs(d, td), ~MASK, bitwise, f"step {k} after the second reset, unmasked")
    for f in ("step_type", "discount"):
      assert torch.equal(getattr(ta, f), getattr(tc, f)), (k, f)
  for e in (a, c, d):
    e.close()


def test_per_building_lengths_against_plain_twins(monkeypatch):
  """episode_steps per building over 30 steps against one plain twin per distinct length L (num_days_in_episode = L / 288,
  driven through step() and its automatic reset()): LAST at the same steps, the reward and final_observation of the twin's
  LAST TimeStep, the twin's following FIRST observation as the returned one, every MID step equal, bitwise; the episode
  positions and time stamps follow the twin's clock.

  Then reset(): by then the batch position (30) lies far beyond the calendar's max(offsets) + N + 2 rows, which a
  restored calendar must not be asked about.  Every building starts over like its twin after the twin's reset(), at the
  reset and for two steps (the shortest episode's MID steps), in every getter."""
  need_gpu()
  steps = np.array([2, 3, 5, 2, 7, 12, 3])
  offs = np.array([0, 3, 6, 9, 12, 1, 4])
  a, = _make("small", monkeypatch, 1, start=START_SWITCH, start_offsets=[offs], episode_steps=[steps],
             building_params=[_params()])
  assert a.per_building_episodes and a.episode_steps.tolist() == steps.tolist() and a.steps_per_episode == N
  acts = _actions(30, seed=11)
  rec = []   # per step: A's TimeStep, final_observation, positions, time stamps
  ta = a.reset()
  first = ta.observation.clone()
  for t in range(30):
    ta = a.step(acts[t])
    rec.append(dict(step_type=ta.step_type.clone(), reward=ta.reward.clone(), discount=ta.discount.clone(),
                    observation=ta.observation.clone(), final=a.final_observation.clone(), info=a.info.clone(),
                    pos=a.episode_positions().copy(), stamps=a.current_simulation_timestamps()))
  assert rec[0]["pos"].dtype == np.int64
  assert a._cursor.seek_args() == (30, 29) and 29 > N + 2   # (beyond the rows one episode reads)
  again = [_outputs(a, a.reset())]
  assert a.episode_positions().tolist() == [0] * B
  for t in range(2):
    again.append(_outputs(a, a.step(acts[t])))
  assert a.episode_positions().tolist() == [2] * B
  a.close()
  n_last = np.zeros(B, dtype=int)
  for L in sorted(set(steps.tolist())):
    rows = np.nonzero(steps == L)[0]
    idx = torch.as_tensor(rows, device="cuda")
    twin = BatchedEnvironment(_small(), B, num_days_in_episode=L / 288, start_timestamp=START_SWITCH, collect_info=True,
                              holiday_calendar=None, start_offsets=offs, building_params=_params())
    tw = twin.reset()
    assert torch.equal(tw.observation[idx], first[idx])
    for t in range(30):
      tw = twin.step(acts[t])
      r = rec[t]
      what = f"L = {L}, step {t}"
      assert tw.step_type[0].item() in (STEP_MID, STEP_LAST)
      assert torch.equal(r["step_type"][idx], tw.step_type[idx]), what
      assert torch.equal(r["reward"][idx], tw.reward[idx]) and torch.equal(r["discount"][idx], tw.discount[idx]), what
      assert torch.equal(r["info"][idx], twin.info[idx]), what
      if tw.step_type[0].item() == STEP_LAST:
        assert torch.equal(r["final"][idx], tw.observation[idx]), what
        n_last[rows] += 1
        tw = twin.step(acts[t])   # the twin's automatic reset: FIRST
        assert tw.step_type[0].item() == STEP_FIRST
      assert torch.equal(r["observation"][idx], tw.observation[idx]), what
      stamps = twin.current_simulation_timestamps()
      for b in rows:
        assert r["stamps"][b] == stamps[b], what
        assert r["pos"][b] == (stamps[b] - START_SWITCH) // DT - offs[b] == (t + 1) % (L + 1), what
    tw = twin.reset()
    for t in range(3):
      _assert_rows(again[t], _outputs(twin, tw), steps == L, True, f"L = {L}, call {t} after the last reset")
      if t < 2:
        tw = twin.step(acts[t])
        assert tw.step_type[0].item() == STEP_MID
    twin.close()
  assert n_last.tolist() == [30 // (int(L) + 1) for L in steps]


def _state(sim, obs):
  out = dict(obs=obs, temps=sim.temps(), zone_temps=sim.zone_temps(), scalars=sim.scalars(), modes=sim.modes(),
             zone_power=sim.zone_power())
  if sim.solver == "gauss_seidel":   # the whole state, scal[16..19] included
    st = sim.save_state()
    out.update(grid=st.grid, zone=st.zone, mode=st.mode, scal=st.scal)
  return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("layout", ["small", "small-jacobi", "r9-roll"])
def test_masked_entries_leave_the_other_buildings_alone(layout, monkeypatch):
  """sb_observe_buildings and sb_reset_buildings: every state getter's output and the observation buffer before and
  after, the unmasked rows bitwise; an all-zero mask changes nothing at all."""
  need_gpu()
  a, = _make(layout, monkeypatch, 1, start_offsets=[OFFSETS], per_building_episodes=[True])
  acts = _actions(4, seed=5)
  ts = a.reset()
  for t in range(4):
    ts = a.step(acts[t])
  sim, obs = a.sim, ts.observation
  si = _ffi.StepIn()
  none, keep = np.zeros(B, dtype=bool), torch.as_tensor(np.nonzero(~MASK)[0], device="cuda")
  touched = torch.as_tensor(np.nonzero(MASK)[0], device="cuda")
  s0 = _state(sim, obs)
  sim.clock_seek(4, 3)
  sim.observe_buildings(none, si, obs)
  sim.reset_buildings(torch.as_tensor(none, device="cuda"), restart_pos=4)
  s1 = _state(sim, obs)
  for k in s0:
    assert torch.equal(s0[k], s1[k]), f"all-zero mask: {k} changed"
  sim.observe_buildings(MASK.astype(np.uint8), si, obs)
  s2 = _state(sim, obs)
  for k in s0:
    assert torch.equal(s0[k][keep], s2[k][keep]), f"sb_observe_buildings: {k} of an unmasked building changed"
  sim.reset_buildings(torch.as_tensor(MASK, device="cuda"), restart_pos=4)
  s3 = _state(sim, obs)
  for k in s0:
    assert torch.equal(s2[k][keep], s3[k][keep]), f"sb_reset_buildings: {k} of an unmasked building changed"
  t0 = a.config.initial_temp
  assert torch.equal(s3["temps"][touched], torch.full_like(s3["temps"][touched], t0))
  assert not torch.equal(s3["temps"][keep], torch.full_like(s3["temps"][keep], t0))
  a.close()


def test_feature_off_and_on_without_an_early_end_agree(monkeypatch):
  """The default environment and one with per_building_episodes=True (no start_offsets: the all-zero calendar) agree
  bitwise on everything 8 steps return."""
  need_gpu()
  off, on = _make("small", monkeypatch, 2, building_params=[_params()] * 2, per_building_episodes=[False, True])
  assert off._cursor is None and off.final_observation is None and not off.per_building_episodes
  assert on.episode_steps.tolist() == [N] * B
  acts = _actions(8, seed=9)
  t0, t1 = off.reset(), on.reset()
  for t in range(9):
    for f in ("step_type", "reward", "discount", "observation"):
      assert torch.equal(getattr(t0, f), getattr(t1, f)), (t, f)
    o0, o1 = _outputs(off, t0), _outputs(on, t1)
    for k in o0:
      assert torch.equal(o0[k], o1[k]), (t, k)
    assert on.current_simulation_timestamps() == off.current_simulation_timestamps()
    assert on.episode_positions().tolist() == off.episode_positions().tolist() == [t] * B
    if t < 8:
      t0, t1 = off.step(acts[t]), on.step(acts[t])
  off.close()
  on.close()


def test_python_refusals(monkeypatch):
  need_gpu()
  plan = _small()
  occ = host_inputs.BatchedRandomizedArrivalDepartureOccupancy(3, 7, 9, 16, 18, 300, seed=5, holiday_calendar=None)
  with pytest.raises(ValueError, match="advances every building's occupants"):
    BatchedEnvironment(plan, B, occupancy=occ, per_building_episodes=True, **SHORT)
  shared = host_inputs.RandomizedArrivalDepartureOccupancy(3, 7, 9, 16, 18, 300, seed=5, holiday_calendar=None)
  with pytest.raises(ValueError, match="one stateful instance"):   # what start_offsets refuses
    BatchedEnvironment(plan, B, occupancy=shared, per_building_episodes=True, **SHORT)
  with pytest.raises(ValueError, match=r"building 1: 13 is outside 1 \.\. 12"):
    BatchedEnvironment(plan, B, episode_steps=[2, 13, 2, 2, 2, 2, 2], **SHORT)
  with pytest.raises(ValueError, match="MixedBatchedEnvironment"):
    MixedBatchedEnvironment([(plan, B)], per_building_episodes=True, **SHORT)
  off, on = _make("small", monkeypatch, 2, per_building_episodes=[False, True])
  with pytest.raises(ValueError, match="per_building_episodes=True"):
    off.reset_buildings(MASK)
  with pytest.raises(ValueError, match=r"reset\(\) first"):
    on.reset_buildings(MASK)
  on.reset()
  for call, what in ((on.snapshot, "snapshot"), (lambda: on.restore(None), "restore"),
                     (lambda: on.fork(torch.arange(B, device="cuda")), "fork")):
    with pytest.raises(ValueError, match=f"{what}.*episode positions are not in the snapshot"):
      call()
  before = _outputs(on, on.reset_buildings(np.zeros(B, dtype=bool)))
  for bad, msg in ((MASK[:-1], "shape"), (np.stack([MASK, MASK]), "shape"), (MASK.astype(np.int32), "bool or uint8"),
                   (MASK.astype(np.float32), "bool or uint8"), (torch.as_tensor(MASK.astype(np.int64), device="cuda"), "bool or uint8"),
                   (torch.ones(B + 1, dtype=torch.bool, device="cuda"), "shape")):
    with pytest.raises(ValueError, match=msg):
      on.reset_buildings(bad)
    with pytest.raises(ValueError, match=msg):
      on.sim.reset_buildings(bad)
    with pytest.raises(ValueError, match=msg):
      on.sim.observe_buildings(bad, _ffi.StepIn(), on._obs)
  with pytest.raises(ValueError, match="out must be"):
    on.sim.observe_buildings(MASK, _ffi.StepIn(), on._obs[:, :-1])
  after = _outputs(on, on.reset_buildings(np.zeros(B, dtype=bool)))
  for k in before:
    assert torch.equal(before[k], after[k]), k
  off.close()
  on.close()


def test_c_refusals_leave_the_handle_unchanged(monkeypatch):
  """Every refusal of the two entries and of sb_clock_seek is SB_ERR_INVALID, decided on the host; afterwards the handle
  steps like an untouched twin."""
  need_gpu()
  lib = _ffi.load()
  reset_b, observe_b = _ffi.episodes_entry("sb_reset_buildings"), _ffi.episodes_entry("sb_observe_buildings")
  err = lambda: lib.sb_last_error().decode()
  a, twin = _make("small", monkeypatch, 2, start_offsets=[OFFSETS] * 2, per_building_episodes=[True, True])
  h, mask = a.sim._h, np.ascontiguousarray(MASK, dtype=np.uint8)
  mp = mask.ctypes.data_as(C.c_void_p)
  stream = lambda: a.sim._stream()
  si = _ffi.StepIn()
  obs = torch.zeros_like(a._obs)
  op = C.c_void_p(obs.data_ptr())
  last = [None]

  def unchanged(fresh=False):
    """Every getter and the observation buffer against the last accepted state (fresh: take it)."""
    now = _state(a.sim, obs)
    if not fresh:
      for k in now:
        assert torch.equal(now[k], last[0][k]), f"a refused call changed {k}"
    last[0] = now

  # before the first sb_reset: sb_create resets once itself, so a handle is in that state only after sb_state_load put a
  # snapshot's "never reset" into it
  st = a.sim.save_state()
  st.clock = (st.clock[0], st.clock[1], 0, 0)
  a.sim.load_state(st)
  unchanged(fresh=True)
  assert reset_b(h, mp, 0, 294.0, None, stream()) == -1 and "sb_reset first" in err()
  unchanged()
  acts = _actions(6, seed=13)
  a.reset(), twin.reset()
  for t in range(3):
    a.step(acts[t]), twin.step(acts[t])
  # (the clock stands at position 2; the table has max(OFFSETS) + N + 2 = 54 rows)
  unchanged(fresh=True)
  assert reset_b(None, mp, 0, 294.0, None, stream()) == -1 and "null" in err()
  assert reset_b(h, None, 0, 294.0, None, stream()) == -1 and "null" in err()
  assert observe_b(h, None, C.byref(si), op, stream()) == -1 and "null" in err()
  assert observe_b(h, mp, None, op, stream()) == -1 and observe_b(h, mp, C.byref(si), None, stream()) == -1
  assert reset_b(h, mp, -1, 294.0, None, stream()) == -1 and "restart_pos must be >= 0" in err()
  unchanged()
  # a restart that leaves a building without two rows: the clock far ahead of the restart position
  lone = np.zeros(B, dtype=np.uint8)
  lone[3] = 1   # offset 40
  lp = lone.ctypes.data_as(C.c_void_p)
  clock_seek = _ffi.clock_entry("sb_clock_seek")
  assert reset_b(h, lp, 13, 294.0, None, stream()) == 0          # building 3 restarts at 13 ...
  unchanged(fresh=True)
  assert clock_seek(h, 12, 11) == -1 and "below a building's restart position 13" in err()   # a seek below it
  assert clock_seek(h, 25, 24) == 0                                # ... its row 40 + 12 = 52 = n_rows - 2
  assert clock_seek(h, 26, 25) == -1 and "runs past the table" in err()
  assert reset_b(h, lp, 0, 294.0, None, stream()) == -1            # restarting it at 0 now: row 40 + 25
  assert "building 3" in err() and "leaves no two rows" in err()
  unchanged()
  # a snapshot does not carry the restart positions: no load between a partial reset and the next sb_reset
  with pytest.raises(_ffi.SbsimError, match="reset by themselves"):
    a.sim.load_state(a.sim.save_state())
  unchanged()
  assert reset_b(h, lp, 24, 294.0, None, stream()) == 0            # (row 41: fine)
  unchanged(fresh=True)
  # a capturing stream
  s = torch.cuda.Stream()
  graph = torch.cuda.CUDAGraph()
  scratch = torch.zeros(4, device="cuda")
  with torch.cuda.stream(s):
    graph.capture_begin()
    try:
      scratch.add_(1.0)
      rc0 = reset_b(h, mp, 25, 294.0, None, C.c_void_p(s.cuda_stream))
      msg0 = err()
      rc1 = observe_b(h, mp, C.byref(si), op, C.c_void_p(s.cuda_stream))
      msg1 = err()
    finally:
      graph.capture_end()
  assert rc0 == -1 and "captured" in msg0 and rc1 == -1 and "captured" in msg1
  assert torch.equal(obs, torch.zeros_like(obs))
  unchanged()
  # the host shadow and the buildings start over with a full reset, after which the handle steps like the twin, which
  # saw none of this
  a.reset(), twin.reset()
  for t in range(3, 6):
    ta, tt = a.step(acts[t]), twin.step(acts[t])
    oa, ot = _outputs(a, ta), _outputs(twin, tt)
    for k in oa:
      assert torch.equal(oa[k], ot[k]), (t, k)
  a.close()
  twin.close()


def test_gym_view(monkeypatch):
  need_gpu()
  steps = np.array([2, 3, 5, 2, 7, 12, 3])
  a, plain = _make("small", monkeypatch, 2, episode_steps=[steps, None])
  va, vp = GymVectorEnv(a), GymVectorEnv(plain)
  acts = _actions(6, seed=17)
  obs, info = va.reset()
  assert set(info) == {"step_type"}
  obs_p, info_p = vp.reset()
  assert torch.equal(obs, obs_p)
  for t in range(6):
    obs, reward, terminated, truncated, info = va.step(acts[t])
    want = [(t + 1) % (int(L) + 1) == 0 for L in steps]
    assert truncated.tolist() == want and not terminated.any()
    assert info["autoreset_mode"] == "same_step" and info["final_obs"] is a.final_observation
    assert info["discount"].tolist() == [0.0 if w else 1.0 for w in want]
    out = vp.step(acts[t])
    assert set(out[4]) == {"step_type", "discount"}                     # what it was
    assert not out[3].any() and not out[2].any()
    if t < 2:   # nobody has restarted yet: the two views agree
      assert torch.equal(obs, out[0]) and torch.equal(reward, out[1])
  term = GymVectorEnv(a, time_limit_is_truncation=False).step(acts[0])
  assert term[2].tolist() == [(7 % (int(L) + 1)) == 0 for L in steps] and not term[3].any()
  a.close()
  plain.close()
