"""Episode starts on the GPU (sb_episode_starts_attach; host_inputs.EpisodeStarts through BatchedSimulator and
BatchedEnvironment).

The yardsticks: the values in force against ``EpisodeStarts.values`` (tests/episode_starts_cases.py); an environment with
the starts against a hand-driven twin without them, which gets the same values through set_start_offsets / set_weather;
an environment with ``start_offsets``; plain one-building environments started at the drawn instant.  Both sides run the
same kernels on inputs of the same bits: every comparison is bitwise.

5 to 7 buildings of the 12 x 23 test plan, episodes of 2 to 4 steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sbsim_amd import _ffi, host_inputs  # noqa: E402
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator  # noqa: E402
from sbsim_amd.host_inputs import (Choice, EpisodeRandomization, EpisodeStarts, InitialConditions, Uniform,  # noqa: E402
                                   UniformInt)
from tests import episode_starts_cases as ec  # noqa: E402
from tests import randomization_cases as rc  # noqa: E402
from tests.parity import need_gpu  # noqa: E402

LDS, REG, JACOBI = 0, 1, 7   # sb_sweep_kernel


def _np(t):
  return t.cpu().numpy()


def _actions(n, B, seed=5):
  return torch.tensor(np.random.RandomState(seed).uniform(-1, 1, size=(n, B, 2)).astype(np.float32), device="cuda")


def _assert_in_force(env, es, base, episodes, what, buildings=None):
  """The offsets and weather entries in force are those of ``episodes`` (building b: values(b, episodes[b]))."""
  want = ec.in_force(es, base, episodes, buildings)
  got = env.episode_start_values()
  pick = slice(None) if buildings is None else list(buildings)
  assert set(got) == set(want), (set(got), set(want))
  for name, v in want.items():
    if name == "offsets":
      assert _np(got[name]).astype(np.int64)[pick].tolist() == np.asarray(v)[pick].tolist(), f"{what}: {name} differ"
    else:
      assert ec.same_bits(_np(got[name])[pick], np.asarray(v)[pick]), f"{what}: {name} differ"
  return want


def _held(env):
  """Everything of a building a reset of ANOTHER building must not touch."""
  sim = env.sim
  offs, eff = sim.clock_offsets_in_force()
  vals = env.episode_start_values()
  out = dict(offs=offs, eff=eff, counters=sim.episode_start_episodes(), temps=sim.temps(), scalars=sim.scalars(),
             zone_temps=sim.zone_temps(), modes=sim.modes())
  out.update({k: v for k, v in vals.items() if k != "offsets"})
  return {k: v.clone() for k, v in out.items()}


# ---------------------------------------------------------------- 5. the values in force
def test_values_in_force_are_the_restatement_and_a_partial_reset_touches_no_other_building():
  need_gpu()
  B, plan = 7, rc.plan_small()
  lengths = np.array([2, 3, 4, 2, 3, 4, 2])
  weather, es = ec.sinusoid_weather(B), ec.sinusoid_starts()
  base = ec.base_values(weather, B)
  env = BatchedEnvironment(plan, B, weather=weather, episode_steps=lengths, episode_starts=es, start_timestamp=ec.START, **ec.SHORT)
  sim = env.sim
  assert env.timeline.n_rows == ec.MAX_OFFSET + ec.EPISODE_ROWS + 2
  episodes = np.full(B, -1)
  _assert_in_force(env, es, base, episodes, "attached")             # nothing is drawn before a reset
  assert sim.episode_start_episodes().tolist() == [0] * B
  assert ("episode_starts", es.digest()) in sim.state_fingerprint()
  for n in range(2):
    env.reset()
    episodes += 1
    want = _assert_in_force(env, es, base, episodes, f"reset {n}")
    assert sim.episode_start_episodes().tolist() == [n + 1] * B
    offs, eff = sim.clock_offsets_in_force()
    assert torch.equal(offs, eff)                                   # every building restarts at position 0
    stamps = env.current_simulation_timestamps()
    assert stamps == [ec.START + int(o) * ec.DT for o in want["offsets"]]
  acts = _actions(4, B)
  env.step(acts[0])
  for mask in (np.zeros(B, bool), np.arange(B) == 4, np.arange(B) % 2 == 0, np.ones(B, bool)):
    before = _held(env)
    env.reset_buildings(mask)
    episodes = episodes + mask
    want = _assert_in_force(env, es, base, episodes, f"mask {mask.astype(int)}")
    after = _held(env)
    assert _np(after["counters"]).tolist() == (episodes + 1).tolist()
    assert _np(after["eff"])[mask].tolist() == (want["offsets"][mask] - env._cursor.pos).tolist()   # restart at the batch position
    keep = torch.from_numpy(~mask).cuda()
    for k in before:
      assert torch.equal(before[k][keep], after[k][keep]), (k, mask)
  # the autoreset draws too: three steps end the episodes of length 2 that were reset together just now
  position, ended = np.zeros(B, int), 0
  for n in range(1, 4):
    before = _held(env)
    env.step(acts[n])
    position += 1
    mask = position == lengths + 1
    episodes = episodes + mask
    position[mask] = 0
    ended += int(mask.sum())
    _assert_in_force(env, es, base, episodes, f"step {n}")
    after = _held(env)
    for k in ("offs", "eff", "counters", "weather_low", "weather_high"):
      assert torch.equal(before[k][~torch.from_numpy(mask).cuda()], after[k][~torch.from_numpy(mask).cuda()]), (k, n)
  assert ended == 3
  env.set_episode_starts(None)
  assert not any(isinstance(x, tuple) and x and x[0] == "episode_starts" for x in sim.state_fingerprint())
  env.close()


# ---------------------------------------------------------------- 6. the autoreset against a hand-driven twin
LAYOUTS = {   # name -> (environment variables, BatchedEnvironment arguments, the kernel)
    "register": ((), {}, REG),
    "lds": ((("SBSIM_FORCE_LDS_PATH", "1"),), {}, LDS),
    "jacobi": ((), dict(solver="jacobi_fp32"), JACOBI),
}


@pytest.mark.parametrize("weather_kind", ["sinusoid", "replay"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_autoreset_is_a_twin_given_the_same_values_by_hand(layout, weather_kind, monkeypatch):
  need_gpu()
  env_vars, extra, kernel = LAYOUTS[layout]
  for k, v in env_vars:
    monkeypatch.setenv(k, v)
  B, plan, lengths = 5, rc.plan_small(), ec.LENGTHS
  weather, es, start, top = ec.case(weather_kind, B)
  base = ec.base_values(weather(), B)
  common = dict(ec.SHORT, collect_info=True, start_timestamp=start, **extra)
  a = BatchedEnvironment(plan, B, weather=weather(), episode_steps=lengths, episode_starts=es, **common)
  t = BatchedEnvironment(plan, B, weather=weather(), per_building_episodes=True, max_start_offset=top, **common)
  assert a.sim.launch_info["kernel"] == kernel == t.sim.launch_info["kernel"], (a.sim.launch_info, t.sim.launch_info)
  assert ec.same_bits(a.timeline.rows, t.timeline.rows)

  def give(values, mask):
    """The twin's host route: the masked buildings' values in force, the others' left as they are."""
    t.set_start_offsets(values["offsets"])
    if weather_kind == "sinusoid":
      t.set_weather(low_temps=values["weather_low"], high_temps=values["weather_high"])
    else:
      t.set_weather(offsets_sec=values["weather_shift"])

  episodes = np.zeros(B, int)
  give(ec.in_force(es, base, episodes), np.ones(B, bool))
  ra, rt = a.reset(), t.reset()
  assert torch.equal(ra.observation, rt.observation)
  acts = _actions(12, B)
  position, restarts = np.zeros(B, int), 0
  for n in range(12):
    sa = a.step(acts[n])
    st = t.step(acts[n])   # (the twin's episodes last 16 steps: it is reset by hand alone)
    t_obs, t_rew = st.observation.clone(), st.reward.clone()
    assert torch.equal(sa.reward, t_rew), (layout, n)         # the last step of the old episode ran at the old instant
    position += 1
    mask = position == lengths + 1   # (episode_steps transitions plus the terminal step)
    if mask.any():
      restarts += int(mask.sum())
      episodes = episodes + mask
      position[mask] = 0
      give(ec.in_force(es, base, episodes), mask)
      first = t.reset_buildings(mask).observation
      on, off = torch.from_numpy(mask).cuda(), torch.from_numpy(~mask).cuda()
      assert torch.equal(a.final_observation[on], t_obs[on]), (layout, n)
      assert torch.equal(sa.observation[on], first[on]), (layout, n)
      assert torch.equal(sa.observation[off], t_obs[off]), (layout, n)
    else:
      assert torch.equal(sa.observation, t_obs), (layout, n)
  assert restarts == 4 + 3 + 2 + 4 + 3 and a.sim.episode_start_episodes().tolist() == (episodes + 1).tolist()
  _assert_in_force(a, es, base, episodes, layout)
  assert torch.equal(a.sim.clock_offsets_in_force()[1], t.sim.clock_offsets_in_force()[1])
  assert a.current_simulation_timestamps() == t.current_simulation_timestamps()
  a.close(), t.close()


# ---------------------------------------------------------------- 7. a degenerate draw
@pytest.mark.parametrize("dist", ["choice", "uniform_int"])
def test_a_degenerate_draw_is_start_offsets(dist):
  need_gpu()
  B, plan, k, T = 5, rc.plan_small(), 141, 4     # (141: the comfort switch at row 144 inside every episode)
  short = dict(num_days_in_episode=(T + 0.5) * 300.0 / 86400.0, holiday_calendar=None, start_timestamp=ec.START, collect_info=True)
  es = EpisodeStarts(offsets=Choice([k]) if dist == "choice" else UniformInt(k, k), seed=3)
  a = BatchedEnvironment(plan, B, episode_starts=es, **short)
  t = BatchedEnvironment(plan, B, start_offsets=np.full(B, k), **short)
  assert ec.same_bits(a.timeline.rows, t.timeline.rows)
  acts = _actions(3 * (T + 2), B)
  kinds = []
  for n in range(3 * (T + 2)):   # three episodes: reset, T transitions, the terminal step
    sa, st = a.step(acts[n]), t.step(acts[n])
    kinds.append(int(sa.step_type[0]))
    for name in ("step_type", "reward", "discount", "observation"):
      assert torch.equal(getattr(sa, name), getattr(st, name)), (n, name)
    assert torch.equal(a.info, t.info) and torch.equal(a.sim.temps(), t.sim.temps()), n
  assert kinds == [0, 1, 1, 1, 1, 2] * 3
  assert a.sim.episode_start_episodes().tolist() == [3] * B
  a.close(), t.close()


# ---------------------------------------------------------------- 8. the first episode against plain environments
def test_first_episode_equals_plain_environments_started_at_the_drawn_instant():
  need_gpu()
  B, plan = 5, rc.plan_small()
  weather, es = ec.sinusoid_weather(B), ec.sinusoid_starts()
  env = BatchedEnvironment(plan, B, weather=weather, episode_starts=es, start_timestamp=ec.START, collect_info=True, **ec.SHORT)
  acts = _actions(4, B)
  got = [env.reset().observation.clone()]
  rewards = []
  for n in range(4):
    ts = env.step(acts[n])
    got.append(ts.observation.clone())
    rewards.append(ts.reward.clone())
  env.close()
  drawn = [es.values(b, 0) for b in range(B)]
  assert len({v["offsets"] for v in drawn}) >= 2
  for b, v in enumerate(drawn):
    plain = BatchedEnvironment(plan, 1, weather=host_inputs.BatchedSinusoidWeather([v["weather_low"]], [v["weather_high"]], 100.0),
                               start_timestamp=ec.START + v["offsets"] * ec.DT, collect_info=True, **ec.SHORT)
    assert plain.timeline is None
    assert torch.equal(plain.reset().observation[0], got[0][b]), b
    for n in range(4):
      ts = plain.step(acts[n, b:b + 1].contiguous())
      assert torch.equal(ts.observation[0], got[n + 1][b]) and torch.equal(ts.reward[0], rewards[n][b]), (b, n)
    plain.close()


# ---------------------------------------------------------------- 9. shards
def test_shards_draw_what_the_whole_batch_draws():
  need_gpu()
  B, plan = 6, rc.plan_small()
  lengths = np.array([2, 3, 4, 2, 3, 4])
  es = ec.sinusoid_starts(seed=21)
  w = ec.sinusoid_weather(B)
  part_weather = lambda lo: host_inputs.BatchedSinusoidWeather(w.low[lo:lo + 3], w.high[lo:lo + 3], 100.0)
  common = dict(ec.SHORT, start_timestamp=ec.START)
  whole = BatchedEnvironment(plan, B, weather=w, episode_steps=lengths, episode_starts=es, **common)
  parts = [BatchedEnvironment(plan, 3, weather=part_weather(lo), episode_steps=lengths[lo:lo + 3], episode_starts=es.rows(lo), **common)
           for lo in (0, 3)]
  assert [p.episode_starts.first_building for p in parts] == [0, 3]
  acts = _actions(6, B, seed=6)
  outs = [whole.reset().observation.clone()]
  part_outs = [[p.reset().observation.clone() for p in parts]]
  for n in range(6):
    outs.append(whole.step(acts[n]).observation.clone())
    part_outs.append([p.step(acts[n, lo:lo + 3].contiguous()).observation.clone() for p, lo in zip(parts, (0, 3))])
  for n in range(7):
    assert torch.equal(outs[n], torch.cat(part_outs[n])), n
  vals = whole.episode_start_values()
  for name, v in vals.items():
    assert torch.equal(v, torch.cat([p.episode_start_values()[name] for p in parts])), name
  assert len(set(_np(vals["offsets"]).tolist())) >= 2
  for e in [whole] + parts:
    e.close()


# ---------------------------------------------------------------- 10. independence
def test_the_other_draws_do_not_change_by_one_bit():
  need_gpu()
  B, plan = 5, rc.plan_small()
  er = rc.randomization(materials=True, seed=7)     # parameters and materials, the convection coefficient among them
  ic = InitialConditions(initial_temp=np.linspace(290.0, 296.0, B), jitter=(-0.5, 0.5, 7))   # (the same seed: only the tags differ)
  es = ec.sinusoid_starts(seed=7)
  common = dict(ec.SHORT, start_timestamp=ec.START, episode_steps=ec.LENGTHS, building_params=rc.building_params(B),
                building_materials=rc.building_materials(plan, B), episode_randomization=er, initial_conditions=ic)
  a = BatchedEnvironment(plan, B, weather=ec.sinusoid_weather(B), episode_starts=es, **common)
  t = BatchedEnvironment(plan, B, weather=ec.sinusoid_weather(B), **common)
  seen = []

  def same(what):
    assert torch.equal(a.sim.building_param_rows(), t.sim.building_param_rows()), what
    assert torch.equal(a.sim.building_material_rows(), t.sim.building_material_rows()), what
    assert torch.equal(a.sim.building_coef(), t.sim.building_coef()), what     # (the fold of the material rows)
    va, vt = a.randomized_values(), t.randomized_values()
    assert set(va) == set(vt) and all(torch.equal(va[k], vt[k]) for k in va), what
    seen.append(a.sim.building_material_rows().clone())
    assert torch.equal(a.sim.temps(), t.sim.temps()), what
    assert torch.equal(a.sim.randomization_episodes(), t.sim.randomization_episodes()), what
    assert torch.equal(a.sim.initial_condition_episodes(), t.sim.initial_condition_episodes()), what

  for n in range(2):
    a.reset(), t.reset()
    same(f"reset {n}")
  for mask in (np.arange(B) == 2, np.arange(B) % 2 == 0):
    a.reset_buildings(mask), t.reset_buildings(mask)
    same(f"mask {mask.astype(int)}")
  assert a.sim.episode_start_episodes().tolist() == [3, 2, 4, 2, 3]
  assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])   # (the material rows were re-drawn)
  assert not torch.equal(a.reset().observation, t.reset().observation)     # (the starts did something)
  a.close(), t.close()


# ---------------------------------------------------------------- 11. checkpoint and detach
def test_the_counters_are_the_checkpoint():
  need_gpu()
  B, plan, T = 5, rc.plan_small(), 3
  weather, es = ec.sinusoid_weather(B), ec.sinusoid_starts(seed=44)
  env = BatchedEnvironment(plan, B, weather=weather, episode_starts=es, start_timestamp=ec.START, holiday_calendar=None,
                           num_days_in_episode=(T + 0.5) * 300.0 / 86400.0)
  acts = _actions(12, B, seed=8)
  env.reset()
  for n in range(2):
    env.step(acts[n])
  counters, snap = env.sim.episode_start_episodes().clone(), env.snapshot()
  assert counters.tolist() == [1] * B

  def run_on():
    out = []
    for n in range(2, 12):   # the rest of this episode, the reset, all of the next one, the reset after it
      ts = env.step(acts[n])
      out.append((ts.step_type.clone(), ts.reward.clone(), ts.observation.clone(), env.sim.clock_offsets_in_force()[0].clone()))
    return out

  first = run_on()
  assert env.sim.episode_start_episodes().tolist() == [3] * B
  assert not torch.equal(first[0][3], first[-1][3])     # the offsets in force moved on
  env.restore(snap)
  env.sim.set_episode_start_episodes(counters)
  assert torch.equal(env.sim.episode_start_episodes(), counters)
  _assert_in_force(env, es, ec.base_values(weather, B), np.zeros(B, int), "restored")
  again = run_on()
  for n, (x, y) in enumerate(zip(first, again)):
    assert all(torch.equal(p, q) for p, q in zip(x, y)), n
  # counters of 0: the attached values
  env.sim.set_episode_start_episodes(torch.zeros(B, dtype=torch.int32, device="cuda"))
  _assert_in_force(env, es, ec.base_values(weather, B), np.full(B, -1), "counters 0")
  env.close()


def test_detach_returns_every_building_at_its_next_reset():
  need_gpu()
  B, plan = 5, rc.plan_small()
  weather, es = ec.sinusoid_weather(B), ec.sinusoid_starts(seed=45)
  base = ec.base_values(weather, B, np.array([3, 0, 7, 1, 5]))
  env = BatchedEnvironment(plan, B, weather=weather, episode_steps=ec.LENGTHS, episode_starts=es, start_offsets=base["offsets"],
                           start_timestamp=ec.START, **ec.SHORT)
  env.reset()
  env.step(_actions(1, B)[0])
  drawn = _assert_in_force(env, es, base, np.zeros(B, int), "drawn")
  assert not np.array_equal(drawn["offsets"], base["offsets"])
  with pytest.raises(ValueError, match="set_start_offsets: the attached episode_starts draw offsets"):
    env.set_start_offsets(np.zeros(B, int))
  with pytest.raises(ValueError, match="set_weather: the attached episode_starts draw weather_low"):
    env.set_weather(low_temps=weather.low)
  env.set_episode_starts(None)
  with pytest.raises(ValueError, match="no episode starts"):
    env.sim.episode_start_episodes()
  _assert_in_force(env, es, base, np.zeros(B, int), "detached: the episodes in progress stay")
  mask = np.arange(B) % 2 == 1
  env.reset_buildings(mask)
  _assert_in_force(env, es, base, np.where(mask, -1, 0), "detached: the reset buildings are back")
  env.reset()
  _assert_in_force(env, es, base, np.full(B, -1), "detached: every building is back")
  offs, eff = env.sim.clock_offsets_in_force()
  assert torch.equal(offs, eff) and _np(offs).tolist() == base["offsets"].tolist()
  env.set_start_offsets(np.array([1, 1, 2, 2, 3]))     # the host route is open again
  env.reset()
  assert _np(env.episode_start_values()["offsets"]).tolist() == [1, 1, 2, 2, 3]
  env.close()


def test_new_starts_replace_the_old_and_inherit_the_attached_values():
  """Starts A (offsets and low), then B (high alone): A's fields return to the ATTACHED values at a building's next
  reset, B draws from episode 0; then new starts while a detach is still restoring."""
  need_gpu()
  B, plan = 5, rc.plan_small()
  weather = ec.sinusoid_weather(B)
  base = ec.base_values(weather, B, np.array([3, 0, 7, 1, 5]))
  first = EpisodeStarts(offsets=UniformInt(132, ec.MAX_OFFSET, step=4), weather_low=Uniform(262.0, 269.0), seed=31)
  second = EpisodeStarts(weather_high=Uniform(290.0, 300.0), seed=32)
  third = EpisodeStarts(offsets=Choice([10, 20, 30, 40]), seed=33)
  env = BatchedEnvironment(plan, B, weather=weather, episode_steps=ec.LENGTHS, episode_starts=first, start_offsets=base["offsets"],
                           start_timestamp=ec.START, **ec.SHORT)
  got = lambda: {k: _np(v) for k, v in env.episode_start_values().items()}

  def check(want, what):
    have = got()
    assert have["offsets"].tolist() == np.asarray(want["offsets"]).tolist(), what
    for k in ("weather_low", "weather_high"):
      assert ec.same_bits(have[k], want[k]), (what, k)

  env.reset()
  env.step(_actions(1, B)[0])
  drawn = _assert_in_force(env, first, base, np.zeros(B, int), "the first starts")
  assert not np.array_equal(drawn["offsets"], base["offsets"]) and not ec.same_bits(drawn["weather_low"], base["weather_low"])
  env.set_episode_starts(second)
  assert env.episode_starts is second and ("episode_starts", second.digest()) in env.sim.state_fingerprint()
  assert env.sim.episode_start_episodes().tolist() == [0] * B                 # new starts count from 0
  check(drawn, "replaced: the episodes in progress stay")
  stamps = env.current_simulation_timestamps()
  assert stamps == [ec.START + (int(o) + 1) * ec.DT for o in drawn["offsets"]]   # (still on the drawn rows, one step in)
  mask = np.arange(B) % 2 == 1
  env.reset_buildings(mask)
  want = {k: np.where(mask, base[k], drawn[k]) for k in ("offsets", "weather_low")}
  want["weather_high"] = ec.in_force(second, base, np.where(mask, 0, -1))["weather_high"]
  check(want, "replaced: the reset buildings are on the attached offset and low, and the second starts' high")
  assert not ec.same_bits(want["weather_high"][mask], base["weather_high"][mask])
  assert env.sim.episode_start_episodes().tolist() == mask.astype(int).tolist()
  env.reset()
  want = dict(base, weather_high=ec.in_force(second, base, mask.astype(int))["weather_high"])
  check(want, "replaced: every building")
  offs, eff = env.sim.clock_offsets_in_force()
  assert torch.equal(offs, eff)
  # detach, and new starts before any building has been reset: the high returns to the attached one as well
  env.set_episode_starts(None)
  env.set_episode_starts(third)
  check(want, "a third attachment: the episodes in progress stay")
  env.reset_buildings(mask)
  back = ec.in_force(third, base, np.where(mask, 0, -1))
  check(dict(offsets=back["offsets"], weather_low=base["weather_low"], weather_high=np.where(mask, base["weather_high"], want["weather_high"])),
        "a third attachment: the reset buildings")
  env.reset()
  check(dict(base, offsets=ec.in_force(third, base, mask.astype(int))["offsets"]), "a third attachment: every building")
  with pytest.raises(ValueError, match="offsets: building 0: an episode that starts at the largest possible offset 149 needs"):
    env.set_episode_starts(EpisodeStarts(offsets=UniformInt(0, ec.MAX_OFFSET + 1), seed=1))      # beyond the table there is
  assert env.episode_starts is third
  env.close()


def test_new_starts_are_checked_against_the_replay_trace():
  need_gpu()
  B, plan = 5, rc.plan_small()
  env = BatchedEnvironment(plan, B, weather=ec.replay_weather(B), episode_starts=ec.replay_starts(), start_timestamp=ec.START_TRACE, **ec.SHORT)
  env.reset()
  with pytest.raises(ValueError, match="episode_starts: building 0: with offset 85 and weather shift 7200.0 s drawn, its episode ends at"):
    env.set_episode_starts(EpisodeStarts(offsets=Choice([0, 85]), weather_shift=Choice([0.0, 7200.0]), seed=1))
  assert env.episode_starts.digest() == ec.replay_starts().digest()
  env.set_episode_starts(ec.replay_starts(seed=2))
  env.reset()
  _assert_in_force(env, ec.replay_starts(seed=2), ec.base_values(ec.replay_weather(B), B), np.zeros(B, int), "new starts inside the trace")
  env.close()


def test_the_host_route_applies_at_the_next_reset_and_refuses_what_it_cannot_take():
  need_gpu()
  B, plan = 5, rc.plan_small()
  weather = ec.sinusoid_weather(B)
  low0, high0 = weather.low.copy(), weather.high.copy()
  env = BatchedEnvironment(plan, B, weather=weather, per_building_episodes=True, max_start_offset=20, start_timestamp=ec.START, **ec.SHORT)
  acts = _actions(2, B)
  env.reset()
  env.step(acts[0])
  assert env.current_simulation_timestamps() == [ec.START + ec.DT] * B
  new = np.array([4, 8, 12, 16, 20])
  env.set_start_offsets(new)
  assert env.current_simulation_timestamps() == [ec.START + ec.DT] * B      # the episodes in progress keep their rows
  mask = np.arange(B) % 2 == 0
  env.reset_buildings(mask)
  assert env.current_simulation_timestamps() == [ec.START + (int(new[b]) if mask[b] else 1) * ec.DT for b in range(B)]
  env.step(acts[1])
  assert env.current_simulation_timestamps() == [ec.START + (int(new[b]) + 1 if mask[b] else 2) * ec.DT for b in range(B)]
  env.reset()
  assert env.current_simulation_timestamps() == [ec.START + int(o) * ec.DT for o in new]
  # set_weather's refusals change nothing
  nan = low0.copy()
  nan[3] = float("nan")
  for kw, message in ((dict(offsets_sec=np.zeros(B)), "needs weather=BatchedReplayWeather"),
                      (dict(), "needs weather=BatchedSinusoidWeather"),
                      (dict(low_temps=high0 + 1.0), "set_weather: building 0: low above high"),
                      (dict(high_temps=np.where(np.arange(B) == 2, low0 - 1.0, high0)), "set_weather: building 2: low above high"),
                      (dict(low_temps=low0 + 20.0, high_temps=high0), "set_weather: building 0: low above high"),
                      (dict(low_temps=nan), "low_temps: building 3 is not finite"),
                      (dict(high_temps=high0[:3]), "high_temps must have shape \\[5\\]")):
    with pytest.raises(ValueError, match=message):
      env.set_weather(**kw)
  vals = env.episode_start_values()
  assert ec.same_bits(_np(vals["weather_low"]), low0) and ec.same_bits(_np(vals["weather_high"]), high0)
  assert ec.same_bits(env.weather.low, low0) and ec.same_bits(env.weather.high, high0)
  env.set_weather(low_temps=low0 + 20.0, high_temps=high0 + 20.0)     # (both at once: compared with each other)
  vals = env.episode_start_values()
  assert ec.same_bits(_np(vals["weather_low"]), low0 + 20.0) and ec.same_bits(_np(vals["weather_high"]), high0 + 20.0)
  env.set_weather(low_temps=low0, high_temps=high0)
  # with starts that draw the high, a new low is compared with the high in force on the device
  es = EpisodeStarts(weather_high=Uniform(282.0, 300.0), seed=2)
  env.set_episode_starts(es)
  env.reset()
  high_now = _np(env.episode_start_values()["weather_high"])
  assert ec.same_bits(high_now, [es.values(b, 0)["weather_high"] for b in range(B)])
  with pytest.raises(ValueError, match="set_weather: the attached episode_starts draw weather_high"):
    env.set_weather(high_temps=high0)
  with pytest.raises(ValueError, match="set_weather: building 4: low above high"):
    env.set_weather(low_temps=np.where(np.arange(B) == 4, high_now + 0.5, low0))
  env.set_weather(low_temps=high_now - 0.5)      # above every attached high, below every drawn one
  assert ec.same_bits(_np(env.episode_start_values()["weather_low"]), high_now - 0.5)
  env.close()
  replay = BatchedEnvironment(plan, B, weather=ec.replay_weather(B), start_timestamp=ec.START_TRACE, **ec.SHORT)
  for kw in (dict(low_temps=low0), dict(offsets_sec=np.zeros(B), high_temps=high0)):
    with pytest.raises(ValueError, match="set_weather"):
      replay.set_weather(**kw)
  replay.set_weather(offsets_sec=np.full(B, 60.0))
  assert _np(replay.episode_start_values()["weather_shift"]).tolist() == [60.0] * B
  replay.close()


def test_a_new_clock_table_forgets_the_starts():
  need_gpu()
  B = 4
  sim = BatchedSimulator(rc.plan_two_rooms(), rc.config(), B, rc.H_CONV)
  table, offsets = np.zeros((64, _ffi.SB_CLOCK_FIELDS)), np.zeros(B, dtype=np.int32)
  es = EpisodeStarts(offsets=UniformInt(0, 50), seed=3)
  sim.clock_attach(table, offsets)
  plain = sim.state_fingerprint()
  sim.episode_starts_attach(es)
  assert sim.episode_starts is es and set(sim.state_fingerprint()) == set(plain) | {("episode_starts", es.digest())}
  sim.clock_attach(table, offsets)      # the library drops the starts with the table they indexed
  assert sim.episode_starts is None and sim.state_fingerprint() == plain
  with pytest.raises(ValueError, match="no episode starts"):
    sim.episode_start_episodes()
  sim.reset()
  assert _np(sim.clock_offsets_in_force()[0]).tolist() == [0] * B       # nothing draws any more
  sim.episode_starts_attach(es)
  sim.clock_detach()
  assert sim.episode_starts is None and not any(isinstance(x, tuple) and x and x[0] == "episode_starts" for x in sim.state_fingerprint())
  sim.close()


# ---------------------------------------------------------------- 12. beyond one pass of the capped grid
def test_work_beyond_one_pass_of_the_capped_grid():
  need_gpu()
  plan = rc.plan_two_rooms()
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  one_pass = cus * _ffi.SB_STARTS_BLOCKS_PER_CU * _ffi.SB_STARTS_THREADS
  B = one_pass + 4099
  assert B % 64 != 0 and B < 1_000_000
  sim = BatchedSimulator(plan, rc.config(), B, rc.H_CONV)
  sim.clock_attach(np.zeros((64, _ffi.SB_CLOCK_FIELDS)), np.zeros(B, dtype=np.int32))
  lohi = torch.stack([torch.full((B,), 270.0, dtype=torch.float64, device="cuda"),
                      torch.full((B,), 290.0, dtype=torch.float64, device="cuda")], dim=1).contiguous()
  es = EpisodeStarts(offsets=UniformInt(0, 50), weather_low=Uniform(260.0, 275.0), weather_high=Choice([280.0, 285.0, 300.0]), seed=3)
  sim.episode_starts_attach(es, weather_lohi=lohi)
  sim.reset()
  mask = np.arange(B) % 5 == 2     # set and clear entries in every wavefront
  sim.reset_buildings(mask)
  episodes = mask.astype(int)
  sample = sorted({0, 1, 2, 63, 64, 255, 256, 257, B // 2, B // 2 + 1, one_pass - 1, one_pass, one_pass + 1, one_pass + 2, B - 3, B - 2, B - 1}
                  | set(np.random.RandomState(9).randint(0, B, 24).tolist()))
  offs, eff = (_np(x) for x in sim.clock_offsets_in_force())
  got = _np(lohi)
  for b in sample:
    v = es.values(b, int(episodes[b]))
    assert offs[b] == v["offsets"] == eff[b], b
    assert ec.same_bits(got[b], [v["weather_low"], v["weather_high"]]), b
  assert sim.episode_start_episodes().tolist() == (episodes + 1).tolist()
  sim.close()


# ---------------------------------------------------------------- 13. what the library refuses
def test_device_side_refusals_leave_the_handle_unchanged():
  need_gpu()
  B, plan = 5, rc.plan_small()
  common = dict(ec.SHORT, start_timestamp=ec.START, weather=None)
  make = lambda **kw: BatchedEnvironment(plan, B, **dict(common, weather=ec.sinusoid_weather(B), **kw))
  a, t = make(start_offsets=np.arange(B)), make(start_offsets=np.arange(B))
  plain = make()                                                     # no clock
  a.reset(), t.reset()
  L = _ffi.load()
  err = lambda: (L.sb_last_error() or b"").decode()
  attach = _ffi.episode_starts_entry("sb_episode_starts_attach")
  stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
  out = torch.zeros(B, dtype=torch.int32, device="cuda")
  for name in ("sb_episode_starts_episodes_get", "sb_episode_starts_episodes_set"):
    assert _ffi.episode_starts_entry(name)(a.sim._h, C.c_void_p(out.data_ptr()), stream()) == -5 and "no episode starts" in err()
  lohi = a._weather_lohi.data_ptr()

  def desc(es, lohi_ptr=lohi, **edit):
    d, keep = es.c_desc(lohi_ptr, 0)
    for k, v in edit.items():
      field, attr = k.split("__")
      setattr(d.field[host_inputs.START_FIELDS.index(field)], attr, v)
    return d, keep

  offs = EpisodeStarts(offsets=UniformInt(0, 8), seed=1)
  low = EpisodeStarts(weather_low=Uniform(260.0, 270.0), seed=1)
  pick = EpisodeStarts(offsets=Choice([0, 4, 8]), seed=1)
  low_pick = EpisodeStarts(weather_low=Choice([262.0, 264.0]), seed=1)

  def choice(es, j, v):
    """The descriptor of ``es`` with choice j of its one field replaced (values EpisodeStarts itself refuses)."""
    d, keep = desc(es)
    keep[0][j] = v
    return d, keep

  cases = [(desc(offs, offsets__hi=-1.0, offsets__lo=-3.0), -1, "offsets: lo and hi must be whole numbers of rows in 0 .. 2^22"),
           (desc(offs, offsets__hi=float("nan")), -1, "offsets: lo and hi must be finite"),
           (desc(pick, offsets__n_choices=0), -1, "offsets: a choice needs 1 .. 65,536 values, got 0"),
           (desc(pick, offsets__n_choices=65537), -1, "offsets: a choice needs 1 .. 65,536 values, got 65537"),
           (desc(pick, offsets__choices=None), -1, "offsets: a choice needs 1 .. 65,536 values"),
           (choice(pick, 1, float("nan")), -1, "offsets: choice 1 is not finite"),
           (choice(pick, 2, -4.0), -1, "offsets: choice 2 must be a whole number of rows"),
           (choice(pick, 0, 2.5), -1, "offsets: choice 0 must be a whole number of rows"),
           (choice(pick, 2, 40.0), -1, "building 0: the largest possible offset 40 leaves no two rows"),
           (choice(low_pick, 1, float("inf")), -1, "weather_low: choice 1 is not finite"),
           (choice(low_pick, 1, 279.0), -1, "weather_low: building 0: low can be"),
           (desc(offs, offsets__lo=9.0), -1, "lo 9"),
           (desc(offs, offsets__lo=0.5), -1, "whole numbers"),
           (desc(offs, offsets__step=0), -1, "step must be >= 1"),
           (desc(offs, offsets__hi=float(1 << 22)), -1, "more than 2^22"),
           (desc(offs, offsets__kind=_ffi.SB_RAND_UNIFORM), -1, "not one this field takes"),
           (desc(offs, offsets__hi=40.0), -1, "building 0: the largest possible offset 40 leaves no two rows"),
           (desc(low, weather_low__kind=_ffi.SB_RAND_UNIFORM_INT), -1, "not one this field takes"),
           (desc(low, weather_low__hi=float("inf")), -1, "finite"),
           (desc(low, weather_low__hi=279.0), -1, "weather_low: building 0: low can be"),
           (desc(low, lohi_ptr=0), -1, "weather_lohi_dev"),
           (desc(EpisodeStarts(weather_shift=Choice([0.0]), seed=1)), -1, "weather_offset_dev"),
           (desc(offs, offsets__present=0), -1, "no field is present")]
  for (d, keep), rc_want, message in cases:
    assert attach(a.sim._h, C.byref(d), ) == rc_want and message in err(), (message, err())
  d, keep = desc(offs)
  d.first_building = -1
  assert attach(a.sim._h, C.byref(d)) == -1 and "first_building" in err()
  assert attach(a.sim._h, None) == -1 and "null" in err()
  d, keep = desc(offs)
  assert attach(plain.sim._h, C.byref(d)) == -5 and "no clock" in err()
  # attach while the stream is being captured: refused before the library is called.  (The C entry's own refusal is
  # its hipDeviceSynchronize failing; under the capture mode torch uses that call also invalidates the capture in
  # progress, so no test makes it -- the guard in front of it is what a caller meets.)
  s = torch.cuda.Stream()
  graph = torch.cuda.CUDAGraph()
  scratch = torch.zeros(4, device="cuda")
  with torch.cuda.stream(s):
    graph.capture_begin()
    try:
      scratch.add_(1.0)
      with pytest.raises(ValueError, match="captured"):
        a.sim.episode_starts_attach(offs)
    finally:
      graph.capture_end()
  assert a.sim.episode_starts is None
  set_offsets = _ffi.episode_starts_entry("sb_clock_set_offsets")
  bad = np.array([0, 1, 2, 3, 400], dtype=np.int32)
  assert set_offsets(a.sim._h, bad.ctypes.data_as(C.c_void_p), stream()) == -1 and "building 4" in err()
  assert set_offsets(plain.sim._h, bad.ctypes.data_as(C.c_void_p), stream()) == -5 and "no clock" in err()
  # nothing of this changed the handle: it steps as its twin does
  acts = _actions(2, B)
  for n in range(2):
    sa, st = a.step(acts[n]), t.step(acts[n])
    assert torch.equal(sa.observation, st.observation) and torch.equal(sa.reward, st.reward), n
  assert torch.equal(a.sim.clock_offsets_in_force()[1], t.sim.clock_offsets_in_force()[1])
  # the offsets belong to the starts while they are attached
  a.sim.episode_starts_attach(offs)
  good = np.zeros(B, dtype=np.int32)
  assert set_offsets(a.sim._h, good.ctypes.data_as(C.c_void_p), stream()) == -1 and "draw the offsets" in err()
  for e in (a, t, plain):
    e.close()
