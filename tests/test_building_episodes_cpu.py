"""Episodes per building, the host-only pieces: ``host_inputs.check_episode_steps``, ``host_inputs.EpisodeCursor`` against
a per-building brute-force count, and ``_ffi.episodes_entry`` on a library without the entries."""
import numpy as np
import pytest

from sbsim_amd import _ffi, host_inputs
from sbsim_amd.host_inputs import EpisodeCursor, check_episode_steps


def test_check_episode_steps_refusals_name_the_building():
  ok = check_episode_steps([2, 3, 12, 1], 4, 12)
  assert ok.dtype == np.int64 and ok.tolist() == [2, 3, 12, 1]
  assert check_episode_steps(np.array([5, 5], dtype=np.int32), 2, 5).tolist() == [5, 5]
  with pytest.raises(ValueError, match=r"shape \[4\]"):
    check_episode_steps([2, 3, 4], 4, 12)
  with pytest.raises(ValueError, match=r"shape \[2\]"):
    check_episode_steps([[2, 3]], 2, 12)
  with pytest.raises(ValueError, match="integers"):
    check_episode_steps([2.0, 3.0], 2, 12)
  with pytest.raises(ValueError, match="integers"):
    check_episode_steps([True, False], 2, 12)
  with pytest.raises(ValueError, match=r"building 2: 0 is outside 1 \.\. 12"):
    check_episode_steps([2, 3, 0, 4], 4, 12)
  with pytest.raises(ValueError, match=r"building 1: -3 "):
    check_episode_steps([2, -3, 0, 4], 4, 12)
  with pytest.raises(ValueError, match=r"building 3: 13 is outside 1 \.\. 12"):
    check_episode_steps([2, 3, 12, 13], 4, 12)


class _Brute:
  """Every building counted on its own: the steps it has taken in its episode and the batch steps since reset()."""

  def __init__(self, B):
    self.own = [0] * B
    self.batch = 0

  def step(self):
    self.own = [k + 1 for k in self.own]
    self.batch += 1

  def restart(self, mask):
    self.own = [0 if m else k for k, m in zip(self.own, mask)]


def test_cursor_rows_after_restarts_equal_a_brute_force_count():
  B = 7
  rs = np.random.RandomState(5)
  offsets = rs.randint(0, 40, size=B)
  cur, ref = EpisodeCursor(B), _Brute(B)
  assert cur.seek_args() == (0, -1)
  for t in range(60):
    r = cur.rows(offsets)
    assert r["now"].tolist() == [int(o) + k for o, k in zip(offsets, ref.own)]
    assert r["next"].tolist() == [int(o) + k + 1 for o, k in zip(offsets, ref.own)]
    assert cur.positions().tolist() == ref.own and cur.positions().dtype == np.int64
    assert cur.seek_args() == (ref.batch, ref.batch - 1 if t else -1)
    cur.advance()
    ref.step()
    if t % 3 != 1:   # a restart after most steps, also of nobody and of everybody
      mask = rs.rand(B) < (0.0, 0.3, 1.0)[t % 4 % 3]
      cur.restart(mask)
      ref.restart(mask)
      # the library's bound: the batch position never lies below a building's restart position
      assert (cur.restart_pos <= cur.pos).all() and (cur.positions() >= 0).all()


def test_cursor_ended_gives_episodes_of_length_plus_one_steps():
  steps = np.array([1, 2, 3, 5, 12, 2, 7])
  B = len(steps)
  cur = EpisodeCursor(B)
  taken = np.zeros(B, dtype=int)       # steps of the current episode
  lengths = [[] for _ in range(B)]
  for _ in range(80):
    cur.advance()
    taken += 1
    ended = cur.ended(steps)
    assert ended.dtype == bool and ended.shape == (B,)
    # the batch's rule (BatchedEnvironment.step): the step whose count before it had reached the length is LAST
    assert ended.tolist() == [bool(k - 1 >= n) for k, n in zip(taken, steps)]
    for b in np.nonzero(ended)[0]:
      lengths[b].append(int(taken[b]))
      taken[b] = 0
    cur.restart(ended)
  for b in range(B):
    assert lengths[b] and set(lengths[b]) == {int(steps[b]) + 1}, (b, lengths[b])


def test_cursor_reset_restores_everything():
  cur = EpisodeCursor(4)
  for _ in range(5):
    cur.advance()
  cur.restart(np.array([True, False, True, False]))
  cur.advance()
  assert cur.positions().tolist() == [1, 6, 1, 6] and cur.seek_args() == (6, 5)
  cur.reset()
  assert cur.pos == 0 and cur.restart_pos.tolist() == [0, 0, 0, 0] and cur.positions().tolist() == [0, 0, 0, 0]
  assert cur.rows([3, 0, 9, 1])["now"].tolist() == [3, 0, 9, 1]
  # no batch position survives a reset: it may lie beyond the restored calendar (the previous thermostat update is the
  # building's own, on the device)
  assert cur.prev is None and cur.seek_args() == (0, -1)
  for _ in range(40):   # far beyond any episode length: the batch runs on across the buildings' restarts
    cur.advance()
    cur.restart(cur.ended([3, 3, 3, 3]))
  assert cur.seek_args() == (40, 39) and cur.positions().max() <= 4
  cur.reset()
  assert cur.seek_args() == (0, -1)
  assert not cur.ended([1, 1, 1, 1]).any()


def test_episodes_entry_asks_for_a_rebuild_on_a_library_without_the_entries(monkeypatch):
  class Stub:   # a library of the same ABI version built before the entries existed
    def sb_reset(self):
      pass
  monkeypatch.setattr(_ffi, "_lib", Stub())
  for name in _ffi.EPISODES_ENTRIES:
    with pytest.raises(_ffi.SbsimError, match=f"has no {name}: rebuild"):
      _ffi.episodes_entry(name)
  assert set(_ffi.EPISODES_ENTRIES) == {"sb_reset_buildings", "sb_observe_buildings"} <= set(_ffi.EXPORTS)


class _EpisodesEnv:   # what the refusals look at
  per_building_episodes = True
  start_offsets = None

  def action_spec(self):
    raise AssertionError("refused before anything is asked of the environment")

  observation_spec = action_spec


def test_next_step_consumers_refuse_an_environment_with_episodes_per_building(tmp_path):
  from sbsim_amd import adapters, episode_writer
  with pytest.raises(ValueError, match="tf_agents_environment has next-step autoreset semantics"):
    adapters.tf_agents_environment(_EpisodesEnv())
  with pytest.raises(ValueError, match="gymnasium_vector_env has next-step autoreset semantics"):
    adapters.gymnasium_vector_env(_EpisodesEnv())
  with pytest.raises(ValueError, match="BuildingLogger stamps one time on a whole step.*per_building_episodes"):
    episode_writer.BuildingLogger(_EpisodesEnv(), str(tmp_path), [0])
