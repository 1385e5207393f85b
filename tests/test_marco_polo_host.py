"""Marco Polo exploration, CPU only: the restatement (marco_polo_host.py) against the reference's own MarcoPoloExploration and
RandomWalkAgent, imported unmodified under oracle/ref_shims with jax.random.uniform / normal patched to return the same injected draws.
Action for action over a few thousand steps, with episodes shorter than 80 steps and longer than 120."""
import collections

import numpy as np
import pytest

import marco_polo_host as mh
import ref_shims

LANES, STEPS = 6, 3000


@pytest.fixture(scope='module')
def reference():
  if not ref_shims.available():
    pytest.skip('the reference tree is not on this machine')
  ref_shims.install()
  import jax
  from balloon_learning_environment.agents import marco_polo_exploration, random_walk_agent
  queue = collections.deque()

  def uniform(key, shape=(), dtype=None, minval=None, maxval=None):
    u = np.float32(queue.popleft())
    if minval is None:
      return np.float64(u)
    return np.float64(max(np.float32(minval), u * (np.float32(maxval) - np.float32(minval)) + np.float32(minval)))

  def normal(key, shape=(), dtype=None):
    return np.float64(queue.popleft())
  saved = jax.random.uniform, jax.random.normal
  jax.random.uniform, jax.random.normal = uniform, normal
  yield marco_polo_exploration, random_walk_agent, queue
  jax.random.uniform, jax.random.normal = saved


def test_against_reference(reference):
  mpe, rwa, queue = reference
  rng = np.random.default_rng(5)
  lanes = []
  for i in range(LANES):
    queue.append(0.5)                                    # the draw RandomWalkAgent.__init__ takes (its target is redrawn at begin)
    lanes.append(mpe.MarcoPoloExploration(3, (1099,), exploratory_episode_probability=0.8,
                                          exploratory_agent_constructor=rwa.RandomWalkAgent, seed=i))
  host = mh.MarcoPolo(LANES, 0.8)
  # episode lengths: short (< 80), middling and long (> 120, several phase changes)
  left = np.zeros(LANES, np.int64)
  seen_short = seen_long = 0
  toggles = 0
  for s in range(STEPS):
    begin = left == 0
    lengths = rng.choice([rng.integers(5, 79), rng.integers(80, 121), rng.integers(121, 400)], size=LANES)
    left = np.where(begin, lengths, left) - 1
    seen_short += int((begin & (lengths < 80)).sum())
    seen_long += int((begin & (lengths > 120)).sum())
    f0 = rng.random(LANES).astype(np.float32) * np.float32(0.8) + np.float32(0.1)
    agent = rng.integers(0, 3, LANES).astype(np.uint8)
    ut, ue, z = mh.u24(rng.random(LANES)), mh.u24(rng.random(LANES)), rng.standard_normal(LANES)
    before = host.exploratory_phase.copy()
    got = host(f0, agent, begin.astype(np.uint8), ut, ue, z)
    toggles += int((before != host.exploratory_phase).sum())
    for i, ref in enumerate(lanes):
      obs = np.zeros(1099, np.float32)
      obs[0] = f0[i]
      if begin[i]:
        queue.extend([float(ut[i]), float(ue[i])])
        want = ref.begin_episode(obs, int(agent[i]))
      else:
        if ref._exploratory_episode and (ref._exploratory_phase or ref._phase_time_elapsed.total_seconds() + 180 >= 4 * 3600):
          queue.append(float(z[i]))                     # (the normal is drawn only in the exploratory phase)
        want = ref.step(0.0, obs, int(agent[i]))
      assert len(queue) == 0 or not ref._exploratory_phase, (s, i)
      queue.clear()
      assert int(want) == int(got[i]), (s, i, begin[i])
      assert bool(ref._exploratory_episode) == bool(host.exploratory_episode[i])
      assert bool(ref._exploratory_phase) == bool(host.exploratory_phase[i]), (s, i)
      assert ref._phase_time_elapsed.total_seconds() == 180 * host.phase_clock[i]
      assert ref._exploratory_agent._time_elapsed.total_seconds() == 180 * host.walk_clock[i]
      assert float(ref._exploratory_agent._target_pressure) == host.target[i], (s, i)
  assert seen_short > 10 and seen_long > 10 and toggles > 50
