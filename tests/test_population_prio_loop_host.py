"""train_lib.run_population_training_loop_vec with an explorer and a prioritized population replay, without a GPU, on the
recording fakes of population_td_fakes.py: the explorer's position in a step's call order, its begin mask (ones, then the last
episode_end), the replay storing the explored action, sample -> update -> set_priority per grouped update (PopulationQTrainer._update
over a recording replay), and exploration=None reproducing the loop's call list without the argument."""
import pytest
import torch

import population_td_fakes as fakes
from balloon_learning_environment_amd import train_lib
from balloon_learning_environment_amd.agents import population, qnet_train

P, R, N, B = fakes.P, fakes.R, fakes.N, fakes.BATCH


class RecordingExplorer:
  """A stand-in for VecPopulationMarcoPoloExploration: records (obs, the actions handed in, begin) and flies action 2 in every
  environment whose number is odd."""

  def __init__(self, log):
    self.log = log

  def __call__(self, obs, actions, begin):
    self.log.append(('marco_polo', obs.clone(), actions.clone(), begin.clone()))
    actions[1::2] = 2
    return actions


def _run(monkeypatch, explorer=True, iterations=2, steps=4, pass_none=False, **kw):
  log = fakes.Log()
  monkeypatch.setattr(qnet_train, 'explore_grouped', fakes.recording_explore(log))
  env, tr, rp = fakes.FakePopEnv(log), fakes.FakePopQTrainer(log), fakes.FakePopReplay(log)
  args = dict(num_iterations=iterations, steps_per_iteration=steps, max_episode_length=fakes.LIMIT, min_replay_history=9, update_period=2,
              target_update_period=6, epsilon=0.0, batch_size=B)
  args.update(kw)
  if explorer:
    args['exploration'] = RecordingExplorer(log)
  elif pass_none:
    args['exploration'] = None
  return log, train_lib.run_population_training_loop_vec(env, tr, rp, **args)


def test_explorer_comes_after_epsilon_greedy_and_before_the_step(monkeypatch):
  log, _ = _run(monkeypatch, iterations=1)
  names = [e[0] for e in log]
  step0 = ['reset', 'act', 'explore', 'marco_polo', 'step', 'add']
  assert names[:6] == step0 and names[6:11] == step0[1:]
  third = names.index('update')
  assert names[third - 5:third + 1] == ['act', 'explore', 'marco_polo', 'step', 'add', 'update']
  assert names.count('marco_polo') == names.count('explore') == names.count('step') == 4
  # epsilon 0 needs no special case: the grouped epsilon-greedy still runs, at rate 0 for every member, keyed by the step
  explores = log.named('explore')
  assert [e[0] for e in explores] == [[0.0, 0.0]] * 4 and [e[2] for e in explores] == [0, 1, 2, 3]
  # the explorer sees the observation acted on and the actions act and epsilon-greedy left
  for k, (ex, mp) in enumerate(zip(explores, log.named('marco_polo'))):
    assert torch.equal(mp[0], torch.full((N, 2), float(k)))
    assert mp[1].tolist() == ex[3].tolist() == [(k + e) % 3 for e in range(N)]


def test_begin_mask_is_ones_then_the_last_episode_end(monkeypatch):
  log, _ = _run(monkeypatch)
  begins = [mp[2] for mp in log.named('marco_polo')]
  ends = [ad[4] for ad in log.named('add')]
  assert len(begins) == len(ends) == 8
  assert begins[0].dtype == torch.uint8 and begins[0].tolist() == [1] * N
  for k in range(1, 8):
    assert begins[k].tolist() == ends[k - 1].tolist(), k
  # every environment's episode ends on its 4th step (the limit): the 5th step begins an episode everywhere, no other does
  assert [b.tolist() for b in begins[1:]] == [[0] * N] * 3 + [[1] * N] + [[0] * N] * 3


def test_replay_stores_the_explored_action(monkeypatch):
  log, _ = _run(monkeypatch, iterations=1)
  for k, (st, ad) in enumerate(zip(log.named('step'), log.named('add'))):
    want = [2 if e % 2 else (k + e) % 3 for e in range(N)]
    assert st[1].tolist() == ad[1].tolist() == want
    assert want != [(k + e) % 3 for e in range(N)]                     # (the explorer changed something at every step)


@pytest.mark.parametrize('pass_none', [False, True])
def test_without_an_explorer_the_call_list_is_todays(monkeypatch, pass_none):
  """exploration=None (given or left out) against the run with an explorer that changes nothing: the same calls with the same tensors,
  the explorer's own entries aside."""
  plain, stats = _run(monkeypatch, explorer=False, pass_none=pass_none, epsilon=[0.0, 0.5])
  names = [e[0] for e in plain]
  assert 'marco_polo' not in names and names[:5] == ['reset', 'act', 'explore', 'step', 'add']

  class Idle(RecordingExplorer):
    def __call__(self, obs, actions, begin):
      self.log.append(('marco_polo',))
      return actions
  log = fakes.Log()
  monkeypatch.setattr(qnet_train, 'explore_grouped', fakes.recording_explore(log))
  env, tr, rp = fakes.FakePopEnv(log), fakes.FakePopQTrainer(log), fakes.FakePopReplay(log)
  with_idle = train_lib.run_population_training_loop_vec(
      env, tr, rp, num_iterations=2, steps_per_iteration=4, max_episode_length=fakes.LIMIT, min_replay_history=9, update_period=2,
      target_update_period=6, epsilon=[0.0, 0.5], batch_size=B, exploration=Idle(log))
  rest = [e for e in log if e[0] != 'marco_polo']
  assert len(rest) == len(plain)
  for a, b in zip(rest, plain):
    assert a[0] == b[0] and len(a) == len(b)
    for x, y in zip(a[1:], b[1:]):
      assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, a[0]
  assert with_idle == stats
  # the schedule of test_population_td_loop_host.py: 1.5 updates per step from the third step on, a sync every third update
  marks = [n for n in names if n in ('add', 'update', 'sync')]
  assert marks.count('update') == 9 and marks.count('sync') == 3 and marks[:4] == ['add', 'add', 'add', 'update']


class RecordingPrioReplay:
  """VecPopulationPrioritizedReplayBuffer's face towards PopulationQTrainer._update."""
  prioritized = True

  def __init__(self, log, members):
    self.log, self.members = log, members

  def sample(self, batch_size, seeds, counter):
    self.log.append(('sample', batch_size, seeds, counter))
    return 'the batch'

  def set_priority(self, batch, loss):
    self.log.append(('set_priority', batch, loss))
    return 'the weighted losses'


def _bare_trainer(log, members):
  """A PopulationQTrainer without a device: _update reads members, seeds, counter and train_on_batch only."""
  tr = population.PopulationQTrainer.__new__(population.PopulationQTrainer)
  tr.members, tr.seeds, tr.counter = members, 'the seeds', 'the counter'
  tr.train_on_batch = lambda batch: log.append(('update', batch)) or 'the losses'
  return tr


def test_a_grouped_update_is_sample_update_set_priority():
  log = fakes.Log()
  tr = _bare_trainer(log, 3)
  assert tr._update(RecordingPrioReplay(log, 3), 32) == 'the weighted losses'
  assert list(log) == [('sample', 32, 'the seeds', 'the counter'), ('update', 'the batch'), ('set_priority', 'the batch', 'the losses')]
  # a uniform population replay: no set_priority, the update's own losses
  log = fakes.Log()
  tr = _bare_trainer(log, 3)
  uniform = RecordingPrioReplay(log, 3)
  uniform.prioritized = False
  assert tr._update(uniform, 32) == 'the losses' and [e[0] for e in log] == ['sample', 'update']


def test_a_plain_prioritized_buffer_or_another_member_count_is_refused_as_before():
  log = fakes.Log()
  tr = _bare_trainer(log, 3)
  message = 'PopulationQTrainer samples a VecPopulationReplayBuffer of its 3 members'

  class Plain:                                                          # VecPrioritizedReplayBuffer: prioritized, no members
    prioritized = True
  for bad in (Plain(), RecordingPrioReplay(log, 2), RecordingPrioReplay(log, 1)):
    with pytest.raises(ValueError, match=message):
      tr._update(bad, 32)
  assert not list(log)
  assert tr._update(RecordingPrioReplay(log, 3), 32) == 'the weighted losses'      # (its own member count: taken)
