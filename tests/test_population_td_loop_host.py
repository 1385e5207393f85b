"""train_lib.run_population_training_loop_vec without a GPU, on the recording fakes of population_td_fakes.py: Dopamine's
schedule applied PER MEMBER -- a vector step gives each of the P members R transitions, not P R --, the carried fraction of the update
count, the target sync every target_update_period // update_period UPDATES, min_replay_history per member, the epsilon ladder and the
per-member seeds reaching explore_grouped, the call order of a step, the stats, and the PBT round's copies and lineage."""
import pytest
import torch

import population_td_fakes as fakes
from balloon_learning_environment_amd import train_lib
from balloon_learning_environment_amd.agents import qnet_train

P, R, N, B = fakes.P, fakes.R, fakes.N, fakes.BATCH


def _run(monkeypatch, iterations=2, steps=4, **kw):
  log = fakes.Log()
  monkeypatch.setattr(qnet_train, 'explore_grouped', fakes.recording_explore(log))
  env, tr, rp = fakes.FakePopEnv(log), fakes.FakePopQTrainer(log), fakes.FakePopReplay(log)
  # R = 3 transitions per member and step; one update per 2 transitions: 1.5 updates per step; a sync every 6 // 2 = 3 updates;
  # updates from 9 transitions per member on, i.e. from the third step
  args = dict(num_iterations=iterations, steps_per_iteration=steps, max_episode_length=fakes.LIMIT, min_replay_history=9, update_period=2,
              target_update_period=6, epsilon=[0.0, 0.5], batch_size=B)
  args.update(kw)
  return log, tr, train_lib.run_population_training_loop_vec(env, tr, rp, **args)


def _updates_per_step(log):
  """The number of updates after each add, in step order."""
  counts = []
  for e in log:
    if e[0] == 'add':
      counts.append(0)
    elif e[0] == 'update':
      counts[-1] += 1
  return counts


def test_schedule_counts_r_transitions_per_member(monkeypatch):
  log, _, stats = _run(monkeypatch)
  # per member 3, 6, 9, ... transitions: the third step is the first to update (a loop counting P R = 6 per step would start at the
  # second, and run 3 updates per step); 1.5 per step with the fraction carried: 1, 2, 1, 2, ...
  assert _updates_per_step(log) == [0, 0, 1, 2, 1, 2, 1, 2]
  updates = log.named('update')
  assert [u[0] for u in updates] == ['capture'] + ['train_step'] * 8 and all(u[1] == B for u in updates)
  assert [s['updates'] for s in stats] == [3, 6]
  assert [s['transitions'] for s in stats] == [4 * N, 8 * N]


def test_sync_every_three_updates_not_every_step(monkeypatch):
  log, _, _ = _run(monkeypatch)
  marks = [e[0] for e in log if e[0] in ('add', 'update', 'sync')]
  want = []
  for count in [0, 0, 1, 2, 1, 2, 1, 2]:
    want.append('add')
    for _ in range(count):
      want.append('update')
      if want.count('update') % 3 == 0:
        want.append('sync')
  assert marks == want and marks.count('sync') == 3
  # the syncs fall inside steps 3, 5 and 7, right after the 3rd, 6th and 9th update
  assert [i for i, m in enumerate(marks) if m == 'sync'] == [7, 13, 19]


def test_updates_per_step_overrides_and_history_is_per_member(monkeypatch):
  log, _, _ = _run(monkeypatch, updates_per_step=2, min_replay_history=10)
  assert _updates_per_step(log) == [0, 0, 0, 2, 2, 2, 2, 2]       # 12 >= 10 transitions per member after the fourth step
  log, _, _ = _run(monkeypatch, min_replay_history=0)
  assert _updates_per_step(log)[:3] == [0, 1, 2]                   # the ring holds update_horizon + 1 steps from the second step


def test_call_order_ladder_and_seeds(monkeypatch):
  log, tr, _ = _run(monkeypatch, iterations=1)
  names = [e[0] for e in log]
  step0 = ['reset', 'act', 'explore', 'step', 'add']
  assert names[:5] == step0 and names[5:9] == step0[1:]
  third = names.index('update')
  assert names[third - 4:third + 1] == ['act', 'explore', 'step', 'add', 'update']
  assert names[-3:] == ['env_check', 'replay_check', 'trainer_check']
  explores = log.named('explore')
  assert [e[2] for e in explores] == [0, 1, 2, 3]                                    # the step the draws are keyed by
  assert all(e[0] == [0.0, 0.5] and e[1] == tr.seeds.tolist() == [11, 12] for e in explores)
  # the actions explored are the ones act wrote, and the ones flown and stored
  for k, (ex, st, ad) in enumerate(zip(explores, log.named('step'), log.named('add'))):
    want = [(k + e) % 3 for e in range(N)]
    assert ex[3].tolist() == st[1].tolist() == ad[1].tolist() == want
    assert st[2].tolist() == ([1] * N if k == 3 else [0] * N)                        # the 4th step reaches the episode limit
    assert ad[4].tolist() == st[2].tolist() and not ad[3].any()                      # episode_end without a terminal
    assert torch.equal(ad[0], torch.full((N, 2), float(k)))                          # the observation acted on


def test_epsilon_as_a_function_of_a_members_transitions(monkeypatch):
  seen = []

  def eps(transitions):
    seen.append(transitions)
    return 0.25
  log, _, _ = _run(monkeypatch, iterations=1, epsilon=eps)
  assert seen == [0, R, 2 * R, 3 * R]                              # a member's transitions, not the population's
  assert [e[0] for e in log.named('explore')] == [0.25] * 4
  log, _, _ = _run(monkeypatch, iterations=1, epsilon=0.125)
  assert [e[0] for e in log.named('explore')] == [[0.125, 0.125]] * 4
  with pytest.raises(ValueError):
    _run(monkeypatch, epsilon=[0.0, 1.5])
  with pytest.raises(ValueError):
    _run(monkeypatch, epsilon=[0.0, 0.1, 0.2])


def test_stats_per_member(monkeypatch):
  _, _, stats = _run(monkeypatch)
  first, later = fakes.FIRST_LOSS, fakes.LATER_LOSS
  # iteration 0: the captured update, then two more; iteration 1: six
  assert stats[0]['member_mean_loss'] == pytest.approx([(first[p] + 2 * later[p]) / 3 for p in range(P)])
  assert stats[1]['member_mean_loss'] == pytest.approx(list(later))
  assert stats[0]['mean_loss'] == pytest.approx(sum(stats[0]['member_mean_loss']) / P)
  for s in stats:
    assert s['member_episodes'] == [R, R] and s['episodes'] == N
    assert s['member_mean_return'] == [4.0, 16.0] and s['mean_return'] == pytest.approx(10.0)
    assert s['lr'] == [1.0, 2.0] and 'round' not in s and 'lineage' not in s
    assert s['time_within_radius'] == pytest.approx(5 / 6)                           # rewards 1 .. 5 of 0 .. 5 are above 0.5


def test_pbt_round_copies_and_lineage(monkeypatch):
  log, tr, stats = _run(monkeypatch, ready_every=1, truncation=0.5, perturb=(0.5, 4.0), seed=3)
  g = torch.Generator().manual_seed(3)
  factors = []
  for _ in range(2):                                               # pbt_decide's draws with k = 1: the source, then the factor
    torch.randint(0, 1, (1,), generator=g)
    factors.append([0.5, 4.0][int(torch.randint(0, 2, (1, 1), generator=g))])
  # member 0 (mean return 4) becomes a copy of member 1 (16) after each iteration, its lr member 1's times a factor
  assert log.named('copy') == [([1], [0]), ([1], [0])]
  assert log.named('scale') == [('lr', [0], [factors[0]]), ('lr', [0], [factors[1]])]
  assert [s['lineage'] for s in stats] == [[1, 1], [1, 1]]
  assert [s['round'] for s in stats] == [{'fitness': [4.0, 16.0], 'src': [1], 'dst': [0]}] * 2
  assert stats[0]['lr'] == [2.0 * factors[0], 2.0] and stats[1]['lr'] == [2.0 * factors[1], 2.0]
  assert tr.lr.tolist() == stats[1]['lr']
  # the round comes after the iteration's updates and before its checks
  names = [e[0] for e in log]
  assert names[names.index('copy') - 1] in ('update', 'sync') and names[names.index('copy') + 2] == 'env_check'
  # truncation 0 (the default) with rounds: a plain seed study that reports its fitness
  log, _, stats = _run(monkeypatch, ready_every=2)
  assert not log.named('copy') and not log.named('scale')
  assert [s['round'] for s in stats] == [None, {'fitness': [4.0, 16.0], 'src': [], 'dst': []}]
  assert all(s['lineage'] == [0, 1] for s in stats)


def test_controller_continues(monkeypatch):
  log = fakes.Log()
  monkeypatch.setattr(qnet_train, 'explore_grouped', fakes.recording_explore(log))
  env, tr, rp = fakes.FakePopEnv(log), fakes.FakePopQTrainer(log), fakes.FakePopReplay(log)
  c = train_lib.PBTController(P, 'cpu', ready_every=2, truncation=0.5, perturb=(0.5, 4.0), explore=('lr',), seed=3)
  kw = dict(steps_per_iteration=4, max_episode_length=fakes.LIMIT, min_replay_history=9, update_period=2, target_update_period=6,
            batch_size=B, controller=c)
  a = train_lib.run_population_training_loop_vec(env, tr, rp, num_iterations=1, **kw)
  b = train_lib.run_population_training_loop_vec(env, tr, rp, num_iterations=1, **kw)
  assert a[0]['round'] is None and b[0]['round'] is not None and b[0]['round']['dst'] == [0] and c.rounds == 1
