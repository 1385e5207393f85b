"""The twins of the acting and collecting half of training (collect_host.py: epsilon-greedy and the uniform replay draw)
held to their own laws, and run_training_loop_vec's schedule on CPU tensors with recording fakes (loop_fakes.py).  No GPU.

 * the twins' Philox is the published one (test_plan_host's known answers) and Streams pops out[3] first;
 * epsilon-greedy: explored count, chi-squared of the actions, correlations of the masks; the strict threshold uf < epsilon;
 * uniform draw: every valid (t, env) equally often over 200 counters x 1024 rows, both ends of the candidate range, no invalid window;
 * the loop: the explore step counter, the callable epsilon, Dopamine's update and target-sync schedule, the per-environment episode
   limit, episode_end, the explorer's begin mask, the iteration dicts.
"""
import numpy as np
import pytest
import scipy.stats
import torch

import collect_host
import loop_fakes
import plan_host
import reset_draws_host
import test_plan_host


# ------------------------------------------------------------------------------------------------------------------------------ Philox
def test_streams_are_the_published_philox():
  test_plan_host.test_twin_philox_known_answers()                    # plan_host.philox4x32 is Random123's Philox4x32-10
  g = reset_draws_host.Streams(0, 0, 0)
  assert [int(g.u32()[0]) for _ in range(4)] == [0x9b00dbd8, 0xbc57ac4c, 0xe169c58d, 0x6627e8d5]      # the zero vector, out[3] first
  # counter = (block, episode, key lo, key hi), key = (seed lo, seed hi); block 1 follows block 0
  seed, key, episode = 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0xDEADBEEF
  g = reset_draws_host.Streams(seed, key, episode, blocks=1)
  for block in (0, 1):
    counter = np.array([[block, episode, key & 0xFFFFFFFF, key >> 32]], np.uint64)
    want = plan_host.philox4x32(counter, np.array([[seed & 0xFFFFFFFF, seed >> 32]], np.uint64))[0]
    assert [int(g.u32()[0]) for _ in range(4)] == [int(w) for w in want[::-1]]


# ---------------------------------------------------------------------------------------------------------------------- epsilon-greedy
def _twin_run(actions, epsilon, seed, step):
  return collect_host.explore(actions, epsilon, seed, step)[0]


def test_explore_twin_laws():
  collect_host.assert_explore_laws(_twin_run, 'twin')


def test_explore_twin_words():
  """The contract's own words, once by hand: lane i reads block 0 of counter (0, step lo, i, 0) under key (seed lo, seed hi ^ step hi);
  u = out[3], r = out[2]."""
  seed, step, n = 2 ** 40 + 5, 2 ** 32 + 1, 5
  uf, random = collect_host.explore_draws(n, seed, step)
  for i in range(n):
    out = plan_host.philox4x32(np.array([[0, step & 0xFFFFFFFF, i, 0]], np.uint64),
                               np.array([[seed & 0xFFFFFFFF, (seed >> 32) ^ (step >> 32)]], np.uint64))[0]
    u, r = int(out[3]), int(out[2])
    assert uf[i] == np.float32(u >> 8) * np.float32(2.0 ** -24) and 0.0 <= uf[i] < 1.0
    assert random[i] == (r * 3) >> 32


def test_explore_twin_threshold():
  n, seed, step = 257, 3, 7
  held = np.random.default_rng(0).integers(0, 3, n).astype(np.uint8)
  _, _, uf, random = collect_host.explore(held, 0.5, seed, step)
  j = int(np.argmin(np.abs(uf - np.float32(0.3))))
  at, above = uf[j], np.nextafter(uf[j], np.float32(1.0))
  assert at.dtype == np.float32 and above > at
  assert not collect_host.explore(held, at, seed, step)[1][j], 'uf == epsilon was replaced: the rule is uf < epsilon'
  new, mask, _, _ = collect_host.explore(held, above, seed, step)
  assert mask[j] and new[j] == random[j]
  new, mask, _, _ = collect_host.explore(held, 0.0, seed, step)
  assert not mask.any() and np.array_equal(new, held)
  new, mask, _, _ = collect_host.explore(held, 1.0, seed, step)
  assert mask.all() and np.array_equal(new, random)


# ------------------------------------------------------------------------------------------------------------- the uniform replay draw
def test_uniform_draw_twin_laws():
  """A ring with a known set of valid windows: N = 5, capacity 12, horizon 3, count 20 (wrapped: lo_t = 8, span 9).  Over 200
  counters x 1024 rows every valid (t, env) is drawn equally often (chi-squared at the 0.1 % point), both ends of the candidate range
  are drawn and nothing invalid is."""
  cap, n_env, hz, count, batch, counters = 12, 5, 3, 20, 1024, 200
  terminal, episode_end = collect_host.random_ring(np.random.default_rng(5), cap, n_env, 0.05, 0.15)
  lo_t, span = collect_host.candidates(count, cap, hz)
  assert (lo_t, span) == (8, 9)
  valid = collect_host.valid_windows(terminal, episode_end, count, cap, hz)
  assert valid[0].any() and valid[-1].any() and 10 <= valid.sum() < valid.size, 'the ring must have valid windows at both ends, and invalid ones'
  hits = np.zeros(valid.shape, np.int64)
  for c in list(range(counters - 2)) + [2 ** 32 - 1, 2 ** 32 + 5]:
    index, tries = collect_host.uniform_draws(terminal, episode_end, count, cap, hz, batch, 11, c, valid=valid)
    assert (index >= 0).all() and (tries >= 1).all(), 'a row failed on a ring with valid windows'       # (P(64 invalid tries) ~ 1e-30)
    np.add.at(hits, (index[:, 0] - lo_t, index[:, 1]), 1)
  assert hits.sum() == counters * batch and not hits[~valid].any(), 'an invalid window was drawn'
  assert hits[0].sum() > 0 and hits[-1].sum() > 0, 't = lo_t or t = lo_t + span - 1 is never drawn'
  cells = hits[valid].astype(np.float64)
  expect = cells.sum() / cells.size
  chi2 = float(((cells - expect) ** 2 / expect).sum())
  bound = float(scipy.stats.chi2.ppf(0.999, cells.size - 1))
  print(f'uniform draw: {cells.size} valid of {valid.size} windows, chi2 = {chi2:.2f} (0.1 % point {bound:.2f}), min / max hits '
        f'{int(cells.min())} / {int(cells.max())}')
  assert chi2 < bound, (chi2, bound)


def test_uniform_draw_twin_edges():
  terminal, episode_end = collect_host.random_ring(np.random.default_rng(1), 6, 3, 0.0, 0.0)     # no ends: every window is valid
  # span 0 and below: every row fails without reading a word
  for count in (0, 4, 5):
    index, tries = collect_host.uniform_draws(terminal, episode_end, count, 6, 5, 7, 1, 0)
    assert (index == -1).all() and not tries.any()
  # span 1: every row draws t = lo_t at the first try, below the capacity (lo_t = 0) and wrapped (capacity 6, count 6 + 5 -> lo_t = 5)
  index, tries = collect_host.uniform_draws(terminal, episode_end, 6, 6, 5, 64, 1, 0)
  assert (index[:, 0] == 0).all() and (tries == 1).all() and set(index[:, 1]) == {0, 1, 2}
  index, tries = collect_host.uniform_draws(terminal, episode_end, 11, 6, 5, 64, 1, 0)
  assert (index[:, 0] == 5).all() and (tries == 1).all()
  # every step a time-limit end: max_tries tries, then (-1, -1)
  ends = np.ones((6, 3), np.uint8)
  for max_tries in (3, 64):
    index, tries = collect_host.uniform_draws(np.zeros((6, 3), np.uint8), ends, 6, 6, 5, 9, 1, 0, max_tries=max_tries)
    assert (index == -1).all() and (tries == max_tries).all()
  # a terminal ends a window validly, a time-limit end before it does not (train_host.nstep's rule)
  term, end = np.zeros((6, 1), np.uint8), np.zeros((6, 1), np.uint8)
  term[2, 0] = end[2, 0] = 1
  assert collect_host.valid_windows(term, end, 6, 6, 3).ravel().tolist() == [True, True, True]
  term[2, 0] = 0
  assert collect_host.valid_windows(term, end, 6, 6, 3).ravel().tolist() == [False, False, False]
  # the stream does not restart between tries and rows do not share one: rows differ, and so do counters that differ in the high word
  a = collect_host.uniform_draws(terminal, episode_end, 17, 6, 1, 256, 1, 5)[0]
  b = collect_host.uniform_draws(terminal, episode_end, 17, 6, 1, 256, 1, 2 ** 32 + 5)[0]
  assert len({tuple(r) for r in a}) > 8 and not np.array_equal(a, b)


def test_retry_and_failure_rings():
  """The two rings of the GPU test do exercise the retry and the failure path (on the twin, so no sampler passes by luck): figures
  of counter 2^32 + 5, seed 11, B = 1025."""
  (easy, hard) = collect_host.easy_and_hard_ring()
  out = {}
  for name, (terminal, episode_end) in (('easy', easy), ('hard', hard)):
    valid = collect_host.valid_windows(terminal, episode_end, 60, 24, 5)
    index, tries = collect_host.uniform_draws(terminal, episode_end, 60, 24, 5, 1025, 11, 2 ** 32 + 5, valid=valid)
    failed = index[:, 0] < 0
    out[name] = (round(float(valid.mean()), 3), int(failed.sum()), int((tries >= 3).sum()), int(tries.max()),
                 int((~failed & (tries >= 10)).sum()))
    print(name, 'valid share, failed rows, rows with >= 3 tries, max tries, rows that succeed after >= 10 tries:', out[name],
          'tries histogram', np.bincount(tries).tolist())
    assert (index[failed] == -1).all() and (tries[failed] == 64).all()
  # (with NumPy's default_rng(0) as it is today: easy (0.771, 0, 56, 5, 0), hard (0.054, 25, 935, 64, 624))
  assert out['hard'][1] >= 10 and out['hard'][4] >= 10 and out['easy'][2] >= 20 and out['easy'][1] == 0


# ------------------------------------------------------------------------------------------------- the schedule of run_training_loop_vec
STEPS = 14
N_ENV, END_MASK = loop_fakes.N_ENV, loop_fakes.END_MASK      # (three environments whose terminals stagger their episode clocks)
# min_replay_history = 9 holds after step 2 (9 transitions), cursor > update_horizon = 4 after step 4: from step 4 on, 3 / 4 of an
# update per step with the fraction carried: 0.75 -> 0, 1.5 -> 1, 1.25 -> 1, 1.0 -> 1, 0.75 -> 0, ...
UPDATES = (0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1)
_Log, _FakeEnv, _FakeTrainer, _FakeReplay = loop_fakes.Log, loop_fakes.FakeEnv, loop_fakes.FakeTrainer, loop_fakes.FakeReplay


def _run(monkeypatch, epsilon, exploration=False, update_horizon=4, **kw):
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.agents import qnet_train
  log = _Log()

  def explore(actions, eps, seed, step):
    log.append(('explore', actions.clone(), eps, seed, step))
    actions.add_(1).remainder_(3)                     # (in place, as the kernel: the env and the replay must see it)
    return actions
  monkeypatch.setattr(qnet_train, 'explore', explore)

  def explorer(obs, actions, begin):
    log.append(('explorer', actions.clone(), begin.clone()))
  stats = train_lib.run_training_loop_vec(_FakeEnv(log), _FakeTrainer(log), _FakeReplay(log, update_horizon), num_iterations=2, steps_per_iteration=7,
                                          max_episode_length=4, min_replay_history=9, update_period=4, target_update_period=12,
                                          epsilon=epsilon, batch_size=8, seed=21, exploration=explorer if exploration else None, **kw)
  return log, stats


_u8 = loop_fakes.u8


def test_training_loop_schedule(monkeypatch):
  asked = []

  def epsilon(transitions):
    asked.append(transitions)
    return 0.5 - 0.01 * transitions

  log, stats = _run(monkeypatch, epsilon)
  # the explore kernel's step: 0 .. 13, not restarted by the second iteration; epsilon is asked with the transitions added so far
  explores = log.named('explore')
  assert [e[3] for e in explores] == list(range(STEPS)) and all(e[2] == 21 for e in explores)
  assert asked == [N_ENV * s for s in range(STEPS)]
  assert [e[1] for e in explores] == [0.5 - 0.01 * (N_ENV * s) for s in range(STEPS)]
  for s, e in enumerate(explores):                    # it is handed the greedy actions of this step
    assert torch.equal(e[0], _u8([(s + i) % 3 for i in range(N_ENV)]))
  # per step: act, explore, env.step, add, then the updates; end_mask where an environment's own episode reaches its 4th step
  steps, adds = log.named('step'), log.named('add')
  assert len(steps) == len(adds) == STEPS
  for s in range(STEPS):
    _, actions, end_mask, terminal = steps[s]
    taken = _u8([(s + i + 1) % 3 for i in range(N_ENV)])             # what the explore recorder left in the tensor
    assert torch.equal(actions, taken), s
    assert torch.equal(end_mask, _u8(END_MASK.get(s, (0, 0, 0)))), (s, end_mask)
    obs, action, reward, term, episode_end = adds[s]
    assert torch.equal(obs, torch.full((N_ENV, 2), float(s))), 'the replay stores the observation the action was taken on'
    assert torch.equal(action, taken) and torch.equal(reward, torch.tensor([1.0, 0.25, 0.0]) + s) and torch.equal(term, terminal)
    assert torch.equal(episode_end, terminal | end_mask), s
  # the updates of every step, and a target sync after every third update
  per_step, syncs_after, updates, step = [], [], 0, -1
  for e in log:
    if e[0] == 'add':
      step += 1
      per_step.append(0)
    elif e[0] == 'update':
      assert e[2] == 8
      per_step[step] += 1
      updates += 1
    elif e[0] == 'sync':
      syncs_after.append(updates)
  assert tuple(per_step) == UPDATES, per_step
  assert syncs_after == [3, 6], syncs_after
  kinds = [e[0] for e in log.named('update')]
  assert kinds == ['capture'] + ['train_step'] * 6, 'the first update captures the graph, the others replay it'
  # the iteration dicts
  assert [s['updates'] for s in stats] == [2, 5]
  assert [s['episodes'] for s in stats] == [6, 6]
  assert [s['transitions'] for s in stats] == [21, 42]
  assert stats[0]['mean_loss'] == pytest.approx((1.0 + 3.0) / 2) and stats[1]['mean_loss'] == pytest.approx(3.0)
  assert [e[0] for e in log if e[0].endswith('_check')] == ['env_check', 'replay_check', 'trainer_check'] * 2
  assert len(log.named('reset')) == 1


def _updates_per_step(log):
  per_step = []
  for e in log:
    if e[0] == 'add':
      per_step.append(0)
    elif e[0] == 'update':
      per_step[-1] += 1
  return tuple(per_step)


def test_training_loop_history_gate_alone(monkeypatch):
  """With update_horizon = 1 the ring's gate (cursor > update_horizon) opens after step 1, so min_replay_history = 9 (after step 2)
  is the gate that binds: the carry starts at step 2.  In the runs above the ring's gate binds (step 4), the history gate being open
  since step 2: each gate is held on its own."""
  log, stats = _run(monkeypatch, 0.25, update_horizon=1)
  assert _updates_per_step(log) == (0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1)
  assert [s['updates'] for s in stats] == [3, 6]
  order = [e[0] for e in log if e[0] in ('update', 'sync')]
  assert [i - k for k, i in enumerate(j for j, e in enumerate(order) if e == 'sync')] == [3, 6, 9]


def test_training_loop_without_capture(monkeypatch):
  log, stats = _run(monkeypatch, 0.25, capture_graph=False)
  assert [e[0] for e in log.named('update')] == ['train_step'] * 7
  assert [e[1] for e in log.named('explore')] == [0.25] * STEPS
  assert [s['updates'] for s in stats] == [2, 5]


def test_training_loop_updates_per_step(monkeypatch):
  """updates_per_step replaces the carried fraction, not the two gates."""
  log, stats = _run(monkeypatch, 0.25, updates_per_step=2)
  assert [s['updates'] for s in stats] == [2 * 3, 2 * 7]
  syncs = [i for i, e in enumerate([e for e in log if e[0] in ('update', 'sync')]) if e[0] == 'sync']
  assert len(syncs) == 20 // 3


def test_training_loop_explorer_begin_mask(monkeypatch):
  log, _ = _run(monkeypatch, 0.25, exploration=True)
  calls, adds = log.named('explorer'), log.named('add')
  assert len(calls) == STEPS and len(log.named('explore')) == STEPS
  assert torch.equal(calls[0][1], torch.ones(N_ENV, dtype=torch.uint8))
  for s in range(1, STEPS):
    assert torch.equal(calls[s][1], adds[s - 1][4]), (s, 'begin is the previous episode_end')
  assert any(c[1].any() for c in calls[1:]) and not all(c[1].all() for c in calls[1:])
  for s, c in enumerate(calls):                        # the explorer comes after epsilon-greedy
    assert torch.equal(c[0], _u8([(s + i + 1) % 3 for i in range(N_ENV)]))


def test_training_loop_skips_explore_only_with_an_explorer(monkeypatch):
  log, _ = _run(monkeypatch, 0.0, exploration=True)
  assert not log.named('explore') and len(log.named('explorer')) == STEPS
  log, _ = _run(monkeypatch, 0.0)
  assert [e[1] for e in log.named('explore')] == [0.0] * STEPS and [e[3] for e in log.named('explore')] == list(range(STEPS))


def test_explore_refuses_what_it_would_miswrite():
  """qnet_train.explore hands the kernel data_ptr() and numel(): a strided view or another dtype would have other bytes written."""
  from balloon_learning_environment_amd.agents import qnet_train
  for bad in (torch.zeros(8, dtype=torch.uint8)[::2], torch.zeros(4, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.uint8).t()):
    with pytest.raises(ValueError):
      qnet_train.explore(bad, 0.5, 0, 0)
