"""train_lib.run_dagger_loop_vec's call order and block contract on CPU tensors with recording fakes (loop_fakes.py's environment and
rollout, dagger_fakes.py's learner and expert), CPU only.  The same check is run on four loops that each make one mistake -- storing
the flown action, labelling the next observation, skipping the bootstrap act, mixing before asking the expert -- and must fail on
every one."""
import pytest
import torch

import dagger_fakes as df
import loop_fakes as lf
from balloon_learning_environment_amd import train_lib

HORIZON, EPOCHS, BATCH, LIMIT = 7, 2, 4, 4


def _mistaken_loop(mistake):
  """run_dagger_loop_vec restated with one mistake (None: without)."""
  def loop(env, trainer, expert, rollout, *, num_iterations, beta, epochs=1, batch_size, max_episode_length=960, gamma=0.993, lam=0.95,
           capture_graph=True):
    n = env.num_envs
    obs = env.reset()
    learner, label, actions, took = (torch.zeros(n, dtype=torch.uint8) for _ in range(4))
    logp, value = torch.zeros(n), torch.zeros(n)
    book = train_lib._EpisodeBook(n, env.device, max_episode_length)
    captured, stats = False, []
    for it in range(num_iterations):
      beta_i = float(beta(it) if callable(beta) else beta)
      took_sum, agree_sum = 0.0, 0.0
      for t in range(rollout.horizon):
        trainer.act(obs, learner, logp, value)
        if mistake == 'mix_first':
          trainer.mix(learner, label, beta_i, actions, took)
          expert.act(obs, label)
        elif mistake != 'label_next':
          expert.act(obs, label)
          trainer.mix(learner, label, beta_i, actions, took)
        else:
          trainer.mix(learner, label, beta_i, actions, took)
        end_mask = book.end_mask()
        next_obs, reward, terminal = env.step(actions, end_mask=end_mask)
        if mistake == 'label_next':
          expert.act(next_obs, label)
        episode_end = terminal | end_mask
        rollout.add(t, obs, actions if mistake == 'store_flown' else label, logp, value, reward, terminal, episode_end)
        book.step(reward, episode_end)
        took_sum += float(took.sum())
        obs = next_obs
      if mistake != 'no_bootstrap':
        trainer.act(obs, learner, logp, value)
      rollout.finish(value, gamma, lam, normalize=False)
      for _ in range(epochs):
        for batch in rollout.minibatches(batch_size):
          if capture_graph and not captured:
            loss, captured = trainer.capture(batch), True
          else:
            loss = trainer.train_step(batch)
          book.update(loss)
          agree_sum += float(trainer.views(batch_size)['aux'][:, 1].mean())
      env.check_errors()
      trainer.check_errors()
      if hasattr(expert, 'check_errors'):
        expert.check_errors()
      updates = book.updates
      s = book.finish_iteration(rollout.horizon)
      s['agreement'], s['expert_share'] = agree_sum / max(updates, 1), took_sum / (n * rollout.horizon)
      stats.append(s)
    return stats
  return loop


def _check(loop, beta, want_betas):
  """Two iterations of `loop` on the fakes, max_episode_length = 4, T = 7: asserts the whole contract."""
  log = lf.Log()
  trainer = df.FakeBCTrainer(log)
  stats = loop(lf.FakeEnv(log), trainer, df.FakeExpert(log), lf.FakeRollout(log, HORIZON), num_iterations=2, beta=beta, epochs=EPOCHS,
               batch_size=BATCH, max_episode_length=LIMIT, gamma=0.75, lam=0.5)
  per_pass = HORIZON * lf.N_ENV // BATCH
  assert per_pass == 5
  # the order of the calls of one iteration, twice; one reset
  one = (['act', 'expert', 'mix', 'step', 'add'] * HORIZON + ['act', 'finish'] + (['pass'] + ['update', 'views'] * per_pass) * EPOCHS +
         ['env_check', 'trainer_check', 'expert_check'])
  assert [e[0] for e in log] == ['reset'] + one * 2, 'the call order'
  acts, experts, mixes, steps, adds = (log.named(k) for k in ('act', 'expert', 'mix', 'step', 'add'))
  assert len(acts) == 2 * (HORIZON + 1) and trainer.acts == 2 * (HORIZON + 1), 'act_step ends at T + 1 per iteration: the bootstrap act'
  flown_differs = 0
  s = 0
  for it in range(2):
    for t in range(HORIZON):
      k = it * (HORIZON + 1) + t                        # (the bootstrap act of iteration 0 is act number T)
      seen = torch.full((lf.N_ENV, 2), float(s))
      assert acts[k][0] == k and torch.equal(acts[k][1], seen), 'act sees the last returned observation'
      assert torch.equal(experts[s][0], seen), 'the expert labels the observation the learner acted on'
      a, l, v = lf.ppo_act(k)
      want_label = df.label_of(seen)
      m, m_learner, m_expert, m_beta = mixes[s]
      assert m == s and torch.equal(m_learner, a) and torch.equal(m_expert, want_label), 'mix takes this step\'s learner action and label'
      assert m_beta == want_betas[it] and isinstance(m_beta, float), (it, m_beta)
      flown = torch.where(df.took_of(s).bool(), want_label, a)
      _, actions, end_mask, terminal = steps[s]
      assert steps[s][0] == s and torch.equal(actions, flown), 'the stepped action is the mix'
      assert torch.equal(end_mask, lf.u8(lf.END_MASK.get(s, (0, 0, 0)))), (s, end_mask)
      at, obs, action, logp, value, reward, term, episode_end = adds[s]
      assert at == t
      assert torch.equal(obs, seen), 'the block stores the observation the action was taken on'
      assert torch.equal(action, want_label), 'the stored action is the label, not the action flown'
      flown_differs += int((flown != want_label).sum())
      assert torch.equal(logp, l) and torch.equal(value, v), 'the learner at that observation and draw'
      assert torch.equal(reward, lf.reward_of(s)) and torch.equal(term, terminal)
      assert torch.equal(episode_end, terminal | end_mask), s
      s += 1
    k = it * (HORIZON + 1) + HORIZON
    assert torch.equal(acts[k][1], torch.full((lf.N_ENV, 2), float(s))), 'the bootstrap act sees the observation after the last step'
    boot, gamma, lam, normalize = log.named('finish')[it]
    assert torch.equal(boot, lf.ppo_act(k)[2]) and (gamma, lam, normalize) == (0.75, 0.5, False)
  assert s == 14 and flown_differs > 0, 'the fakes tell the label from the action flown'
  # the updates: every token of every pass once, in order; the first update captures, the others replay
  updates = log.named('update')
  assert [u[1] for u in updates] == [(p, j) for p in range(2 * EPOCHS) for j in range(per_pass)]
  assert [u[0] for u in updates] == ['capture'] + ['train_step'] * (2 * EPOCHS * per_pass - 1)
  assert all(p[1] == BATCH for p in log.named('pass')) and all(v[0] == BATCH for v in log.named('views'))
  # the iteration dicts: run_training_loop_vec's, plus agreement and expert_share
  assert [d['updates'] for d in stats] == [EPOCHS * per_pass] * 2
  assert [d['episodes'] for d in stats] == [6, 6] and [d['transitions'] for d in stats] == [21, 42]
  assert stats[0]['mean_loss'] == pytest.approx((1.0 + 3.0 * 9) / 10) and stats[1]['mean_loss'] == pytest.approx(3.0)
  assert set(stats[0]) == {'mean_loss', 'updates', 'episodes', 'mean_return', 'time_within_radius', 'transitions', 'agreement', 'expert_share'}
  for it in range(2):
    want = sum(float(df.agree_of(u).mean()) for u in range(10 * it, 10 * it + 10)) / 10
    assert stats[it]['agreement'] == pytest.approx(want), it
    share = sum(int(df.took_of(m).sum()) for m in range(7 * it, 7 * it + 7)) / 21
    assert stats[it]['expert_share'] == pytest.approx(share), it


def test_dagger_loop_call_order_and_block_contract():
  _check(train_lib.run_dagger_loop_vec, 0.25, [0.25, 0.25])


def test_beta_as_a_function_of_the_iteration():
  _check(train_lib.run_dagger_loop_vec, lambda i: 0.5 ** i, [1.0, 0.5])
  _check(train_lib.run_dagger_loop_vec, 1, [1.0, 1.0])                # (an int is handed on as a float)


def test_the_check_passes_the_restated_loop():
  _check(_mistaken_loop(None), 0.25, [0.25, 0.25])


@pytest.mark.parametrize('mistake', ['store_flown', 'label_next', 'no_bootstrap', 'mix_first'])
def test_the_check_fails_a_mistaken_loop(mistake):
  with pytest.raises(AssertionError):
    _check(_mistaken_loop(mistake), 0.25, [0.25, 0.25])


def test_dagger_loop_without_capture_and_an_expert_without_checks():
  log = lf.Log()
  stats = train_lib.run_dagger_loop_vec(lf.FakeEnv(log), df.FakeBCTrainer(log), df.FakeExpert(log, checks=False), lf.FakeRollout(log, 4),
                                        num_iterations=1, beta=0.0, epochs=3, batch_size=6, max_episode_length=4, capture_graph=False)
  assert [u[0] for u in log.named('update')] == ['train_step'] * (3 * 2)
  assert [int(s[2].sum()) for s in log.named('step')] == [0, 0, 0, 1]
  assert not log.named('expert_check') and len(log.named('trainer_check')) == 1
  assert log.named('finish')[0][1:] == (0.993, 0.95, False)             # the defaults
  assert stats[0]['updates'] == 6
