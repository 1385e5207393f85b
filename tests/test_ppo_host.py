"""The float64 / float32 restatement of the on-policy kernels (ppo_host.py), CPU only: its dL/dlogits against torch autograd of the same
objective, generalised advantage estimation on cases worked by hand and its two limits, float32 against float64 inside the derived
running bound, the normalisation's stated order against float64 and against three mistakes on the inputs the GPU test uses,
run_ppo_loop_vec's call order and block contract on recording fakes (loop_fakes.py), the actor stream against the epsilon-greedy
stream, the descriptors against the header, and init_params('actor_critic')."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import plan_host
import ppo_host
from balloon_learning_environment_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def _rows(b, seed):
  """b rows: logits, actions, returns, and old log-probabilities placed so that rho cycles through: inside the band, clipped from
  above, clipped from below; advantages of both signs, so that every (region, sign) pair occurs at b = 7."""
  rng = np.random.default_rng(seed)
  z = rng.standard_normal((b, 6)) * 1.5
  act = rng.integers(0, 3, b)
  lp, _ = ppo_host.log_softmax(z[:, [0, 2, 4]])
  lpa = lp[np.arange(b), act]
  shift = np.array([0.05, 0.5, -0.5, -0.05, 0.4, -0.6, 0.0])[np.arange(b) % 7]      # log rho
  adv = np.array([1.3, 0.7, -0.9, -1.1, -0.4, 0.8, 0.6])[np.arange(b) % 7] * (1.0 + 0.1 * rng.random(b))
  if b == 1:
    shift, adv = np.array([0.5]), np.array([-0.8])        # clipped from above, A < 0: the unclipped branch is the minimum
  return z, act, lpa - shift, adv, rng.standard_normal(b)


def _autograd(z, act, old, adv, ret, clip, cv, ce):
  zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
  lp = torch.log_softmax(zt[:, [0, 2, 4]], dim=1)
  p = lp.exp()
  h = -(p * lp).sum(dim=1)
  lpa = lp[torch.arange(len(act)), torch.tensor(act)]
  rho = (lpa - torch.tensor(old)).exp()
  a = torch.tensor(adv)
  surr = torch.minimum(rho * a, rho.clamp(1.0 - clip, 1.0 + clip) * a)
  loss = -surr + cv * (zt[:, 1] - torch.tensor(ret)) ** 2 - ce * h
  loss.mean().backward()
  return loss.detach().numpy(), zt.grad.numpy(), rho.detach().numpy()


@pytest.mark.parametrize('b', [1, 7])
def test_ppo_loss_gradient_against_autograd(b):
  clip, cv, ce = 0.2, 0.5, 0.01
  z, act, old, adv, ret = _rows(b, seed=b)
  loss, aux, d = ppo_host.ppo_loss(z, act, old, adv, ret, clip, cv, ce)
  want_loss, want_d, rho = _autograd(z, act, old, adv, ret, clip, cv, ce)
  if b == 7:      # every region with both signs of A among the rows
    above, below, inside = rho > 1 + clip, rho < 1 - clip, (rho > 1 - clip) & (rho < 1 + clip)
    assert above.any() and below.any() and inside.any() and (adv[above | below] > 0).any() and (adv[above | below] < 0).any()
    assert (adv[inside] > 0).any() and (adv[inside] < 0).any()
  scale = np.abs(want_d).max()
  assert np.abs(d - want_d).max() <= 1e-12 * scale, (np.abs(d - want_d).max(), scale)
  assert np.abs(loss - want_loss).max() <= 1e-12 * np.abs(want_loss).max()
  assert not d[:, [3, 5]].any()
  lp, _ = ppo_host.log_softmax(z[:, [0, 2, 4]])
  assert np.array_equal(aux[:, 0], lp[np.arange(b), act])


def test_ppo_loss_clipped_rows_keep_the_entropy_term_only():
  z, act, old, adv, ret = _rows(7, seed=3)
  _, _, d = ppo_host.ppo_loss(z, act, old, adv, ret, 0.2, 0.5, 0.01)
  _, _, d0 = ppo_host.ppo_loss(z, act, old, np.zeros(7), ret, 0.2, 0.5, 0.01)      # A = 0: the entropy and value terms alone
  lp, _ = ppo_host.log_softmax(z[:, [0, 2, 4]])
  rho = np.exp(lp[np.arange(7), act] - old)
  clipped = ((rho > 1.2) & (adv > 0)) | ((rho < 0.8) & (adv < 0))
  assert clipped.any() and not clipped.all()
  assert np.array_equal(d[clipped], d0[clipped]) and not np.array_equal(d[~clipped], d0[~clipped])


def test_ppo_loss_invalid_action_row_is_zero():
  z, act, old, adv, ret = _rows(7, seed=4)
  act[2] = 3
  loss, aux, d = ppo_host.ppo_loss(z, act, old, adv, ret)
  assert loss[2] == 0 and not aux[2].any() and not d[2].any() and loss[[0, 1, 3]].all()


def test_log_softmax_saturated_logits_stay_finite():
  z = np.array([[1000.0, -1000.0, 0.0], [-3e4, 3e4, 3e4]], np.float32)
  lp, p = ppo_host.log_softmax(z)
  assert lp.dtype == np.float32 and np.isfinite(lp).all() and np.isfinite(p).all()
  assert p[0].tolist() == [1.0, 0.0, 0.0] and p[1].tolist() == [0.0, 0.5, 0.5]


def test_sample_is_the_inverse_cdf():
  p = np.array([[0.25, 0.5, 0.25]] * 6, np.float32)
  u = np.array([0.0, 0.2499, 0.25, 0.7499, 0.75, 0.9999], np.float32)
  assert ppo_host.sample(p, u).tolist() == [0, 0, 1, 1, 2, 2]
  assert ppo_host.sample(np.array([[0.0, 0.0, 1.0]], np.float32), np.array([0.0], np.float32)).tolist() == [2]


def test_greedy_rule():
  z = np.zeros((5, 6), np.float32)
  z[:, [0, 2, 4]] = [[1, 2, 3], [2, 2, 1], [0, 0, 0], [1, np.nan, 5], [np.nan, 7, np.nan]]
  z[:, [1, 3, 5]] = 99.0           # the value and the unread outputs do not take part
  assert ppo_host.greedy(z).tolist() == [2, 0, 0, 1, 0]


# ---- generalised advantage estimation ------------------------------------------------------------------------------------------------
def _assert_gae(reward, value, boot, terminal, end, gamma, lam, want_adv):
  args = (np.array(reward, np.float32), np.array(value, np.float32), np.array(boot, np.float32), np.array(terminal), np.array(end))
  a32, r32 = ppo_host.gae_f32(*args, gamma, lam)
  a64, r64 = ppo_host.gae_f64(*args, float(np.float32(gamma)), float(np.float32(lam)))
  assert a32.dtype == np.float32 and r32.dtype == np.float32
  np.testing.assert_allclose(a64, np.array(want_adv, np.float64), rtol=1e-6, atol=1e-6)
  np.testing.assert_allclose(a32, a64, rtol=1e-5, atol=1e-6)
  np.testing.assert_allclose(r32, r64, rtol=1e-5, atol=1e-6)
  np.testing.assert_allclose(r64, a64 + args[1], rtol=1e-12)


def test_gae_cases_worked_by_hand():
  g, l = 0.5, 0.5      # gl = 0.25
  # T = 1: delta = r + g boot - v
  _assert_gae([[1.0]], [[2.0]], [4.0], [[0]], [[0]], g, l, [[1.0 + 2.0 - 2.0]])
  # T = 3, a terminal at t = 0: it bootstraps nothing and takes nothing from t = 1
  #   t2: 1 + .5 * 8 - 2 = 3;  t1: 1 + .5 * 2 - 4 + .25 * 3 = -1.25;  t0: 1 - 2 = -1
  _assert_gae([[1.0], [1.0], [1.0]], [[2.0], [4.0], [2.0]], [8.0], [[1], [0], [0]], [[1], [0], [0]], g, l, [[-1.0], [-1.25], [3.0]])
  # a terminal at t = T - 1: boot_value is not read
  #   t2: 1 - 2 = -1;  t1: 1 + .5 * 2 - 4 + .25 * -1 = -2.25;  t0: 1 + .5 * 4 - 2 + .25 * -2.25 = 0.4375
  _assert_gae([[1.0], [1.0], [1.0]], [[2.0], [4.0], [2.0]], [np.nan], [[0], [0], [1]], [[0], [0], [1]], g, l, [[0.4375], [-2.25], [-1.0]])
  # a time-limit end in the middle (t = 1): it bootstraps from its own value and cuts the trace
  #   t2: 3;  t1: 1 + .5 * 4 - 4 = -1;  t0: 1 + .5 * 4 - 2 + .25 * -1 = 0.75
  _assert_gae([[1.0], [1.0], [1.0]], [[2.0], [4.0], [2.0]], [8.0], [[0], [0], [0]], [[0], [1], [0]], g, l, [[0.75], [-1.0], [3.0]])


def test_gae_discards_the_value_a_select_does_not_take():
  """value[t + 1] = NaN behind a terminal or a time-limit end at t does not reach step t."""
  value = np.array([[1.0, 1.0], [np.nan, np.nan], [2.0, 2.0]], np.float32)
  term = np.array([[1, 0], [0, 0], [0, 0]])
  end = np.array([[1, 1], [0, 0], [0, 0]])
  adv, ret = ppo_host.gae_f32(np.ones((3, 2), np.float32), value, np.zeros(2, np.float32), term, end, 0.9, 0.9)
  assert np.isfinite(adv[0]).all() and np.isfinite(ret[0]).all() and np.isnan(adv[1]).all()


def test_gae_lambda_one_is_the_discounted_return():
  rng = np.random.default_rng(0)
  steps, n, g = 9, 5, 0.93
  r, v, boot = rng.standard_normal((steps, n)), rng.standard_normal((steps, n)), rng.standard_normal(n)
  none = np.zeros((steps, n), np.uint8)
  _, ret = ppo_host.gae_f64(r, v, boot, none, none, g, 1.0)
  for t in range(steps):
    want = sum(g ** (k - t) * r[k] for k in range(t, steps)) + g ** (steps - t) * boot
    np.testing.assert_allclose(ret[t], want, rtol=1e-12, atol=1e-12)
  a32, r32 = ppo_host.gae_f32(r, v, boot, none, none, g, 1.0)
  np.testing.assert_allclose(r32, ret, rtol=1e-5, atol=1e-5)


def test_gae_lambda_zero_is_the_td_error():
  rng = np.random.default_rng(1)
  steps, n, g = 6, 4, 0.9
  r, v, boot = rng.standard_normal((steps, n)), rng.standard_normal((steps, n)), rng.standard_normal(n)
  term = (rng.random((steps, n)) < 0.2).astype(np.uint8)
  end = np.maximum(term, (rng.random((steps, n)) < 0.2).astype(np.uint8))
  adv, _ = ppo_host.gae_f64(r, v, boot, term, end, g, 0.0)
  nv = np.concatenate([v[1:], boot[None]])
  want = r + g * np.where(term != 0, 0.0, np.where(end != 0, v, nv)) - v
  np.testing.assert_allclose(adv, want, rtol=1e-12, atol=1e-12)


def test_normalize_f64():
  a = np.random.default_rng(2).standard_normal(1000).astype(np.float32) * 3 + 5
  out = ppo_host.normalize_f64(a)
  assert abs(out.mean()) < 1e-12 and abs(out.std() - 1.0) < 1e-7


def _flight_block(steps, n, seed):
  """A block at the flight's scale: rewards in [0, 1], values about 60 +- 30, 1 % terminals and 1 % time-limit ends."""
  rng = np.random.default_rng(seed)
  term = rng.random((steps, n)) < 0.01
  end = term | (rng.random((steps, n)) < 0.01)
  return (rng.random((steps, n)).astype(np.float32), (60 + 30 * rng.standard_normal((steps, n))).astype(np.float32),
          (60 + 30 * rng.standard_normal(n)).astype(np.float32), term.astype(np.uint8), end.astype(np.uint8))


@pytest.mark.parametrize('steps,n', [(960, 7), (17, 300), (64, 1025)])
def test_gae_f32_within_its_derived_bound_of_f64(steps, n):
  """|gae_f32 - gae_f64| <= gae_f32_error_bound, the running bound 5 u M_t carried by gamma lambda and cut at an end.  Measured: at
  most 0.40 of the bound over these blocks (the worst at 17 x 300)."""
  worst = 0.0
  for gamma, lam in ((0.993, 0.95), (0.999, 1.0), (0.5, 0.0)):
    block = _flight_block(steps, n, seed=steps + n)
    g64, l64 = float(np.float32(gamma)), float(np.float32(lam))
    a32, _ = ppo_host.gae_f32(*block, gamma, lam)
    a64, _ = ppo_host.gae_f64(*block, g64, l64)
    bound = ppo_host.gae_f32_error_bound(*block, g64, l64)
    assert block[3].any() and (block[4] != block[3]).any() and (bound > 0).all()
    share = float((np.abs(a32.astype(np.float64) - a64) / bound).max())
    worst = max(worst, share)
    assert share <= 1.0, (gamma, lam, share)
  print('T x N', steps, n, 'worst |a32 - a64| / E', worst)


def test_gae_bound_is_cut_at_an_end():
  """By hand, gamma = lambda = 0.5, T = 2, one environment: without an end M_1 = 1 + .5 * 8 + 2 = 7, M_0 = 1 + .5 * 2 + 4 + .25 * 7 =
  7.75, E_0 = .25 * 5u * 7 + 5u * 7.75; with a time-limit end at t = 0 the step bootstraps from its own value and carries nothing."""
  u = 2.0 ** -24
  r, v, boot, none = np.ones((2, 1)), np.array([[4.0], [2.0]]), np.array([8.0]), np.zeros((2, 1), np.uint8)
  e = ppo_host.gae_f32_error_bound(r, v, boot, none, none, 0.5, 0.5)
  assert e[1, 0] == 5 * u * 7 and e[0, 0] == 0.25 * (5 * u * 7) + 5 * u * 7.75
  end = np.array([[1], [0]], np.uint8)
  e = ppo_host.gae_f32_error_bound(r, v, boot, none, end, 0.5, 0.5)
  assert e[0, 0] == 5 * u * (1 + 0.5 * 4 + 4)
  e = ppo_host.gae_f32_error_bound(r, v, boot, end, end, 0.5, 0.5)
  assert e[0, 0] == 5 * u * (1 + 4)


# ---- the advantage normalisation -----------------------------------------------------------------------------------------------------
def test_strided_sum_is_the_stated_order():
  """Thread k owns k, k + 256, ...; the partials are added ascending.  1e16 and ones: the order decides which ones are absorbed."""
  x = np.zeros(513)
  x[0], x[256], x[512], x[1] = 1e16, 1.0, 1.0, 2.0
  # thread 0: (1e16 + 1) + 1 = 1e16 (each 1 is absorbed); then + thread 1's 2 = 1e16 + 2
  assert ppo_host.strided_sum(x) == 1e16 + 2.0
  assert ppo_host.strided_sum(np.arange(1, 1001)) == 500500.0 and ppo_host.strided_sum([3.0]) == 3.0


def test_normalisation_inputs_tell_the_stated_kernel_from_three_mistakes():
  """On every input of ppo_host.normalisation_cases the stated order lies within one float32 ulp of normalize_f64 (measured: at most
  0.5); each mistake lies outside on the input that names it.  So the GPU test's one-ulp bound over these inputs passes the kernel
  as stated and nothing else.  Measured ulps here (NumPy's default_rng as it is today): no epsilon 5.5e6 ('tiny'), 17 ('offset'),
  NaN where every advantage is equal; M - 1 at least 1.2e2 (M = 65 537) on every input with M > 1 that is not constant, 2.5e6 on
  'pair'; one pass 1.7e3 ('offset')."""
  def no_epsilon(a):
    a = a.astype(np.float64)
    d = a - ppo_host.strided_sum(a) / a.size
    with np.errstate(invalid='ignore', divide='ignore'):
      return (d / np.sqrt(ppo_host.strided_sum(d * d) / a.size)).astype(np.float32)

  def m_minus_one(a):
    a = a.astype(np.float64)
    d = a - ppo_host.strided_sum(a) / a.size
    with np.errstate(invalid='ignore', divide='ignore'):
      return (d / (np.sqrt(ppo_host.strided_sum(d * d) / (a.size - 1)) + 1e-8)).astype(np.float32)

  def one_pass(a):
    a = a.astype(np.float64)
    mean = ppo_host.strided_sum(a) / a.size
    var = ppo_host.strided_sum(a * a) / a.size - mean * mean
    with np.errstate(invalid='ignore'):
      return ((a - mean) / (np.sqrt(var) + 1e-8)).astype(np.float32)

  def worst(f, a):
    err = ppo_host.ulps_from(f(a), ppo_host.normalize_f64(a))
    return float('inf') if np.isnan(err).any() else float(err.max())

  cases = ppo_host.normalisation_cases()
  assert [len(cases[f'normal_{m}']) for m in (1, 2, 255, 256, 257, 511, 513, 65537)] == [1, 2, 255, 256, 257, 511, 513, 65537]
  assert (len(cases['equal']), len(cases['tiny']), len(cases['offset'])) == (300, 1025, 4097)
  assert cases['pair'].tolist() == [1.0, 3.0] and cases['triple'].tolist() == [1.0, 2.0, 4.5]
  for name, a in cases.items():
    got = ppo_host.normalize_ordered(a)
    w = worst(ppo_host.normalize_ordered, a)
    print(name, 'ordered', w, 'no epsilon', worst(no_epsilon, a), 'M - 1', worst(m_minus_one, a), 'one pass', worst(one_pass, a))
    assert got.dtype == np.float32 and np.isfinite(got).all() and w <= 1.0, (name, w)
    if len(a) > 1:
      assert worst(m_minus_one, a) > 1.0 or name == 'equal', name
  assert not ppo_host.normalize_ordered(cases['normal_1']).any() and not ppo_host.normalize_ordered(cases['equal']).any()
  assert not np.isfinite(no_epsilon(cases['equal'])).any() and not np.isfinite(no_epsilon(cases['normal_1'])).any()      # 0 / 0
  assert worst(no_epsilon, cases['tiny']) > 1e3
  assert worst(one_pass, cases['offset']) > 1e2
  assert worst(m_minus_one, cases['pair']) > 1e3 and worst(m_minus_one, cases['triple']) > 1e3
  # the pair by hand: mean 2, var 1 (not 2): -1 and 1 over 1 + 1e-8
  assert np.array_equal(ppo_host.normalize_ordered(cases['pair']), np.array([-1.0, 1.0], np.float32) / np.float32(1 + 1e-8))


# ---- the loop's schedule -------------------------------------------------------------------------------------------------------------
def test_ppo_loop_call_order_and_block_contract():
  """run_ppo_loop_vec on CPU tensors with recording fakes (loop_fakes.py), max_episode_length = 4, T = 7, two iterations: per step act,
  end_mask, env.step(actions, end_mask=), add, book.step; one more act after step T - 1 whose value goes to finish; epochs x
  (T N // batch_size) updates; the end_mask of an environment on the 4th step of its own episode, restarting after a terminal."""
  import loop_fakes as lf
  from balloon_learning_environment_amd import train_lib
  horizon, epochs, batch = 7, 2, 4
  log = lf.Log()
  trainer = lf.FakePPOTrainer(log)
  stats = train_lib.run_ppo_loop_vec(lf.FakeEnv(log), trainer, lf.FakeRollout(log, horizon), num_iterations=2, epochs=epochs,
                                     batch_size=batch, max_episode_length=4)
  per_pass = horizon * lf.N_ENV // batch
  assert per_pass == 5
  # the order of the calls of one iteration, twice; one reset
  one = ['act', 'step', 'add'] * horizon + ['act', 'finish'] + (['pass'] + ['update'] * per_pass) * epochs + ['env_check', 'trainer_check']
  assert [e[0] for e in log] == ['reset'] + one * 2
  acts, steps, adds, finishes = log.named('act'), log.named('step'), log.named('add'), log.named('finish')
  assert len(acts) == 2 * (horizon + 1) and trainer.acts == 2 * (horizon + 1)
  s = 0
  for it in range(2):
    for t in range(horizon):
      k = it * (horizon + 1) + t                        # (the bootstrap act of iteration 0 is act number T)
      assert acts[k][0] == k and torch.equal(acts[k][1], torch.full((lf.N_ENV, 2), float(s))), 'act sees the last returned observation'
      a, l, v = lf.ppo_act(k)
      _, actions, end_mask, terminal = steps[s]
      assert steps[s][0] == s and torch.equal(actions, a)
      assert torch.equal(end_mask, lf.u8(lf.END_MASK.get(s, (0, 0, 0)))), (s, end_mask)
      at, obs, action, logp, value, reward, term, episode_end = adds[s]
      assert at == t
      assert torch.equal(obs, torch.full((lf.N_ENV, 2), float(s))), 'the block stores the observation the action was taken on'
      assert torch.equal(action, a) and torch.equal(logp, l) and torch.equal(value, v), 'the policy at that observation and draw'
      assert torch.equal(reward, lf.reward_of(s)) and torch.equal(term, terminal)
      assert torch.equal(episode_end, terminal | end_mask), s
      s += 1
    k = it * (horizon + 1) + horizon
    assert torch.equal(acts[k][1], torch.full((lf.N_ENV, 2), float(s))), 'the bootstrap act sees the observation after the last step'
    boot, gamma, lam, normalize = finishes[it]
    assert torch.equal(boot, lf.ppo_act(k)[2]) and (gamma, lam, normalize) == (0.75, 0.5, True)
  assert s == 14 and len(finishes) == 2
  # the updates: every token of every pass once, in order; the first update captures, the others replay
  updates = log.named('update')
  assert [u[1] for u in updates] == [(p, j) for p in range(2 * epochs) for j in range(per_pass)]
  assert [u[0] for u in updates] == ['capture'] + ['train_step'] * (2 * epochs * per_pass - 1)
  assert all(p[1] == batch for p in log.named('pass'))
  # the iteration dicts (test_collect_host.py's episodes: the same environment and limit)
  assert [d['updates'] for d in stats] == [epochs * per_pass] * 2
  assert [d['episodes'] for d in stats] == [6, 6] and [d['transitions'] for d in stats] == [21, 42]
  assert stats[0]['mean_loss'] == pytest.approx((1.0 + 3.0 * 9) / 10) and stats[1]['mean_loss'] == pytest.approx(3.0)
  rewards = torch.stack([lf.reward_of(i) for i in range(14)])
  assert [d['time_within_radius'] for d in stats] == [int((rewards[:7] > 0.5).sum()) / 21, int((rewards[7:] > 0.5).sum()) / 21]
  # mean_return: the summed rewards of the episodes that ended in the iteration
  ends = torch.stack([a[7] for a in adds]).bool()
  want, running = [], torch.zeros(lf.N_ENV, dtype=torch.float64)
  for it in range(2):
    done = []
    for i in range(it * 7, it * 7 + 7):
      running += rewards[i].double()
      done += running[ends[i]].tolist()
      running[ends[i]] = 0.0
    want.append(sum(done) / len(done))
  assert [d['mean_return'] for d in stats] == pytest.approx(want, rel=1e-6)


def test_ppo_loop_without_capture():
  import loop_fakes as lf
  from balloon_learning_environment_amd import train_lib
  log = lf.Log()
  train_lib.run_ppo_loop_vec(lf.FakeEnv(log), lf.FakePPOTrainer(log), lf.FakeRollout(log, 4), num_iterations=1, epochs=3, batch_size=6,
                             max_episode_length=4, capture_graph=False)
  assert [u[0] for u in log.named('update')] == ['train_step'] * (3 * 2)
  assert [int(s[2].sum()) for s in log.named('step')] == [0, 0, 0, 1]


# ---- the actor stream ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  return ppo_host.build_actor_draws(tmp_path_factory.mktemp('acd'))


@pytest.mark.parametrize('seed,env,step', [(0, 0, 0), (11, 64, 1), (0xFEDCBA9876543210, 3000, 7), (11, 5, 2 ** 32 + 3), (3, 70000, 2 ** 40)])
def test_actor_draws_are_philox4x32(draws, seed, env, step):
  """Environment e's stream at `step`: key = (seed ^ "ACTOR") low word, high word ^ the step's high word; counter block 0 =
  (0, step low, e low, e high); the first word used is the block's last."""
  got = int(draws(seed, env, 1, step)[0])
  s = seed ^ ppo_host.ACTOR_STREAM
  key = np.array([s & 0xFFFFFFFF, (s >> 32) ^ (step >> 32)], np.uint64)
  out = plan_host.philox4x32(np.array([0, step & 0xFFFFFFFF, env & 0xFFFFFFFF, env >> 32], np.uint64), key)
  assert got == int(out[3])
  assert int(draws(seed, 0, env + 1, step)[env]) == got                   # env_offset + i is the key, not the row
  assert int(draws(seed, env, 1, step + 1)[0]) != got


def test_actor_stream_differs_from_the_epsilon_greedy_stream(draws):
  """For equal (seed, environment, step) the two streams share no word: the actor head and ble_qnet_explore_u8 of one seed draw
  independently."""
  for seed, step in ((0, 0), (11, 3), (2 ** 63 + 5, 2 ** 32 + 1)):
    a, e = draws(seed, 0, 4096, step), draws.explore(seed, 0, 4096, step)
    assert (a != e).mean() > 0.999
    assert abs(np.corrcoef(ppo_host.uniform24(a), ppo_host.uniform24(e))[0, 1]) < 0.06      # (4 sigma of 1 / sqrt(4096))
  u = ppo_host.uniform24(draws(5, 0, 4096, 9))
  assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12 / 4096)


# ---- the descriptors and the parameters ----------------------------------------------------------------------------------------------
_CTYPE = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'float': ctypes.c_float, 'unsigned long long': ctypes.c_uint64}


def _header_fields(name):
  header = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  body = header[header.index(f'typedef struct {name} {{'):header.index(f'}} {name};')]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  fields = []
  for decl in body.split('{', 1)[1].split(';'):
    decl = decl.strip()
    if not decl:
      continue
    if '*' in decl:
      fields.append((decl.rsplit('*', 1)[1].strip(), ctypes.c_void_p))
      continue
    m = re.match(r'(unsigned long long|\w+)\s+(.*)$', decl)
    fields += [(n.strip(), _CTYPE[m.group(1)]) for n in m.group(2).split(',')]
  return fields


@pytest.mark.parametrize('name,mirror,size', [('ble_ac_rows_f32', _abi.BleAcRowsF32, 56), ('ble_ac_sample', _abi.BleAcSample, 32),
                                              ('ble_gae_block_f32', _abi.BleGaeBlockF32, 80), ('ble_ppo_f32', _abi.BlePpoF32, 32)])
def test_structs_match_header(name, mirror, size):
  rename = {'lambda': 'lam'}
  assert [(rename.get(n, n), t) for n, t in _header_fields(name)] == list(mirror._fields_)
  assert ctypes.sizeof(mirror) == size


def test_new_entry_points_are_additive_and_declared_without_int64():
  lib = _lib.lib()
  assert _lib.ABI_VERSION == 5
  for name in ('ble_ac_act_f32', 'ble_gae_f32', 'ble_adv_normalize_f32', 'ble_qnet_ppo_step_f32'):
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS
    assert ctypes.c_int64 not in getattr(lib, name).argtypes, name


def test_init_params_actor_critic():
  from balloon_learning_environment_amd.agents import actor_critic, qnet
  p = actor_critic.init_params('actor_critic', 3, 3, 32)['params']
  assert [p[f'Dense_{i}']['kernel'].shape for i in range(3)] == [(1099, 32), (32, 32), (32, 6)]
  assert all(not p[f'Dense_{i}']['bias'].any() for i in range(3))
  last = p['Dense_2']['kernel']
  limit = np.sqrt(6.0 / (32 + 6))
  assert np.abs(last[:, [1, 3, 5]]).max() <= limit and np.abs(last[:, [1, 3, 5]]).max() > 0.5 * limit
  assert np.abs(last[:, [0, 2, 4]]).max() <= 0.01 * limit * (1 + 1e-6) and last[:, [0, 2, 4]].any()
  assert np.abs(p['Dense_0']['kernel']).max() <= np.sqrt(6.0 / (1099 + 32))
  again = actor_critic.init_params('actor_critic', 3, 3, 32)['params']
  assert all(np.array_equal(p[k]['kernel'], again[k]['kernel']) for k in p)
  net = qnet.QNetwork.from_params({'params': p}, num_atoms=2)
  assert net.shape == (3, 32, 2)
  with pytest.raises(ValueError):
    actor_critic.init_params('quantile')
  with pytest.raises(ValueError, match='two-atom'):
    actor_critic.VecActorCriticAgent(qnet.QNetwork.from_params(qnet.init_params('mlp', 0, 2, 8)))
