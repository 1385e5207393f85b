"""Expert iteration on the device: ble_plan_prior_u16, ble_plan_sample_prior_u8, ble_plan_action_values_f32,
ble_qnet_soft_bc_step_f32, VecLookaheadAgent's prior and action values, agents/expert_iteration.py and train_lib.run_exit_loop_vec.

References.  The prior counts, the sampler with a prior and the action values: the NumPy twins written from the definitions
(tests/exit_host.py), bit for bit -- integers, an order on float32 values, and one float32 product.  The soft loss: its float64 twin on
the device's own logits within test_gpu_td.py's bounds; ble_qnet_bc_step_f32 itself, bit for bit, on rows with one valid value; float64
backprop for the gradient image.  The planner with a prior: the flight itself (wind='truth').  The loop: a recording environment and a
recording planner.  Learning: test_gpu_train.py's contextual bandit, held to its 90 % bar on a float64 torch-autograd restatement first."""
import ctypes

import numpy as np
import pytest
import torch

import exit_host
import imitation_host
import plan_host
import ppo_host
import train_host

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
POLICY = [0, 2, 4]


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import actor_critic, expert_iteration, imitation, qnet, qnet_train
  return qnet, qnet_train, actor_critic, imitation, expert_iteration


@pytest.fixture(scope='module')
def observations():
  """1024 device observations of real balloons (reset + a few random steps), float32 [1024, 1099]."""
  from balloon_learning_environment_amd.env import balloon_env
  env = balloon_env.VecBalloonEnv(256, seed=3)
  rows = [env.reset().clone()]
  g = torch.Generator(device='cuda').manual_seed(0)
  for _ in range(3):
    obs, _, _ = env.step(torch.randint(0, 3, (256,), dtype=torch.uint8, device='cuda', generator=g))
    rows.append(obs.clone())
  env.check_errors()
  return torch.cat(rows)


@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  return ppo_host.build_actor_draws(tmp_path_factory.mktemp('exd'))


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lib():
  from balloon_learning_environment_amd import _abi, _lib as lib, device as dev
  return _abi, lib, dev


# ------------------------------------------------------------------------------------------------------------------- 1: prior counts
SPECIAL_ROWS = np.array([[1.0, 0.0, 0.0], [1 / 3, 1 / 3, 1 / 3], [1e-40, 0.5, 0.5], [np.nan, 0.5, 0.5], [-0.25, 0.75, 0.5], [1.5, 0.25, 0.25],
                         [0.999, 5e-4, 5e-4]], np.float32)


def _gpu_prior(probs, strength, segments):
  _abi, lib, dev = _lib()
  n = len(probs)
  p = _dev(np.asarray(probs, np.float32))
  counts = torch.full((n, segments, 3), -1, dtype=torch.int16, device=DEVICE)
  pr = _abi.BlePlanPrior(n, segments, strength, p.data_ptr(), counts.data_ptr())
  lib.check(lib.lib().ble_plan_prior_u16(ctypes.byref(pr), dev.stream_ptr(torch.device(DEVICE))), 'ble_plan_prior_u16')
  torch.cuda.synchronize()
  return counts.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_prior_counts_against_the_twin(n):
  rng = np.random.default_rng(n)
  random_rows = rng.dirichlet(np.ones(3), n).astype(np.float32)
  batches = [SPECIAL_ROWS[i:i + 1] for i in range(len(SPECIAL_ROWS))] if n == 1 else [np.concatenate([SPECIAL_ROWS, random_rows])[:n]]
  for probs in batches:
    for segments in (1, 6, 17, 240):
      for strength in (0, 1, 64, 65535):
        got = _gpu_prior(probs, strength, segments)
        assert np.array_equal(got, exit_host.prior_counts(probs, strength, segments)), (n, segments, strength)
        assert not got[:, 16:].any() and (strength > 0 or not got.any())


# ------------------------------------------------------------------------------------------------------- 2: the sampler with a prior
def _gpu_sample(n, K, H, segment, iteration, decision, prior=None, seed=0, env_seed=None, env_offset=0, counts=None, best_plan=None):
  """ble_plan_sample_prior_u8 with prior counts, ble_plan_sample_u8 with prior=None."""
  _abi, lib, dev = _lib()
  counter = _dev(np.array([decision & (2 ** 64 - 1)], np.uint64).view(np.int64))
  env_seed_t = None if env_seed is None else _dev(np.asarray(env_seed, np.uint64).view(np.int64))
  counts_t = None if counts is None else _dev(np.asarray(counts, np.uint16).view(np.int16))
  prior_t = None if prior is None else _dev(np.asarray(prior, np.uint16).view(np.int16))
  best = _dev(np.full((H, n), 1, np.uint8) if best_plan is None else best_plan)
  plans = torch.full((H, n, K), 9, dtype=torch.uint8, device=DEVICE)
  fields = (n, K, H, segment, iteration, seed & (2 ** 64 - 1), dev.ptr(env_seed_t), env_offset, counter.data_ptr(), dev.ptr(counts_t),
            best.data_ptr(), plans.data_ptr())
  stream = dev.stream_ptr(torch.device(DEVICE))
  if prior is None:
    lib.check(lib.lib().ble_plan_sample_u8(ctypes.byref(_abi.BlePlanSample(*fields)), stream), 'ble_plan_sample_u8')
  else:
    lib.check(lib.lib().ble_plan_sample_prior_u8(ctypes.byref(_abi.BlePlanSamplePrior(*fields, prior_t.data_ptr())), stream),
              'ble_plan_sample_prior_u8')
  torch.cuda.synchronize()
  return plans.cpu().numpy()


SAMPLER_SHAPES = [(1, 1, 1), (4, 24, 4), (5, 24, 4), (64, 24, 4), (65, 24, 4), (1024, 24, 4), (4, 960, 4)]      # K, H, segment


@pytest.mark.parametrize('env_seeds', [False, True], ids=['ScalarSeed', 'EnvSeed'])
@pytest.mark.parametrize('K,H,segment', SAMPLER_SHAPES)
def test_sampler_with_a_prior(K, H, segment, env_seeds):
  n = 3 if K == 1024 else 65
  S = -(-H // segment)
  rng = np.random.default_rng(K + H)
  prev = rng.integers(0, 3, (H, n)).astype(np.uint8)
  decision = int(rng.integers(0, 2 ** 40))
  kw = dict(env_seed=rng.integers(0, 2 ** 63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1)) if env_seeds else dict(seed=17, env_offset=1000)
  # zero counts: ble_plan_sample_u8's plans, bit for bit
  zero = _gpu_sample(n, K, H, segment, 0, decision, prior=np.zeros((n, S, 3), np.uint16), best_plan=prev, **kw)
  assert np.array_equal(zero, _gpu_sample(n, K, H, segment, 0, decision, best_plan=prev, **kw))
  # counts: the twin's plans, bit for bit
  prior = exit_host.prior_counts(rng.dirichlet(np.ones(3) * 0.5, n).astype(np.float32), 65535 if K % 2 else 64, S)
  prior[0, 0] = (65535, 65535, 65535)
  got = _gpu_sample(n, K, H, segment, 0, decision, prior=prior, best_plan=prev, **kw)
  assert np.array_equal(got, exit_host.sample_prior(n, K, H, segment, 0, decision, prior, best_plan=prev, **kw))
  assert np.array_equal(got[:, :, :4], zero[:, :, :4])                   # the fixed slots and the warm start stay
  if K >= 64:
    assert not np.array_equal(got, zero)
  # iterations >= 1 read elite_counts, not the prior
  counts = rng.integers(0, 9, (n, S, 3)).astype(np.uint16)
  later = _gpu_sample(n, K, H, segment, 1, decision, prior=prior, counts=counts, best_plan=prev, **kw)
  assert np.array_equal(later, _gpu_sample(n, K, H, segment, 1, decision, counts=counts, best_plan=prev, **kw))


def test_sampler_with_a_prior_batch_invariance():
  """Plan k of an environment is the same at any n, any K and any position in the batch (DESIGN 3k's contract, with a prior)."""
  rng = np.random.default_rng(2)
  n, H, segment = 65, 7, 3
  seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64)
  prev = rng.integers(0, 3, (H, n)).astype(np.uint8)
  prior = rng.integers(0, 70, (n, 3, 3)).astype(np.uint16)
  batch = _gpu_sample(n, 67, H, segment, 0, 4, prior=prior, env_seed=seeds, best_plan=prev)
  for e in (0, 17, 64):
    alone = _gpu_sample(1, 67, H, segment, 0, 4, prior=prior[e:e + 1], env_seed=seeds[e:e + 1], best_plan=prev[:, e:e + 1])
    assert np.array_equal(alone[:, 0], batch[:, e]), e
  assert np.array_equal(_gpu_sample(n, 5, H, segment, 0, 4, prior=prior, env_seed=seeds, best_plan=prev), batch[:, :, :5])
  whole = _gpu_sample(n, 9, H, segment, 0, 9, prior=prior, seed=3)
  assert np.array_equal(_gpu_sample(3, 9, H, segment, 0, 9, prior=prior[40:43], seed=3, env_offset=40), whole[:, 40:43])


# --------------------------------------------------------------------------------------------------------------- 3: action values
def _gpu_action_values(ret, first, stored=None):
  _abi, lib, dev = _lib()
  n, K = ret.shape
  ret_t, first_t = _dev(np.asarray(ret, np.float32)), _dev(np.asarray(first, np.uint8))
  if stored is None:
    q = torch.full((n, 3), 123.0, dtype=torch.float32, device=DEVICE)
    q_k, visits = (torch.full((n, 3), 77, dtype=torch.int32, device=DEVICE) for _ in range(2))
  else:
    q, q_k, visits = (_dev(np.array(s)) for s in stored)
  av = _abi.BlePlanActionValues(n, K, 0 if stored is None else 1, ret_t.data_ptr(), first_t.data_ptr(), q.data_ptr(), q_k.data_ptr(),
                                visits.data_ptr())
  lib.check(lib.lib().ble_plan_action_values_f32(ctypes.byref(av), dev.stream_ptr(torch.device(DEVICE))), 'ble_plan_action_values_f32')
  torch.cuda.synchronize()
  return q.cpu().numpy(), q_k.cpu().numpy(), visits.cpu().numpy()


def _same_values(got, want, what):
  assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, 'q')
  assert np.array_equal(got[1], want[1]), (what, 'q_k')
  assert np.array_equal(got[2], want[2]), (what, 'visits')


def _returns(rng, n, K):
  """NaN, +-Inf, -0 and +0 together, and many exact ties."""
  ret = (rng.integers(0, 6, (n, K)).astype(np.float32) - np.float32(2.0)) * np.float32(0.25)
  for value in (np.nan, np.inf, -np.inf, -0.0, 0.0):
    ret[rng.random((n, K)) < 0.1] = np.float32(value)
  return ret


@pytest.mark.parametrize('n', [1, 65])
@pytest.mark.parametrize('K', [1, 3, 4, 64, 65, 1024])
def test_action_values_against_the_twin(K, n):
  rng = np.random.default_rng(K + n)
  ret, first = _returns(rng, n, K), rng.integers(0, 3, (n, K)).astype(np.uint8)
  first[0] = np.where(first[0] == 1, 2, first[0])                      # an action no plan takes
  if K >= 5:
    ret[0, :5] = (np.nan, np.inf, -np.inf, -0.0, 0.0)
  if n > 2:
    ret[1] = np.nan                                                    # an environment without a finite plan
    first[2, K // 2] = 7                                               # (>= 2 counts as 2)
  got = _gpu_action_values(ret, first)
  want = exit_host.action_values(ret, first)
  _same_values(got, want, (K, n))
  assert got[2][0, 1] == 0 and got[0][0, 1] == -np.inf and got[1][0, 1] == -1
  assert (got[2].sum(1) == K).all()
  # a second call accumulates: against the same plans (every entry ties), a better, a worse and a non-finite newcomer
  newcomers = {'tie': ret.copy(), 'better': np.where(np.isfinite(ret), ret + np.float32(0.25), ret),
               'worse': np.where(np.isfinite(ret), ret - np.float32(0.25), ret), 'non_finite': np.full_like(ret, np.nan),
               'mixed': _returns(rng, n, K)}
  for name, ret2 in newcomers.items():
    first2 = first if name != 'mixed' else rng.integers(0, 3, (n, K)).astype(np.uint8)
    got2 = _gpu_action_values(ret2, first2, got)
    _same_values(got2, exit_host.action_values(ret2, first2, want), (K, n, name))
    if name in ('tie', 'worse', 'non_finite'):
      assert np.array_equal(_bits(got2[0]), _bits(got[0])) and (got2[1] == -1).all(), name
    if name == 'better':
      assert np.array_equal(got2[1], got[1]), name                      # the same plans win again, with their new returns


@pytest.mark.parametrize('wind,iterations', [('forecast', 1), ('forecast', 2), ('scenarios', 1), ('scenarios', 2)])
def test_action_values_after_a_real_decision(wind, iterations):
  """The invariant with the selection: q[e][action[e]] has best_return[e]'s bits and no other entry of q[e] comes before it."""
  from balloon_learning_environment_amd.env import balloon_env
  n, K, H = 8, 8, 8
  env = balloon_env.VecBalloonEnv(n, seed=3, auto_reset=False)
  obs = env.reset()
  kw = dict(num_scenarios=4, risk_tail=2) if wind == 'scenarios' else {}
  agent = env.planner(num_plans=K, horizon=H, segment=2, wind=wind, iterations=iterations, elite=3, seed=5, action_values=True, **kw)
  plain = env.planner(num_plans=K, horizon=H, segment=2, wind=wind, iterations=iterations, elite=3, seed=5, **kw)
  for decision in range(3):
    action = agent.act(obs).clone()
    assert torch.equal(plain.act(obs), action) and torch.equal(plain.best_return.view(torch.int32), agent.best_return.view(torch.int32))
    q, visits = (t.cpu().numpy() for t in agent.action_values())
    best, act = agent.best_return.cpu().numpy(), action.cpu().numpy()
    assert np.isfinite(best).all() and (visits.sum(1) == K * iterations).all()
    for e in range(n):
      assert _bits(q[e, act[e]]) == _bits(best[e]), (decision, e)
      assert q[e, plan_host.order(q[e])[0]] == q[e, act[e]], (decision, e, 'an entry of q comes before the chosen action')
    if iterations == 1:
      _same_values((q, agent.q_k.cpu().numpy(), visits), exit_host.action_values(agent.returns.cpu().numpy(), agent.plans[0].cpu().numpy()),
                   decision)
    obs, _, _ = env.step(action)
  env.check_errors()
  with pytest.raises(ValueError, match='action_values=True'):
    plain.action_values()


# -------------------------------------------------------------------------------------------------------------------- 4: the soft loss
SHAPES = [(2, 64), (3, 256), (8, 600)]


def _params(qnet, ac, layers, hidden, seed=7, bias=1e-2):
  """QuantileNetwork-scale kernels with two atoms and small random biases (policies far from uniform); init_params' own at (3, 256)."""
  if (layers, hidden) == (3, 256):
    return ac.init_params('actor_critic', seed, layers, hidden)
  params = qnet.init_params('quantile', seed, layers, hidden, 2)
  rng = np.random.default_rng(seed + 1)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * bias).astype(np.float32)
  return params


def _soft(mods, layers, hidden, **kw):
  qnet, _, ac, _, ei = mods
  params = _params(qnet, ac, layers, hidden)
  return params, ei.SoftBCTrainer(qnet.QNetwork.from_params(params, num_atoms=2), **kw)


def _close(got, want, name):
  scale = np.abs(want).max()
  assert np.allclose(got, want, rtol=2e-6, atol=1e-7 * scale), (name, np.abs(got - want).max(), scale)


def _ratio(got, want):
  """|got - want| as a fraction of _close's bound."""
  return float((np.abs(got - want) / (2e-6 * np.abs(want) + 1e-7 * np.abs(want).max() + 1e-300)).max())


def _views(tr, b):
  return {k: t.cpu().numpy() for k, t in tr.views(b).items() if k != 'acts'}


def _target_q(rng, b):
  """Rows with three, two, one and no valid value in turn (row 0: three), the invalid ones NaN, +Inf or -Inf; a few exact ties."""
  q = (rng.standard_normal((b, 3)) * 2).astype(np.float32)
  q[rng.random((b, 3)) < 0.2] = np.float32(0.5)
  for i in range(b):
    kind = i % 4
    bad = rng.permutation(3)[:kind]
    q[i, bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(bad))
  return q


@pytest.mark.parametrize('b,layers,hidden', [(b, l, h) for l, h in SHAPES for b in (1, 32, 300)])
def test_soft_loss_aux_and_dlogits(mods, observations, layers, hidden, b):
  """Measured on an MI355X over the nine shapes and the three (beta, s, c_v) triples (one run), the worst |device - twin| as a fraction
  of _close's bound: loss 0.104, aux[:, 0] 0.081, dlogits 0.517 (all at (3, 256), B = 300; the last at s = 0, c_v = 0).
  test_gpu_td.py's bounds stand unwidened."""
  ei = mods[4]
  _, tr = _soft(mods, layers, hidden)
  rng = np.random.default_rng(b)
  x = observations.cpu().numpy()[rng.integers(0, len(observations), b)]
  q = _target_q(rng, b)
  ret = rng.standard_normal(b).astype(np.float32)
  bt = ei.SoftBatch.from_tensors(x, q, ret, 'cuda')
  for temperature, s, cv in ((1.0, 0.0, 0.0), (0.5, 0.1, 0.5), (2.0, 0.0, 0.5)):
    tr.temperature, tr.label_smoothing, tr.value_coef = temperature, s, cv
    tr.workspace(b)
    tr.views(b)['dlogits'].fill_(float('nan'))                          # every column up to ld is written by the call
    loss_d = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
    tr.check_errors()                                                   # a row without a valid value raises no flag
    v = _views(tr, b)
    loss, aux, dlog = exit_host.soft_bc_loss(v['logits'], q, ret, 1.0 / temperature, s, cv)
    print('B', b, (layers, hidden), 'T', temperature, 's', s, 'c_v', cv, 'err / bound: loss', _ratio(loss_d, loss), 'lp_star',
          _ratio(v['aux'][:, 0], aux[:, 0]), 'dlogits', _ratio(v['dlogits'][:, :6], dlog))
    _close(loss_d, loss, 'loss')
    _close(v['aux'][:, 0], aux[:, 0], 'lp_star')
    _close(v['dlogits'][:, :6], dlog, 'dlogits')
    assert np.array_equal(v['aux'][:, 1], aux[:, 1].astype(np.float32)), 'agree'
    assert _bits(v['dlogits'][:, 6:]).max(initial=0) == 0 and _bits(v['dlogits'][:, [3, 5]]).max() == 0      # +0.0 over the NaN fill
    assert v['dlogits'].shape[1] >= max(hidden, 6) and not np.isnan(v['dlogits']).any()
    dead = ~np.isfinite(q).any(axis=1)
    assert dead.sum() == b // 4
    for name, a in (('loss', loss_d), ('aux', v['aux']), ('dlogits', v['dlogits'])):
      assert _bits(a[dead]).max(initial=0) == 0, (name, 'a row without a valid value is all zeros')
    if cv == 0.0:
      assert not v['dlogits'][:, 1].any()


def test_a_two_valid_row_gives_the_invalid_action_zero_exactly(mods, observations):
  """s = 0: t'_a = t_a, so the invalid action's gradient is p_a / B, the acting head's own probability (the same bits: the training
  forward is the acting forward) divided once."""
  ei = mods[4]
  _, tr = _soft(mods, 2, 64, temperature=0.5)
  b = 32
  rng = np.random.default_rng(3)
  obs = observations[100:100 + b]
  q = (rng.standard_normal((b, 3)) * 2).astype(np.float32)
  bad = rng.integers(0, 3, b)
  q[np.arange(b), bad] = np.where(np.arange(b) % 2 == 0, np.nan, -np.inf).astype(np.float32)
  tr.train_on_batch(ei.SoftBatch.from_tensors(obs.cpu().numpy(), q, np.zeros(b), 'cuda'), apply_update=False)
  probs = torch.zeros(b, 3, device='cuda')
  tr.act_greedy(obs, probs=probs)
  p = probs.cpu().numpy()
  d = _views(tr, b)['dlogits']
  assert np.array_equal(_bits(d[np.arange(b), 2 * bad]), _bits(p[np.arange(b), bad] / np.float32(b)))
  t = exit_host.soft_target(q, 2.0, 0.0)
  assert not t[np.arange(b), bad].any()


@pytest.mark.parametrize('smoothing,value_coef', [(0.0, 0.0), (0.1, 0.0), (0.0, 0.5), (0.1, 0.5)])
def test_rows_with_one_valid_value_equal_the_cloning_step_bit_for_bit(mods, observations, smoothing, value_coef):
  qnet, _, ac, im, ei = mods
  b = 32
  rng = np.random.default_rng(5)
  x = observations.cpu().numpy()[rng.integers(0, len(observations), b)]
  label = rng.integers(0, 3, b).astype(np.uint8)
  ret = rng.standard_normal(b).astype(np.float32)
  q = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), (b, 3))
  q[np.arange(b), label] = (rng.standard_normal(b) * 50).astype(np.float32)
  params = _params(qnet, ac, 2, 64)
  hard = im.BCTrainer(qnet.QNetwork.from_params(params, num_atoms=2), label_smoothing=smoothing, value_coef=value_coef)
  hard.train_on_batch(ac.PPOBatch.from_tensors(x, ret, label, np.zeros(b), np.zeros(b), 'cuda'), apply_update=False)
  want = _views(hard, b)
  for temperature in (0.25, 1.0, 3.0):
    soft = ei.SoftBCTrainer(qnet.QNetwork.from_params(params, num_atoms=2), temperature=temperature, label_smoothing=smoothing,
                            value_coef=value_coef)
    soft.train_on_batch(ei.SoftBatch.from_tensors(x, q, ret, 'cuda'), apply_update=False)
    got = _views(soft, b)
    for name in ('logits', 'loss', 'aux', 'dlogits'):
      assert np.array_equal(_bits(got[name]), _bits(want[name])), (name, temperature)
    assert np.array_equal(_bits(soft.grad.cpu().numpy()), _bits(hard.grad.cpu().numpy()))
  assert want['loss'].all()


def test_soft_gradient_against_float64_backprop(mods, observations):
  """The gradient image within backward_magnitude's 1e-5 bound at B = 32 on (3, 256), as the PPO and BC tests hold theirs."""
  qnet, qnet_train, ac, _, ei = mods
  layers, hidden, b = 3, 256, 32
  params, tr = _soft(mods, layers, hidden, temperature=0.5, label_smoothing=0.1, value_coef=0.5)
  rng = np.random.default_rng(4)
  x = observations.cpu().numpy()[rng.integers(0, len(observations), b)]
  tr.train_on_batch(ei.SoftBatch.from_tensors(x, _target_q(rng, b), rng.standard_normal(b).astype(np.float32), 'cuda'), apply_update=False)
  v = tr.views(b)
  acts = [a.cpu().numpy() for a in v['acts']]
  acts = [a[:, :hidden] for a in acts[:-1]] + [acts[-1][:, :6]]
  dlog = v['dlogits'].cpu().numpy()[:, :6]
  want, mag = train_host.backward(params, x, dlog, acts), train_host.backward_magnitude(params, x, dlog, acts)
  got = qnet_train.unpack(tr._net, tr.grad.cpu().numpy())['params']
  worst = 0.0
  for l in range(layers):
    for leaf, i in (('kernel', 0), ('bias', 1)):
      err = np.abs(got[f'Dense_{l}'][leaf] - want[l][i])
      worst = max(worst, float((err / (1e-5 * mag[l][i] + 1e-30)).max()))
  print('B', b, 'worst |g - g64| / (1e-5 S)', worst)
  assert worst <= 1.0, worst
  assert any(np.abs(want[l][0]).max() > 0 for l in range(layers))
  last = got[f'Dense_{layers - 1}']
  assert not last['kernel'][:, [3, 5]].any() and not last['bias'][[3, 5]].any()


def _student(mods, seed=2, **kw):
  qnet, _, ac, _, ei = mods
  return ei.SoftBCTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', seed, 2, 64), num_atoms=2), lr=1e-3, temperature=0.5,
                          label_smoothing=0.1, value_coef=0.5, **kw)


def _fill(bt, rows):
  x, q, ret = rows
  bt.state[:, :1099].copy_(torch.from_numpy(x))
  bt.target_q.copy_(torch.from_numpy(q))
  bt.ret.copy_(torch.from_numpy(ret))


def test_soft_graph_replay_equals_eager_and_resume(mods, observations):
  ei = mods[4]
  rng = np.random.default_rng(8)
  x = observations.cpu().numpy()
  data = [(x[rng.integers(0, len(x), 128)], _target_q(rng, 128), rng.standard_normal(128).astype(np.float32)) for _ in range(5)]
  eager, graph = _student(mods), _student(mods)
  bt_e, bt_g = ei.SoftBatch(128, 'cuda'), ei.SoftBatch(128, 'cuda')
  first = eager.weights.cpu().numpy().copy()
  sd = None
  for k, rows in enumerate(data):
    _fill(bt_e, rows)
    eager.train_on_batch(bt_e)
    _fill(bt_g, rows)
    loss = graph.capture(bt_g) if k == 0 else graph.train_step(bt_g)
    assert np.array_equal(_bits(loss.cpu().numpy()), _bits(eager.views(128)['loss'].cpu().numpy())), k
    if k == 1:
      sd = eager.state_dict()
  assert 128 in graph._graphs and graph._graphs[128][1] is bt_g
  we = eager.weights.cpu().numpy()
  assert int(eager.adam_step.item()) == 5 and int(graph.adam_step.item()) == 5
  assert np.array_equal(_bits(we), _bits(graph.weights.cpu().numpy())), 'graph replay differs from eager'
  assert not np.array_equal(we, first)
  eager.check_errors()
  graph.check_errors()
  # a state_dict taken after two updates resumes to the same bits; a changed hyperparameter drops the captured graphs
  other = _student(mods, seed=9)
  other.temperature = 2.0
  bt_o = ei.SoftBatch(128, 'cuda')
  _fill(bt_o, data[0])
  other.capture(bt_o)
  assert other._graphs
  other.load_state_dict(sd)
  assert not other._graphs and other.temperature == 0.5 and (other.label_smoothing, other.value_coef) == (0.1, 0.5)
  assert int(other.adam_step.item()) == 2
  for rows in data[2:]:
    _fill(bt_o, rows)
    other.train_step(bt_o)
  assert np.array_equal(_bits(we), _bits(other.weights.cpu().numpy())), 'resume differs'


def test_label_buffer_minibatches(mods, observations):
  """VecRolloutBuffer.minibatches' contract: one yielded batch object, distinct rows per pass, a generator whose state can be restored."""
  ei = mods[4]
  t, n = 4, 64
  buf = ei.VecPlanLabelBuffer(n, t)
  for step in range(t):
    obs = observations[step * n:(step + 1) * n].clone()
    ids = torch.arange(step * n, (step + 1) * n, device='cuda', dtype=torch.float32)
    buf.add(step, obs, torch.stack([ids, ids + 0.25, ids + 0.5], 1), -ids)
  state = buf.state_dict()
  seen, objects, order = [], set(), []
  for bt in buf.minibatches(48):
    objects.add(id(bt))
    ids = (-bt.ret).cpu().numpy().astype(np.int64)
    assert torch.equal(bt.state[:, :1099], observations[torch.from_numpy(ids).cuda()])
    assert np.array_equal(bt.target_q.cpu().numpy(), np.stack([ids, ids + 0.25, ids + 0.5], 1).astype(np.float32))
    seen.extend(ids.tolist())
    order.append(ids)
  assert len(objects) == 1 and len(order) == t * n // 48 and len(set(seen)) == len(seen) == 48 * (t * n // 48)
  again = [(-bt.ret).cpu().numpy().astype(np.int64) for bt in buf.minibatches(48)]
  assert not all(np.array_equal(a, b) for a, b in zip(order, again))
  buf.load_state_dict(state)
  assert all(np.array_equal(a, (-bt.ret).cpu().numpy().astype(np.int64)) for a, bt in zip(order, buf.minibatches(48)))
  g = torch.Generator(device='cuda').manual_seed(5)
  one = [(-bt.ret).cpu().numpy().copy() for bt in buf.minibatches(48, g)]
  g.manual_seed(5)
  assert all(np.array_equal(a, (-bt.ret).cpu().numpy()) for a, bt in zip(one, buf.minibatches(48, g)))


# ------------------------------------------------------------------------------------------------------ 5: the planner with a prior
def _planning_env(n, seed=8, steps=3):
  from balloon_learning_environment_amd.env import balloon_env
  env = balloon_env.VecBalloonEnv(n, seed=seed, auto_reset=False)
  obs = env.reset()
  rng = np.random.default_rng(seed)
  for a in rng.integers(0, 3, (steps, n)).astype(np.uint8):
    obs, _, _ = env.step(_dev(a))
  return env, obs.clone()


def _actor(mods, seed=2):
  qnet, _, ac, _, _ = mods
  return ac.VecActorCriticAgent(qnet.QNetwork.from_params(_params(qnet, ac, 2, 64, seed=seed), num_atoms=2))


def test_the_plan_chosen_under_a_prior_is_real(mods):
  """wind='truth': the chosen plan flown with env.step earns best_return bit for bit (DESIGN 3k's property, with a prior)."""
  n, K, H = 4, 8, 6
  env, obs = _planning_env(n)
  probs = torch.zeros(n, 3, device=DEVICE)
  _actor(mods).act(obs, probs=probs)
  agent = env.planner(num_plans=K, horizon=H, segment=2, wind='truth', seed=n, prior_strength=64, action_values=True)
  plain = env.planner(num_plans=K, horizon=H, segment=2, wind='truth', seed=n)
  agent.act(obs, prior_probs=probs)
  plain.act(obs)
  assert not torch.equal(agent.plans, plain.plans), 'the prior moved no plan'
  assert torch.equal(agent.plans[:, :, :4], plain.plans[:, :, :4])
  want = exit_host.sample_prior(n, K, H, 2, 0, 0, exit_host.prior_counts(probs.cpu().numpy(), 64, 3), seed=n)
  assert np.array_equal(agent.plans.cpu().numpy(), want)
  best_plan, best_return = (t.clone() for t in agent.plan())
  q, _ = agent.action_values()
  assert torch.equal(q[torch.arange(n), best_plan[0].long()].view(torch.int32), best_return.view(torch.int32))
  rewards = torch.stack([env.step(best_plan[h].contiguous())[1] for h in range(H)]).cpu().numpy()
  acc, disc = np.zeros(n, np.float64), 1.0
  for t in range(H):                                     # the kernel's order: the product and the sum rounded separately
    term = disc * rewards[t].astype(np.float64)
    acc += term
    disc *= agent.gamma
  assert np.array_equal(_bits(acc.astype(np.float32)), _bits(best_return.cpu().numpy()))
  env.check_errors()


def test_no_prior_is_todays_planner(mods):
  """prior_strength = 0, or no prior_probs: the decisions of an agent built without the arguments, bit for bit, over 5 decisions."""
  n = 4
  env, obs = _planning_env(n, seed=5)
  actor = _actor(mods)
  probs = torch.zeros(n, 3, device=DEVICE)
  kw = dict(num_plans=8, horizon=6, segment=2, wind='truth', iterations=2, elite=3, seed=1)
  agents = {'plain': env.planner(**kw), 'strength_0': env.planner(prior_strength=0, **kw), 'no_probs': env.planner(prior_strength=64, **kw),
            'values_only': env.planner(action_values=True, **kw)}
  assert agents['plain'].prior_counts is None and agents['plain'].q is None and sorted(agents['no_probs'].state_dict()) == ['best_plan', 'counter']
  for decision in range(5):
    actor.act(obs, probs=probs)
    action = agents['plain'].act(obs).clone()
    for name, agent in agents.items():
      if name == 'plain':
        continue                                           # (it has decided: a second act would be its next decision)
      got = agent.act(obs, prior_probs=probs if name == 'strength_0' else None)
      assert torch.equal(got, action), (decision, name)
      assert torch.equal(agent.best_return.view(torch.int32), agents['plain'].best_return.view(torch.int32)), (decision, name)
      assert torch.equal(agent.plans, agents['plain'].plans) and torch.equal(agent.best_plan, agents['plain'].best_plan), (decision, name)
    obs, _, _ = env.step(action)
  env.check_errors()


def test_a_captured_decision_with_a_prior_replays_to_the_eager_one(mods):
  from balloon_learning_environment_amd import device as dev
  n, decisions = 4, 4
  runs = {}
  for mode in ('eager', 'graph'):
    env, start = _planning_env(n, seed=9)
    actor = _actor(mods)
    agent = env.planner(num_plans=8, horizon=6, segment=2, wind='truth', iterations=2, elite=3, seed=2, prior_strength=64, action_values=True)
    actions = torch.ones(n, dtype=torch.uint8, device=DEVICE)
    probs = torch.zeros(n, 3, device=DEVICE)
    obs = start.clone()

    def body():
      actor.act(obs, probs=probs)
      agent.act(obs, out=actions, prior_probs=probs)
      env._step_eager(actions, obs_out=obs)
    body()                                               # (lazy allocations happen here, in both modes)
    graph = dev.capture(env.device, body)[0] if mode == 'graph' else None
    log = []
    for _ in range(decisions):
      graph.replay() if graph is not None else body()
      torch.cuda.synchronize()
      log.append((actions.cpu().numpy().copy(), _bits(agent.best_return.cpu().numpy()).copy(), int(agent.counter.item()),
                  _bits(agent.q.cpu().numpy()).copy(), agent.visits.cpu().numpy().copy(), agent.prior_counts.cpu().numpy().copy(),
                  obs.cpu().numpy().copy()))
    runs[mode] = log
    env.check_errors()
  for d, (a, b) in enumerate(zip(runs['eager'], runs['graph'])):
    assert a[2] == b[2] == d + 2
    assert all(np.array_equal(x, y) for x, y in zip(a, b) if not isinstance(x, int)), d
  assert any(r[5].any() for r in runs['graph'])


def test_prior_planner_agent_is_the_composition(mods):
  """VecPriorPlannerAgent: the policy's greedy probabilities handed to the planner, decision after decision."""
  ei = mods[4]
  n = 4
  env, obs = _planning_env(n, seed=6)
  kw = dict(num_plans=8, horizon=6, segment=2, wind='forecast', seed=3, prior_strength=64)
  agent = ei.VecPriorPlannerAgent(_actor(mods), env.planner(**kw).__class__(device=DEVICE, **kw)).bind(env.arena.sim)
  by_hand, actor = env.planner(**kw), _actor(mods)
  probs = torch.zeros(n, 3, device=DEVICE)
  for decision in range(3):
    actor.act(obs, probs=probs)
    want = by_hand.act(obs, prior_probs=probs).clone()
    assert torch.equal(agent.act(obs), want), decision
    assert torch.equal(agent.planner.plans, by_hand.plans) and bool(agent.planner.prior_counts.any())
    obs, _, _ = env.step(want)
  assert agent.get_name() == 'PriorLookaheadAgent'
  agent.check_errors()
  env.check_errors()


# ------------------------------------------------------------------------------------------------------------------- 6: the loop
class _RecordingEnv:
  """Forwards reset, step, num_envs, device and check_errors of a VecBalloonEnv and keeps clones of what went in and out."""

  def __init__(self, env):
    self.env, self.num_envs, self.device = env, env.num_envs, env.device
    self.reset_obs, self.steps = None, []

  def reset(self):
    obs = self.env.reset()
    self.reset_obs = obs.clone()
    return obs

  def step(self, actions, end_mask=None):
    went_in = {'actions': actions.clone(), 'end_mask': end_mask.clone()}
    obs, reward, terminal = self.env.step(actions, end_mask=end_mask)
    self.steps.append({**went_in, 'obs': obs.clone(), 'reward': reward.clone(), 'terminal': terminal.clone()})
    return obs, reward, terminal

  def check_errors(self):
    self.env.check_errors()


class _RecordingPlanner:
  """Forwards act, action_values, plan and check_errors of a VecLookaheadAgent and keeps clones of every decision."""

  def __init__(self, agent):
    self.agent, self.decisions = agent, []

  def act(self, obs, out=None, prior_probs=None):
    got = self.agent.act(obs, out, prior_probs=prior_probs)
    q, visits = self.agent.action_values()
    self.decisions.append({'obs': obs.clone(), 'prior': prior_probs.clone(), 'label': got.clone(), 'q': q.clone(), 'visits': visits.clone(),
                           'best_return': self.agent.best_return.clone()})
    return got

  def action_values(self):
    return self.agent.action_values()

  def plan(self):
    return self.agent.plan()

  def check_errors(self):
    self.agent.check_errors()


LOOP_T, LOOP_N, LOOP_LIMIT, LOOP_SEED, LOOP_BETA = 8, 64, 5, 4, 0.5


def test_loop_block_is_what_happened(mods, draws):
  """One iteration of run_exit_loop_vec through a recording environment and a recording planner, against a second trainer of the same
  parameters and seed: target_q[t] is the planner's action_values() at step t, obs[t] the observation that step acted on (across
  auto-resets), the prior this step's probs, the stepped action the twin's mix of (learner, label) at mix step t."""
  qnet, _, ac, _, ei = mods
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.env import balloon_env
  inner = balloon_env.VecBalloonEnv(LOOP_N, seed=1)
  env = _RecordingEnv(inner)
  planner = _RecordingPlanner(inner.planner(num_plans=8, horizon=4, segment=2, wind='forecast', seed=3, prior_strength=64, action_values=True))

  def make():
    return ei.SoftBCTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', 2, 2, 64), num_atoms=2), lr=1e-3, seed=LOOP_SEED,
                            temperature=0.5, value_coef=0.5)
  tr, twin = make(), make()
  buf = ei.VecPlanLabelBuffer(LOOP_N, LOOP_T)
  stats = train_lib.run_exit_loop_vec(env, tr, planner, buf, num_iterations=1, beta=LOOP_BETA, epochs=2, batch_size=128,
                                      max_episode_length=LOOP_LIMIT, capture_graph=False)
  n = LOOP_N
  assert len(env.steps) == LOOP_T == len(planner.decisions) and len(stats) == 1
  ep_steps = np.zeros(n, np.int64)
  took_total, differs, resets = 0, 0, 0
  for t in range(LOOP_T):
    rec, dec = env.steps[t], planner.decisions[t]
    seen = env.reset_obs if t == 0 else env.steps[t - 1]['obs']
    assert torch.equal(buf.obs[t, :, :1099].view(torch.int32), seen.view(torch.int32)), (t, 'obs[t] is not the observation acted on')
    assert torch.equal(dec['obs'].view(torch.int32), seen.view(torch.int32)), (t, 'the planner decided on another observation')
    assert torch.equal(buf.target_q[t].view(torch.int32), dec['q'].view(torch.int32)), (t, "target_q[t] is not the planner's action values")
    assert torch.equal(buf.ret[t].view(torch.int32), dec['best_return'].view(torch.int32)), t
    assert int(dec['visits'].sum()) == 8 * n
    twin.act_step.fill_(t)
    learner = torch.zeros(n, dtype=torch.uint8, device='cuda')
    logp, value, probs = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda'), torch.zeros(n, 3, device='cuda')
    twin.act(seen, learner, logp, value, probs)
    assert torch.equal(dec['prior'].view(torch.int32), probs.view(torch.int32)), (t, "the prior is not this step's probs")
    label = dec['label'].cpu().numpy()
    want, took = imitation_host.mix(learner.cpu().numpy(), label, LOOP_BETA, imitation_host.dagger_words(draws, LOOP_SEED, 0, n, t))
    assert np.array_equal(rec['actions'].cpu().numpy(), want), (t, 'the stepped action is not the mix')
    took_total += int(took.sum())
    differs += int((want != label).sum())
    terminal, end_mask = rec['terminal'].cpu().numpy(), rec['end_mask'].cpu().numpy()
    assert np.array_equal(end_mask, (ep_steps + 1 >= LOOP_LIMIT).astype(np.uint8)), t
    resets += int((terminal | end_mask).astype(bool).sum())
    ep_steps = np.where((terminal | end_mask) != 0, 0, ep_steps + 1)
  assert resets >= n, 'no auto-reset happened inside the block'
  assert differs > 0 and int(tr.act_step.item()) == LOOP_T and int(tr.mix_step.item()) == LOOP_T
  s = stats[0]
  assert s['updates'] == 2 * (LOOP_T * n // 128) and int(tr.adam_step.item()) == s['updates'] and np.isfinite(s['loss'])
  assert s['transitions'] == LOOP_T * n and s['episodes'] == resets
  assert s['expert_share'] == took_total / (LOOP_T * n) and 0.3 < s['expert_share'] < 0.7
  assert 0.0 <= s['agreement'] <= 1.0
  best = torch.stack([d['best_return'] for d in planner.decisions])
  assert torch.isfinite(best).all() and abs(s['mean_best_return'] - float(best.mean().item())) <= 1e-4 * abs(float(best.mean().item())) + 1e-6
  print('loop: expert_share', s['expert_share'], 'agreement', s['agreement'], 'loss', s['loss'], 'mean_best_return', s['mean_best_return'])


# ------------------------------------------------------------------------------------------------------------------------ 7: learns
LEARN_UPDATES, LEARN_B, LEARN_LR, LEARN_TEMPERATURE = 300, 128, 1e-3, 0.25      # the BC bandit test's budget


def _twin_run(params, x, q, order, x_test, label_test):
  """float64 torch autograd of the mean soft cross-entropy on the (2, 64) student with optax's Adam (eps 1e-5) over the minibatches
  `order` [updates, B]: the held-out greedy accuracy after."""
  layers = [(torch.tensor(params['params'][f'Dense_{i}']['kernel'], dtype=torch.float64, requires_grad=True),
             torch.tensor(params['params'][f'Dense_{i}']['bias'], dtype=torch.float64, requires_grad=True)) for i in range(2)]
  leaves = [t for pair in layers for t in pair]
  m, v = [torch.zeros_like(t) for t in leaves], [torch.zeros_like(t) for t in leaves]
  xt = torch.tensor(x, dtype=torch.float64)
  target = torch.softmax(torch.tensor(q, dtype=torch.float64) / LEARN_TEMPERATURE, dim=1)

  def logits(inp):
    h = torch.relu(inp @ layers[0][0] + layers[0][1])
    return (h @ layers[1][0] + layers[1][1])[:, POLICY]
  b1, b2, eps = 0.9, 0.999, 1e-5
  for t, idx in enumerate(order, start=1):
    loss = -(target[idx] * torch.log_softmax(logits(xt[idx]), dim=1)).sum(1).mean()
    grads = torch.autograd.grad(loss, leaves)
    with torch.no_grad():
      for w, g, mi, vi in zip(leaves, grads, m, v):
        mi.mul_(b1).add_((1 - b1) * g)
        vi.mul_(b2).add_((1 - b2) * g * g)
        w.sub_(LEARN_LR * (mi / (1 - b1 ** t)) / (torch.sqrt(vi / (1 - b2 ** t)) + eps))
  with torch.no_grad():
    z6 = np.zeros((len(x_test), 6))
    z6[:, POLICY] = logits(torch.tensor(x_test, dtype=torch.float64)).numpy()
  return float((ppo_host.greedy(z6) == label_test).mean())


def test_learns_the_contextual_bandit_from_soft_targets(mods, observations):
  """test_gpu_train.py's bandit with soft targets: q_a is the bandit's reward of action a (1 for the right action -- 0 or 2 as the most
  varied feature within [0, 1] is below or above its median -- else 0), temperature 0.25, a (2, 64) network, 300 updates of B = 128 at
  Adam 1e-3 (the BC bandit test's budget).  The bar is the bandit's own: >= 90 % held-out greedy accuracy, met first by the float64
  torch-autograd restatement of the same objective, budget, initial parameters and minibatch order, then by the device."""
  qnet, _, ac, _, ei = mods
  x = observations.cpu().numpy()
  std = np.where((x.min(axis=0) >= 0) & (x.max(axis=0) <= 1), x.std(axis=0), 0.0)
  col = int(np.argmax(std))
  label = np.where(x[:, col] > np.median(x[:, col]), 2, 0).astype(np.uint8)
  q = (np.arange(3)[None, :] == label[:, None]).astype(np.float32)
  perm = np.random.default_rng(0).permutation(len(x))
  train_i, test_i = perm[:768], perm[768:]
  order = train_i[np.random.default_rng(100).integers(0, len(train_i), (LEARN_UPDATES, LEARN_B))]
  params = ac.init_params('actor_critic', 7, 2, 64)
  twin_acc = _twin_run(params, x, q, order, x[test_i], label[test_i])
  print('float64 restatement: held-out greedy accuracy', twin_acc)
  assert twin_acc >= 0.9, twin_acc
  tr = ei.SoftBCTrainer(qnet.QNetwork.from_params(params, num_atoms=2), lr=LEARN_LR, temperature=LEARN_TEMPERATURE)
  bt = ei.SoftBatch(LEARN_B, 'cuda')
  q_d = torch.from_numpy(q).cuda()
  for k, idx in enumerate(order):
    i = torch.from_numpy(idx).cuda()
    bt.state[:, :1099].copy_(observations[i])
    bt.target_q.copy_(q_d[i])
    tr.capture(bt) if k == 0 else tr.train_step(bt)
  tr.check_errors()
  assert int(tr.adam_step.item()) == LEARN_UPDATES
  act = tr.act_greedy(observations[torch.from_numpy(test_i).cuda()]).cpu().numpy()
  acc = float((act == label[test_i]).mean())
  print('device: held-out greedy accuracy', acc)
  assert acc >= 0.9, acc
  # what was learnt is a QNetwork: VecActorCriticAgent takes it as it is
  agent = ac.VecActorCriticAgent(tr.network())
  assert float((agent.act(observations[torch.from_numpy(test_i).cuda()]).cpu().numpy() == label[test_i]).mean()) == acc
