"""On-policy training on the device (csrc/ble_actor.h, agents/actor_critic.py, train_lib.run_ppo_loop_vec) against its
restatement (ppo_host.py) and the float64 twins of the backward pass and Adam (train_host.py), case for case after test_gpu_td.py and
with its tolerances:

 * the head: probs, logp and value against the twin on the device's own float32 logits; the sampled action equals the float32 inverse
   CDF of the device's probs at the twin's Philox uniform, exactly, at the 256-lane block's edges too; a row's action at any n,
   position, stride and env_offset split; the greedy rule with ties and NaN logits; the action frequencies over 64 steps x 300 rows;
 * generalised advantage estimation bit for bit against the float32 restatement (T up to 960, N at the block's edges), ends at t = 0,
   t = T - 1 and in runs, a NaN a select must discard; float32 against float64 inside a derived running bound;
 * the normalisation within one float32 ulp of float64 on inputs that three mistakes (no 1e-8, M - 1, a one-pass variance) fail;
 * minibatches: the five gathered tensors name the same rows, every kept row once per pass;
 * loss, aux and dL/dlogits against the twin; exact zeros up to ld; clipped rows keep the entropy term alone; an action of 3;
   saturated logits;
 * rows fed back with unchanged weights: the training forward's log-probability is the acting forward's, bit for bit (rho == 1);
 * the gradient image against float64 backprop at test_gpu_train.py's batch edges; Adam over 10 updates;
 * head, loss, rho == 1 and gradient at the default (3, 256) and the reference-sized (8, 600) stack as well (WIDE);
 * determinism: two trainers, graph vs eager, a state_dict of trainer and rollout restored mid-iteration;
 * run_ppo_loop_vec's block against a recording environment and a second trainer: obs, action, logp, value, ends, bootstrap, stats;
 * it learns test_gpu_train.py's contextual bandit on-policy; run_ppo_loop_vec end to end, its policy through eval_agent_vec.
"""
import numpy as np
import pytest
import torch

import ppo_host
import train_host

pytestmark = pytest.mark.gpu

POLICY = [0, 2, 4]
SHAPES = [(2, 64), (1, 0)]          # (layers, hidden): two Dense layers of 64, and the one-layer 1099 -> 6
WIDE = [(3, 256), (8, 600)]         # actor_critic.init_params' default and the reference-sized stack: more than one column group


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import actor_critic, qnet, qnet_train
  return qnet, qnet_train, actor_critic


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
  return ppo_host.build_actor_draws(tmp_path_factory.mktemp('acd'))


def _params(qnet, layers, hidden, seed=7, bias=1e-2, logit_scale=1.0):
  """QuantileNetwork-scale kernels with two atoms and small random biases: policies far from uniform.  logit_scale multiplies the
  last layer (kernel and bias)."""
  params = qnet.init_params('quantile', seed, layers, hidden, 2)
  rng = np.random.default_rng(seed + 1)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * bias).astype(np.float32)
  last = params['params'][f'Dense_{layers - 1}']
  last['kernel'] = (last['kernel'] * np.float32(logit_scale)).astype(np.float32)
  last['bias'] = (last['bias'] * np.float32(logit_scale)).astype(np.float32)
  return params


def _trainer(mods, layers, hidden, logit_scale=1.0, **kw):
  qnet, _, ac = mods
  params = _params(qnet, layers, hidden, logit_scale=logit_scale)
  return params, ac.PPOTrainer(qnet.QNetwork.from_params(params, num_atoms=2), **kw)


def _close(got, want, name):
  scale = np.abs(want).max()
  assert np.allclose(got, want, rtol=2e-6, atol=1e-7 * scale), (name, np.abs(got - want).max(), scale)


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def _rows(observations, start, n):
  """n rows of the fixture from `start` on, tiled where it is too short."""
  if start + n <= len(observations):
    return observations[start:start + n]
  return observations[(start + torch.arange(n, device=observations.device)) % len(observations)]


def _logits(tr, ac, x):
  """The device's float32 logits [n, 6] of rows x (the training forward: an update that applies nothing)."""
  n = len(x)
  bt = ac.PPOBatch.from_tensors(x, np.zeros(n), np.zeros(n, np.uint8), np.zeros(n), np.zeros(n), 'cuda')
  tr.train_on_batch(bt, apply_update=False)
  return tr.views(n)['logits'].cpu().numpy().copy()


def _act(agent, obs, probs=True):
  n = obs.shape[0]
  out = torch.full((n,), 9, dtype=torch.uint8, device='cuda')
  logp, value = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
  p = torch.zeros(n, 3, device='cuda') if probs else None
  agent.act(obs, out, logp, value, p)
  return out.cpu().numpy(), logp.cpu().numpy(), value.cpu().numpy(), None if p is None else p.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize('n,layers,hidden', [(n, l, h) for l, h in SHAPES for n in (1, 65, 300)] + [(65, l, h) for l, h in WIDE] +
                         [(n, 2, 64) for n in (255, 256, 257, 1025)])      # (the 256-lane block's edges, and past four blocks)
def test_head_against_twin(mods, observations, draws, layers, hidden, n):
  """Measured on an MI355X at (3, 256) | (8, 600), n = 65, the worst |device - twin|: probs 6.0e-8 | 6.0e-8 (half an ulp of a
  probability), logp 2.4e-7 | 2.4e-7 at |logp| <= 1.24 | 1.12 -- what (2, 64) gives at n = 65 to 1025 too."""
  _, _, ac = mods
  _, tr = _trainer(mods, layers, hidden, seed=13)
  obs = _rows(observations, 100, n)
  z = _logits(tr, ac, obs.cpu().numpy())
  lp64, p64 = ppo_host.log_softmax(z[:, POLICY])
  for step in range(3):
    assert int(tr.act_step.item()) == step
    act, logp, value, probs = _act(tr, obs)
    u = ppo_host.uniform24(draws(13, 0, n, step))
    assert np.array_equal(act, ppo_host.sample(probs, u)), step
    print('n', n, 'probs', np.abs(probs - p64).max(), 'logp', np.abs(logp - lp64[np.arange(n), act]).max(), np.abs(lp64).max())
    _close(probs, p64, 'probs')
    _close(logp, lp64[np.arange(n), act], 'logp')
    assert np.array_equal(_bits(value), _bits(z[:, 1]))
  assert len(set(act.tolist())) > 1 or n == 1
  # greedy: the same probs, value and the argmax rule; the step counter stays
  g_act, g_logp, g_value, g_probs = _act(ac.VecActorCriticAgent(tr.network()), obs)
  assert np.array_equal(g_act, ppo_host.greedy(z)) and np.array_equal(_bits(g_probs), _bits(probs)) and np.array_equal(_bits(g_value), _bits(value))
  _close(g_logp, lp64[np.arange(n), g_act], 'greedy logp')
  assert int(tr.act_step.item()) == 3


def test_action_of_a_row_is_the_same_in_any_batch(mods, observations, draws):
  """n, the row's position, the row stride and the env_offset split do not change environment e's draw at a step."""
  qnet, _, ac = mods
  net = qnet.QNetwork.from_params(_params(qnet, 2, 64), num_atoms=2)
  whole = ac.VecActorCriticAgent(net, deterministic=False, seed=5)
  obs = observations[:300]
  whole.step.fill_(7)
  act, logp, value, probs = _act(whole, obs)
  assert int(whole.step.item()) == 8
  assert np.array_equal(act, ppo_host.sample(probs, ppo_host.uniform24(draws(5, 0, 300, 7))))
  padded = torch.zeros(300, 1104, device='cuda')
  padded[:, :1099] = obs
  padded[:, 1099:] = float('nan')                                   # nothing past a row's 1099 features is read
  for lo, hi, rows in ((0, 300, padded), (0, 1, obs[:1]), (37, 38, padded[37:38]), (64, 129, obs[64:129]), (129, 300, padded[129:300]),
                       (299, 300, obs[299:300])):
    part = ac.VecActorCriticAgent(net, deterministic=False, seed=5, env_offset=lo)
    part.step.fill_(7)
    a, l, v, p = _act(part, rows)
    assert np.array_equal(a, act[lo:hi]) and np.array_equal(_bits(l), _bits(logp[lo:hi])) and np.array_equal(_bits(v), _bits(value[lo:hi]))
    assert np.array_equal(_bits(p), _bits(probs[lo:hi]))
  other = ac.VecActorCriticAgent(net, deterministic=False, seed=5)
  other.step.fill_(8)
  assert not np.array_equal(_act(other, obs)[0], act)
  other = ac.VecActorCriticAgent(net, deterministic=False, seed=6)
  other.step.fill_(7)
  assert not np.array_equal(_act(other, obs)[0], act)
  big = ac.VecActorCriticAgent(net, deterministic=False, seed=5)
  big.step.fill_(2 ** 32 + 7)                                       # the step's high word is part of the key
  a = _act(big, obs)[0]
  assert np.array_equal(a, ppo_host.sample(probs, ppo_host.uniform24(draws(5, 0, 300, 2 ** 32 + 7)))) and not np.array_equal(a, act)


_SENTINELS = (101.0, 102.0, 103.0)


def _selector_network(qnet):
  """One layer whose policy logits are features 0, 1, 2 and whose value is feature 9.  The policy biases are sentinels, so that the test
  finds their slots in the packed image and can make a logit NaN in every row (no finite parameter does: inside the fused
  multiply-adds a finite product never meets an infinity of the other sign)."""
  k = np.zeros((1099, 6), np.float32)
  k[0, 0] = k[1, 2] = k[2, 4] = k[9, 1] = 1.0
  bias = np.zeros(6, np.float32)
  bias[POLICY] = _SENTINELS
  return qnet.QNetwork.from_params({'Dense_0': {'kernel': k, 'bias': bias}}, num_atoms=2)


def test_greedy_rule_with_ties_and_nan(mods):
  qnet, _, ac = mods
  rows = [[1, 2, 3], [2, 2, 1], [0, 0, 0], [1, 3, 3], [-1, -1, -2], [3, 3, 3], [5, 1, 0], [0, 7, 0], [-2, -1, -1]]
  x = np.zeros((len(rows), 1099), np.float32)
  x[:, :3], x[:, 9] = rows, 10 + np.arange(len(rows))
  net = _selector_network(qnet)
  slots = [int(np.flatnonzero(net.packed_host == s)[0]) for s in _SENTINELS]
  assert all((net.packed_host == s).sum() == 1 for s in _SENTINELS)
  agent = ac.VecActorCriticAgent(net)
  first_nan = {(): None, (1,): 1, (0, 2): 0, (2,): 2, (0, 1, 2): 0, (1, 2): 1, (0,): 0}
  for nans, want in first_nan.items():
    for a, slot in enumerate(slots):
      net.packed[slot] = float('nan') if a in nans else 0.0
    act, logp, value, probs = _act(agent, torch.from_numpy(x).cuda())
    z = np.zeros((len(rows), 6), np.float32)
    z[:, POLICY] = rows
    z[:, [2 * a for a in nans]] = np.nan
    assert np.array_equal(act, ppo_host.greedy(z)), nans
    assert value.tolist() == [10.0 + i for i in range(len(rows))]
    if want is None:
      assert act.tolist() == [2, 0, 0, 1, 0, 0, 0, 1, 1]          # the lowest index among equal maxima
      lp64, p64 = ppo_host.log_softmax(np.array(rows, np.float64))
      _close(probs, p64, 'probs')
      _close(logp, lp64[np.arange(len(rows)), act], 'logp')
    else:
      assert (act == want).all(), nans                              # the first NaN
      assert np.isnan(probs).all() and np.isnan(logp).all()


def test_action_frequencies_follow_probs(mods):
  """64 steps x 300 rows at one fixed policy: every action's count lies within 4 binomial standard deviations of its probability."""
  qnet, _, ac = mods
  bias = np.array([0.3, 0.0, 1.2, 0.0, -0.7, 0.0], np.float32)
  net = qnet.QNetwork.from_params({'Dense_0': {'kernel': np.zeros((1099, 6), np.float32), 'bias': bias}}, num_atoms=2)
  agent = ac.VecActorCriticAgent(net, deterministic=False, seed=21)
  obs = torch.zeros(300, 1099, device='cuda')
  out = torch.zeros(64, 300, dtype=torch.uint8, device='cuda')
  probs = torch.zeros(300, 3, device='cuda')
  for s in range(64):
    agent.act(obs, out[s], probs=probs)
  p = probs.cpu().numpy().astype(np.float64)
  assert (p == p[0]).all() and p[0].min() > 0.05 and p[0].max() - p[0].min() > 0.3
  m = 64 * 300
  counts = np.bincount(out.cpu().numpy().ravel(), minlength=3)
  assert counts.sum() == m and len(counts) == 3
  sigma = np.sqrt(m * p[0] * (1 - p[0]))
  print('counts', counts, 'expected', m * p[0], 'sigma', sigma)
  assert (np.abs(counts - m * p[0]) <= 4 * sigma).all(), (counts, m * p[0], sigma)
  assert not np.array_equal(out[0].cpu().numpy(), out[1].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------------- GAE
def _block(steps, n, seed):
  """A [T, N] block with terminals and time-limit ends at t = 0, t = T - 1 and in runs, and NaNs exactly where a select must discard
  them: value[t + 1] (or boot_value) behind a terminal or a time-limit end at t."""
  rng = np.random.default_rng(seed)
  b = {'reward': rng.standard_normal((steps, n)).astype(np.float32), 'value': (rng.standard_normal((steps, n)) * 3).astype(np.float32),
       'boot': rng.standard_normal(n).astype(np.float32)}
  term = rng.random((steps, n)) < 0.1
  end = term | (rng.random((steps, n)) < 0.1)
  for e in range(n):
    kind = e % 6
    if kind == 0:
      term[0, e] = end[0, e] = True
    elif kind == 1:
      term[steps - 1, e] = end[steps - 1, e] = True
    elif kind == 2:
      term[0, e], end[0, e] = False, True
    elif kind == 3:
      term[steps - 1, e], end[steps - 1, e] = False, True
    elif kind == 4:
      end[steps // 3:steps // 3 + 4, e] = True                        # a run of ends
      term[steps // 3:steps // 3 + 2, e] = True
  b['terminal'], b['episode_end'] = term.astype(np.uint8), end.astype(np.uint8)
  return b


def _device_gae(ac, b, gamma, lam, normalize=False):
  steps, n = b['reward'].shape
  ro = ac.VecRolloutBuffer(n, steps, 'cuda')
  for name in ('reward', 'value', 'terminal', 'episode_end'):
    getattr(ro, name).copy_(torch.from_numpy(b[name]))
  before = {k: getattr(ro, k).clone() for k in ('reward', 'value', 'terminal', 'episode_end', 'logp', 'action')}
  ro.finish(torch.from_numpy(b['boot']).cuda(), gamma, lam, normalize)
  assert all(torch.equal(getattr(ro, k), t) or bool(torch.isnan(t).any()) for k, t in before.items())
  return ro.advantage.cpu().numpy(), ro.ret.cpu().numpy()


@pytest.mark.parametrize('steps,n', [(1, 1), (2, 65), (17, 300), (960, 3), (3, 255), (3, 256), (3, 257), (5, 1025)])
def test_gae_bit_equal_to_float32_twin(mods, steps, n):
  ac = mods[2]
  for gamma, lam in ((0.993, 0.95), (0.9, 1.0), (0.5, 0.0)):
    b = _block(steps, n, seed=steps)
    want = ppo_host.gae_f32(b['reward'], b['value'], b['boot'], b['terminal'], b['episode_end'], gamma, lam)
    got = _device_gae(ac, b, gamma, lam)
    assert np.isfinite(want[0]).all()
    for g, w, name in zip(got, want, ('advantage', 'ret')):
      assert np.array_equal(_bits(g), _bits(w)), (name, gamma, lam, np.abs(g - w).max())
    w64 = ppo_host.gae_f64(b['reward'], b['value'], b['boot'], b['terminal'], b['episode_end'], float(np.float32(gamma)), float(np.float32(lam)))
    assert np.allclose(got[0], w64[0], rtol=1e-4, atol=1e-4)
    # what float32 allows: the running bound 5 u M_t, carried by gamma lambda and cut at an end (ppo_host.gae_f32_error_bound)
    bound = ppo_host.gae_f32_error_bound(b['reward'], b['value'], b['boot'], b['terminal'], b['episode_end'], float(np.float32(gamma)),
                                         float(np.float32(lam)))
    assert (np.abs(got[0].astype(np.float64) - w64[0]) <= bound).all(), (gamma, lam, (np.abs(got[0] - w64[0]) / bound).max())


@pytest.mark.parametrize('steps,n', [(1, 1), (2, 65), (17, 300)])
def test_gae_discards_nan_behind_an_end(mods, steps, n):
  ac = mods[2]
  b = _block(steps, n, seed=steps + 100)
  if steps == 1:
    b['terminal'][0, 0] = b['episode_end'][0, 0] = 1
  poisoned = 0
  for e in range(n):
    if b['episode_end'][steps - 1, e]:
      b['boot'][e] = np.nan
      poisoned += 1
  clean = {k: v.copy() for k, v in b.items()}
  got = _device_gae(ac, b, 0.993, 0.95)
  want = ppo_host.gae_f32(clean['reward'], clean['value'], clean['boot'], clean['terminal'], clean['episode_end'], 0.993, 0.95)
  assert poisoned > 0 and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
  assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
  if steps > 1:      # value[t + 1] = NaN behind an end at t: step t stays finite and equal, step t + 1 is NaN on both sides
    t, e = map(int, np.argwhere(b['episode_end'][:-1] != 0)[0])
    b['value'][t + 1, e] = np.nan
    got = _device_gae(ac, b, 0.993, 0.95)
    want = ppo_host.gae_f32(b['reward'], b['value'], b['boot'], b['terminal'], b['episode_end'], 0.993, 0.95)
    assert np.isnan(got[0][t + 1, e]) and np.isfinite(got[0][t, e])
    ok = ~np.isnan(want[0])
    assert np.array_equal(np.isnan(got[0]), ~ok) and np.array_equal(_bits(got[0][ok]), _bits(want[0][ok]))
    assert np.array_equal(_bits(got[1][ok]), _bits(want[1][ok]))
    assert ok[:, np.arange(n) != e].all()


@pytest.mark.parametrize('steps,n', [(1, 3), (17, 300)])
def test_normalisation_within_one_ulp_of_float64(mods, steps, n):
  ac = mods[2]
  b = _block(steps, n, seed=5)
  raw, ret = _device_gae(ac, b, 0.993, 0.95)
  got, ret2 = _device_gae(ac, b, 0.993, 0.95, normalize=True)
  want = ppo_host.normalize_f64(raw)
  ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
  print('M', steps * n, 'worst |A - A64| / ulp', (np.abs(got - want) / ulp).max())
  assert (np.abs(got - want) <= ulp).all()
  assert np.array_equal(_bits(ret), _bits(ret2))                      # the returns are not normalised
  assert abs(got.astype(np.float64).mean()) < 1e-6 and abs(got.astype(np.float64).std() - 1.0) < 1e-5


NORM_CASES = ppo_host.normalisation_cases()


@pytest.mark.parametrize('name', sorted(NORM_CASES))
def test_normalisation_held_to_what_it_computes(mods, name):
  """ppo_host.normalisation_cases through finish(normalize=True): within one float32 ulp of normalize_f64 and finite; exactly 0.0 for
  M = 1 and for equal advantages.  test_ppo_host.py shows that dropping the 1e-8, dividing by M - 1 and a one-pass variance each leave
  the bound on one of these inputs, and that the stated order stays inside on all.  A block of T = 1 whose every step is terminal with
  value 0 has A = reward bit for bit (delta = (r + gamma 0) - 0, nothing carried), so the reward written is the advantage normalised:
  ret, which is not normalised, shows it."""
  ac = mods[2]
  a = NORM_CASES[name]
  m = len(a)
  ro = ac.VecRolloutBuffer(m, 1, 'cuda')
  ro.reward.copy_(torch.from_numpy(a).view(1, m))
  ro.terminal.fill_(1)
  ro.episode_end.fill_(1)
  ro.finish(torch.zeros(m, device='cuda'), 0.993, 0.95, normalize=False)
  assert np.array_equal(_bits(ro.advantage.cpu().numpy().ravel()), _bits(a))
  ro.finish(torch.zeros(m, device='cuda'), 0.993, 0.95, normalize=True)
  got = ro.advantage.cpu().numpy().ravel()
  assert np.array_equal(_bits(ro.ret.cpu().numpy().ravel()), _bits(a))
  want = ppo_host.normalize_f64(a)
  err = ppo_host.ulps_from(got, want)
  print(name, 'M', m, 'worst |A - A64| / ulp', err.max())
  assert np.isfinite(got).all()
  assert (err <= 1.0).all(), (name, err.max())
  if name in ('normal_1', 'equal'):
    assert not got.any() and not np.signbit(got).any()                 # exactly 0.0: (A - mean) = 0 over sqrt(0) + 1e-8
  elif name == 'pair':
    assert np.array_equal(got, np.array([-1.0, 1.0], np.float32) / np.float32(1 + 1e-8))      # var = 1 (/ M), not 2


# -------------------------------------------------------------------------------------------------------------------------- minibatches
def test_minibatches_gather_the_same_rows_once_per_pass(mods):
  """N = 64, T = 8 with the row id written into every buffer a minibatch gathers: the five tensors of a minibatch name the same rows;
  the 5 x 96 kept rows of a pass are distinct (32 dropped); the yielded object is one PPOBatch; a second pass has another order; a
  generator restored with set_state repeats the first."""
  ac = mods[2]
  ro = ac.VecRolloutBuffer(64, 8, 'cuda')
  ids = torch.arange(512, device='cuda')
  ro.ret.view(-1).copy_(ids)
  ro.advantage.view(-1).copy_(ids + 0.5)
  ro.logp.view(-1).copy_(-ids)
  ro.action.view(-1).copy_(ids % 3)
  ro.obs.view(512, -1)[:, 0].copy_(ids)
  state = ro.generator.get_state().clone()

  def one_pass():
    seen, first = [], None
    for bt in ro.minibatches(96):
      first = bt if first is None else first
      assert bt is first and isinstance(bt, ac.PPOBatch) and bt.batch_size == 96
      i = bt.ret.cpu().numpy()
      assert np.array_equal(bt.advantage.cpu().numpy(), i + 0.5) and np.array_equal(bt.old_logp.cpu().numpy(), -i)
      assert np.array_equal(bt.action.cpu().numpy(), i.astype(np.int64) % 3) and np.array_equal(bt.state[:, 0].cpu().numpy(), i)
      assert not bt.state[:, 1:].any()
      seen.append(i.astype(np.int64))
    assert len(seen) == 5
    seen = np.concatenate(seen)
    assert len(set(seen.tolist())) == 480 and seen.min() >= 0 and seen.max() < 512
    return seen

  a, b = one_pass(), one_pass()
  assert not np.array_equal(a, b) and not np.array_equal(a, np.sort(a))
  ro.generator.set_state(state)
  assert np.array_equal(one_pass(), a)
  own = torch.Generator(device='cuda').manual_seed(5)                  # a generator handed in is the one used
  state = own.get_state().clone()
  c = np.concatenate([bt.ret.cpu().numpy() for bt in ro.minibatches(96, own)])
  own.set_state(state)
  assert np.array_equal(np.concatenate([bt.ret.cpu().numpy() for bt in ro.minibatches(96, own)]), c)


# ------------------------------------------------------------------------------------------------------------------------------ loss
_SHIFTS = np.array([0.05, 0.5, -0.5, -0.05, 0.4, -0.6, 0.0])          # log rho: inside the band, above it, below it
_ADVS = np.array([1.3, 0.7, -0.9, -1.1, -0.4, 0.8, 0.6])


def _ppo_batch(mods, tr, observations, b, seed, invalid=()):
  """b rows of real observations with random actions and returns; old_logp = the device's own log-probability minus a cycling shift,
  so that rho lies inside the band, above and below it with advantages of both signs."""
  ac = mods[2]
  rng = np.random.default_rng(seed)
  x = observations.cpu().numpy()[rng.integers(0, len(observations), b)]
  act = rng.integers(0, 3, b).astype(np.uint8)
  z = _logits(tr, ac, x)
  lp, _ = ppo_host.log_softmax(z[:, POLICY])
  old = (lp[np.arange(b), act] - _SHIFTS[np.arange(b) % 7]).astype(np.float32)
  adv = (_ADVS[np.arange(b) % 7] * (1.0 + 0.1 * rng.random(b))).astype(np.float32)
  ret = rng.standard_normal(b).astype(np.float32)
  for i in invalid:
    act[i] = 3
  return x, ac.PPOBatch.from_tensors(x, ret, act, old, adv, 'cuda'), (act, old, adv, ret)


@pytest.mark.parametrize('b,layers,hidden', [(b, l, h) for l, h in SHAPES for b in (1, 32, 300)] + [(32, l, h) for l, h in WIDE])
def test_loss_and_dlogits(mods, observations, layers, hidden, b):
  """Measured on an MI355X (both networks, B = 1, 32, 300), the worst |device - twin| / (2e-6 |twin| + 1e-7 scale): loss 0.26 (B = 300),
  aux 0.10, dlogits 0.15.  expf / logf keep every case inside test_gpu_td.py's _close bounds, which stand unwidened."""
  _, tr = _trainer(mods, layers, hidden)
  _, bt, (act, old, adv, ret) = _ppo_batch(mods, tr, observations, b, seed=b)
  tr.views(b)['dlogits'].fill_(float('nan'))                           # every column up to ld is written by the call
  loss_d = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  tr.check_errors()
  v = {k: t.cpu().numpy() for k, t in tr.views(b).items() if k != 'acts'}
  loss, aux, dlog = ppo_host.ppo_loss(v['logits'], act, old, adv, ret, tr.clip, tr.value_coef, tr.entropy_coef)

  def ratio(got, want):
    return float((np.abs(got - want) / (2e-6 * np.abs(want) + 1e-7 * np.abs(want).max())).max())
  print('B', b, 'err / bound: loss', ratio(loss_d, loss), 'aux', ratio(v['aux'], aux), 'dlogits', ratio(v['dlogits'][:, :6], dlog))
  _close(loss_d, loss, 'loss')
  _close(v['aux'][:, 0], aux[:, 0], 'lp_act')
  _close(v['aux'][:, 1], aux[:, 1], 'entropy')
  _close(v['dlogits'][:, :6], dlog, 'dlogits')
  assert not v['dlogits'][:, [3, 5]].any() and not v['dlogits'][:, 6:].any()
  assert v['dlogits'].shape[1] >= max(hidden, 6) and not np.isnan(v['dlogits']).any()      # (the whole [B, ld] view)
  # clipped rows: the policy gradient is the entropy term alone -- what the same rows give at A = 0
  rho = np.exp(aux[:, 0] - old.astype(np.float64))
  clipped = ((rho > 1 + tr.clip) & (adv > 0)) | ((rho < 1 - tr.clip) & (adv < 0))
  bt.advantage.zero_()
  tr.train_on_batch(bt, apply_update=False)
  d0 = tr.views(b)['dlogits'].cpu().numpy()
  if b >= 7:
    assert clipped.any() and not clipped.all()
    assert (v['dlogits'][~clipped][:, POLICY] != d0[~clipped][:, POLICY]).any(axis=1).all()
  assert (v['dlogits'][clipped][:, POLICY] == d0[clipped][:, POLICY]).all()
  assert np.array_equal(v['dlogits'][:, 1], d0[:, 1])


def test_action_out_of_range_flags_and_zeroes_the_row(mods, observations):
  _, tr = _trainer(mods, 2, 64)
  _, bt, _ = _ppo_batch(mods, tr, observations, 8, seed=2, invalid=(2, 5))
  bt.action[5] = 200
  loss = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  v = tr.views(8)
  dl, aux = v['dlogits'].cpu().numpy(), v['aux'].cpu().numpy()
  assert loss[2] == 0 and loss[5] == 0 and not dl[2].any() and not dl[5].any() and not aux[[2, 5]].any()
  assert loss[[0, 1, 3, 4, 6, 7]].all() and dl[[0, 1, 3, 4, 6, 7]].any(axis=1).all()
  with pytest.raises(ValueError):
    tr.check_errors()
  tr.check_errors()                                                   # (the flag is cleared once raised)


@pytest.mark.parametrize('layers,hidden', SHAPES)
def test_saturated_logits_give_finite_loss_and_gradient(mods, observations, layers, hidden):
  """Logits scaled by 200: p saturates to exact 0 and 1 in float32; no NaN or inf in the loss, the gradient or the head."""
  ac = mods[2]
  _, tr = _trainer(mods, layers, hidden, logit_scale=200.0)
  b = 32
  _, bt, (act, old, adv, ret) = _ppo_batch(mods, tr, observations, b, seed=9)
  bt.old_logp.copy_(torch.from_numpy(np.maximum(old, -3.0).astype(np.float32)))      # (a finite log-probability a policy could have had)
  loss = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  v = {k: t.cpu().numpy() for k, t in tr.views(b).items() if k != 'acts'}
  _, p = ppo_host.log_softmax(v['logits'][:, POLICY].astype(np.float32))
  assert (p == 0).any() and (p == 1).any()
  assert np.isfinite(loss).all() and np.isfinite(v['dlogits']).all() and np.isfinite(v['aux']).all() and np.isfinite(tr.grad.cpu().numpy()).all()
  act_d, logp, value, probs = _act(tr, bt.state)
  assert np.isfinite(logp).all() and np.isfinite(probs).all() and (probs == 0).any() and (probs == 1).any()


# -------------------------------------------------------------------------------------------------------------------------- rho == 1
@pytest.mark.parametrize('n,layers,hidden', [(n, l, h) for l, h in SHAPES for n in (1, 65, 300)] +
                         [(n, l, h) for l, h in WIDE for n in (1, 129, 300)])
def test_rows_fed_back_unchanged_have_ratio_one(mods, observations, layers, hidden, n):
  """The training forward's log-probability of the action taken is the acting forward's, bit for bit: rho = exp(0) = 1 exactly, no row
  is clipped, and the policy loss is -A."""
  ac = mods[2]
  _, tr = _trainer(mods, layers, hidden, entropy_coef=0.0, value_coef=0.0)
  obs = observations[200:200 + n]
  act, logp, value, _ = _act(tr, obs)
  rng = np.random.default_rng(n)
  adv = rng.standard_normal(n).astype(np.float32)
  bt = ac.PPOBatch.from_tensors(obs.cpu().numpy(), value, act, logp, adv, 'cuda')
  loss = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  v = {k: t.cpu().numpy() for k, t in tr.views(n).items() if k != 'acts'}
  assert np.array_equal(_bits(v['aux'][:, 0]), _bits(logp))
  assert np.array_equal(_bits(v['logits'][:, 1]), _bits(value))
  assert np.array_equal(loss, -adv)                                    # rho = 1, c_v = c_e = 0
  assert adv.all() and np.array_equal(-loss / adv, np.ones(n, np.float32))      # rho = 1.0f exactly: the loss is -(rho A)
  _, _, dlog = ppo_host.ppo_loss(v['logits'], act, logp, adv, value, tr.clip, 0.0, 0.0)
  _close(v['dlogits'][:, :6], dlog, 'dlogits')
  assert (v['dlogits'][:, POLICY] != 0).any(axis=1).all()              # the unclipped gradient


# -------------------------------------------------------------------------------------------------------------------------- gradient
EDGE_BATCHES = (1, 7, 9, 33, 129, 511, 513, 4097)          # test_gpu_train.py's batch edges of the backward pass


@pytest.mark.parametrize('layers,hidden,b', [(1, 0, 32), (3, 37, 32), (2, 64, 600)] + [(2, 64, b) for b in EDGE_BATCHES] +
                         [(3, 256, 32), (8, 600, 32), (3, 256, 4097)])      # (4097: kWgradMaxSlabs' cap, at a wider ld than 64)
def test_gradient_against_float64_backprop(mods, observations, layers, hidden, b):
  """Measured on an MI355X, the worst |g - g64| / (1e-5 S): 0.015 at (3, 256, 32), 0.017 at (8, 600, 32), 0.018 at (3, 256, 4097);
  0.023 (B = 511) is the worst at (2, 64)."""
  qnet, qnet_train, _ = mods
  params, tr = _trainer(mods, layers, hidden)
  x, bt, _ = _ppo_batch(mods, tr, observations, b, seed=4)
  tr.train_on_batch(bt, apply_update=False)
  v = tr.views(b)
  acts = [a.cpu().numpy() for a in v['acts']]
  acts = [a[:, :hidden] for a in acts[:-1]] + [acts[-1][:, :6]]
  dlog = v['dlogits'].cpu().numpy()[:, :6]
  want, mag = train_host.backward(params, x, dlog, acts), train_host.backward_magnitude(params, x, dlog, acts)
  g = tr.grad.cpu().numpy()
  got = qnet_train.unpack(tr._net, g)['params']
  worst = 0.0
  for l in range(layers):
    for leaf, i in (('kernel', 0), ('bias', 1)):
      err = np.abs(got[f'Dense_{l}'][leaf] - want[l][i])
      worst = max(worst, float((err / (1e-5 * mag[l][i] + 1e-30)).max()))
  print('B', b, 'worst |g - g64| / (1e-5 S)', worst)
  assert worst <= 1.0, worst
  assert any(np.abs(want[l][0]).max() > 0 for l in range(layers))
  last = got[f'Dense_{layers - 1}']
  assert not last['kernel'][:, [3, 5]].any() and not last['bias'][[3, 5]].any()      # the outputs that are not read
  # the padding of the gradient image is exactly zero: packing the unpacked gradient gives the image back
  assert np.array_equal(_bits(qnet.QNetwork.from_params({'params': got}, num_atoms=2).packed_host), _bits(g))


# ------------------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_against_optax_arithmetic(mods, observations):
  qnet, qnet_train, _ = mods
  _, tr = _trainer(mods, 3, 37, lr=1e-3, eps=2e-5)
  _, bt, _ = _ppo_batch(mods, tr, observations, 64, seed=3)
  w, m, v = (t.cpu().numpy().astype(np.float64) for t in (tr.weights, tr.adam_m, tr.adam_v))
  first = tr.weights.cpu().numpy().copy()
  for t in range(1, 11):
    tr.train_on_batch(bt)
    g = tr.grad.cpu().numpy()
    w64, m64, v64 = train_host.adam(w, g, m, v, t, lr=1e-3, eps=2e-5)
    wd, md, vd = (x.cpu().numpy() for x in (tr.weights, tr.adam_m, tr.adam_v))
    ulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
    assert (np.abs(wd - w64) <= 4 * ulp + 1e-6 * 1e-3).all(), (t, np.abs(wd - w64).max())
    assert (np.abs(md - m64) <= 1e-6 * (0.1 * np.abs(g) + 0.9 * np.abs(m)) + 1e-38).all(), t
    assert (np.abs(vd - v64) <= 1e-6 * v64 + 1e-38).all(), t
    w, m, v = wd.astype(np.float64), md.astype(np.float64), vd.astype(np.float64)
  assert int(tr.adam_step.item()) == 10
  wd = tr.weights.cpu().numpy()
  assert np.array_equal(_bits(qnet.QNetwork.from_params(qnet_train.unpack(tr._net, wd), num_atoms=2).packed_host), _bits(wd))
  assert not np.array_equal(wd, first)
  wt = tr.weights_t.cpu().numpy().copy()
  tr._retranspose()                                                   # the transposed image follows the weights
  assert np.array_equal(_bits(wt), _bits(tr.weights_t.cpu().numpy()))


# ----------------------------------------------------------------------------------------------------------------------- determinism
def _loop(mods, capture_graph, iterations=1, seed=4):
  qnet, _, ac = mods
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.env import balloon_env
  env = balloon_env.VecBalloonEnv(64, seed=1)
  tr = ac.PPOTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', 2, 2, 64), num_atoms=2), lr=1e-3, seed=seed)
  ro = ac.VecRolloutBuffer(64, 8, 'cuda')
  stats = train_lib.run_ppo_loop_vec(env, tr, ro, num_iterations=iterations, epochs=2, batch_size=128, max_episode_length=5,
                                     capture_graph=capture_graph)
  return tr, ro, stats


def test_determinism_graph_and_resume(mods):
  qnet, _, ac = mods
  a, ro_a, stats = _loop(mods, False)
  b, _, _ = _loop(mods, False)
  c, _, stats_c = _loop(mods, True)
  wa = a.weights.cpu().numpy()
  assert stats[0]['updates'] == 8 and int(a.adam_step.item()) == 8 and int(a.act_step.item()) == 9
  assert np.array_equal(_bits(wa), _bits(b.weights.cpu().numpy())), 'two trainers differ'
  assert np.array_equal(_bits(wa), _bits(c.weights.cpu().numpy())), 'graph replay differs from eager'
  assert stats == stats_c
  assert ro_a.episode_end.any() and not ro_a.terminal.cpu().numpy().all()
  other, _, _ = _loop(mods, False, seed=5)
  assert not np.array_equal(wa, other.weights.cpu().numpy())
  # a state_dict of trainer and rollout, taken between two passes over the block, resumes to the same bits
  for bt in ro_a.minibatches(128):
    a.train_on_batch(bt)
  sd_t, sd_r = a.state_dict(), ro_a.state_dict()
  for bt in ro_a.minibatches(128):
    a.train_on_batch(bt)
  d = ac.PPOTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', 9, 2, 64), num_atoms=2), lr=1e-3, seed=77)
  ro_d = ac.VecRolloutBuffer(64, 8, 'cuda')
  ro_d.generator.manual_seed(123)
  d.load_state_dict(sd_t)
  ro_d.load_state_dict(sd_r)
  for bt in ro_d.minibatches(128):
    d.train_on_batch(bt)
  assert np.array_equal(_bits(a.weights.cpu().numpy()), _bits(d.weights.cpu().numpy())), 'resume differs'
  assert not np.array_equal(a.weights.cpu().numpy(), wa)
  obs = ro_a.obs[0]
  assert np.array_equal(_act(a, obs)[0], _act(d, obs)[0]) and int(d.act_step.item()) == int(a.act_step.item())


# -------------------------------------------------------------------------------------------------------------- the loop's block contract
class _RecordingEnv:
  """Forwards reset, step, num_envs, device and check_errors of a VecBalloonEnv and keeps clones of what went in and out.  Before it
  forwards step `burst_step` it adds 30 000 mol to mols_air of `burst_lanes` (far above the superpressure limit, as
  test_gpu_scenarios.py does): those balloons burst in that step, so the block holds real terminals and their auto-resets."""

  def __init__(self, env, burst_step, burst_lanes):
    self.env, self.num_envs, self.device = env, env.num_envs, env.device
    self.burst_step, self.burst_lanes = burst_step, list(burst_lanes)
    self.reset_obs, self.steps = None, []

  def reset(self):
    obs = self.env.reset()
    self.reset_obs = obs.clone()
    return obs

  def step(self, actions, end_mask=None):
    if len(self.steps) == self.burst_step:
      self.env.arena.sim.state['mols_air'][self.burst_lanes] += 30000.0
    went_in = {'actions': actions.clone(), 'end_mask': end_mask.clone()}
    obs, reward, terminal = self.env.step(actions, end_mask=end_mask)
    self.steps.append({**went_in, 'obs': obs.clone(), 'reward': reward.clone(), 'terminal': terminal.clone()})
    return obs, reward, terminal

  def check_errors(self):
    self.env.check_errors()


LOOP_T, LOOP_N, LOOP_LIMIT, LOOP_SEED, BURST = 8, 64, 5, 4, (5, 40)


def _recorded_loop(mods, normalize):
  qnet, _, ac = mods
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.env import balloon_env
  env = _RecordingEnv(balloon_env.VecBalloonEnv(LOOP_N, seed=1), 2, BURST)
  kw = {} if normalize else {'normalize_advantage': False}            # (True is the default)
  tr = ac.PPOTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', 2, 2, 64), num_atoms=2), lr=1e-3, seed=LOOP_SEED, **kw)
  ro = ac.VecRolloutBuffer(LOOP_N, LOOP_T, 'cuda')
  stats = train_lib.run_ppo_loop_vec(env, tr, ro, num_iterations=1, epochs=2, batch_size=128, max_episode_length=LOOP_LIMIT,
                                     capture_graph=False)
  return env, tr, ro, stats


def test_loop_block_is_what_happened(mods, draws):
  """One iteration of run_ppo_loop_vec through a recording environment, against a second trainer of the same parameters and seed whose
  act_step is set to t: row t of the block is the observation the action was taken on (across auto-resets too) with that trainer's
  action, logp and value there; reward and terminal are the environment's; episode_end = terminal | end_mask with the limit counted
  per environment; boot_value is the value of act number T on the last observation; advantage and ret are gae_f32 of the block; the
  stats count what happened.  With normalize_advantage (the default) ret stays and advantage is normalize_f64 of the twin's within
  one ulp."""
  qnet, _, ac = mods
  env, tr, ro, stats = _recorded_loop(mods, normalize=False)
  steps_n, n = LOOP_T, LOOP_N
  assert len(env.steps) == steps_n and len(stats) == 1
  twin = ac.PPOTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', 2, 2, 64), num_atoms=2), lr=1e-3, seed=LOOP_SEED)
  blk = {k: getattr(ro, k).cpu().numpy() for k in ('action', 'logp', 'value', 'reward', 'terminal', 'episode_end', 'boot_value', 'advantage', 'ret')}
  ep_steps = np.zeros(n, np.int64)
  limit_ends = 0
  for t in range(steps_n):
    rec = env.steps[t]
    seen = env.reset_obs if t == 0 else env.steps[t - 1]['obs']
    assert torch.equal(ro.obs[t, :, :1099].view(torch.int32), seen.view(torch.int32)), (t, 'obs[t] is not the observation acted on')
    assert not ro.obs[t, :, 1099:].any()
    twin.act_step.fill_(t)
    act, logp, value, probs = _act(twin, seen)
    assert np.array_equal(act, ppo_host.sample(probs, ppo_host.uniform24(draws(LOOP_SEED, 0, n, t)))), t
    assert np.array_equal(blk['action'][t], act) and np.array_equal(rec['actions'].cpu().numpy(), act), t
    assert np.array_equal(_bits(blk['logp'][t]), _bits(logp)) and np.array_equal(_bits(blk['value'][t]), _bits(value)), t
    assert np.array_equal(_bits(blk['reward'][t]), _bits(rec['reward'].cpu().numpy())), t
    terminal, end_mask = rec['terminal'].cpu().numpy(), rec['end_mask'].cpu().numpy()
    assert np.array_equal(blk['terminal'][t], terminal), t
    want_mask = (ep_steps + 1 >= LOOP_LIMIT).astype(np.uint8)          # the 5th step of the environment's own episode
    assert np.array_equal(end_mask, want_mask), (t, end_mask)
    assert np.array_equal(blk['episode_end'][t], terminal | end_mask), t
    limit_ends += int((want_mask & ~terminal & 1).sum())
    ep_steps = np.where((terminal | end_mask) != 0, 0, ep_steps + 1)
  assert blk['terminal'][2, list(BURST)].all() and blk['terminal'].sum() >= 2, 'the burst lanes are terminal at t = 2'
  others = np.setdiff1d(np.arange(n), BURST)
  if not blk['terminal'][:, others].any():                             # (no other balloon died: the two clocks, spelt out)
    assert np.flatnonzero(blk['episode_end'][:, others].any(axis=1)).tolist() == [4]
    assert [np.flatnonzero(blk['episode_end'][:, e]).tolist() for e in BURST] == [[2, 7], [2, 7]]
  assert limit_ends >= n - 2
  # the bootstrap: act number T on the last returned observation; the counter ends at T + 1
  twin.act_step.fill_(steps_n)
  _, _, boot, _ = _act(twin, env.steps[-1]['obs'])
  assert np.array_equal(_bits(blk['boot_value']), _bits(boot))
  assert int(tr.act_step.item()) == steps_n + 1
  adv, ret = ppo_host.gae_f32(blk['reward'], blk['value'], blk['boot_value'], blk['terminal'], blk['episode_end'], tr.gamma, tr.lam)
  assert np.array_equal(_bits(blk['advantage']), _bits(adv)) and np.array_equal(_bits(blk['ret']), _bits(ret))
  # the stats count what happened
  s = stats[0]
  assert s['episodes'] == int(blk['episode_end'].astype(bool).sum()) and s['transitions'] == steps_n * n == 512
  assert s['updates'] == 2 * (512 // 128) and np.isfinite(s['mean_loss'])
  assert s['time_within_radius'] == float((blk['reward'] > 0.5).mean())
  running, done = np.zeros(n), []
  for t in range(steps_n):
    running += blk['reward'][t].astype(np.float64)
    ended = blk['episode_end'][t] != 0
    done += running[ended].tolist()
    running[ended] = 0.0
  # (torch's float32 reduction order is not ours: at most ~100 terms of magnitude at most 5 keep it three orders inside 1e-5)
  assert len(done) == s['episodes'] and abs(s['mean_return'] - np.mean(done)) <= 1e-5 * abs(np.mean(done)), (s['mean_return'], np.mean(done))
  # the same loop with the normalisation
  env_n, _, ro_n, stats_n = _recorded_loop(mods, normalize=True)
  assert np.array_equal(_bits(ro_n.ret.cpu().numpy()), _bits(ret)), 'the returns are not normalised'
  err = ppo_host.ulps_from(ro_n.advantage.cpu().numpy(), ppo_host.normalize_f64(adv))
  print('loop: episodes', s['episodes'], 'terminals', int(blk['terminal'].sum()), 'normalised advantage, worst ulp', err.max())
  assert (err <= 1.0).all(), err.max()
  assert stats_n[0]['episodes'] == s['episodes'] and stats_n[0]['mean_return'] == s['mean_return']


# ---------------------------------------------------------------------------------------------------------------------------- learns
def test_learns_a_contextual_bandit_on_policy(mods, observations):
  """test_gpu_train.py's bandit, on-policy: every step terminal, reward 1 for the labelled action (0 or 2 as the most varied feature
  within [0, 1] is below or above its median), blocks of T = 1 x 256 sampled actions, 4 epochs of B = 128 per block.  After 60 blocks
  (480 updates) the greedy policy is right on >= 90 % of the held-out rows and the mean sampled reward of the last 10 blocks is >= 0.8.
  Measured: DESIGN §3m."""
  qnet, _, ac = mods
  x = observations.cpu().numpy()
  std = np.where((x.min(axis=0) >= 0) & (x.max(axis=0) <= 1), x.std(axis=0), 0.0)
  col = int(np.argmax(std))
  label = np.where(x[:, col] > np.median(x[:, col]), 2, 0).astype(np.uint8)
  rng = np.random.default_rng(0)
  perm = rng.permutation(len(x))
  train_i, test_i = perm[:768], perm[768:]
  n_env, blocks = 256, 60
  label_d = torch.from_numpy(label).cuda()
  tr = ac.PPOTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', 7, 2, 64), num_atoms=2), lr=1e-3, seed=5)
  ro = ac.VecRolloutBuffer(n_env, 1, 'cuda')
  actions = torch.zeros(n_env, dtype=torch.uint8, device='cuda')
  logp, value = torch.zeros(n_env, device='cuda'), torch.zeros(n_env, device='cuda')
  ones, zeros = torch.ones(n_env, dtype=torch.uint8, device='cuda'), torch.zeros(n_env, device='cuda')
  rewards = torch.zeros(blocks, device='cuda')
  for k in range(blocks):
    i = torch.from_numpy(rng.choice(train_i, n_env)).cuda()
    obs = observations[i]
    tr.act(obs, actions, logp, value)
    reward = (actions == label_d[i]).to(torch.float32)
    rewards[k] = reward.mean()
    ro.add(0, obs, actions, logp, value, reward, ones)
    ro.finish(zeros, tr.gamma, tr.lam, tr.normalize_advantage)
    for _ in range(4):
      for bt in ro.minibatches(128):
        tr.train_on_batch(bt)
  tr.check_errors()
  assert int(tr.adam_step.item()) == blocks * 8
  agent = ac.VecActorCriticAgent(tr.network())
  act = agent.act(observations[torch.from_numpy(test_i).cuda()]).cpu().numpy()
  acc = float((act == label[test_i]).mean())
  last = float(rewards[-10:].mean().item())
  print('held-out accuracy', acc, 'mean sampled reward of the last 10 blocks', last, 'of the first 3', float(rewards[:3].mean().item()))
  assert acc >= 0.9, acc
  assert last >= 0.8, last


# ------------------------------------------------------------------------------------------------------------------------ end to end
def test_ppo_loop_end_to_end(mods):
  qnet, _, ac = mods
  from balloon_learning_environment_amd.eval import eval_lib, suites
  tr, ro, stats = _loop(mods, True, iterations=2)
  assert len(stats) == 2
  for s in stats:
    assert s['updates'] == 8 and np.isfinite(s['mean_loss']) and s['episodes'] >= 64 and np.isfinite(s['mean_return'])
    assert 0.0 <= s['time_within_radius'] <= 1.0
  assert stats[1]['transitions'] == 2 * 8 * 64
  tr.check_errors()
  assert np.isfinite(tr.weights.cpu().numpy()).all() and np.isfinite(ro.advantage.cpu().numpy()).all()
  agent = ac.VecActorCriticAgent(tr.network())
  assert agent.get_name() == 'ActorCriticAgent'
  res = eval_lib.eval_agent_vec(agent, suites.get_eval_suite('small_eval'))
  assert len(res) == 100 and all(np.isfinite(r.cumulative_reward) for r in res)
