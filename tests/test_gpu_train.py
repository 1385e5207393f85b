"""The device QR-DQN trainer (csrc/ble_train.h, agents/qnet_train.py, train_lib.run_training_loop_vec) against the float64 restatement
of Dopamine 4.0.0's update (train_host.py):

 * replay: sampled windows, returns, discounts, actions and rows equal a host restatement exactly; no invalid window is drawn;
 * the loss, the targets and dL/dlogits against the oracle evaluated on the device's own float32 logits and targets;
 * the gradient image against float64 backprop on the device's activations, within the magnitude bound; the padding exactly zero;
   at B = 32 and 600 and at the batch edges 1, 7, 9, 33, 129, 511, 513 and 4097 (EDGE_BATCHES);
 * Adam against float64 optax arithmetic over 10 steps, and over 3 on a two-slab gradient; the padding of the weights stays zero;
 * determinism: two trainers, graph vs eager, and a state_dict restored mid-run give the same bits;
 * it learns a contextual bandit over real observations;
 * run_training_loop_vec end to end, its policy through eval_agent_vec.
"""
import numpy as np
import pytest
import torch

import qnet_host
import train_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import qnet, qnet_train
  return qnet, qnet_train


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


def _params(qnet, layers, hidden, atoms, seed=7, bias=1e-2):
  params = qnet.init_params('quantile', seed, layers, hidden, atoms)
  rng = np.random.default_rng(seed + 1)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * bias).astype(np.float32)
  return params


def _trainer(mods, layers, hidden, atoms, **kw):
  qnet, qnet_train = mods
  params = _params(qnet, layers, hidden, atoms)
  return params, qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(params), **kw)


def _batch(mods, observations, b, seed, ret_scale=1.0):
  _, qnet_train = mods
  rng = np.random.default_rng(seed)
  x = observations.cpu().numpy()
  i, j = rng.integers(0, len(x), b), rng.integers(0, len(x), b)
  disc = np.where(rng.random(b) < 0.2, 0.0, 0.993 ** 5).astype(np.float32)
  ret = (rng.standard_normal(b) * ret_scale).astype(np.float32)
  return x[i], qnet_train.TrainBatch.from_tensors(x[i], x[j], ret, disc, rng.integers(0, 3, b), 'cuda')


# ---------------------------------------------------------------------------------------------------------------------------- replay
def _fill(qnet_train, n_env=8, cap=40, steps=60, horizon=5, seed=0, end_p=0.05, term_p=0.08):
  rng = np.random.default_rng(seed)
  rp = qnet_train.VecReplayBuffer(n_env, cap, horizon, 0.993)
  hist = {'obs': rng.random((steps, n_env, 1099), dtype=np.float32), 'action': rng.integers(0, 3, (steps, n_env)).astype(np.uint8),
          'reward': (np.arange(steps)[:, None] * 100 + np.arange(n_env)[None, :] + rng.random((steps, n_env))).astype(np.float32),
          'terminal': (rng.random((steps, n_env)) < term_p).astype(np.uint8)}
  hist['episode_end'] = np.maximum(hist['terminal'], (rng.random((steps, n_env)) < end_p).astype(np.uint8))
  for s in range(steps):
    rp.add(*[torch.from_numpy(hist[k][s]).cuda() for k in ('obs', 'action', 'reward', 'terminal', 'episode_end')])
  return rp, hist


def test_replay_sample_matches_host(mods):
  _, qnet_train = mods
  rp, h = _fill(qnet_train)
  steps, n = h['reward'].shape
  cap, hz = rp.capacity, rp.update_horizon
  counter = torch.zeros(1, dtype=torch.int64, device='cuda')
  seen = 0
  for draw in range(4):
    bt = rp.sample(300, seed=11, counter=counter)
    idx = bt.index.cpu().numpy()
    st, ns = bt.state.cpu().numpy(), bt.next_state.cpu().numpy()
    ret, disc, act = bt.ret.cpu().numpy(), bt.discount.cpu().numpy(), bt.action.cpu().numpy()
    rp.check_errors()
    for b, (t, e) in enumerate(idx):
      assert steps - cap <= t and t + hz <= steps - 1 and 0 <= e < n, (t, e)
      w = train_host.nstep(h['reward'], h['terminal'], h['episode_end'], t, e, hz, 0.993)
      assert w is not None, ('an invalid window was sampled', t, e)
      m, r, d, _ = w
      assert ret[b].view(np.uint32) == r.view(np.uint32), (t, e, ret[b], r)
      assert disc[b].view(np.uint32) == d.view(np.uint32)
      assert act[b] == h['action'][t, e]
      assert np.array_equal(st[b, :1099], h['obs'][t, e]) and np.array_equal(ns[b, :1099], h['obs'][t + m, e])
      assert not st[b, 1099:].any() and not ns[b, 1099:].any()
      seen += 1
    assert int(counter.item()) == draw + 1
  assert seen == 1200
  # the same (seed, counter) draws the same windows; another counter others
  a = rp.sample(64, seed=11, counter=torch.zeros(1, dtype=torch.int64, device='cuda')).index.cpu().numpy().copy()
  b = rp.sample(64, seed=11, counter=torch.zeros(1, dtype=torch.int64, device='cuda')).index.cpu().numpy().copy()
  c = rp.sample(64, seed=11, counter=torch.ones(1, dtype=torch.int64, device='cuda')).index.cpu().numpy().copy()
  assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_replay_without_valid_window_flags(mods):
  _, qnet_train = mods
  rp, _ = _fill(qnet_train, steps=20, end_p=1.0, term_p=0.0)      # every step a time-limit end: no window is valid
  bt = rp.sample(4, seed=1)
  assert (bt.index.cpu().numpy() == -1).all() and not bt.discount.cpu().numpy().any()
  with pytest.raises(RuntimeError):
    rp.check_errors()


# ------------------------------------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize('atoms', [51, 1])
@pytest.mark.parametrize('b', [1, 32, 300])
def test_loss_and_dlogits(mods, observations, atoms, b):
  _, tr = _trainer(mods, 2, 64, atoms)
  tr.target.mul_(1.5)                 # a target network other than the online one
  _, bt = _batch(mods, observations, b, seed=b)
  tr.train_on_batch(bt, apply_update=False)
  v = {k: (x.cpu().numpy() if k != 'acts' else None) for k, x in tr.views(b).items()}
  ret, disc, act = bt.ret.cpu().numpy(), bt.discount.cpu().numpy(), bt.action.cpu().numpy()
  t64 = train_host.targets(v['target_logits'], ret, disc, atoms)
  assert np.allclose(v['targets'], t64, rtol=1e-6, atol=1e-6 * np.abs(t64).max())
  loss, dlog = train_host.quantile_loss(v['logits'], v['targets'], act, atoms)
  assert np.allclose(v['loss'], loss, rtol=2e-6, atol=1e-7 * loss.max()), np.abs(v['loss'] - loss).max()
  out = 3 * atoms
  assert np.allclose(v['dlogits'][:, :out], dlog, rtol=2e-6, atol=1e-7 * np.abs(dlog).max())
  assert not v['dlogits'][:, out:].any()
  assert (v['dlogits'][:, :out][dlog == 0] == 0).all()


def test_loss_finite_on_extreme_targets(mods, observations):
  _, tr = _trainer(mods, 2, 64, 51)
  _, bt = _batch(mods, observations, 32, seed=9, ret_scale=1e20)
  loss = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  v = tr.views(32)
  assert np.isfinite(loss).all() and np.isfinite(v['dlogits'].cpu().numpy()).all() and np.isfinite(tr.grad.cpu().numpy()).all()
  # |u| >> kappa: every clipped derivative is +-kappa, so |dL/dtheta_i| = (sum_j |tau_i - 1{u < 0}|) / (A B) <= 1 / B
  assert np.abs(v['dlogits'].cpu().numpy()).max() <= 1.0 / 32 * (1 + 1e-6)


# -------------------------------------------------------------------------------------------------------------------------- gradient
def _repacked(qnet, tree, atoms):
  return qnet.QNetwork.from_params(tree, num_atoms=atoms).packed_host


# Batch edges of the backward pass: one row, either side of the 8-row MFMA step, a ragged last dX tile, the last size with one dW slab
# and the first with two (slabs of ceil(513 / 2) = 257 rows), and the first size past 16 slabs (4097: slabs of 257 rows again).
EDGE_BATCHES = (1, 7, 9, 33, 129, 511, 513, 4097)


@pytest.mark.parametrize('layers,hidden,atoms,b', [(2, 64, 51, 32), (3, 37, 7, 32), (8, 600, 51, 32), (2, 64, 51, 600)] +
                         [(2, 64, 51, b) for b in EDGE_BATCHES] + [(3, 37, 7, 1), (3, 37, 7, 513)])
def test_gradient_against_float64_backprop(mods, observations, layers, hidden, atoms, b):
  qnet, qnet_train = mods
  params, tr = _trainer(mods, layers, hidden, atoms)
  x, bt = _batch(mods, observations, b, seed=layers)
  tr.train_on_batch(bt, apply_update=False)
  v = tr.views(b)
  out = 3 * atoms
  acts = [a.cpu().numpy() for a in v['acts']]
  acts = [a[:, :hidden] for a in acts[:-1]] + [acts[-1][:, :out]]
  dlog = v['dlogits'].cpu().numpy()[:, :out]
  want = train_host.backward(params, x, dlog, acts)
  mag = train_host.backward_magnitude(params, x, dlog, acts)
  g = tr.grad.cpu().numpy()
  got = qnet_train.unpack(tr._net, g)['params']
  worst = 0.0
  for l in range(layers):
    for leaf, i in (('kernel', 0), ('bias', 1)):
      err = np.abs(got[f'Dense_{l}'][leaf] - want[l][i])
      bound = 1e-5 * mag[l][i] + 1e-30
      worst = max(worst, float((err / bound).max()))
  print('B', b, 'worst |g - g64| / (1e-5 S)', worst)
  assert worst <= 1.0, worst
  # the padding of the gradient image is exactly zero: packing the unpacked gradient gives the image back
  assert np.array_equal(_repacked(qnet, {'params': got}, atoms).view(np.uint32), g.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_against_optax_arithmetic(mods, observations):
  _adam_against_optax_arithmetic(mods, observations, 64, 10)


def test_adam_against_optax_arithmetic_on_a_two_slab_gradient(mods, observations):
  """B = 513: the gradient Adam reads is the sum of two slab images; three steps."""
  _adam_against_optax_arithmetic(mods, observations, 513, 3)


def _adam_against_optax_arithmetic(mods, observations, b, steps):
  qnet, qnet_train = mods
  _, tr = _trainer(mods, 3, 37, 7, lr=1e-3, eps=2e-5)
  _, bt = _batch(mods, observations, b, seed=3)
  w, m, v = (t.cpu().numpy().astype(np.float64) for t in (tr.weights, tr.adam_m, tr.adam_v))
  for t in range(1, steps + 1):
    tr.train_on_batch(bt)
    g = tr.grad.cpu().numpy()
    w64, m64, v64 = train_host.adam(w, g, m, v, t, lr=1e-3, eps=2e-5)
    wd, md, vd = (x.cpu().numpy() for x in (tr.weights, tr.adam_m, tr.adam_v))
    ulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
    assert (np.abs(wd - w64) <= 4 * ulp + 1e-6 * 1e-3).all(), (t, np.abs(wd - w64).max())
    # (m can cancel: its error is bounded by the magnitudes of its two terms)
    assert (np.abs(md - m64) <= 1e-6 * (0.1 * np.abs(g) + 0.9 * np.abs(m)) + 1e-38).all(), t
    assert (np.abs(vd - v64) <= 1e-6 * v64 + 1e-38).all(), t
    w, m, v = wd.astype(np.float64), md.astype(np.float64), vd.astype(np.float64)
  assert int(tr.adam_step.item()) == steps
  wd = tr.weights.cpu().numpy()
  assert np.array_equal(_repacked(qnet, qnet_train.unpack(tr._net, wd), 7).view(np.uint32), wd.view(np.uint32))
  assert not np.array_equal(wd, qnet.QNetwork.from_params(_params(qnet, 3, 37, 7)).packed_host)
  # the transposed image follows the weights
  wt = tr.weights_t.cpu().numpy().copy()
  tr._retranspose()
  assert np.array_equal(wt.view(np.uint32), tr.weights_t.cpu().numpy().view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------- determinism
def test_determinism_graph_and_resume(mods):
  _, qnet_train = mods
  rp, _ = _fill(qnet_train, n_env=16, cap=64, steps=64)
  runs = []
  for graph in (False, True):
    _, tr = _trainer(mods, 2, 64, 51, lr=1e-3)
    if graph:
      tr.capture(rp, 32)
      for _ in range(49):
        tr.train_step(rp, 32)
    else:
      for _ in range(50):
        tr.train_step(rp, 32)
    runs.append(tr.weights.cpu().numpy().copy())
  _, tr2 = _trainer(mods, 2, 64, 51, lr=1e-3)
  for _ in range(50):
    tr2.train_step(rp, 32)
  assert np.array_equal(runs[0].view(np.uint32), tr2.weights.cpu().numpy().view(np.uint32)), 'two trainers differ'
  assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), 'graph replay differs from eager'
  # state_dict mid-run
  _, a = _trainer(mods, 2, 64, 51, lr=1e-3)
  for _ in range(25):
    a.train_step(rp, 32)
  sd = a.state_dict()
  for k in range(25):
    a.train_step(rp, 32)
    if k == 9:
      a.sync_target()
  _, c = _trainer(mods, 2, 64, 51, lr=1e-3, seed=99)
  c.load_state_dict(sd)
  for k in range(25):
    c.train_step(rp, 32)
    if k == 9:
      c.sync_target()
  assert np.array_equal(a.weights.cpu().numpy().view(np.uint32), c.weights.cpu().numpy().view(np.uint32)), 'resume differs'


# ---------------------------------------------------------------------------------------------------------------------------- learns
def test_learns_a_contextual_bandit(mods, observations):
  """Every transition terminal; reward 1 for the right action, 0 otherwise, the right action being 0 or 2 as one observation feature
  (the most varied of those within [0, 1]) is below or above its median: after a few hundred updates the greedy action is right on
  >= 90 % of held-out states and the mean |q - r| is below 0.2."""
  qnet, qnet_train = mods
  x = observations.cpu().numpy()
  std = np.where((x.min(axis=0) >= 0) & (x.max(axis=0) <= 1), x.std(axis=0), 0.0)
  col = int(np.argmax(std))
  label = np.where(x[:, col] > np.median(x[:, col]), 2, 0).astype(np.uint8)
  rng = np.random.default_rng(0)
  perm = rng.permutation(len(x))
  train_i, test_i = perm[:768], perm[768:]
  n_env, steps = 64, 48
  rp = qnet_train.VecReplayBuffer(n_env, steps, update_horizon=1, gamma=0.99)
  for s in range(steps):
    i = rng.choice(train_i, n_env)
    a = rng.integers(0, 3, n_env).astype(np.uint8)
    r = (a == label[i]).astype(np.float32)
    rp.add(torch.from_numpy(x[i]).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(r).cuda(), torch.ones(n_env, dtype=torch.uint8,
                                                                                                              device='cuda'))
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(_params(qnet, 2, 64, 51, bias=0.0)), lr=1e-3, update_horizon=1, seed=5)
  for _ in range(600):
    tr.train_step(rp, 128)
  tr.check_errors()
  rp.check_errors()
  agent = qnet.VecQNetworkAgent(tr.network())
  q = torch.empty(len(test_i), 3, dtype=torch.float32, device='cuda')
  act = agent.act(torch.from_numpy(x[test_i]).cuda(), q_values=q).cpu().numpy()
  acc = float((act == label[test_i]).mean())
  r = (np.arange(3)[None, :] == label[test_i][:, None]).astype(np.float64)
  err = float(np.abs(q.cpu().numpy() - r).mean())
  assert acc >= 0.9, acc
  assert err <= 0.2, err


# ------------------------------------------------------------------------------------------------------------------------ end to end
def test_training_loop_end_to_end(mods):
  qnet, qnet_train = mods
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.env import balloon_env
  from balloon_learning_environment_amd.eval import eval_lib, suites
  finals = []
  for _ in range(2):
    env = balloon_env.VecBalloonEnv(256, seed=1)
    params = _params(qnet, 2, 64, 51)
    tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(params), lr=1e-4, seed=2)
    rp = qnet_train.VecReplayBuffer(256, 32, update_horizon=5, gamma=0.993)
    stats = train_lib.run_training_loop_vec(env, tr, rp, num_iterations=2, steps_per_iteration=8, max_episode_length=7,
                                            min_replay_history=256 * 6, updates_per_step=4, epsilon=0.1, seed=3)
    assert len(stats) == 2 and stats[1]['updates'] == 32 and np.isfinite(stats[1]['mean_loss'])
    assert stats[0]['episodes'] >= 256 and stats[1]['episodes'] >= 256          # the 7-step time limit ends every episode
    assert 0.0 <= stats[1]['time_within_radius'] <= 1.0
    w = tr.weights.cpu().numpy()
    assert not np.array_equal(w, qnet.QNetwork.from_params(params).packed_host)
    assert rp.episode_end.any() and int(rp.count.item()) == 16
    finals.append(w.copy())
  assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))
  res = eval_lib.eval_agent_vec(qnet.VecQNetworkAgent(tr.network()), suites.get_eval_suite('small_eval'))
  assert len(res) == 100 and all(np.isfinite(r.cumulative_reward) for r in res)
