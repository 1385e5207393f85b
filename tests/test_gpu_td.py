"""The device DQN and SARSA learners (csrc/ble_train.h's TD losses and SGD, agents/dqn_agent.py, agents/mlp_agent.py,
train_lib.run_online_loop_vec) against their float64 restatements (td_host.py, train_host.py), case for case after test_gpu_train.py and
with its tolerances:

 * loss, targets and dL/dlogits of each kind against the twin evaluated on the device's own float32 logits; exact zeros; a masked row;
 * returns scaled by 1e20: Huber stays finite and bounded, MSE gives no NaN;
 * the gradient image of SARSA's two branches and of DQN's losses against float64 backprop, within the magnitude bound, at
   test_gpu_train.py's batch edges too; the padding exactly zero;
 * SGD against float64 arithmetic over 10 updates; the transposed image follows; the padding stays zero;
 * determinism: two instances, graph vs eager, a state_dict restored mid-run;
 * VecMLPAgent: pre-update actions, N = 1 against sequential twin updates, eval mode, masked rows' observations do not matter;
 * they learn the contextual bandit of test_gpu_train.py to its bars;
 * run_training_loop_vec with DQNTrainer and run_online_loop_vec with VecMLPAgent end to end.
"""
import numpy as np
import pytest
import torch

import td_host
import train_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import dqn_agent, mlp_agent, qnet, qnet_train
  return qnet, qnet_train, dqn_agent, mlp_agent


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


def _params(qnet, layers, hidden, seed=7, bias=1e-2):
  params = qnet.init_params('mlp', seed, layers, hidden)
  rng = np.random.default_rng(seed + 1)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * bias).astype(np.float32)
  return params


def _dqn(mods, layers, hidden, **kw):
  qnet, _, dqn_agent, _ = mods
  params = _params(qnet, layers, hidden)
  return params, dqn_agent.DQNTrainer(qnet.QNetwork.from_params(params), **kw)


def _mlp(mods, n, layers, hidden, **kw):
  qnet, _, _, mlp_agent = mods
  params = _params(qnet, layers, hidden)
  return params, mlp_agent.VecMLPAgent(n, qnet.QNetwork.from_params(params), **kw)


def _batch(mods, observations, b, seed, ret_scale=1.0):
  qnet_train = mods[1]
  rng = np.random.default_rng(seed)
  x = observations.cpu().numpy()
  i, j = rng.integers(0, len(x), b), rng.integers(0, len(x), b)
  disc = np.where(rng.random(b) < 0.2, 0.0, 0.993 ** 5).astype(np.float32)
  ret = (rng.standard_normal(b) * ret_scale).astype(np.float32)
  return x[i], qnet_train.TrainBatch.from_tensors(x[i], x[j], ret, disc, rng.integers(0, 3, b), 'cuda')


def _transitions(agent, observations, seed, ret_scale=1.0, mask_p=0.25):
  """Fills a VecMLPAgent's own buffers with N random transitions; returns them on the host (float32 / uint8)."""
  rng = np.random.default_rng(seed)
  x = observations.cpu().numpy()
  n = agent.num_envs
  i, j = rng.integers(0, len(x), n), rng.integers(0, len(x), n)
  t = {'state': x[i], 'next_state': x[j], 'reward': (rng.standard_normal(n) * ret_scale).astype(np.float32),
       'action': rng.integers(0, 3, n).astype(np.uint8), 'next_action': rng.integers(0, 3, n).astype(np.uint8),
       'mask': (rng.random(n) < mask_p).astype(np.uint8)}
  if n > 1 and mask_p > 0:
    t['mask'][0], t['mask'][1] = 1, 0
  agent.last_obs[:, :1099].copy_(torch.from_numpy(t['state']))
  agent.obs[:, :1099].copy_(torch.from_numpy(t['next_state']))
  for name, buf in (('reward', agent.reward), ('action', agent.last_action), ('next_action', agent.action), ('mask', agent.mask)):
    buf.copy_(torch.from_numpy(t[name]))
  return t


def _close(got, want, name):
  scale = np.abs(want).max()
  assert np.allclose(got, want, rtol=2e-6, atol=1e-7 * scale), (name, np.abs(got - want).max(), scale)


# ------------------------------------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize('kind', ['mse', 'huber'])
@pytest.mark.parametrize('b', [1, 32, 300])
def test_dqn_loss_and_dlogits(mods, observations, kind, b):
  _, tr = _dqn(mods, 2, 64, loss_type=kind)
  tr.target.mul_(1.5)                 # a target network other than the online one
  _, bt = _batch(mods, observations, b, seed=b)
  tr.train_on_batch(bt, apply_update=False)
  tr.check_errors()
  v = {k: x.cpu().numpy() for k, x in tr.views(b).items() if k != 'acts'}
  ret, disc, act = bt.ret.cpu().numpy(), bt.discount.cpu().numpy(), bt.action.cpu().numpy()
  assert not np.array_equal(v['logits'], v['target_logits'])
  t64 = td_host.dqn_targets(v['target_logits'], ret, disc)
  print('targets', np.abs(v['targets'][:, 0] - t64).max(), np.abs(t64).max())
  assert np.allclose(v['targets'][:, 0], t64, rtol=1e-6, atol=1e-6 * np.abs(t64).max())
  loss, dlog = td_host.dqn_loss(v['logits'], v['targets'][:, 0], act, kind)
  print('loss', np.abs(v['loss'] - loss).max(), loss.max(), 'dlogits', np.abs(v['dlogits'][:, :3] - dlog).max(), np.abs(dlog).max())
  _close(v['loss'], loss, 'loss')
  _close(v['dlogits'][:, :3], dlog, 'dlogits')
  assert not v['dlogits'][:, 3:].any()
  assert (v['dlogits'][:, :3][dlog == 0] == 0).all()


@pytest.mark.parametrize('b', [1, 32, 300])
def test_sarsa_loss_and_dlogits(mods, observations, b):
  for mask_p in (0.25, 0.0, 1.0):
    _, ag = _mlp(mods, b, 2, 64, gamma=0.9)
    t = _transitions(ag, observations, seed=b, mask_p=mask_p)
    loss_d = ag.train_on_transitions(apply_update=False).cpu().numpy()
    ag.check_errors()
    v = ag.views()
    logits, dl = v['logits'].cpu().numpy(), v['dlogits'].cpu().numpy()
    tgt, loss, ds, dn = td_host.sarsa_loss(logits[0], logits[1], t['reward'], t['action'], t['next_action'], np.float64(np.float32(0.9)),
                                           t['mask'])
    print('b', b, 'mask_p', mask_p, 'targets', np.abs(v['targets'].cpu().numpy() - tgt).max(), 'loss', np.abs(loss_d - loss).max(),
          loss.max(), 'dlogits', np.abs(dl[0, :, :3] - ds).max(), np.abs(dl[1, :, :3] - dn).max(), np.abs(ds).max())
    assert np.allclose(v['targets'].cpu().numpy(), tgt, rtol=1e-6, atol=1e-6 * np.abs(tgt).max())
    masked = t['mask'] != 0
    assert not loss_d[masked].any() and not dl[:, masked].any()          # exactly 0: the loss and both dlogits rows
    if masked.all():
      assert not loss_d.any() and not dl.any()
      continue
    _close(loss_d, loss, 'loss')
    _close(dl[0, :, :3], ds, 'dlogits(state)')
    _close(dl[1, :, :3], dn, 'dlogits(next_state)')
    assert not dl[:, :, 3:].any()
    assert (dl[0, :, :3][ds == 0] == 0).all() and (dl[1, :, :3][dn == 0] == 0).all()


def test_action_out_of_range_flags_and_zeroes_the_row(mods, observations):
  _, ag = _mlp(mods, 8, 2, 64)
  _transitions(ag, observations, seed=1, mask_p=0.0)
  ag.action[3] = 3                    # a next action out of range
  ag.last_action[5] = 200
  loss = ag.train_on_transitions(apply_update=False).cpu().numpy()
  dl = ag.views()['dlogits'].cpu().numpy()
  assert loss[3] == 0 and loss[5] == 0 and not dl[:, 3].any() and not dl[:, 5].any() and loss[[0, 1, 2, 4, 6, 7]].all()
  with pytest.raises(ValueError):
    ag.check_errors()
  _, tr = _dqn(mods, 2, 64)
  _, bt = _batch(mods, observations, 8, seed=2)
  bt.action[2] = 3
  loss = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  assert loss[2] == 0 and not tr.views(8)['dlogits'].cpu().numpy()[2].any()
  with pytest.raises(ValueError):
    tr.check_errors()


def test_loss_on_extreme_returns(mods, observations):
  """ret scaled by 1e20.  Huber: finite, every derivative clipped to +-1 so |dL/dq| <= 1 / B.  MSE (DQN and SARSA): u^2 may overflow to
  inf, but finite input gives no NaN anywhere, the gradient image included."""
  b = 32
  _, tr = _dqn(mods, 2, 64, loss_type='huber')
  _, bt = _batch(mods, observations, b, seed=9, ret_scale=1e20)
  loss = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  dl = tr.views(b)['dlogits'].cpu().numpy()
  assert np.isfinite(loss).all() and np.isfinite(dl).all() and np.isfinite(tr.grad.cpu().numpy()).all()
  assert np.abs(dl).max() <= (1.0 + 1e-6) / b and np.abs(dl).max() > 0
  _, tr = _dqn(mods, 2, 64, loss_type='mse')
  loss = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  assert not np.isnan(loss).any() and not np.isnan(tr.views(b)['dlogits'].cpu().numpy()).any() and not np.isnan(tr.grad.cpu().numpy()).any()
  assert np.isinf(loss).any()                                             # (1e20)^2 is beyond float32
  _, ag = _mlp(mods, b, 2, 64)
  _transitions(ag, observations, seed=9, ret_scale=1e20)
  loss = ag.train_on_transitions(apply_update=False).cpu().numpy()
  assert not np.isnan(loss).any() and not np.isnan(ag.views()['dlogits'].cpu().numpy()).any() and not np.isnan(ag.grad.cpu().numpy()).any()


# -------------------------------------------------------------------------------------------------------------------------- gradient
def _repacked(qnet, tree):
  return qnet.QNetwork.from_params(tree, num_atoms=1).packed_host


def _worst(got, want, mag, layers):
  worst = 0.0
  for l in range(layers):
    for leaf, i in (('kernel', 0), ('bias', 1)):
      err = np.abs(got[f'Dense_{l}'][leaf] - want[l][i])
      worst = max(worst, float((err / (1e-5 * mag[l][i] + 1e-30)).max()))
  return worst


EDGE_BATCHES = (1, 7, 9, 33, 129, 511, 513, 4097)          # test_gpu_train.py's batch edges of the backward pass


@pytest.mark.parametrize('layers,hidden,b', [(1, 0, 32), (2, 64, 32), (3, 37, 32), (8, 600, 32), (2, 64, 600)] +
                         [(2, 64, b) for b in EDGE_BATCHES])
def test_sarsa_gradient_against_float64_backprop(mods, observations, layers, hidden, b):
  """Both branches into the one gradient image: |g - g64| <= 1e-5 S, S = train_host.backward_magnitude summed over the branches, on the
  device's own activations and dlogits.  B = 600 takes the slab path (2 slabs per branch)."""
  qnet, qnet_train = mods[0], mods[1]
  params, ag = _mlp(mods, b, layers, hidden)
  t = _transitions(ag, observations, seed=layers, mask_p=0.25 if b > 1 else 0.0)      # (B = 1: the one row takes part)
  ag.train_on_transitions(apply_update=False)
  v = ag.views()
  width = lambda l: 3 if l == layers - 1 else hidden
  acts = [[a[br].cpu().numpy()[:, :width(l)] for l, a in enumerate(v['acts'])] for br in range(2)]
  dl = v['dlogits'].cpu().numpy()[:, :, :3]
  want = td_host.sarsa_backward(params, t['state'], t['next_state'], dl[0], dl[1], acts[0], acts[1])
  mag = td_host.sarsa_backward(params, t['state'], t['next_state'], dl[0], dl[1], acts[0], acts[1], magnitude=True)
  g = ag.grad.cpu().numpy()
  got = qnet_train.unpack(ag._net, g)['params']
  worst = _worst(got, want, mag, layers)
  print('B', b, 'worst |g - g64| / (1e-5 S)', worst)
  assert worst <= 1.0, worst
  assert any(np.abs(want[l][0]).max() > 0 for l in range(layers))
  # the padding of the gradient image is exactly zero: packing the unpacked gradient gives the image back
  assert np.array_equal(_repacked(qnet, {'params': got}).view(np.uint32), g.view(np.uint32))


@pytest.mark.parametrize('kind,layers,hidden,b', [pytest.param(kind, 3, 37, 32, id=kind) for kind in ('mse', 'huber')] +
                         [(kind, 2, 64, b) for kind in ('mse', 'huber') for b in EDGE_BATCHES])
def test_dqn_gradient_against_float64_backprop(mods, observations, kind, layers, hidden, b):
  qnet, qnet_train = mods[0], mods[1]
  params, tr = _dqn(mods, layers, hidden, loss_type=kind)
  x, bt = _batch(mods, observations, b, seed=4)
  tr.train_on_batch(bt, apply_update=False)
  v = tr.views(b)
  acts = [a.cpu().numpy() for a in v['acts']]
  acts = [a[:, :hidden] for a in acts[:-1]] + [acts[-1][:, :3]]
  dlog = v['dlogits'].cpu().numpy()[:, :3]
  want, mag = train_host.backward(params, x, dlog, acts), train_host.backward_magnitude(params, x, dlog, acts)
  g = tr.grad.cpu().numpy()
  got = qnet_train.unpack(tr._net, g)['params']
  worst = _worst(got, want, mag, layers)
  print(kind, 'B', b, 'worst |g - g64| / (1e-5 S)', worst)
  assert worst <= 1.0, worst
  assert np.array_equal(_repacked(qnet, {'params': got}).view(np.uint32), g.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------- SGD
def test_sgd_against_float64_arithmetic(mods, observations):
  qnet, qnet_train = mods[0], mods[1]
  lr = 1e-3
  _, ag = _mlp(mods, 64, 3, 37, learning_rate=lr)
  _transitions(ag, observations, seed=3)
  w = ag.weights.cpu().numpy().astype(np.float64)
  first = w.copy()
  worst = 0.0
  for t in range(1, 11):
    ag.train_on_transitions()
    w64 = td_host.sgd(w, ag.grad.cpu().numpy(), np.float64(np.float32(lr)))
    wd = ag.weights.cpu().numpy()
    ulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
    worst = max(worst, float((np.abs(wd - w64) / (4 * ulp + 1e-6 * lr)).max()))
    assert (np.abs(wd - w64) <= 4 * ulp + 1e-6 * lr).all(), (t, np.abs(wd - w64).max())
    w = wd.astype(np.float64)
  print('worst |w - w64| / bound', worst)
  wd = ag.weights.cpu().numpy()
  assert np.array_equal(_repacked(qnet, qnet_train.unpack(ag._net, wd)).view(np.uint32), wd.view(np.uint32))      # the padding is zero
  assert not np.array_equal(wd, first.astype(np.float32))
  wt = ag.weights_t.cpu().numpy().copy()                     # the transposed image follows the weights
  ag._retranspose()
  assert np.array_equal(wt.view(np.uint32), ag.weights_t.cpu().numpy().view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------- determinism
def _fill(qnet_train, n_env=16, cap=64, steps=64, horizon=5, seed=0, end_p=0.05, term_p=0.08):
  rng = np.random.default_rng(seed)
  rp = qnet_train.VecReplayBuffer(n_env, cap, horizon, 0.993)
  for s in range(steps):
    term = (rng.random(n_env) < term_p).astype(np.uint8)
    end = np.maximum(term, (rng.random(n_env) < end_p).astype(np.uint8))
    rp.add(torch.from_numpy(rng.random((n_env, 1099), dtype=np.float32)).cuda(), torch.from_numpy(rng.integers(0, 3, n_env).astype(np.uint8)).cuda(),
           torch.from_numpy(rng.random(n_env, dtype=np.float32)).cuda(), torch.from_numpy(term).cuda(), torch.from_numpy(end).cuda())
  return rp


def _bits(t):
  return t.cpu().numpy().view(np.uint32).copy()


@pytest.mark.parametrize('kind', ['mse', 'huber'])
def test_dqn_determinism_graph_and_resume(mods, kind):
  qnet_train = mods[1]
  rp = _fill(qnet_train)
  runs = []
  for graph in (False, True, False):
    _, tr = _dqn(mods, 2, 64, lr=1e-3, loss_type=kind)
    if graph:
      tr.capture(rp, 32)
    for _ in range(49 if graph else 50):
      tr.train_step(rp, 32)
    tr.check_errors()
    runs.append(_bits(tr.weights))
  assert np.array_equal(runs[0], runs[2]), 'two trainers differ'
  assert np.array_equal(runs[0], runs[1]), 'graph replay differs from eager'
  _, a = _dqn(mods, 2, 64, lr=1e-3, loss_type=kind)
  for _ in range(25):
    a.train_step(rp, 32)
  sd = a.state_dict()
  assert sd['loss_type'] == kind
  for k in range(25):
    a.train_step(rp, 32)
    if k == 9:
      a.sync_target()
  _, c = _dqn(mods, 2, 64, lr=1e-3, seed=99, loss_type='huber' if kind == 'mse' else 'mse')
  c.load_state_dict(sd)
  assert c.loss_type == kind
  for k in range(25):
    c.train_step(rp, 32)
    if k == 9:
      c.sync_target()
  assert np.array_equal(_bits(a.weights), _bits(c.weights)), 'resume differs'


def test_dqn_refuses_prioritized_replay(mods):
  qnet_train = mods[1]
  _, tr = _dqn(mods, 2, 64)
  rp = qnet_train.VecPrioritizedReplayBuffer(4, 16)
  with pytest.raises(ValueError, match='uniformly'):
    tr.train_step(rp, 8)
  with pytest.raises(ValueError, match='uniformly'):
    tr.capture(rp, 8)


def _episode_inputs(observations, n, steps, seed):
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(steps + 1):
    i = torch.from_numpy(rng.integers(0, len(observations), n)).cuda()
    out.append((torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda(), observations[i].clone(),
                torch.from_numpy((rng.random(n) < 0.1).astype(np.uint8)).cuda()))
  return out


def _drive(ag, inputs, first, count):
  for reward, obs, end in inputs[first:first + count]:
    ag.step(reward, obs, end)


def test_mlp_determinism_graph_and_resume(mods, observations):
  n, steps = 48, 50
  inputs = _episode_inputs(observations, n, steps, seed=1)
  runs = []
  for graph in (False, True, False):
    _, ag = _mlp(mods, n, 2, 64, learning_rate=1e-3)
    ag.begin_episode(inputs[0][1])
    if graph:
      ag.capture()
    _drive(ag, inputs, 1, steps)
    ag.check_errors()
    runs.append((_bits(ag.weights), ag.last_action.cpu().numpy().copy()))
  assert np.array_equal(runs[0][0], runs[2][0]) and np.array_equal(runs[0][1], runs[2][1]), 'two agents differ'
  assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), 'graph replay differs from eager'
  params, _ = _mlp(mods, 1, 2, 64)
  assert not np.array_equal(runs[0][0], mods[0].QNetwork.from_params(params).packed_host.view(np.uint32))
  _, a = _mlp(mods, n, 2, 64, learning_rate=1e-3)
  a.begin_episode(inputs[0][1])
  _drive(a, inputs, 1, 25)
  sd = a.state_dict()
  _drive(a, inputs, 26, 25)
  _, c = _mlp(mods, n, 2, 64, learning_rate=0.5, gamma=0.1, seed=9)
  c.load_state_dict(sd)
  _drive(c, inputs, 26, 25)
  assert np.array_equal(_bits(a.weights), _bits(c.weights)) and np.array_equal(_bits(a.weights), runs[0][0]), 'resume differs'


# ---------------------------------------------------------------------------------------------------------------------- VecMLPAgent
def test_mlp_acts_with_the_pre_update_parameters(mods, observations):
  qnet = mods[0]
  n = 64
  inputs = _episode_inputs(observations, n, 3, seed=2)
  _, ag = _mlp(mods, n, 2, 64, learning_rate=1e-2)
  before = qnet.VecQNetworkAgent(ag.network())
  assert np.array_equal(ag.begin_episode(inputs[0][1]).cpu().numpy(), before.act(inputs[0][1]).cpu().numpy())
  for reward, obs, end in inputs[1:]:
    before = qnet.VecQNetworkAgent(ag.network())          # the parameters before this step's update
    w0 = _bits(ag.weights)
    got = ag.step(reward, obs, end).cpu().numpy().copy()
    assert not np.array_equal(w0, _bits(ag.weights))
    assert np.array_equal(got, before.act(obs).cpu().numpy())
  ag.set_mode('eval')                                     # eval mode acts and leaves the weights' bits untouched
  w0 = _bits(ag.weights)
  before = qnet.VecQNetworkAgent(ag.network())
  for reward, obs, end in inputs[1:]:
    assert np.array_equal(ag.step(reward, obs, end).cpu().numpy(), before.act(obs).cpu().numpy())
  assert np.array_equal(w0, _bits(ag.weights))


def test_mlp_single_environment_is_the_reference_update(mods, observations):
  """N = 1 (the default one-layer network, gamma 0.9, lr 1e-3) over three steps against three sequential float64 twin updates of the
  reference's loss, the device's own actions given: the SGD bound, 4 ulp(w) + 1e-6 lr."""
  qnet, qnet_train, _, mlp_agent = mods
  lr, gamma = 1e-3, 0.9
  ag = mlp_agent.VecMLPAgent(1, gamma=gamma, learning_rate=lr, seed=4)
  assert (ag.num_layers, ag.hidden_units) == (1, 0)
  params = {'params': {k: {kk: vv.astype(np.float64) for kk, vv in v.items()} for k, v in ag.params()['params'].items()}}
  inputs = _episode_inputs(observations, 1, 3, seed=5)
  s = inputs[0][1].cpu().numpy().astype(np.float64)
  a = ag.begin_episode(inputs[0][1]).cpu().numpy().copy()
  for reward, obs, _ in inputs[1:]:
    a2 = ag.step(reward, obs).cpu().numpy().copy()
    s2 = obs.cpu().numpy().astype(np.float64)
    qs, qn = train_host.forward_all(params, s)[-1], train_host.forward_all(params, s2)[-1]
    _, _, ds, dn = td_host.sarsa_loss(qs, qn, reward.cpu().numpy(), a, a2, np.float64(np.float32(gamma)))
    grads = td_host.sarsa_backward(params, s, s2, ds, dn)
    leaf = params['params']['Dense_0']
    leaf['kernel'], leaf['bias'] = td_host.sgd(leaf['kernel'], grads[0][0], np.float64(np.float32(lr))), td_host.sgd(leaf['bias'], grads[0][1], np.float64(np.float32(lr)))
    s, a = s2, a2
  got = ag.params()['params']['Dense_0']
  worst = 0.0
  for name in ('kernel', 'bias'):
    w64 = params['params']['Dense_0'][name]
    bound = 4 * np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64) + 1e-6 * lr
    worst = max(worst, float((np.abs(got[name] - w64) / bound).max()))
  print('worst |w - w64| / bound after three updates', worst)
  assert worst <= 1.0, worst
  first = qnet.init_params('mlp', 4, num_layers=1)['params']['Dense_0']['kernel']
  assert not np.array_equal(got['kernel'], first)


def test_mlp_masked_rows_observations_do_not_matter(mods, observations):
  n = 32
  grads = []
  for variant in range(2):
    _, ag = _mlp(mods, n, 2, 64)
    t = _transitions(ag, observations, seed=6)
    masked = np.flatnonzero(t['mask'])
    assert len(masked) >= 2
    if variant:
      other = observations[500:500 + len(masked)].clone()
      ag.last_obs[torch.from_numpy(masked).cuda(), :1099] = other
      ag.obs[torch.from_numpy(masked).cuda(), :1099] = other.flip(0)
    ag.train_on_transitions(apply_update=False)
    grads.append(_bits(ag.grad))
  assert np.array_equal(grads[0], grads[1]) and grads[0].any()


def test_reference_shaped_agents(mods, observations):
  qnet, _, dqn_agent, mlp_agent = mods
  from balloon_learning_environment_amd.agents import agent_registry
  x = observations.cpu().numpy()
  params = _params(qnet, 2, 64)
  ag = agent_registry.agent_constructor('dqn')(3, [1099], params=params)
  want = qnet.VecQNetworkAgent(qnet.QNetwork.from_params(params)).act(observations[:4]).cpu().numpy()
  assert [ag.begin_episode(x[0])] + [ag.step(0.0, x[i]) for i in (1, 2, 3)] == list(want)
  with pytest.raises(NotImplementedError):
    ag.set_mode('train')
  with pytest.raises(ValueError):
    dqn_agent.DQNAgent(3, [1099], params=qnet.init_params('quantile', 0, 2, 8, 5))
  m = agent_registry.agent_constructor('mlp')(3, [1099], seed=1)
  w0 = _bits(m._vec.weights)
  acts = [m.begin_episode(x[0]), m.step(0.5, x[1]), m.step(-0.5, x[2])]
  m.end_episode(0.0, True)
  assert all(a in (0, 1, 2) for a in acts) and not np.array_equal(w0, _bits(m._vec.weights))      # mode 'train' from construction
  m.set_mode('eval')
  w1 = _bits(m._vec.weights)
  m.step(0.5, x[3])
  assert np.array_equal(w1, _bits(m._vec.weights))


# ---------------------------------------------------------------------------------------------------------------------------- learns
def _bandit(observations):
  x = observations.cpu().numpy()
  std = np.where((x.min(axis=0) >= 0) & (x.max(axis=0) <= 1), x.std(axis=0), 0.0)
  col = int(np.argmax(std))
  label = np.where(x[:, col] > np.median(x[:, col]), 2, 0).astype(np.uint8)
  rng = np.random.default_rng(0)
  perm = rng.permutation(len(x))
  return x, label, rng, perm[:768], perm[768:]


def _score(qnet, network, x, label, test_i):
  agent = qnet.VecQNetworkAgent(network)
  q = torch.empty(len(test_i), 3, dtype=torch.float32, device='cuda')
  act = agent.act(torch.from_numpy(x[test_i]).cuda(), q_values=q).cpu().numpy()
  r = (np.arange(3)[None, :] == label[test_i][:, None]).astype(np.float64)
  return float((act == label[test_i]).mean()), float(np.abs(q.cpu().numpy() - r).mean())


DQN_BANDIT_UPDATES = 600
MLP_BANDIT_UPDATES, MLP_BANDIT_LR = 600, 1e-3


@pytest.mark.parametrize('kind', ['mse', 'huber'])
def test_dqn_learns_a_contextual_bandit(mods, observations, kind):
  """test_gpu_train.py's task and bars (>= 90 % held-out accuracy, mean |q - r| <= 0.2) with DQNTrainer on a (2, 64) one-atom network:
  DQN_BANDIT_UPDATES = 600 updates of 128 rows, Adam 1e-3, as the QR-DQN test."""
  qnet, qnet_train = mods[0], mods[1]
  x, label, rng, train_i, test_i = _bandit(observations)
  n_env, steps = 64, 48
  rp = qnet_train.VecReplayBuffer(n_env, steps, update_horizon=1, gamma=0.99)
  for s in range(steps):
    i = rng.choice(train_i, n_env)
    a = rng.integers(0, 3, n_env).astype(np.uint8)
    r = (a == label[i]).astype(np.float32)
    rp.add(torch.from_numpy(x[i]).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(r).cuda(), torch.ones(n_env, dtype=torch.uint8, device='cuda'))
  tr = mods[2].DQNTrainer(qnet.QNetwork.from_params(_params(qnet, 2, 64, bias=0.0)), loss_type=kind, lr=1e-3, update_horizon=1, seed=5)
  for _ in range(DQN_BANDIT_UPDATES):
    tr.train_step(rp, 128)
  tr.check_errors()
  rp.check_errors()
  acc, err = _score(qnet, tr.network(), x, label, test_i)
  print(kind, 'accuracy', acc, 'mean |q - r|', err)
  assert acc >= 0.9, acc
  assert err <= 0.2, err


def test_mlp_learns_a_contextual_bandit(mods, observations):
  """The same task and bars with VecMLPAgent's SARSA update at gamma = 0, where the loss's fixed point is q(s)[a] = r: a (2, 64)
  network, MLP_BANDIT_UPDATES updates of 128 uniformly random (state, action, reward) rows each with plain SGD at MLP_BANDIT_LR.  The
  transitions are written into the agent's buffers (the actions are random: a greedy learner would not explore this bandit)."""
  qnet = mods[0]
  x, label, rng, train_i, test_i = _bandit(observations)
  n = 128
  ag = mods[3].VecMLPAgent(n, qnet.QNetwork.from_params(_params(qnet, 2, 64, bias=0.0)), gamma=0.0, learning_rate=MLP_BANDIT_LR)
  xs = torch.from_numpy(x).cuda()
  ag.mask.zero_()
  for _ in range(MLP_BANDIT_UPDATES):
    i = rng.choice(train_i, n)
    a = rng.integers(0, 3, n).astype(np.uint8)
    ag.last_obs[:, :1099].copy_(xs[torch.from_numpy(i).cuda()])
    ag.last_action.copy_(torch.from_numpy(a))
    ag.reward.copy_(torch.from_numpy((a == label[i]).astype(np.float32)))
    ag.train_on_transitions()
  ag.check_errors()
  acc, err = _score(qnet, ag.network(), x, label, test_i)
  print('sarsa accuracy', acc, 'mean |q - r|', err)
  assert acc >= 0.9, acc
  assert err <= 0.2, err


# ------------------------------------------------------------------------------------------------------------------------ end to end
def test_dqn_training_loop_end_to_end(mods):
  qnet, qnet_train = mods[0], mods[1]
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.env import balloon_env
  env = balloon_env.VecBalloonEnv(64, seed=1)
  params = _params(qnet, 2, 64)
  tr = mods[2].DQNTrainer(qnet.QNetwork.from_params(params), lr=1e-4, seed=2)
  rp = qnet_train.VecReplayBuffer(64, 32, update_horizon=5, gamma=0.993)
  stats = train_lib.run_training_loop_vec(env, tr, rp, num_iterations=2, steps_per_iteration=8, max_episode_length=7,
                                          min_replay_history=64 * 6, updates_per_step=4, epsilon=0.1, seed=3)
  assert len(stats) == 2 and stats[1]['updates'] > 0 and all(np.isfinite(s['mean_loss']) for s in stats)
  assert int(tr.err_flags.item()) == 0 and int(rp.err_flags.item()) == 0
  assert not np.array_equal(tr.weights.cpu().numpy(), qnet.QNetwork.from_params(params).packed_host)


def test_online_loop_end_to_end(mods):
  qnet = mods[0]
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.env import balloon_env
  finals = []
  for _ in range(2):
    env = balloon_env.VecBalloonEnv(64, seed=1)
    params, ag = _mlp(mods, 64, 2, 64, learning_rate=1e-4)
    stats = train_lib.run_online_loop_vec(env, ag, num_iterations=2, steps_per_iteration=8, max_episode_length=7)
    assert len(stats) == 2 and stats[0]['updates'] == 8 and stats[1]['updates'] == 8
    assert all(np.isfinite(s['mean_loss']) and s['mean_loss'] > 0 for s in stats)
    assert stats[0]['episodes'] >= 64 and stats[1]['transitions'] == 2 * 8 * 64 and 0.0 <= stats[1]['time_within_radius'] <= 1.0
    assert int(ag.err_flags.item()) == 0
    w = ag.weights.cpu().numpy()
    assert not np.array_equal(w, qnet.QNetwork.from_params(params).packed_host)
    finals.append(w.copy())
  assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))
