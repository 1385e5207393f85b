"""Imitation on the device (csrc/ble_imitate.h, agents/imitation.py, train_lib.run_dagger_loop_vec) against its
restatement (imitation_host.py) and the float64 twins of the backward pass (train_host.py), with test_gpu_td.py's tolerances:

 * the loss head: loss, aux and dL/dlogits against the twin on the device's own float32 logits, agree exactly; without a value term and
   with ret NULL, over a NaN-filled workspace, the columns no gradient belongs to are exactly zero; a label of 3;
 * rows labelled with act_greedy's own actions: the training forward's log-probability is the acting forward's, bit for bit, agree 1;
 * the gradient image against float64 backprop at B = 32 and B = 4 097 on (3, 256);
 * the mixture against the twin on the DAGGER stream's words at the 256-lane block's edges, beta 0 and 1, a shard, action aliasing
   learner, the counter -- inside a captured graph too;
 * determinism: graph replay against eager over 5 updates, a state_dict restored mid-run;
 * the replay-ring route: a batch a VecReplayBuffer of update_horizon 1 sampled;
 * one iteration of run_dagger_loop_vec through a recording environment with a StationSeeker expert;
 * it learns a fixed teacher's greedy policy, next to a float64 torch-autograd twin under three minibatch orders.
"""
import numpy as np
import pytest
import torch

import imitation_host
import ppo_host
import train_host

pytestmark = pytest.mark.gpu

POLICY = [0, 2, 4]
SHAPES = [(2, 64), (1, 0)]
WIDE = [(3, 256), (8, 600)]


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import actor_critic, imitation, qnet, qnet_train
  return qnet, qnet_train, actor_critic, imitation


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
  return ppo_host.build_actor_draws(tmp_path_factory.mktemp('dgd'))


def _params(qnet, layers, hidden, seed=7, bias=1e-2):
  """QuantileNetwork-scale kernels with two atoms and small random biases: policies far from uniform."""
  params = qnet.init_params('quantile', seed, layers, hidden, 2)
  rng = np.random.default_rng(seed + 1)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * bias).astype(np.float32)
  return params


def _trainer(mods, layers, hidden, **kw):
  qnet, _, _, im = mods
  params = _params(qnet, layers, hidden)
  return params, im.BCTrainer(qnet.QNetwork.from_params(params, num_atoms=2), **kw)


def _close(got, want, name):
  scale = np.abs(want).max()
  assert np.allclose(got, want, rtol=2e-6, atol=1e-7 * scale), (name, np.abs(got - want).max(), scale)


def _ratio(got, want):
  """|got - want| as a fraction of _close's bound."""
  return float((np.abs(got - want) / (2e-6 * np.abs(want) + 1e-7 * np.abs(want).max() + 1e-300)).max())


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def _batch(ac, x, label, ret=None):
  n = len(label)
  return ac.PPOBatch.from_tensors(x, np.zeros(n) if ret is None else ret, label, np.zeros(n), np.zeros(n), 'cuda')


def _views(tr, b):
  return {k: t.cpu().numpy() for k, t in tr.views(b).items() if k != 'acts'}


# ------------------------------------------------------------------------------------------------------------------------- loss head
@pytest.mark.parametrize('b,layers,hidden', [(b, l, h) for l, h in SHAPES for b in (1, 32, 300)] + [(32, l, h) for l, h in WIDE])
def test_loss_aux_and_dlogits(mods, observations, layers, hidden, b):
  """Measured on an MI355X over all eight shapes and the three (s, c_v) pairs (one run), the worst |device - twin| as a fraction of
  _close's bound: loss 0.097 ((1, 0), B = 32), aux[:, 0] 0.096 ((1, 0), B = 300), dlogits 0.076 ((2, 64), B = 300).
  test_gpu_td.py's bounds stand unwidened."""
  ac = mods[2]
  _, tr = _trainer(mods, layers, hidden)
  rng = np.random.default_rng(b)
  x = observations.cpu().numpy()[rng.integers(0, len(observations), b)]
  label = rng.integers(0, 3, b).astype(np.uint8)
  ret = rng.standard_normal(b).astype(np.float32)
  bt = _batch(ac, x, label, ret)
  for s, cv in ((0.0, 0.0), (0.1, 0.5), (0.0, 0.5)):
    tr.label_smoothing, tr.value_coef = s, cv
    tr.workspace(b)
    tr.views(b)['dlogits'].fill_(float('nan'))                          # every column up to ld is written by the call
    loss_d = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
    tr.check_errors()
    v = _views(tr, b)
    loss, aux, dlog = imitation_host.bc_loss(v['logits'], label, ret, s, cv)
    print('B', b, (layers, hidden), 's', s, 'c_v', cv, 'err / bound: loss', _ratio(loss_d, loss), 'lp_act', _ratio(v['aux'][:, 0], aux[:, 0]),
          'dlogits', _ratio(v['dlogits'][:, :6], dlog))
    _close(loss_d, loss, 'loss')
    _close(v['aux'][:, 0], aux[:, 0], 'lp_act')
    _close(v['dlogits'][:, :6], dlog, 'dlogits')
    assert np.array_equal(v['aux'][:, 1], aux[:, 1].astype(np.float32)), 'agree'
    assert np.array_equal(v['aux'][:, 1], (ppo_host.greedy(v['logits']) == label).astype(np.float32))
    assert not v['dlogits'][:, [3, 5]].any() and not v['dlogits'][:, 6:].any()
    assert v['dlogits'].shape[1] >= max(hidden, 6) and not np.isnan(v['dlogits']).any()      # (the whole [B, ld] view)
    if cv == 0.0:
      assert not v['dlogits'][:, 1].any()
      lp, _ = ppo_host.log_softmax(v['logits'][:, POLICY])
      _close(loss_d, -lp[np.arange(b), label], 'L = CE = -lp[label] at s = 0')
    else:
      assert v['dlogits'][:, 1].all()


@pytest.mark.parametrize('b,layers,hidden', [(1, 2, 64), (300, 2, 64), (32, 1, 0), (32, 3, 256)])
def test_no_value_term_reads_no_ret(mods, observations, layers, hidden, b):
  """c_v = 0 with batch->ret NULL, the whole workspace NaN before the call: the loss is the twin's, and dlogits columns 1, 3, 5 and
  6..ld are exactly zero."""
  ac = mods[2]
  _, tr = _trainer(mods, layers, hidden, label_smoothing=0.1)
  rng = np.random.default_rng(b + 1)
  x = observations.cpu().numpy()[rng.integers(0, len(observations), b)]
  label = rng.integers(0, 3, b).astype(np.uint8)
  bt = _batch(ac, x, label)
  bt.struct.ret = None
  ws, _, _ = tr.workspace(b)
  ws.fill_(float('nan'))
  loss_d = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  tr.check_errors()
  v = _views(tr, b)
  loss, aux, dlog = imitation_host.bc_loss(v['logits'], label, None, 0.1, 0.0)
  _close(loss_d, loss, 'loss')
  _close(v['dlogits'][:, :6], dlog, 'dlogits')
  d = v['dlogits']
  assert _bits(d[:, [1, 3, 5]]).max() == 0 and _bits(d[:, 6:]).max(initial=0) == 0       # +0.0, not -0.0 and not NaN
  assert d[:, POLICY].all() and np.isfinite(tr.grad.cpu().numpy()).all()
  got = mods[1].unpack(tr._net, tr.grad.cpu().numpy())['params'][f'Dense_{layers - 1}']
  assert not got['kernel'][:, [1, 3, 5]].any() and not got['bias'][[1, 3, 5]].any()      # the value column is not trained


def test_label_out_of_range_flags_and_zeroes_its_row_only(mods, observations):
  ac = mods[2]
  _, tr = _trainer(mods, 2, 64, label_smoothing=0.1, value_coef=0.5)
  rng = np.random.default_rng(2)
  x = observations.cpu().numpy()[:8]
  label = rng.integers(0, 3, 8).astype(np.uint8)
  ret = rng.standard_normal(8).astype(np.float32)
  tr.train_on_batch(_batch(ac, x, label, ret), apply_update=False)
  tr.check_errors()
  clean = _views(tr, 8)
  clean_loss = clean['loss'].copy()
  bad = label.copy()
  bad[2], bad[5] = 3, 200
  loss = tr.train_on_batch(_batch(ac, x, bad, ret), apply_update=False).cpu().numpy()
  v = _views(tr, 8)
  assert loss[2] == 0 and loss[5] == 0 and not v['dlogits'][[2, 5]].any() and not v['aux'][[2, 5]].any()
  keep = [0, 1, 3, 4, 6, 7]
  assert np.array_equal(_bits(loss[keep]), _bits(clean_loss[keep])) and np.array_equal(_bits(v['dlogits'][keep]), _bits(clean['dlogits'][keep]))
  assert np.array_equal(_bits(v['aux'][keep]), _bits(clean['aux'][keep])) and loss[keep].all()
  with pytest.raises(ValueError):
    tr.check_errors()
  tr.check_errors()                                                   # (the flag is cleared once raised)


# ------------------------------------------------------------------------------------------------------------- same bits as acting
@pytest.mark.parametrize('n,layers,hidden', [(n, l, h) for l, h in ((2, 64), (3, 256)) for n in (1, 129, 300)])
def test_rows_labelled_by_the_greedy_head_agree_bit_for_bit(mods, observations, layers, hidden, n):
  ac = mods[2]
  _, tr = _trainer(mods, layers, hidden)
  obs = observations[200:200 + n]
  act = torch.full((n,), 9, dtype=torch.uint8, device='cuda')
  logp, value = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
  tr.act_greedy(obs, act, logp, value)
  assert int(tr.act_step.item()) == 0
  tr.train_on_batch(_batch(ac, obs.cpu().numpy(), act.cpu().numpy()), apply_update=False)
  v = _views(tr, n)
  assert np.array_equal(_bits(v['aux'][:, 0]), _bits(logp.cpu().numpy()))
  assert np.array_equal(v['aux'][:, 1], np.ones(n, np.float32))
  assert np.array_equal(_bits(v['logits'][:, 1]), _bits(value.cpu().numpy()))
  assert np.array_equal(_bits(v['loss']), _bits(-logp.cpu().numpy()))  # s = 0, c_v = 0: L = -lp[label]


# -------------------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize('b', [32, 4097])
def test_gradient_against_float64_backprop(mods, observations, b):
  """Measured on an MI355X at (3, 256), the worst |g - g64| / (1e-5 S): 0.013 at B = 32, 0.0098 at B = 4 097."""
  qnet, qnet_train, ac, _ = mods
  layers, hidden = 3, 256
  params, tr = _trainer(mods, layers, hidden, label_smoothing=0.1, value_coef=0.5)
  rng = np.random.default_rng(4)
  x = observations.cpu().numpy()[rng.integers(0, len(observations), b)]
  bt = _batch(ac, x, rng.integers(0, 3, b).astype(np.uint8), rng.standard_normal(b).astype(np.float32))
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
  assert not last['kernel'][:, [3, 5]].any() and not last['bias'][[3, 5]].any()
  assert np.array_equal(_bits(qnet.QNetwork.from_params({'params': got}, num_atoms=2).packed_host), _bits(g))
  assert np.array_equal(_bits(tr.weights.cpu().numpy()), _bits(qnet.QNetwork.from_params(params, num_atoms=2).packed_host))      # nothing applied


# ------------------------------------------------------------------------------------------------------------------------------- mix
def _pair(n, seed):
  rng = np.random.default_rng(seed)
  return rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 3, n).astype(np.uint8)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1025])
def test_mix_against_twin(mods, draws, n):
  _, tr = _trainer(mods, 1, 0, seed=11)
  learner, expert = _pair(n, n)
  ld, ed = torch.from_numpy(learner).cuda(), torch.from_numpy(expert).cuda()
  out = torch.full((n,), 9, dtype=torch.uint8, device='cuda')
  took = torch.full((n,), 9, dtype=torch.uint8, device='cuda')
  for step, beta in enumerate((0.37, 0.0, 1.0, 0.9)):
    assert int(tr.mix_step.item()) == step
    got = tr.mix(ld, ed, beta, out, took)
    assert got is out
    want, want_took = imitation_host.mix(learner, expert, beta, imitation_host.dagger_words(draws, 11, 0, n, step))
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(took.cpu().numpy(), want_took), (step, beta)
    if beta == 0.0:
      assert np.array_equal(want, learner) and not want_took.any()
    if beta == 1.0:
      assert np.array_equal(want, expert) and want_took.all()
  assert torch.equal(ld.cpu(), torch.from_numpy(learner)) and torch.equal(ed.cpu(), torch.from_numpy(expert))      # the inputs stay
  # without took_expert, into a fresh tensor
  fresh = tr.mix(ld, ed, 0.5)
  assert np.array_equal(fresh.cpu().numpy(), imitation_host.mix(learner, expert, 0.5, imitation_host.dagger_words(draws, 11, 0, n, 4))[0])
  # action aliasing learner
  alias = ld.clone()
  tr.mix(alias, ed, 0.5, alias)
  assert np.array_equal(alias.cpu().numpy(), imitation_host.mix(learner, expert, 0.5, imitation_host.dagger_words(draws, 11, 0, n, 5))[0])
  assert int(tr.mix_step.item()) == 6 and int(tr.act_step.item()) == 0


def test_mix_shard_counter_and_graph(mods, draws):
  _, tr = _trainer(mods, 1, 0, seed=5)
  n = 500
  learner, expert = _pair(n, 1)
  ld, ed = torch.from_numpy(learner).cuda(), torch.from_numpy(expert).cuda()
  whole, took = torch.zeros(n, dtype=torch.uint8, device='cuda'), torch.zeros(n, dtype=torch.uint8, device='cuda')
  tr.mix_step.fill_(2 ** 32 + 7)                                      # the step's high word is part of the key
  tr.mix(ld, ed, 0.5, whole, took)
  want, want_took = imitation_host.mix(learner, expert, 0.5, imitation_host.dagger_words(draws, 5, 0, n, 2 ** 32 + 7))
  assert np.array_equal(whole.cpu().numpy(), want) and np.array_equal(took.cpu().numpy(), want_took)
  assert 0 < int(want_took.sum()) < n
  low, _ = imitation_host.mix(learner, expert, 0.5, imitation_host.dagger_words(draws, 5, 0, n, 7))
  assert not np.array_equal(low, want)
  # a shard with env_offset = 300, n = 200 is rows 300..499 of the whole
  tr.mix_step.fill_(2 ** 32 + 7)
  part, part_took = torch.zeros(200, dtype=torch.uint8, device='cuda'), torch.zeros(200, dtype=torch.uint8, device='cuda')
  tr.mix(ld[300:].contiguous(), ed[300:].contiguous(), 0.5, part, part_took, env_offset=300)
  assert torch.equal(part, whole[300:]) and torch.equal(part_took, took[300:])
  assert int(tr.mix_step.item()) == 2 ** 32 + 8
  # an empty mix launches nothing and leaves the counter
  empty = torch.zeros(0, dtype=torch.uint8, device='cuda')
  tr.mix(empty, empty, 0.5, empty)
  assert int(tr.mix_step.item()) == 2 ** 32 + 8
  with pytest.raises(ValueError):
    tr.mix(ld, ed, 1.5, whole)
  # inside a captured graph the counter advances by one per replay, and each replay draws its own step
  from balloon_learning_environment_amd import device as dev
  tr.mix_step.fill_(0)
  graph, out = dev.capture(tr.device, lambda: tr.mix(ld, ed, 0.5, whole, took))
  assert out is whole and int(tr.mix_step.item()) == 0                # (recording runs nothing)
  for step in range(3):
    graph.replay()
    assert int(tr.mix_step.item()) == step + 1
    want, want_took = imitation_host.mix(learner, expert, 0.5, imitation_host.dagger_words(draws, 5, 0, n, step))
    assert np.array_equal(whole.cpu().numpy(), want) and np.array_equal(took.cpu().numpy(), want_took), step


# ----------------------------------------------------------------------------------------------------------------------- determinism
def _fixed_batches(mods, observations, count, b=128):
  ac = mods[2]
  rng = np.random.default_rng(8)
  x = observations.cpu().numpy()
  out = []
  for _ in range(count):
    i = rng.integers(0, len(x), b)
    out.append((x[i], rng.integers(0, 3, b).astype(np.uint8), rng.standard_normal(b).astype(np.float32)))
  return out


def _fill(bt, rows):
  x, label, ret = rows
  bt.state[:, :1099].copy_(torch.from_numpy(x))
  bt.action.copy_(torch.from_numpy(label))
  bt.ret.copy_(torch.from_numpy(ret))


def _student(mods, seed=2, **kw):
  qnet, _, ac, im = mods
  return im.BCTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', seed, 2, 64), num_atoms=2), lr=1e-3, label_smoothing=0.1,
                      value_coef=0.5, **kw)


def test_graph_replay_equals_eager_and_resume(mods, observations):
  ac = mods[2]
  data = _fixed_batches(mods, observations, 5)
  eager, graph = _student(mods), _student(mods)
  bt_e, bt_g = ac.PPOBatch(128, 'cuda'), ac.PPOBatch(128, 'cuda')
  first = eager.weights.cpu().numpy().copy()
  losses = []
  sd = None
  for k, rows in enumerate(data):
    _fill(bt_e, rows)
    eager.train_on_batch(bt_e)
    _fill(bt_g, rows)
    loss = graph.capture(bt_g) if k == 0 else graph.train_step(bt_g)
    losses.append(loss.cpu().numpy().copy())
    assert np.array_equal(_bits(loss.cpu().numpy()), _bits(eager.views(128)['loss'].cpu().numpy())), k
    if k == 1:
      eager.mix_step.fill_(3)
      eager.act_step.fill_(4)
      sd = eager.state_dict()
  assert 128 in graph._graphs and graph._graphs[128][1] is bt_g
  we = eager.weights.cpu().numpy()
  assert int(eager.adam_step.item()) == 5 and int(graph.adam_step.item()) == 5
  assert np.array_equal(_bits(we), _bits(graph.weights.cpu().numpy())), 'graph replay differs from eager'
  assert not np.array_equal(we, first) and not np.array_equal(losses[0], losses[4])
  eager.check_errors()
  graph.check_errors()
  # a state_dict taken after two updates resumes to the same bits; a changed hyperparameter drops the captured graphs
  other = _student(mods, seed=9)
  other.lr = 5e-4
  bt_o = ac.PPOBatch(128, 'cuda')
  _fill(bt_o, data[0])
  other.capture(bt_o)
  assert other._graphs
  other.load_state_dict(sd)
  assert not other._graphs and other.lr == 1e-3 and (other.label_smoothing, other.value_coef) == (0.1, 0.5)
  assert int(other.mix_step.item()) == 3 and int(other.act_step.item()) == 4 and int(other.adam_step.item()) == 2
  for rows in data[2:]:
    _fill(bt_o, rows)
    other.train_step(bt_o)
  assert np.array_equal(_bits(we), _bits(other.weights.cpu().numpy())), 'resume differs'
  same = _student(mods)
  same.capture(bt_o)
  same.load_state_dict(sd)
  assert same._graphs                                                 # (the same seed and hyperparameters: the graphs stay valid)


# ------------------------------------------------------------------------------------------------------------------ replay-ring route
def test_replay_ring_batch_trains_as_labelled(mods, observations):
  """A VecReplayBuffer(64, 16, update_horizon=1) filled with expert labels: obs[:, 0] carries a row id, the label is id % 3.  The
  sampled TrainBatch trains as the loss head says on its state and action."""
  _, qnet_train, ac, _ = mods
  _, tr = _trainer(mods, 2, 64, label_smoothing=0.1)
  replay = qnet_train.VecReplayBuffer(64, 16, update_horizon=1)
  zeros_f, zeros_u = torch.zeros(64, device='cuda'), torch.zeros(64, dtype=torch.uint8, device='cuda')
  for t in range(8):
    obs = observations[64 * t:64 * t + 64].clone()
    ids = torch.arange(64 * t, 64 * t + 64, device='cuda')
    obs[:, 0] = ids / 1024.0
    replay.add(obs, (ids % 3).to(torch.uint8), zeros_f + t, zeros_u)
  bt = replay.sample(32, seed=3)
  replay.check_errors()
  assert isinstance(bt, qnet_train.TrainBatch) and not isinstance(bt, ac.PPOBatch)
  ids = np.rint(bt.state[:, 0].cpu().numpy().astype(np.float64) * 1024.0).astype(np.int64)
  label = bt.action.cpu().numpy()
  assert np.array_equal(label, (ids % 3).astype(np.uint8)) and len(set(ids.tolist())) > 16
  want_x = observations[torch.from_numpy(ids).cuda()].clone()
  want_x[:, 0] = torch.from_numpy(ids).cuda() / 1024.0
  assert torch.equal(bt.state[:, :1099], want_x)
  loss_d = tr.train_on_batch(bt, apply_update=False).cpu().numpy()
  tr.check_errors()
  v = _views(tr, 32)
  loss, aux, dlog = imitation_host.bc_loss(v['logits'], label, None, 0.1, 0.0)
  _close(loss_d, loss, 'loss')
  _close(v['aux'][:, 0], aux[:, 0], 'lp_act')
  _close(v['dlogits'][:, :6], dlog, 'dlogits')
  assert np.array_equal(v['aux'][:, 1], aux[:, 1].astype(np.float32))
  # the same rows through a PPOBatch: the same bits
  pb = _batch(ac, bt.state[:, :1099].cpu().numpy(), label)
  loss_p = tr.train_on_batch(pb, apply_update=False).cpu().numpy()
  assert np.array_equal(_bits(loss_p), _bits(loss_d)) and np.array_equal(_bits(_views(tr, 32)['dlogits']), _bits(v['dlogits']))
  # its ret is a reward, not a value target
  tr.value_coef = 0.5
  with pytest.raises(ValueError):
    tr.train_on_batch(bt, apply_update=False)
  tr.train_on_batch(pb, apply_update=False)
  tr.check_errors()


# -------------------------------------------------------------------------------------------------------------- the loop on the device
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


LOOP_T, LOOP_N, LOOP_LIMIT, LOOP_SEED, LOOP_BETA = 8, 64, 5, 4, 0.5


def test_loop_block_is_what_happened(mods, draws):
  """One iteration of run_dagger_loop_vec through a recording environment with a StationSeeker expert, against a second trainer of the
  same parameters and seed and a second StationSeeker: the stored action is the expert's on obs[t], the stepped action the twin's mix
  of (learner, label) at mix step t, ret is gae_f32 of the block, the stats count what happened."""
  qnet, _, ac, im = mods
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.agents import station_seeker_agent
  from balloon_learning_environment_amd.env import balloon_env
  env = _RecordingEnv(balloon_env.VecBalloonEnv(LOOP_N, seed=1))

  def make():
    return im.BCTrainer(qnet.QNetwork.from_params(ac.init_params('actor_critic', 2, 2, 64), num_atoms=2), lr=1e-3, seed=LOOP_SEED,
                        value_coef=0.5)
  tr, twin = make(), make()
  ro = ac.VecRolloutBuffer(LOOP_N, LOOP_T, 'cuda')
  stats = train_lib.run_dagger_loop_vec(env, tr, station_seeker_agent.VecStationSeekerAgent(), ro, num_iterations=1, beta=LOOP_BETA,
                                        epochs=2, batch_size=128, max_episode_length=LOOP_LIMIT, gamma=0.9, lam=0.8, capture_graph=False)
  n = LOOP_N
  assert len(env.steps) == LOOP_T and len(stats) == 1
  seeker = station_seeker_agent.VecStationSeekerAgent()
  blk = {k: getattr(ro, k).cpu().numpy() for k in ('action', 'logp', 'value', 'reward', 'terminal', 'episode_end', 'boot_value', 'advantage', 'ret')}
  ep_steps = np.zeros(n, np.int64)
  took_total, differs = 0, 0
  for t in range(LOOP_T):
    rec = env.steps[t]
    seen = env.reset_obs if t == 0 else env.steps[t - 1]['obs']
    assert torch.equal(ro.obs[t, :, :1099].view(torch.int32), seen.view(torch.int32)), (t, 'obs[t] is not the observation acted on')
    label = seeker.act(seen).cpu().numpy()
    assert np.array_equal(blk['action'][t], label), (t, 'the stored action is not the expert on obs[t]')
    twin.act_step.fill_(t)
    learner = torch.zeros(n, dtype=torch.uint8, device='cuda')
    logp, value = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    twin.act(seen, learner, logp, value)
    want, took = imitation_host.mix(learner.cpu().numpy(), label, LOOP_BETA, imitation_host.dagger_words(draws, LOOP_SEED, 0, n, t))
    assert np.array_equal(rec['actions'].cpu().numpy(), want), (t, 'the stepped action is not the mix')
    took_total += int(took.sum())
    differs += int((want != label).sum())
    assert np.array_equal(_bits(blk['logp'][t]), _bits(logp.cpu().numpy())) and np.array_equal(_bits(blk['value'][t]), _bits(value.cpu().numpy()))
    assert np.array_equal(_bits(blk['reward'][t]), _bits(rec['reward'].cpu().numpy()))
    terminal, end_mask = rec['terminal'].cpu().numpy(), rec['end_mask'].cpu().numpy()
    assert np.array_equal(end_mask, (ep_steps + 1 >= LOOP_LIMIT).astype(np.uint8)), t
    assert np.array_equal(blk['terminal'][t], terminal) and np.array_equal(blk['episode_end'][t], terminal | end_mask), t
    ep_steps = np.where((terminal | end_mask) != 0, 0, ep_steps + 1)
  seeker.check_errors()
  assert differs > 0, 'the block cannot tell the label from the action flown'
  assert int(tr.act_step.item()) == LOOP_T + 1 and int(tr.mix_step.item()) == LOOP_T
  twin.act_step.fill_(LOOP_T)
  boot = torch.zeros(n, device='cuda')
  twin.act(env.steps[-1]['obs'], None, None, boot)
  assert np.array_equal(_bits(blk['boot_value']), _bits(boot.cpu().numpy()))
  adv, ret = ppo_host.gae_f32(blk['reward'], blk['value'], blk['boot_value'], blk['terminal'], blk['episode_end'], 0.9, 0.8)
  assert np.array_equal(_bits(blk['ret']), _bits(ret)) and np.array_equal(_bits(blk['advantage']), _bits(adv))
  s = stats[0]
  assert s['updates'] == 2 * (LOOP_T * n // 128) and int(tr.adam_step.item()) == s['updates'] and np.isfinite(s['mean_loss'])
  assert s['transitions'] == LOOP_T * n and s['episodes'] == int(blk['episode_end'].astype(bool).sum())
  assert s['expert_share'] == took_total / (LOOP_T * n) and 0.3 < s['expert_share'] < 0.7
  assert 0.0 <= s['agreement'] <= 1.0
  print('loop: expert_share', s['expert_share'], 'agreement', s['agreement'], 'mean_loss', s['mean_loss'], 'flown != label', differs)


# ---------------------------------------------------------------------------------------------------------------------------- learns
LEARN_UPDATES, LEARN_B, LEARN_LR = 300, 128, 1e-3
TEACHER_SEED = 30      # chosen by its labels alone: of seeds 21..44 the one whose greedy policy takes all three actions often (385 | 217 | 422)


def _twin_run(params, x, label, order, x_test, label_test):
  """float64 torch autograd of mean CE on the (2, 64) student with optax's Adam (eps 1e-5) over the minibatches `order`
  [updates, B]: (held-out CE before, after, held-out agreement after)."""
  layers = [(torch.tensor(params['params'][f'Dense_{i}']['kernel'], dtype=torch.float64, requires_grad=True),
             torch.tensor(params['params'][f'Dense_{i}']['bias'], dtype=torch.float64, requires_grad=True)) for i in range(2)]
  leaves = [t for pair in layers for t in pair]
  m, v = [torch.zeros_like(t) for t in leaves], [torch.zeros_like(t) for t in leaves]
  xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(label.astype(np.int64))

  def logits(inp):
    h = torch.relu(inp @ layers[0][0] + layers[0][1])
    return (h @ layers[1][0] + layers[1][1])[:, POLICY]

  def held_out():
    with torch.no_grad():
      z = logits(torch.tensor(x_test, dtype=torch.float64))
      ce = torch.nn.functional.cross_entropy(z, torch.tensor(label_test.astype(np.int64)))
      z6 = np.zeros((len(x_test), 6))
      z6[:, POLICY] = z.numpy()
      return float(ce), float((ppo_host.greedy(z6) == label_test).mean())
  before, _ = held_out()
  b1, b2, eps = 0.9, 0.999, 1e-5
  for t, idx in enumerate(order, start=1):
    loss = torch.nn.functional.cross_entropy(logits(xt[idx]), yt[idx])
    grads = torch.autograd.grad(loss, leaves)
    with torch.no_grad():
      for w, g, mi, vi in zip(leaves, grads, m, v):
        mi.mul_(b1).add_((1 - b1) * g)
        vi.mul_(b2).add_((1 - b2) * g * g)
        w.sub_(LEARN_LR * (mi / (1 - b1 ** t)) / (torch.sqrt(vi / (1 - b2 ** t)) + eps))
  after, agree = held_out()
  return before, after, agree


def test_learns_a_teacher_next_to_a_float64_twin(mods, observations):
  """A fixed (2, 64) teacher (QuantileNetwork-scale policy columns, its own seed) labels real observations with its greedy action; a
  (2, 64) student takes 300 updates of B = 128 (test_gpu_train.py's bandit order) on 768 of them.  A float64 torch-autograd twin gets
  the same data, initial parameters, Adam and minibatch order, and two further orders.  Held-out cross-entropy falls on the device and
  on the twin; the device's held-out agreement is at least the twin's minus the spread (max - min) of the twin's three runs.
  Measured on an MI355X (one run): held-out CE 1.0989 -> 0.4054 on the device, -> 0.4054 | 0.4207 | 0.4610 on the twin; agreement
  device 0.8125, twin 0.8125 | 0.8125 | 0.7852, spread 0.0273."""
  qnet, _, ac, im = mods
  x = observations.cpu().numpy()
  teacher = ac.VecActorCriticAgent(qnet.QNetwork.from_params(_params(qnet, 2, 64, seed=TEACHER_SEED), num_atoms=2))
  label = teacher.act(observations).cpu().numpy()
  counts = np.bincount(label, minlength=3)
  assert counts.min() >= len(label) // 10, counts                      # every action is a label often enough to be learnt and missed
  perm = np.random.default_rng(0).permutation(len(x))
  train_i, test_i = perm[:768], perm[768:]
  orders = [train_i[np.random.default_rng(100 + k).integers(0, len(train_i), (LEARN_UPDATES, LEARN_B))] for k in range(3)]
  params = ac.init_params('actor_critic', 7, 2, 64)
  tr = im.BCTrainer(qnet.QNetwork.from_params(params, num_atoms=2), lr=LEARN_LR)
  test_obs, test_label = observations[torch.from_numpy(test_i).cuda()], label[test_i]

  def held_out():
    probs = torch.zeros(len(test_i), 3, device='cuda')
    act = tr.act_greedy(test_obs, probs=probs).cpu().numpy()
    p = probs.cpu().numpy().astype(np.float64)
    return float(-np.log(p[np.arange(len(test_i)), test_label]).mean()), float((act == test_label).mean())
  ce_before, agree_before = held_out()
  bt = ac.PPOBatch(LEARN_B, 'cuda')
  label_d = torch.from_numpy(label).cuda()
  agree_sum = torch.zeros((), device='cuda')
  for k, idx in enumerate(orders[0]):
    i = torch.from_numpy(idx).cuda()
    bt.state[:, :1099].copy_(observations[i])
    bt.action.copy_(label_d[i])
    tr.capture(bt) if k == 0 else tr.train_step(bt)
    agree_sum += tr.views(LEARN_B)['aux'][:, 1].mean()
  tr.check_errors()
  assert int(tr.adam_step.item()) == LEARN_UPDATES
  ce_after, agree_after = held_out()
  twins = [_twin_run(params, x, label, o, x[test_i], test_label) for o in orders]
  twin_agree = [t[2] for t in twins]
  spread = max(twin_agree) - min(twin_agree)
  print('labels', counts, 'device: held-out CE', ce_before, '->', ce_after, 'agreement', agree_before, '->', agree_after,
        'mean batch agreement', float(agree_sum.item()) / LEARN_UPDATES)
  print('twin (three orders): held-out CE', [(t[0], t[1]) for t in twins], 'agreement', twin_agree, 'spread', spread)
  assert abs(twins[0][0] - ce_before) <= 1e-5 * ce_before               # the same initial parameters
  assert ce_after < ce_before
  assert all(t[1] < t[0] for t in twins)
  assert agree_after >= twin_agree[0] - spread, (agree_after, twin_agree, spread)
  # what was learnt is a QNetwork: PPOTrainer takes it as it is
  clone = tr.network()
  ppo = ac.PPOTrainer(clone)
  out = ppo.act_greedy(test_obs).cpu().numpy()
  assert float((out == test_label).mean()) == agree_after
