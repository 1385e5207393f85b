"""A population trained by gradient (csrc/ble_population_train.h, agents/population.py: PopulationPPOTrainer,
agents/actor_critic.py: VecPopulationRolloutBuffer, train_lib.run_pbt_loop_vec).  The contract is 3q's: member p's part of a
grouped call holds the BYTES the plain entry point gives member p alone, so every comparison below is bitwise (NaN patterns included)
and the references are the single-network entry points: PPOTrainer's ble_qnet_ppo_step_f32 and VecActorCriticAgent's ble_ac_act_f32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (2, 64), (3, 256)]                     # (layers, hidden) of two-atom networks
MEMBERS = (1, 2, 5)
ROWS = (1, 7, 9, 33, 129, 515)                           # 515: 2 slabs of 258 rows, a slab boundary inside an 8-row group
NAN = float('nan')


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  import types
  from balloon_learning_environment_amd import _abi, _lib, device, train_lib
  from balloon_learning_environment_amd.agents import actor_critic, population, qnet, qnet_train
  from balloon_learning_environment_amd.env import balloon_env
  from balloon_learning_environment_amd.eval import eval_lib, suites
  return types.SimpleNamespace(_abi=_abi, _lib=_lib, dev=device, train_lib=train_lib, ac=actor_critic, population=population, qnet=qnet,
                               qnet_train=qnet_train, balloon_env=balloon_env, eval_lib=eval_lib, suites=suites)


@pytest.fixture(scope='module')
def observations():
  """1024 device observations of real balloons (reset + a few random steps), float32 [1024, 1099]: test_gpu_ppo.py's."""
  from balloon_learning_environment_amd.env import balloon_env
  env = balloon_env.VecBalloonEnv(256, seed=3)
  rows = [env.reset().clone()]
  g = torch.Generator(device='cuda').manual_seed(0)
  for _ in range(3):
    obs, _, _ = env.step(torch.randint(0, 3, (256,), dtype=torch.uint8, device='cuda', generator=g))
    rows.append(obs.clone())
  env.check_errors()
  return torch.cat(rows)


def _same(a, b):
  """Bitwise equality of two tensors of one dtype (NaN equals NaN of the same bits)."""
  assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
  if a.dtype == torch.float32:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
  return torch.equal(a, b)


def _network(mods, layers, hidden, seed):
  """An independently initialised two-atom network with non-zero biases and policies away from uniform."""
  params = mods.qnet.init_params('quantile', seed, layers, hidden, 2)
  rng = np.random.default_rng(1000 + seed)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * 1e-2).astype(np.float32)
  return mods.qnet.QNetwork.from_params(params, num_atoms=2)


def _hyper(members):
  """Distinct per-member learning rates, clips and coefficients."""
  p = np.arange(members)
  return dict(lr=1e-3 * 1.5 ** p, clip=0.1 + 0.05 * p, value_coef=0.5 + 0.125 * p, entropy_coef=0.01 * (1 + p))


def _population(mods, layers, hidden, members, gap=64, **kw):
  """(networks, population, trainer): distinct members at a stride that leaves `gap` floats between images, filled with NaN in every
  per-member tensor; the gradient NaN throughout (every float of an image is written by an update)."""
  nets = [_network(mods, layers, hidden, seed=11 + p) for p in range(members)]
  packed = int(nets[0].packed_host.size)
  pop = mods.population.QNetworkPopulation.from_networks(nets, member_stride=packed + gap)
  tr = mods.population.PopulationPPOTrainer(pop, seed=5, **{**_hyper(members), **kw})
  for t in (pop.images, tr.adam_m, tr.adam_v):
    t[:, packed:] = NAN
  tr.grad.fill_(NAN)
  if tr.transposed_stride > tr.transposed_floats:
    tr.weights_t[:, tr.transposed_floats:] = NAN
  return nets, pop, tr


def _solo(mods, nets, tr, p, **kw):
  """Member p's own trainer: PPOTrainer on a copy of its network with its hyperparameters."""
  h = {k: float(getattr(tr, k)[p].item()) for k in mods.population.HYPER}
  return mods.ac.PPOTrainer(nets[p], eps=tr.eps, b1=tr.b1, b2=tr.b2, gamma=tr.gamma, lam=tr.lam, seed=tr.seed, **{**h, **kw})


def _with_stride(mods, bt, stride):
  """The batch with its state rows at another stride (a multiple of 4 >= 1099), the padding past column 1098 NaN (never read)."""
  if stride == bt.state.shape[1]:
    return bt
  n = bt.state.shape[0]
  state = torch.full((n, stride), NAN, dtype=torch.float32, device='cuda')
  state[:, :1099] = bt.state[:, :1099]
  bt.state = state
  bt.struct = mods._abi.BleTrainBatchF32(n, stride, state.data_ptr(), None, bt.ret.data_ptr(), None, bt.action.data_ptr(), None)
  return bt


def _batches(mods, observations, members, rows, seed, stride=1104):
  """A grouped batch of P * B rows and the P solo batches of its members' rows."""
  rng = np.random.default_rng(seed)
  n = members * rows
  x = observations[torch.from_numpy(rng.integers(0, len(observations), n)).cuda()]
  act = rng.integers(0, 3, n).astype(np.uint8)
  ret = rng.standard_normal(n).astype(np.float32)
  old = (np.log(1.0 / 3.0) + 0.4 * rng.standard_normal(n)).astype(np.float32)      # rho inside the band, above and below it
  adv = rng.standard_normal(n).astype(np.float32)
  grouped = mods.population.PopulationPPOBatch(members, rows, 'cuda')
  for name, v in (('ret', ret), ('action', act), ('old_logp', old), ('advantage', adv)):
    getattr(grouped, name).copy_(torch.from_numpy(v))
  grouped.state[:, :1099].copy_(x)
  solos = []
  for p in range(members):
    s = slice(p * rows, (p + 1) * rows)
    solos.append(_with_stride(mods, mods.ac.PPOBatch.from_tensors(x[s].cpu().numpy(), ret[s], act[s], old[s], adv[s], 'cuda'), stride))
  return _with_stride(mods, grouped, stride), solos


def _gaps(lay, members, rows, layers):
  """The floats of a grouped workspace that no stage writes -- those that only round a part up to 64 floats, and target_logits, which a
  PPO update has no use for: [(first, end)].  (partial is scratch for the slabs' sums; what follows its use is not looked at.)"""
  n, ld = members * rows, lay.ld
  return [(lay.acts + layers * n * ld, lay.target_logits), (lay.target_logits, lay.targets), (lay.targets + 2 * n, lay.dlogits),
          (lay.dlogits + n * ld, lay.scratch), (lay.scratch + 4 * n * ld, lay.partial), (lay.corrections + 4, lay.total)]


def _compare_member(mods, tr, solo, p, rows, what, state=True):
  """Member p's part of the grouped trainer against its solo trainer: the workspace's rows, the gradient and (state) the images."""
  packed = tr.population.packed_floats
  gv, sv = tr.views(rows), solo.views(rows)
  for k in ('loss', 'aux', 'logits', 'dlogits'):
    assert _same(gv[k][p], sv[k]), (what, p, k)
  for l in range(tr.num_layers):                             # (a layer writes its own padded width of the ld columns)
    width = 64 if l == tr.num_layers - 1 else -(-tr.hidden_units // 64) * 64
    assert _same(gv['acts'][l][p][:, :width], sv['acts'][l][:, :width]), (what, p, 'acts', l)
  assert _same(tr.grad[p, :packed], solo.grad), (what, p, 'grad')
  if state:
    assert _same(tr.images[p, :packed], solo.weights), (what, p, 'weights')
    assert _same(tr.adam_m[p, :packed], solo.adam_m) and _same(tr.adam_v[p, :packed], solo.adam_v), (what, p, 'moments')
    if tr.num_layers > 1:
      assert _same(tr.weights_t[p, :tr.transposed_floats], solo.weights_t[:tr.transposed_floats]), (what, p, 'weights_t')


def _padding_mask(mods, net):
  """True where a float of the packed image is padding: the image of all-ones parameters is 0 there."""
  ones = mods.qnet.QNetwork([np.ones_like(k) for k in net.kernels], [np.ones_like(b) for b in net.biases], 2)
  return torch.from_numpy(ones.packed_host == 0).cuda()


def _grouped_is_each_members_own(mods, observations, layers, hidden, members, rows, stride):
  nets, pop, tr = _population(mods, layers, hidden, members)
  packed = pop.packed_floats
  solos = [_solo(mods, nets, tr, p) for p in range(members)]
  ws, lay, _ = tr.workspace(rows)
  ws.fill_(NAN)
  before = {k: getattr(tr, k).clone() for k in ('adam_m', 'adam_v', 'weights_t')}
  images = pop.images.clone()
  # an update that applies nothing: the gradient only; weights, weights_t, moments and the step counter untouched
  grouped, solo_bt = _batches(mods, observations, members, rows, seed=rows, stride=stride)
  tr.train_on_batch(grouped, apply_update=False)
  for p in range(members):
    solos[p].train_on_batch(solo_bt[p], apply_update=False)
    _compare_member(mods, tr, solos[p], p, rows, 'apply_update=0', state=False)
  assert _same(pop.images, images) and all(_same(getattr(tr, k), v) for k, v in before.items()) and int(tr.adam_step.item()) == 0
  # two consecutive updates: the second reads the weights_t and the moments the first wrote
  for u in range(2):
    grouped, solo_bt = _batches(mods, observations, members, rows, seed=100 * u + rows, stride=stride)
    tr.train_on_batch(grouped)
    for p in range(members):
      solos[p].train_on_batch(solo_bt[p])
      _compare_member(mods, tr, solos[p], p, rows, f'update {u}')
    assert not _same(pop.images[:, :packed], images[:, :packed])
  assert int(tr.adam_step.item()) == 2
  tr.check_errors()
  # the gradient's padding is +0.0; the floats between images and the workspace's gaps keep their NaN
  assert not tr.grad[:, :packed].isnan().any()
  assert (tr.grad[:, :packed][:, _padding_mask(mods, nets[0])].view(torch.int32) == 0).all()
  for t in (pop.images, tr.grad, tr.adam_m, tr.adam_v):
    assert t[:, packed:].isnan().all()
  assert tr.weights_t[:, tr.transposed_floats:].isnan().all()
  for first, end in _gaps(lay, members, rows, layers):
    assert ws[first:end].isnan().all(), (first, end)


# ---- 1. the grouped update is each member's own ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('layers,hidden', SHAPES)
def test_grouped_update_is_each_members_own(mods, observations, layers, hidden, rows):
  """Per member: loss, aux, logits, every layer's activations, dlogits, grad without an update; then weights, weights_t, adam_m and
  adam_v after each of two updates.  State rows at stride 1100 (1099 padded to a multiple of 4) and 1104."""
  for members in MEMBERS:
    _grouped_is_each_members_own(mods, observations, layers, hidden, members, rows, 1100 if members != 2 else 1104)


def test_grouped_update_over_16_slabs(mods, observations):
  """(2, 64, 2) at (P, B) = (2, 4 100): 16 slabs of 257 rows per member."""
  _grouped_is_each_members_own(mods, observations, 2, 64, 2, 4100, 1104)
  assert mods.population.PopulationPPOTrainer(mods.population.QNetworkPopulation(_network(mods, 2, 64, 1), 2)).workspace(4100)[1].slabs == 16


# ---- 2. members do not leak -----------------------------------------------------------------------------------------------------------
def _member_bytes(tr, p, rows):
  packed = tr.population.packed_floats
  v = tr.views(rows)
  return [v[k][p].clone() for k in ('loss', 'aux', 'logits', 'dlogits')] + [t[p, :packed].clone() for t in (tr.grad, tr.images, tr.adam_m, tr.adam_v)]


@pytest.mark.parametrize('rows', [33, 515])
def test_members_do_not_leak(mods, observations, rows):
  members, victim, row = 3, 1, 5
  def run(spoil):
    _, pop, tr = _population(mods, 2, 64, members)
    grouped, _ = _batches(mods, observations, members, rows, seed=3)
    spoil(grouped)
    tr.train_on_batch(grouped)
    return tr, [_member_bytes(tr, p, rows) for p in range(members)]
  _, clean = run(lambda bt: None)
  # a NaN in one member's rows changes that member's bytes only
  def nan_row(bt):
    bt.state[victim * rows + row, 7] = NAN
  tr, got = run(nan_row)
  tr.check_errors()
  for p in range(members):
    equal = [_same(a, b) for a, b in zip(got[p], clean[p])]
    assert all(equal) if p != victim else not any(equal[4:]), (p, equal)
  assert got[victim][4].isnan().any() and not any(t.isnan().any() for p in (0, 2) for t in got[p])
  # an action of 3 in one row: the flag, that row's loss, aux and dlogits zero; the member's other rows and the other members keep their bytes
  def bad_action(bt):
    bt.action[victim * rows + row] = 3
  tr, got = run(bad_action)
  with pytest.raises(ValueError):
    tr.check_errors()
  loss, aux, logits, dlogits = got[victim][:4]
  assert loss[row] == 0 and not aux[row].any() and not dlogits[row].any()
  keep = torch.arange(rows, device='cuda') != row
  for k in range(4):
    assert _same(got[victim][k][keep], clean[victim][k][keep]), k
  assert _same(logits, clean[victim][2]) and not _same(got[victim][4], clean[victim][4])
  for p in (0, 2):
    assert all(_same(a, b) for a, b in zip(got[p], clean[p])), p


# ---- 3. P = 1 grouped equals the plain entry point; a captured update replays to the eager bytes ---------------------------------------
@pytest.mark.parametrize('layers,hidden,rows', [(2, 64, 300), (3, 256, 515)])
def test_one_member_is_the_plain_entry_point_and_graph_replay(mods, observations, layers, hidden, rows):
  nets, pop, eager = _population(mods, layers, hidden, 1, gap=0)
  _, pop_g, graph = _population(mods, layers, hidden, 1, gap=0)
  solo = _solo(mods, nets, eager, 0)
  grouped, solo_bt = _batches(mods, observations, 1, rows, seed=9)
  grouped_g, _ = _batches(mods, observations, 1, rows, seed=9)
  graph.capture(grouped_g)                                   # (update 1, eager)
  for u in range(1, 4):
    if u > 1:
      graph.train_step(grouped_g)                            # (updates 2 and 3: replays)
    eager.train_on_batch(grouped)
    solo.train_on_batch(solo_bt[0])
    _compare_member(mods, eager, solo, 0, rows, f'update {u}')
    assert int(graph.adam_step.item()) == int(eager.adam_step.item()) == int(solo.adam_step.item()) == u
    for k in ('images', 'grad', 'adam_m', 'adam_v', 'weights_t'):
      assert _same(getattr(graph, k), getattr(eager, k)), (u, k)
    assert _same(graph.views(rows)['loss'], eager.views(rows)['loss'])
  assert graph._graphs and graph._graphs[rows][1] is grouped_g


# ---- 4. the sampled act of a population ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('members', [1, 3])
@pytest.mark.parametrize('rows', [1, 33, 129])
def test_grouped_act_is_each_members_own(mods, observations, members, rows):
  nets, pop, tr = _population(mods, 2, 64, members)
  n = members * rows
  obs = observations[100:100 + n]
  def outputs():
    return (torch.full((n,), 9, dtype=torch.uint8, device='cuda'), torch.full((n,), NAN, device='cuda'), torch.full((n,), NAN, device='cuda'),
            torch.full((n, 3), NAN, device='cuda'))
  for step in (0, 2 ** 32 + 7):
    tr.act_step.fill_(step)
    got = outputs()
    tr.act(obs, *got)
    assert int(tr.act_step.item()) == step + 1
    for p in range(members):
      agent = mods.ac.VecActorCriticAgent(nets[p], deterministic=False, seed=tr.seed, env_offset=p * rows)
      agent.step.fill_(step)
      want = outputs()
      agent.act(obs[p * rows:(p + 1) * rows], *(w[:rows] for w in want))
      for g, w, name in zip(got, want, ('action', 'logp', 'value', 'probs')):
        assert _same(g[p * rows:(p + 1) * rows], w[:rows]), (step, p, name)
  # greedy: the existing grouped greedy head, and the counter stays
  got = outputs()
  tr.act_greedy(obs, *got)
  assert int(tr.act_step.item()) == 2 ** 32 + 8
  want = outputs()
  mods.population.VecPopulationAgent(pop, rows, head='actor').act(obs, want[0], None, want[2], want[3])
  for k in (0, 2, 3):
    assert _same(got[k], want[k]), k
  for p in range(members):
    logp = torch.zeros(rows, device='cuda')
    mods.ac.VecActorCriticAgent(nets[p]).act(obs[p * rows:(p + 1) * rows], None, logp)
    assert _same(got[1][p * rows:(p + 1) * rows], logp), p


# ---- the contextual bandit of test_gpu_ppo.py ------------------------------------------------------------------------------------------
class _Bandit:
  """test_gpu_ppo.py's contextual bandit as an environment of N lanes: every step terminal, reward 1 for the labelled action (0 or 2 as
  the most varied feature within [0, 1] is below or above its median).  Block k shows rows drawn from a generator seeded (seed, k): a
  resumed run sees the rows of a straight one."""

  def __init__(self, observations, num_envs, seed=0):
    x = observations.cpu().numpy()
    std = np.where((x.min(axis=0) >= 0) & (x.max(axis=0) <= 1), x.std(axis=0), 0.0)
    col = int(np.argmax(std))
    self.label_host = np.where(x[:, col] > np.median(x[:, col]), 2, 0).astype(np.uint8)
    perm = np.random.default_rng(0).permutation(len(x))
    self.train_i, self.test_i = perm[:768], perm[768:]
    self.observations, self.label = observations, torch.from_numpy(self.label_host).cuda()
    self.num_envs, self.device, self.seed, self.k = num_envs, observations.device, seed, 0
    self._draw()

  def _draw(self):
    rng = np.random.default_rng([self.seed, self.k])
    self.i = torch.from_numpy(rng.choice(self.train_i, self.num_envs)).cuda()

  def reset(self):
    return self.observations[self.i]

  def step(self, actions, end_mask=None):
    reward = (actions == self.label[self.i]).to(torch.float32)
    self.k += 1
    self._draw()
    return self.observations[self.i], reward, torch.ones(self.num_envs, dtype=torch.uint8, device=self.device)

  def check_errors(self):
    pass

  def accuracy(self, mods, network):
    act = mods.ac.VecActorCriticAgent(network).act(self.observations[torch.from_numpy(self.test_i).cuda()]).cpu().numpy()
    return float((act == self.label_host[self.test_i]).mean())


# ---- 5. a population on the bandit is P solo runs -------------------------------------------------------------------------------------
def test_population_on_the_bandit_is_p_solo_runs(mods, observations):
  members, rows, blocks = 4, 256, 10
  lrs = [3e-4, 1e-3, 3e-3, 1e-2]
  net = mods.qnet.QNetwork.from_params(mods.ac.init_params('actor_critic', 7, 2, 64), num_atoms=2)
  pop = mods.population.QNetworkPopulation(net, members)
  tr = mods.population.PopulationPPOTrainer(pop, lr=lrs, seed=5)
  ro = mods.ac.VecPopulationRolloutBuffer(members, rows, 1, 'cuda')
  solo = [mods.ac.PPOTrainer(net, lr=lrs[p], seed=5, env_offset=p * rows) for p in range(members)]
  solo_ro = [mods.ac.VecRolloutBuffer(rows, 1, 'cuda') for _ in range(members)]
  env = _Bandit(observations, members * rows)
  n = members * rows
  new = lambda m: (torch.zeros(m, dtype=torch.uint8, device='cuda'), torch.zeros(m, device='cuda'), torch.zeros(m, device='cuda'))
  actions, logp, value = new(n)
  ones, zeros = torch.ones(n, dtype=torch.uint8, device='cuda'), torch.zeros(n, device='cuda')
  obs = env.reset()
  for _ in range(blocks):
    tr.act(obs, actions, logp, value)
    next_obs, reward, _ = env.step(actions)
    ro.add(0, obs, actions, logp, value, reward, ones)
    ro.finish(zeros, tr.gamma, tr.lam, tr.normalize_advantage)
    for _ in range(4):
      for bt in ro.minibatches(128):
        tr.train_on_batch(bt)
    for p in range(members):
      s = slice(p * rows, (p + 1) * rows)
      a, l, v = new(rows)
      solo[p].act(obs[s], a, l, v)
      assert _same(a, actions[s]) and _same(l, logp[s]) and _same(v, value[s]), p      # (the last block's among them)
      solo_ro[p].add(0, obs[s], a, l, v, reward[s], ones[s])
      solo_ro[p].finish(zeros[s], solo[p].gamma, solo[p].lam, solo[p].normalize_advantage)
      for _ in range(4):
        for bt in solo_ro[p].minibatches(128):
          solo[p].train_on_batch(bt)
    obs = next_obs
  tr.check_errors()
  packed = pop.packed_floats
  assert int(tr.adam_step.item()) == 80
  for p in range(members):
    assert int(solo[p].adam_step.item()) == 80
    assert _same(pop.images[p, :packed], solo[p].weights), p
    assert _same(tr.adam_m[p, :packed], solo[p].adam_m) and _same(tr.adam_v[p, :packed], solo[p].adam_v), p
    assert _same(tr.weights_t[p, :tr.transposed_floats], solo[p].weights_t[:tr.transposed_floats]), p
  # a member's state continues alone: a fresh PPOTrainer that loads it takes member 0's next update
  heir = mods.ac.PPOTrainer(net, lr=1.0, seed=99)
  heir.load_state_dict(tr.member_trainer_state(0))
  assert set(tr.member_trainer_state(0)) == set(solo[0].state_dict()) and np.float32(heir.lr) == np.float32(lrs[0]) and heir.seed == 5
  bt = next(iter(solo_ro[0].minibatches(128)))
  heir.train_on_batch(bt)
  solo[0].train_on_batch(bt)
  assert _same(heir.weights, solo[0].weights) and _same(heir.adam_m, solo[0].adam_m) and _same(heir.weights_t, solo[0].weights_t)
  assert not _same(pop.images[0], pop.images[3])


# ---- 6. copy_members and scale_hyper ---------------------------------------------------------------------------------------------------
def test_copy_members_and_scale_hyper(mods, observations):
  members, rows = 5, 33
  nets, pop, tr = _population(mods, 2, 64, members)
  grouped, _ = _batches(mods, observations, members, rows, seed=1)
  tr.train_on_batch(grouped)                                 # (moments and weights_t that differ between members)
  names = ('images', 'weights_t', 'adam_m', 'adam_v') + mods.population.HYPER
  before = {k: getattr(tr, k).clone() for k in names}
  src, dst = torch.tensor([4, 0], device='cuda'), torch.tensor([1, 3], device='cuda')
  tr.copy_members(src, dst)
  for k in names:
    t = getattr(tr, k)
    assert _same(t[1], before[k][4]) and _same(t[3], before[k][0]), k
    assert all(_same(t[p], before[k][p]) for p in (0, 2, 4)), k
  factor = torch.tensor([0.8, 1.25], dtype=torch.float32, device='cuda')
  tr.scale_hyper('lr', dst, factor)
  tr.scale_hyper('entropy_coef', dst, 1.25)
  want_lr = before['lr'].clone()
  want_lr[1], want_lr[3] = before['lr'][4] * factor[0], before['lr'][0] * factor[1]
  assert _same(tr.lr, want_lr)
  assert _same(tr.entropy_coef[dst], before['entropy_coef'][src] * torch.tensor(1.25, device='cuda')) and _same(tr.clip[dst], before['clip'][src])
  with pytest.raises(ValueError):
    tr.scale_hyper('gamma', dst, 2.0)
  # the next update of a copy on its source's rows is its source's update, where the hyperparameters are the source's too
  tr.lr.copy_(before['lr'][[0, 4, 2, 0, 4]])
  tr.entropy_coef.copy_(before['entropy_coef'][[0, 4, 2, 0, 4]])
  grouped, _ = _batches(mods, observations, members, rows, seed=2)
  for name in ('state', 'ret', 'action', 'old_logp', 'advantage'):
    t = getattr(grouped, name).view(members, rows, -1)
    t[1], t[3] = t[4].clone(), t[0].clone()
  tr.train_on_batch(grouped)
  for d, s in ((1, 4), (3, 0)):
    for a, b in zip(_member_bytes(tr, d, rows), _member_bytes(tr, s, rows)):
      assert _same(a, b), (d, s)
  assert not _same(tr.images[1], tr.images[3])


# ---- 7. population-based training learns the bandit -------------------------------------------------------------------------------------
PBT_MEMBERS, PBT_ROWS, PBT_BLOCKS = 8, 256, 60


def _pbt_objects(mods, observations):
  net = mods.qnet.QNetwork.from_params(mods.ac.init_params('actor_critic', 7, 2, 64), num_atoms=2)
  pop = mods.population.QNetworkPopulation(net, PBT_MEMBERS)
  tr = mods.population.PopulationPPOTrainer(pop, lr=[1e-3] * 4 + [1e-7] * 4, seed=5)
  ro = mods.ac.VecPopulationRolloutBuffer(PBT_MEMBERS, PBT_ROWS, 1, 'cuda')
  env = _Bandit(observations, PBT_MEMBERS * PBT_ROWS)
  pbt = mods.train_lib.PBTController(PBT_MEMBERS, 'cuda', ready_every=5, truncation=0.25, seed=0)
  return env, tr, ro, pbt


def _pbt_run(mods, env, tr, ro, pbt, blocks):
  return mods.train_lib.run_pbt_loop_vec(env, tr, ro, num_iterations=blocks, epochs=4, batch_size=128, ready_every=5, controller=pbt,
                                         max_episode_length=960)


def test_pbt_learns_the_bandit(mods, observations):
  """P = 8 members of R = 256 rows, test_gpu_ppo.py's bandit and budget (60 blocks of T = 1, 4 epochs of B = 128), a round every 5
  blocks at truncation 0.25; four members start at lr 1e-3 and four at 1e-7.  Two runs and a run resumed at block 30 are byte-equal; the
  best member's held-out greedy accuracy is >= 0.9, the solo test's threshold.  Measured: DESIGN 3r."""
  runs = []
  for _ in range(2):
    env, tr, ro, pbt = _pbt_objects(mods, observations)
    stats = _pbt_run(mods, env, tr, ro, pbt, PBT_BLOCKS)
    runs.append((env, tr, pbt, stats))
  (env, tr, pbt, stats), (_, tr_b, pbt_b, stats_b) = runs
  state = ('images', 'weights_t', 'adam_m', 'adam_v', 'adam_step', 'act_step') + mods.population.HYPER
  assert all(_same(getattr(tr, k), getattr(tr_b, k)) for k in state) and _same(pbt.lineage, pbt_b.lineage), 'two runs differ'
  assert repr(stats) == repr(stats_b)                        # (repr: NaN fitness equals itself)
  assert int(tr.adam_step.item()) == PBT_BLOCKS * 8 and pbt.rounds == 12 and stats[-1]['transitions'] == PBT_BLOCKS * PBT_MEMBERS * PBT_ROWS
  # resumed at block 30 from the state_dicts, into fresh objects
  env_c, tr_c, ro_c, pbt_c = _pbt_objects(mods, observations)
  first = _pbt_run(mods, env_c, tr_c, ro_c, pbt_c, 30)
  env_d, tr_d, ro_d, pbt_d = _pbt_objects(mods, observations)
  tr_d.lr.fill_(1.0)
  tr_d.load_state_dict(tr_c.state_dict())
  ro_d.load_state_dict(ro_c.state_dict())
  pbt_d.load_state_dict(pbt_c.state_dict())
  env_d.k = env_c.k
  env_d._draw()
  second = _pbt_run(mods, env_d, tr_d, ro_d, pbt_d, 30)
  assert all(_same(getattr(tr, k), getattr(tr_d, k)) for k in state) and _same(pbt.lineage, pbt_d.lineage), 'resume differs'
  assert [s['lineage'] for s in first + second] == [s['lineage'] for s in stats]
  assert [s['mean_return'] for s in first + second] == [s['mean_return'] for s in stats]
  accuracy = [env.accuracy(mods, tr.member(p)) for p in range(PBT_MEMBERS)]
  print('PBT bandit: lineage', stats[-1]['lineage'], 'lr', tr.lr.tolist(), 'entropy_coef', tr.entropy_coef.tolist())
  print('PBT bandit: held-out greedy accuracy per member', accuracy, 'last block mean return per member', stats[-1]['member_mean_return'])
  assert max(accuracy) >= 0.9, accuracy


# ---- 8. one iteration on a real environment --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('capture_graph', [False, True])
def test_pbt_loop_on_a_real_environment(mods, capture_graph):
  members, rows, steps = 2, 32, 8
  env = mods.balloon_env.VecBalloonEnv(members * rows, seed=1)
  nets = [mods.qnet.QNetwork.from_params(mods.ac.init_params('actor_critic', 2 + p, 2, 64), num_atoms=2) for p in range(members)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  tr = mods.population.PopulationPPOTrainer(pop, lr=[1e-3, 3e-4], seed=4)
  ro = mods.ac.VecPopulationRolloutBuffer(members, rows, steps, 'cuda')
  stats = mods.train_lib.run_pbt_loop_vec(env, tr, ro, num_iterations=1, epochs=2, batch_size=64, ready_every=1, truncation=0.5,
                                          max_episode_length=5, capture_graph=capture_graph)
  assert len(stats) == 1
  s = stats[0]
  assert s['transitions'] == members * rows * steps and s['updates'] == 2 * (rows * steps // 64) and np.isfinite(s['mean_loss'])
  assert np.isfinite(s['mean_return']) and s['episodes'] >= members * rows and all(np.isfinite(v) for v in s['member_mean_return'])
  assert sum(s['member_episodes']) == s['episodes'] and sorted(s['round']['src'] + s['round']['dst']) == [0, 1]
  assert s['lineage'] == [s['round']['src'][0]] * 2 and 0.0 <= s['time_within_radius'] <= 1.0
  tr.check_errors()
  assert int(tr.err_flags.item()) == 0 and int(tr.adam_step.item()) == s['updates'] and int(tr.act_step.item()) == steps + 1
  assert pop.images.isfinite().all() and ro.advantage.isfinite().all()
  assert _same(pop.images[0], pop.images[1])                 # (the round copied the better member over the other)
  res = mods.eval_lib.eval_population_vec(pop, mods.suites.EvaluationSuite([0, 1], 20), head='actor')
  assert len(res) == members and all(len(r) == 2 and all(np.isfinite(x.cumulative_reward) for x in r) for r in res)
