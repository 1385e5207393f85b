"""A population of replay learners (csrc/ble_population_td.h, agents/population.py: PopulationQTrainer, agents/qnet_train.py:
VecPopulationReplayBuffer and explore_grouped, train_lib.run_population_training_loop_vec).  The contract is 3q's and 3r's:
member p's part of a grouped call holds the BYTES the plain entry point gives member p alone, so every comparison below is bitwise (NaN
patterns included) and the references are the single-learner entry points: QNetworkTrainer's ble_qnet_train_step_f32, DQNTrainer's
ble_qnet_td_step_f32, VecReplayBuffer's ble_replay_sample_f32 and explore()'s ble_qnet_explore_u8."""
import ctypes

import numpy as np
import pytest
import torch

import train_host

pytestmark = pytest.mark.gpu

# (layers, hidden, atoms, kind): 65 atoms take the quantile loss's `j += 64` loop round a second time
NETWORKS = [(2, 64, 51, 'quantile'), (2, 64, 65, 'quantile'), (1, 0, 51, 'quantile'), (2, 64, 1, 'dqn_mse'), (2, 64, 1, 'dqn_huber'),
            (1, 0, 1, 'dqn_mse'), (1, 0, 1, 'quantile')]
MEMBERS = (1, 2, 5)
ROWS = (1, 7, 33, 129, 515)                              # 515: 2 slabs of 258 rows, a slab boundary inside an 8-row group
NAN = float('nan')


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  import types
  from balloon_learning_environment_amd import _abi, _lib, device, train_lib
  from balloon_learning_environment_amd.agents import dqn_agent, population, qnet, qnet_train
  from balloon_learning_environment_amd.env import balloon_env
  from balloon_learning_environment_amd.eval import eval_lib, suites
  return types.SimpleNamespace(_abi=_abi, _lib=_lib, dev=device, train_lib=train_lib, dqn=dqn_agent, population=population, qnet=qnet,
                               qnet_train=qnet_train, balloon_env=balloon_env, eval_lib=eval_lib, suites=suites)


@pytest.fixture(scope='module')
def observations():
  """1024 device observations of real balloons (reset + a few random steps), float32 [1024, 1099]: test_gpu_train.py's."""
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


def _network(mods, layers, hidden, atoms, seed):
  """An independently initialised network with non-zero biases."""
  params = mods.qnet.init_params('quantile', seed, layers, hidden, atoms)
  rng = np.random.default_rng(1000 + seed)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * 1e-2).astype(np.float32)
  return mods.qnet.QNetwork.from_params(params, num_atoms=atoms)


def _hyper(members):
  """Distinct per-member learning rates and Huber thresholds (0.25 .. 1.25: the targets' errors fall on both sides of each)."""
  p = np.arange(members)
  return dict(lr=1e-3 * 1.5 ** p, kappa=0.25 + 0.25 * p)


def _population(mods, layers, hidden, atoms, kind, members, gap=64, **kw):
  """(online networks, target networks, population, trainer): distinct online and target images per member at a stride that leaves `gap`
  floats between images, filled with NaN in every per-member tensor; the gradient NaN throughout (an update writes every float of an
  image)."""
  nets = [_network(mods, layers, hidden, atoms, seed=11 + p) for p in range(members)]
  targets = [_network(mods, layers, hidden, atoms, seed=51 + p) for p in range(members)]
  packed = int(nets[0].packed_host.size)
  pop = mods.population.QNetworkPopulation.from_networks(nets, member_stride=packed + gap)
  tr = mods.population.PopulationQTrainer(pop, kind=kind, seed=5, **{**_hyper(members), **kw})
  for p in range(members):
    tr.target[p, :packed] = torch.from_numpy(targets[p].packed_host).cuda()
  for t in (pop.images, tr.target, tr.adam_m, tr.adam_v):
    t[:, packed:] = NAN
  tr.grad.fill_(NAN)
  if tr.transposed_stride > tr.transposed_floats:
    tr.weights_t[:, tr.transposed_floats:] = NAN
  return nets, targets, pop, tr


def _solo(mods, nets, targets, tr, p):
  """Member p's own trainer: QNetworkTrainer / DQNTrainer on a copy of its network with its hyperparameters and its target image."""
  kw = dict(lr=float(tr.lr[p].item()), eps=tr.eps, b1=tr.b1, b2=tr.b2, gamma=tr.gamma, update_horizon=tr.update_horizon,
            seed=int(tr.seeds[p].item()))
  if tr.kind == 'quantile':
    solo = mods.qnet_train.QNetworkTrainer(nets[p], kappa=float(tr.kappa[p].item()), **kw)
  else:
    solo = mods.dqn.DQNTrainer(nets[p], loss_type=tr.kind[len('dqn_'):], **kw)
  solo.target.copy_(torch.from_numpy(targets[p].packed_host).cuda())
  return solo


def _with_stride(mods, bt, stride):
  """The batch with its state rows at another stride (a multiple of 4 >= 1099), the padding past column 1098 NaN (never read)."""
  if stride == bt.state.shape[1]:
    return bt
  n = bt.state.shape[0]
  for name in ('state', 'next_state'):
    wide = torch.full((n, stride), NAN, dtype=torch.float32, device='cuda')
    wide[:, :1099] = getattr(bt, name)[:, :1099]
    setattr(bt, name, wide)
  bt.struct = mods._abi.BleTrainBatchF32(n, stride, bt.state.data_ptr(), bt.next_state.data_ptr(), bt.ret.data_ptr(), bt.discount.data_ptr(),
                                         bt.action.data_ptr(), bt.index.data_ptr())
  return bt


def _batches(mods, observations, members, rows, seed, stride=1104):
  """A grouped batch of P * B rows and the P solo batches of its members' rows; about a fifth of the rows have discount 0."""
  rng = np.random.default_rng(seed)
  n = members * rows
  x = observations.cpu().numpy()
  i, j = rng.integers(0, len(x), n), rng.integers(0, len(x), n)
  disc = np.where(rng.random(n) < 0.2, 0.0, 0.993 ** 5).astype(np.float32)
  if n > 1:
    disc[1] = 0.0
  ret = rng.standard_normal(n).astype(np.float32)
  act = rng.integers(0, 3, n).astype(np.uint8)
  make = mods.qnet_train.TrainBatch.from_tensors
  grouped = _with_stride(mods, make(x[i], x[j], ret, disc, act, 'cuda'), stride)
  solos = []
  for p in range(members):
    s = slice(p * rows, (p + 1) * rows)
    solos.append(_with_stride(mods, make(x[i][s], x[j][s], ret[s], disc[s], act[s], 'cuda'), stride))
  return grouped, solos


def _gaps(lay, members, rows, layers, atoms):
  """The floats of a grouped workspace that no stage writes -- those that only round a part up to 64 floats: [(first, end)].
  (scratch and partial are the stages' own; what is left in them is not looked at.)"""
  n, ld = members * rows, lay.ld
  return [(lay.acts + layers * n * ld, lay.target_logits), (lay.target_logits + n * ld, lay.targets), (lay.targets + n * atoms, lay.dlogits),
          (lay.dlogits + n * ld, lay.scratch), (lay.scratch + 4 * n * ld, lay.partial), (lay.corrections + 4, lay.total)]


def _r64(v):
  return -(-v // 64) * 64


def _compare_member(tr, solo, p, rows, what, state=True):
  """Member p's part of the grouped trainer against its solo trainer: the workspace's rows, the gradient and (state) the images."""
  packed = tr.population.packed_floats
  gv, sv = tr.views(rows), solo.views(rows)
  for k in ('loss', 'logits', 'target_logits', 'targets', 'dlogits'):
    assert _same(gv[k][p], sv[k]), (what, p, k)
  for l in range(tr.num_layers):                             # (a layer writes its own padded width of the ld columns)
    width = _r64(3 * tr.num_atoms) if l == tr.num_layers - 1 else _r64(tr.hidden_units)
    assert _same(gv['acts'][l][p][:, :width], sv['acts'][l][:, :width]), (what, p, 'acts', l)
  assert _same(tr.grad[p, :packed], solo.grad), (what, p, 'grad')
  if state:
    assert _same(tr.images[p, :packed], solo.weights), (what, p, 'weights')
    assert _same(tr.target[p, :packed], solo.target), (what, p, 'target')
    assert _same(tr.adam_m[p, :packed], solo.adam_m) and _same(tr.adam_v[p, :packed], solo.adam_v), (what, p, 'moments')
    if tr.num_layers > 1:
      assert _same(tr.weights_t[p, :tr.transposed_floats], solo.weights_t[:tr.transposed_floats]), (what, p, 'weights_t')


def _padding_mask(mods, net):
  """True where a float of the packed image is padding: the image of all-ones parameters is 0 there."""
  ones = mods.qnet.QNetwork([np.ones_like(k) for k in net.kernels], [np.ones_like(b) for b in net.biases], net.num_atoms)
  return torch.from_numpy(ones.packed_host == 0).cuda()


def _grouped_is_each_members_own(mods, observations, layers, hidden, atoms, kind, members, rows, stride):
  nets, targets, pop, tr = _population(mods, layers, hidden, atoms, kind, members)
  packed = pop.packed_floats
  solos = [_solo(mods, nets, targets, tr, p) for p in range(members)]
  ws, lay, _ = tr.workspace(rows)
  ws.fill_(NAN)
  before = {k: getattr(tr, k).clone() for k in ('adam_m', 'adam_v', 'weights_t', 'target')}
  images = pop.images.clone()
  # an update that applies nothing: the gradient only; weights, weights_t, moments and the step counter untouched
  grouped, solo_bt = _batches(mods, observations, members, rows, seed=rows, stride=stride)
  tr.train_on_batch(grouped, apply_update=False)
  for p in range(members):
    solos[p].train_on_batch(solo_bt[p], apply_update=False)
    _compare_member(tr, solos[p], p, rows, 'apply_update=0', state=False)
  assert _same(pop.images, images) and all(_same(getattr(tr, k), v) for k, v in before.items()) and int(tr.adam_step.item()) == 0
  # two consecutive updates: the second reads the weights_t and the moments the first wrote
  for u in range(2):
    grouped, solo_bt = _batches(mods, observations, members, rows, seed=100 * (u + 1) + rows, stride=stride)
    tr.train_on_batch(grouped)
    for p in range(members):
      solos[p].train_on_batch(solo_bt[p])
      _compare_member(tr, solos[p], p, rows, f'update {u}')
    assert not _same(pop.images[:, :packed], images[:, :packed])
  assert int(tr.adam_step.item()) == 2 and _same(tr.target, before['target'])
  tr.check_errors()
  # the gradient's padding is +0.0; the floats between images and the workspace's gaps keep their NaN
  assert not tr.grad[:, :packed].isnan().any()
  assert (tr.grad[:, :packed][:, _padding_mask(mods, nets[0])].view(torch.int32) == 0).all()
  for t in (pop.images, tr.grad, tr.adam_m, tr.adam_v, tr.target):
    assert t[:, packed:].isnan().all()
  assert tr.weights_t[:, tr.transposed_floats:].isnan().all()
  for first, end in _gaps(lay, members, rows, layers, atoms):
    assert ws[first:end].isnan().all(), (first, end)


# ---- 1. the grouped update is each member's own ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('layers,hidden,atoms,kind', NETWORKS)
def test_grouped_update_is_each_members_own(mods, observations, layers, hidden, atoms, kind, rows):
  """Per member: loss, logits, target_logits, targets, every layer's activations, dlogits, grad without an update; then weights,
  weights_t, adam_m and adam_v after each of two updates.  State rows at stride 1100 (1099 padded to a multiple of 4) and 1104."""
  for members in MEMBERS:
    _grouped_is_each_members_own(mods, observations, layers, hidden, atoms, kind, members, rows, 1100 if members != 2 else 1104)


def test_grouped_update_over_16_slabs(mods, observations):
  """(2, 64, 1) at (P, B) = (2, 4 100): 16 slabs of 257 rows per member."""
  _grouped_is_each_members_own(mods, observations, 2, 64, 1, 'dqn_mse', 2, 4100, 1104)
  pop = mods.population.QNetworkPopulation(_network(mods, 2, 64, 1, 1), 2)
  assert mods.population.PopulationQTrainer(pop, kind='dqn_mse').workspace(4100)[1].slabs == 16


# ---- 2. members do not leak -----------------------------------------------------------------------------------------------------------
def _member_bytes(tr, p, rows):
  packed = tr.population.packed_floats
  v = tr.views(rows)
  return [v[k][p].clone() for k in ('loss', 'targets', 'logits', 'dlogits')] + [t[p, :packed].clone() for t in (tr.grad, tr.images, tr.adam_m, tr.adam_v)]


@pytest.mark.parametrize('kind,atoms', [('quantile', 51), ('dqn_huber', 1)])
@pytest.mark.parametrize('rows', [33, 515])
def test_members_do_not_leak(mods, observations, rows, kind, atoms):
  members, victim, row = 3, 1, 5

  def run(spoil):
    _, _, pop, tr = _population(mods, 2, 64, atoms, kind, members)
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

  # an action of 3 in one row: the flag, that row's loss and dlogits zero (its targets stay, as in the plain kernels); the member's
  # other rows and the other members keep their bytes
  def bad_action(bt):
    bt.action[victim * rows + row] = 3
  tr, got = run(bad_action)
  with pytest.raises(ValueError):
    tr.check_errors()
  loss, targets, logits, dlogits = got[victim][:4]
  assert loss[row] == 0 and not dlogits[row].any()
  keep = torch.arange(rows, device='cuda') != row
  for k in (0, 3):
    assert _same(got[victim][k][keep], clean[victim][k][keep]), k
  assert _same(targets, clean[victim][1]) and _same(logits, clean[victim][2]) and not _same(got[victim][4], clean[victim][4])
  for p in (0, 2):
    assert all(_same(a, b) for a, b in zip(got[p], clean[p])), p


# ---- 3. the replay ring of a population -------------------------------------------------------------------------------------------------
T, P, R = 12, 3, 5
STEPS = 30                                               # the ring wraps: steps 18 .. 29 are held
# (step, column) of the episode ends placed by hand inside the held steps: terminals, and time-limit ends without a terminal
TERMINALS = [(20, 0), (25, 3), (19, 6), (27, 7), (22, 10), (23, 14), (28, 12)]
LIMITS = [(22, 1), (26, 4), (21, 5), (24, 9), (20, 11), (27, 13)]


def _ring(mods, horizon, limits=LIMITS, steps=STEPS, seed=0):
  """(buffer, history): a VecPopulationReplayBuffer(P, R, T) after `steps` adds."""
  rng = np.random.default_rng(seed)
  n = P * R
  rp = mods.qnet_train.VecPopulationReplayBuffer(P, R, T, horizon, 0.993)
  h = {'obs': rng.random((steps, n, 1099), dtype=np.float32), 'action': rng.integers(0, 3, (steps, n)).astype(np.uint8),
       'reward': (np.arange(steps)[:, None] * 100 + np.arange(n)[None, :] + rng.random((steps, n))).astype(np.float32),
       'terminal': np.zeros((steps, n), np.uint8), 'episode_end': np.zeros((steps, n), np.uint8)}
  for s, e in TERMINALS:
    if s < steps:
      h['terminal'][s, e] = h['episode_end'][s, e] = 1
  for s, e in limits:
    if s < steps:
      h['episode_end'][s, e] = 1
  for s in range(steps):
    rp.add(*[torch.from_numpy(h[k][s]).cuda() for k in ('obs', 'action', 'reward', 'terminal', 'episode_end')])
  return rp, h


def _valid_share(h, horizon, p):
  """The share of member p's candidate windows (t + n <= count - 1 inside the ring) that are valid, on the CPU."""
  steps = h['reward'].shape[0]
  lo = max(steps - T, 0)
  cand = [(t, e) for t in range(lo, steps - horizon) for e in range(p * R, (p + 1) * R)]
  ok = [train_host.nstep(h['reward'], h['terminal'], h['episode_end'], t, e, horizon, 0.993) is not None for t, e in cand]
  return sum(ok) / len(cand)


def _sample_grouped(mods, rp, rows, seeds, counter, max_tries=1024):
  bt = mods.qnet_train.TrainBatch(P * rows, 'cuda')
  for t in (bt.state, bt.next_state, bt.ret, bt.discount):
    t.fill_(NAN)
  desc = rp.struct(counter)
  desc.max_tries = max_tries
  mods._lib.call('ble_replay_sample_grouped_f32', ctypes.byref(desc), P, seeds.data_ptr(), ctypes.byref(bt.struct), rp.err_flags.data_ptr(),
                 mods.dev.stream_ptr(rp.device))
  return bt


def _sample_plain(mods, solo, rows, seed, counter, max_tries=1024):
  bt = mods.qnet_train.TrainBatch(rows, 'cuda')
  desc = solo.struct(counter)
  desc.max_tries = max_tries
  mods._lib.call('ble_replay_sample_f32', ctypes.byref(desc), ctypes.byref(bt.struct), seed, solo.err_flags.data_ptr(),
                 mods.dev.stream_ptr(solo.device))
  return bt


def _counter(value):
  return torch.tensor([value], dtype=torch.int64, device='cuda')


def _rows_equal(grouped, plain, p, rows):
  s = slice(p * rows, (p + 1) * rows)
  for k in ('state', 'next_state', 'ret', 'discount', 'action'):
    assert _same(getattr(grouped, k)[s], getattr(plain, k)), (p, k)
  index = plain.index.clone()
  index[:, 1] = torch.where(index[:, 1] >= 0, index[:, 1] + p * R, index[:, 1])
  assert torch.equal(grouped.index[s], index), p


@pytest.mark.parametrize('start', [0, 2 ** 32 + 5])
@pytest.mark.parametrize('rows', [1, 33])
@pytest.mark.parametrize('horizon', [1, 5])
def test_grouped_sampler_is_each_members_own(mods, horizon, rows, start):
  rp, h = _ring(mods, horizon)
  assert int(rp.count.item()) == STEPS > T                          # the ring has wrapped
  # at least a quarter of every member's windows is valid: with 1 024 tries the plain sampler fails a row with probability < 0.75^1024
  assert all(_valid_share(h, horizon, p) >= 0.25 for p in range(P)), [_valid_share(h, horizon, p) for p in range(P)]
  assert any(_valid_share(h, horizon, p) < 1.0 for p in range(P))
  seeds = mods.qnet_train.member_seeds([7, 2 ** 63 + 11, 9], P, 'cuda')
  counter = _counter(start)
  grouped = _sample_grouped(mods, rp, rows, seeds, counter)
  assert int(counter.item()) == start + 1                           # advanced once, not once per member
  rp.check_errors()
  assert (grouped.index >= 0).all()
  for p in range(P):
    solo = rp.member_buffer(p)
    own = _counter(start)
    plain = _sample_plain(mods, solo, rows, [7, 2 ** 63 + 11, 9][p], own)
    solo.check_errors()
    assert int(own.item()) == start + 1
    _rows_equal(grouped, plain, p, rows)
    cols = grouped.index[p * rows:(p + 1) * rows, 1]
    assert (cols >= p * R).all() and (cols < (p + 1) * R).all()
  # every sampled window is a valid one of the history, and its return is the host's
  idx = grouped.index.cpu().numpy()
  for b, (t, e) in enumerate(idx):
    w = train_host.nstep(h['reward'], h['terminal'], h['episode_end'], t, e, horizon, 0.993)
    assert w is not None and STEPS - T <= t and t + horizon <= STEPS - 1
    assert grouped.ret[b].item() == w[1] and np.array_equal(grouped.state[b, :1099].cpu().numpy(), h['obs'][t, e])


def test_grouped_sampler_through_the_class_and_seeds(mods):
  """VecPopulationReplayBuffer.sample: B rows per member; a member's rows depend on its own seed alone."""
  rp, _ = _ring(mods, 5)
  seeds = mods.qnet_train.member_seeds(40, P, 'cuda')
  assert seeds.tolist() == [40, 41, 42]
  a = {k: getattr(rp.sample(33, seeds, _counter(3)), k).clone() for k in ('index', 'ret')}
  other = seeds.clone()
  other[1] = 99
  b = rp.sample(33, other, _counter(3))
  assert b.batch_size == P * 33
  for p in range(P):
    s = slice(p * 33, (p + 1) * 33)
    assert (torch.equal(a['index'][s], b.index[s]) and _same(a['ret'][s], b.ret[s])) == (p != 1), p
  rp.check_errors()


def test_a_member_without_a_valid_window_fails_alone(mods):
  """Member 1's columns hold a time-limit end at every step: its rows are zeros with index (-1, -1) and the flag; members 0 and 2 draw
  what they draw from the ring without that."""
  rows, horizon = 33, 5
  seeds = mods.qnet_train.member_seeds([7, 8, 9], P, 'cuda')
  clean_rp, _ = _ring(mods, horizon)
  clean = _sample_grouped(mods, clean_rp, rows, seeds, _counter(1))
  clean_rp.check_errors()
  every = LIMITS + [(s, e) for s in range(STEPS) for e in range(R, 2 * R)]
  rp, h = _ring(mods, horizon, limits=every)
  rp.terminal[:, R:2 * R] = 0                                        # (member 1: time-limit ends only)
  got = _sample_grouped(mods, rp, rows, seeds, _counter(1))
  with pytest.raises(RuntimeError):
    rp.check_errors()
  s = slice(rows, 2 * rows)
  assert (got.index[s] == -1).all()
  for k in ('state', 'next_state', 'ret', 'discount', 'action'):
    assert not getattr(got, k)[s].any(), k                          # (zeros, not the NaN the buffers held)
  for p in (0, 2):
    s = slice(p * rows, (p + 1) * rows)
    for k in ('state', 'next_state', 'ret', 'discount', 'action', 'index'):
      assert _same(getattr(got, k)[s], getattr(clean, k)[s]), (p, k)


@pytest.mark.parametrize('steps', [0, 3, 5])
def test_an_empty_ring_behaves_as_the_plain_call(mods, steps):
  """count <= n: no candidate window; every row fails, flagged, and the counter still advances -- the plain call's behaviour."""
  rp, _ = _ring(mods, 5, steps=steps)
  seeds = mods.qnet_train.member_seeds(1, P, 'cuda')
  counter = _counter(0)
  got = _sample_grouped(mods, rp, 7, seeds, counter)
  plain_counter = _counter(0)
  plain = _sample_plain(mods, rp.member_buffer(0), 7, 1, plain_counter)
  assert int(counter.item()) == int(plain_counter.item()) == 1
  assert (got.index == -1).all() and (plain.index == -1).all()
  for k in ('state', 'next_state', 'ret', 'discount', 'action'):
    assert not getattr(got, k).any() and _same(getattr(got, k)[:7], getattr(plain, k)), k
  with pytest.raises(RuntimeError):
    rp.check_errors()


# ---- 4. epsilon-greedy per member -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', [7, 2 ** 32 + 7])
def test_grouped_explore_is_each_members_own(mods, step):
  members, rows = 3, 65
  eps, seed = (0.0, 1.0, 0.5), (3, 2 ** 64 - 2, 17)
  greedy = (torch.arange(members * rows, device='cuda') % 3).to(torch.uint8)
  seeds = mods.qnet_train.member_seeds(seed, members, 'cuda')
  got = mods.qnet_train.explore_grouped(greedy.clone(), eps, seeds, step)
  for p in range(members):
    s = slice(p * rows, (p + 1) * rows)
    own = mods.qnet_train.explore(greedy[s].clone(), eps[p], seed[p], step)
    assert torch.equal(got[s], own), p
  assert torch.equal(got[:rows], greedy[:rows]) and not torch.equal(got[rows:2 * rows], greedy[rows:2 * rows])
  changed = (got[2 * rows:] != greedy[2 * rows:]).sum().item()
  assert 0 < changed < rows and (got < 3).all()
  # a device tensor of rates is read as it stands
  again = mods.qnet_train.explore_grouped(greedy.clone(), torch.tensor(eps, dtype=torch.float32, device='cuda'), seeds, step)
  assert torch.equal(again, got)
  with pytest.raises(ValueError):
    mods.qnet_train.explore_grouped(greedy.clone(), (0.0, 1.5, 0.5), seeds, step)


# ---- 5. P = 1 is the plain entry point; a captured update replays to the eager bytes --------------------------------------------------
def _real_ring(mods, members, rows_per_member, steps=40, capacity=24, seed=1):
  """A VecPopulationReplayBuffer filled by `steps` random-action steps of a real VecBalloonEnv of P * R balloons with a 7-step episode
  limit (time-limit ends inside the ring)."""
  n = members * rows_per_member
  env = mods.balloon_env.VecBalloonEnv(n, seed=seed)
  rp = mods.qnet_train.VecPopulationReplayBuffer(members, rows_per_member, capacity, 5, 0.993)
  g = torch.Generator(device='cuda').manual_seed(seed)
  obs = env.reset()
  clock = torch.zeros(n, dtype=torch.int32, device='cuda')
  for _ in range(steps):
    act = torch.randint(0, 3, (n,), dtype=torch.uint8, device='cuda', generator=g)
    end_mask = (clock + 1 >= 7).to(torch.uint8)
    nxt, reward, terminal = env.step(act, end_mask=end_mask)
    end = terminal | end_mask
    rp.add(obs, act, reward, terminal, end)
    clock = torch.where(end.bool(), torch.zeros_like(clock), clock + 1)
    obs = nxt.clone()
  env.check_errors()
  return rp


def _solo_from_state(mods, tr, p):
  """A solo trainer that continues member p: built on another network, then loaded from member_trainer_state(p)."""
  atoms = tr.num_atoms
  other = _network(mods, tr.num_layers, tr.hidden_units, atoms, seed=900 + p)
  solo = mods.qnet_train.QNetworkTrainer(other, seed=123) if tr.kind == 'quantile' else mods.dqn.DQNTrainer(other, seed=123)
  solo.load_state_dict(tr.member_trainer_state(p))
  return solo


def _state_equal(tr, solo, p, what):
  packed = tr.population.packed_floats
  for name, mine in (('weights', tr.images), ('target', tr.target), ('adam_m', tr.adam_m), ('adam_v', tr.adam_v), ('grad', tr.grad)):
    assert _same(mine[p, :packed], getattr(solo, name)), (what, p, name)
  assert int(tr.adam_step.item()) == int(solo.adam_step.item()) and int(tr.counter.item()) == int(solo.counter.item()), what


@pytest.mark.parametrize('layers,hidden,atoms,kind,rows', [(2, 64, 51, 'quantile', 300), (2, 64, 1, 'dqn_huber', 515)])
def test_one_member_is_the_plain_entry_point_from_a_graph(mods, layers, hidden, atoms, kind, rows):
  rp = _real_ring(mods, 1, 16)
  nets, targets, pop, tr = _population(mods, layers, hidden, atoms, kind, 1, gap=0)
  solo = _solo(mods, nets, targets, tr, 0)
  own = rp.member_buffer(0)
  tr.capture(rp, rows)                                               # (update 1, eager)
  for u in range(1, 4):
    if u > 1:
      tr.train_step(rp, rows)                                        # (updates 2 and 3: replays of the graph)
    loss = solo.train_step(own, rows)
    _compare_member(tr, solo, 0, rows, f'update {u}')
    _state_equal(tr, solo, 0, f'update {u}')
    assert _same(tr.views(rows)['loss'][0], loss)
  tr.check_errors(); rp.check_errors(); solo.check_errors(); own.check_errors()
  assert int(tr.adam_step.item()) == 3


# ---- 6. through the classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,atoms', [('quantile', 51), ('dqn_mse', 1)])
def test_train_step_through_the_classes(mods, kind, atoms):
  """PopulationQTrainer.train_step on a VecPopulationReplayBuffer of a real VecBalloonEnv(2 * 32) against two solo trainers loaded from
  member_trainer_state(p) that sample solo VecReplayBuffers of the ring's column slices: three updates with a sync_target in between,
  eager and captured."""
  members, r, rows = 2, 32, 32
  rp = _real_ring(mods, members, r)
  trainers = {}
  for mode in ('eager', 'captured'):
    _, _, pop, tr = _population(mods, 2, 64, atoms, kind, members)
    solos = [_solo_from_state(mods, tr, p) for p in range(members)] if mode == 'eager' else None
    own = [rp.member_buffer(p) for p in range(members)] if mode == 'eager' else None
    for u in range(3):
      if mode == 'captured' and u == 0:
        loss = tr.capture(rp, rows)
      else:
        loss = tr.train_step(rp, rows)
      if mode == 'eager':
        for p in range(members):
          solo_loss = solos[p].train_step(own[p], rows)
          assert _same(loss.view(members, rows)[p], solo_loss), (u, p)
          _state_equal(tr, solos[p], p, f'update {u}')
      if u == 1:
        tr.sync_target()
        if mode == 'eager':
          for s in solos:
            s.sync_target()
    tr.check_errors()
    trainers[mode] = (pop, tr)
  rp.check_errors()
  (pop_e, e), (pop_c, c) = trainers['eager'], trainers['captured']
  for name in ('target', 'grad', 'adam_m', 'adam_v', 'weights_t', 'adam_step', 'counter'):
    assert _same(getattr(e, name), getattr(c, name)), name
  assert _same(pop_e.images, pop_c.images) and int(e.counter.item()) == 3
  packed = pop_e.packed_floats
  assert not _same(e.target[:, :packed], pop_e.images[:, :packed])   # (one more update since the sync)


# ---- 7. the loop, PBT's two steps, checkpoints, evaluation -----------------------------------------------------------------------------
def _loop_run(mods, capture_graph, **kw):
  members, r = 2, 32
  env = mods.balloon_env.VecBalloonEnv(members * r, seed=1)
  nets = [_network(mods, 2, 64, 51, seed=3 + p) for p in range(members)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  tr = mods.population.PopulationQTrainer(pop, kind='quantile', lr=[1e-4, 3e-4], kappa=[1.0, 0.5], seed=[2, 77])
  rp = mods.qnet_train.VecPopulationReplayBuffer(members, r, 16, 5, 0.993)
  args = dict(num_iterations=1, steps_per_iteration=10, max_episode_length=7, min_replay_history=r * 6, updates_per_step=2,
              target_update_period=12, epsilon=[0.05, 0.3], batch_size=16, capture_graph=capture_graph)
  args.update(kw)
  stats = mods.train_lib.run_population_training_loop_vec(env, tr, rp, **args)
  return pop, tr, rp, stats, nets


def test_loop_eager_and_captured_then_pbt_steps_resume_and_eval(mods):
  pop, tr, rp, stats, nets = _loop_run(mods, False)
  pop_c, tr_c, rp_c, stats_c, _ = _loop_run(mods, True)
  s = stats[0]
  assert len(stats) == 1 and s['updates'] == 10 and s['transitions'] == 640 and int(tr.adam_step.item()) == 10 == int(tr.counter.item())
  assert all(np.isfinite(v) for v in s['member_mean_loss']) and s['member_mean_loss'][0] != s['member_mean_loss'][1]
  assert s['mean_loss'] == pytest.approx(sum(s['member_mean_loss']) / 2, rel=1e-5)
  assert sum(s['member_episodes']) == s['episodes'] >= 64 and len(s['member_mean_return']) == 2 and s['lr'] == tr.lr.tolist()
  assert _same(pop.images, pop_c.images) and stats == stats_c
  for name in tr._TENSORS:
    assert _same(getattr(tr, name), getattr(tr_c, name)), name
  for name in rp._TENSORS:
    assert _same(getattr(rp, name), getattr(rp_c, name)), name
  assert not _same(pop.images[0], torch.from_numpy(nets[0].packed_host).cuda()) and not _same(tr.target, pop.images)
  # the checkpoint: three more updates straight, and from a fresh trainer that loaded the state
  sd = tr.state_dict()
  for u in range(3):
    tr.train_step(rp, 16)
    if u == 0:
      tr.sync_target()
  fresh_pop = mods.population.QNetworkPopulation.from_networks([_network(mods, 2, 64, 51, seed=70 + p) for p in range(2)])
  fresh = mods.population.PopulationQTrainer(fresh_pop, kind='quantile', lr=1.0, kappa=9.0, seed=0)
  fresh.load_state_dict(sd)
  for u in range(3):
    fresh.train_step(rp, 16)
    if u == 0:
      fresh.sync_target()
  assert _same(fresh_pop.images, pop.images)
  for name in tr._TENSORS:
    assert _same(getattr(fresh, name), getattr(tr, name)), name
  # PBT's exploit and explore steps: member 0 becomes member 1 (images, target, moments, weights_t, lr, kappa; not the seed)
  src, dst = torch.tensor([1], device='cuda'), torch.tensor([0], device='cuda')
  tr.copy_members(src, dst)
  for t in (pop.images, tr.target, tr.adam_m, tr.adam_v, tr.weights_t, tr.lr, tr.kappa):
    assert _same(t[0], t[1])
  assert tr.seeds.tolist() == [2, 77]
  tr.scale_hyper('lr', dst, 0.5)
  assert tr.lr.tolist() == [float(np.float32(3e-4) * np.float32(0.5)), float(np.float32(3e-4))]
  with pytest.raises(ValueError):
    tr.scale_hyper('seed', dst, 0.5)
  loss = tr.train_step(rp, 16).view(2, 16)
  assert not _same(loss[0], loss[1]) and not _same(pop.images[0], pop.images[1])       # (their own seeds, their own rates)
  tr.check_errors(); rp.check_errors()
  res = mods.eval_lib.eval_population_vec(pop, mods.suites.EvaluationSuite([0, 1], 20))
  assert len(res) == 2 and all(len(r) == 2 and all(np.isfinite(x.cumulative_reward) for x in r) for r in res)


def test_loop_with_a_pbt_round(mods):
  pop, tr, rp, stats, _ = _loop_run(mods, True, num_iterations=2, ready_every=2, truncation=0.5, perturb=(0.5, 2.0), seed=4)
  assert stats[0]['round'] is None and stats[0]['lineage'] == [0, 1]
  rnd = stats[1]['round']
  assert len(rnd['dst']) == 1 and rnd['src'] != rnd['dst'] and stats[1]['lineage'] == [rnd['src'][0]] * 2
  assert _same(pop.images[0], pop.images[1]) and _same(tr.target[0], tr.target[1]) and _same(tr.kappa[0], tr.kappa[1])
  keep = rnd['src'][0]
  assert stats[1]['lr'][keep] == [float(np.float32(1e-4)), float(np.float32(3e-4))][keep]
  assert stats[1]['lr'][1 - keep] in (float(tr.lr[keep] * np.float32(0.5)), float(tr.lr[keep] * np.float32(2.0)))
  assert tr.seeds.tolist() == [2, 77]


# ---- 8. four members learn the contextual bandit as four solo runs do -------------------------------------------------------------------
def test_four_members_learn_the_bandit_as_four_solo_runs(mods, observations):
  """test_gpu_train.py's contextual bandit (every transition terminal; reward 1 for the right action, which is 0 or 2 as one observation
  feature is below or above its median) with DQN 'mse': four members at four learning rates, each on 64 columns of one ring, against
  four solo DQNTrainers on those columns after 80 updates of 128 rows, byte for byte; the best member clears the solo test's bar
  (greedy action right on >= 90 % of held-out states, mean |q - r| <= 0.2)."""
  qnet, qnet_train = mods.qnet, mods.qnet_train
  x = observations.cpu().numpy()
  std = np.where((x.min(axis=0) >= 0) & (x.max(axis=0) <= 1), x.std(axis=0), 0.0)
  col = int(np.argmax(std))
  label = np.where(x[:, col] > np.median(x[:, col]), 2, 0).astype(np.uint8)
  rng = np.random.default_rng(0)
  perm = rng.permutation(len(x))
  train_i, test_i = perm[:768], perm[768:]
  members, r, steps, rows, updates = 4, 64, 48, 128, 80
  n_env = members * r
  rp = qnet_train.VecPopulationReplayBuffer(members, r, steps, update_horizon=1, gamma=0.99)
  for s in range(steps):
    i = rng.choice(train_i, n_env)
    a = rng.integers(0, 3, n_env).astype(np.uint8)
    rew = (a == label[i]).astype(np.float32)
    rp.add(torch.from_numpy(x[i]).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(rew).cuda(),
           torch.ones(n_env, dtype=torch.uint8, device='cuda'))
  lrs = [3e-4, 1e-3, 3e-3, 1e-2]

  def nets():
    out = []
    for p in range(members):
      params = qnet.init_params('quantile', 7 + p, 2, 64, 1)
      out.append(qnet.QNetwork.from_params(params, num_atoms=1))
    return out
  pop = mods.population.QNetworkPopulation.from_networks(nets())
  tr = mods.population.PopulationQTrainer(pop, kind='dqn_mse', lr=lrs, update_horizon=1, gamma=0.99, seed=5)
  tr.capture(rp, rows)
  for _ in range(updates - 1):
    tr.train_step(rp, rows)
  tr.check_errors(); rp.check_errors()
  for p, net in enumerate(nets()):
    solo = mods.dqn.DQNTrainer(net, loss_type='mse', lr=float(np.float32(lrs[p])), update_horizon=1, gamma=0.99, seed=5 + p)
    own = rp.member_buffer(p)
    for _ in range(updates):
      solo.train_step(own, rows)
    solo.check_errors(); own.check_errors()
    assert _same(pop.images[p, :pop.packed_floats], solo.weights), p
  truth = (np.arange(3)[None, :] == label[test_i][:, None]).astype(np.float64)
  agent = mods.population.VecPopulationAgent(pop, len(test_i))
  q = torch.empty(members * len(test_i), 3, dtype=torch.float32, device='cuda')
  held = torch.from_numpy(x[test_i]).cuda()
  act = agent.act(held.repeat(members, 1), q_values=q).cpu().numpy().reshape(members, -1)
  acc = [float((act[p] == label[test_i]).mean()) for p in range(members)]
  err = [float(np.abs(q.view(members, -1, 3)[p].cpu().numpy() - truth).mean()) for p in range(members)]
  print('bandit: accuracy per member', acc, 'mean |q - r| per member', err)
  best = int(np.argmax(acc))
  assert acc[best] >= 0.9, acc
  assert err[best] <= 0.2, err
