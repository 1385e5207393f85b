"""A population of policies in one batch on the device: ble_qnet_forward_grouped_f32 against each member's own forward, bit
for bit; eval_population_vec against eval_agent_vec member by member; the evolution strategy's kernels against the twin
(tests/es_host.py) -- the noise to the normal-deviate twins' tolerance, everything after the noise bit for bit given the device's own
noise --; ble_qnet_apply_grad_f32 against the train step's own optimiser stage; the ES loop learning a quadratic, deterministically."""
import ctypes

import numpy as np
import pytest
import torch

import es_host
import reset_draws_host as rd
from es_host import LEARN_GENERATIONS, learning_problem

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0, 1), (2, 64, 1), (3, 256, 2), (8, 600, 51)]           # (layers, hidden, atoms)
MEMBERS, ROWS = (1, 2, 5), (1, 31, 32, 33, 129)                       # the edges of a wave's 32 rows and a workgroup's 128
N_MAX = max(MEMBERS) * max(ROWS)


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  import types
  from balloon_learning_environment_amd import _abi, _lib, device, train_lib
  from balloon_learning_environment_amd.agents import actor_critic, evolution, population, qnet, qnet_train
  from balloon_learning_environment_amd.eval import eval_lib, suites
  return types.SimpleNamespace(_abi=_abi, _lib=_lib, dev=device, train_lib=train_lib, actor_critic=actor_critic, evolution=evolution,
                               population=population, qnet=qnet, qnet_train=qnet_train, eval_lib=eval_lib, suites=suites)


def _network(mods, layers, hidden, atoms, seed):
  """An independently initialised network with non-zero biases."""
  params = mods.qnet.init_params('mlp' if atoms == 1 else 'quantile', seed, layers, hidden, atoms)
  rng = np.random.default_rng(1000 + seed)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * 1e-2).astype(np.float32)
  return mods.qnet.QNetwork.from_params(params, num_atoms=atoms)


def _rows(n, stride, seed=1):
  """n observation rows in [0, 1) at a row stride, the padding NaN (never read)."""
  buf = torch.full((n, stride), float('nan'), dtype=torch.float32, device='cuda')
  buf[:, :1099] = torch.from_numpy(np.random.default_rng(seed).random((n, 1099), dtype=np.float32)).cuda()
  return buf[:, :1099] if stride > 1099 else buf


def _scratch_floats(mods, struct, n):
  floats = ctypes.c_int64()
  mods._lib.call('ble_qnet_workspace_f32', ctypes.byref(struct), n, None, ctypes.byref(floats))
  return floats.value


def _plain_forward(mods, net, obs):
  """ble_qnet_forward_f32 of one network: (action, q, logits) as bytes-comparable tensors."""
  net.to_device()
  n = obs.shape[0]
  floats = _scratch_floats(mods, net._struct, n)
  scratch = torch.empty(floats, dtype=torch.float32, device='cuda')
  action = torch.empty(n, dtype=torch.uint8, device='cuda')
  q = torch.empty(n, 3, dtype=torch.float32, device='cuda')
  mods._lib.call('ble_qnet_forward_f32', ctypes.byref(net._struct), obs.data_ptr(), obs.stride(0), scratch.data_ptr(), action.data_ptr(),
                 q.data_ptr(), n, mods.dev.stream_ptr(obs.device))
  ld = floats // (2 * n)
  off = ((net.num_layers - 1) & 1) * n * ld
  return action, q, scratch[off:off + n * ld].view(n, ld)[:, :3 * net.num_atoms].clone()


def _grouped_forward(mods, pop, rows_per_member, obs, pad=64):
  """ble_qnet_forward_grouped_f32 with head Q into outputs that are `pad` rows longer than the batch and filled with sentinels:
  (action, q, logits, untouched) -- untouched: nothing past row P R of an output, nor past the scratch's size, was written."""
  n = pop.members * rows_per_member
  floats = _scratch_floats(mods, pop._net, n)
  scratch = torch.full((floats + pad,), float('nan'), dtype=torch.float32, device='cuda')
  action = torch.full((n + pad,), 255, dtype=torch.uint8, device='cuda')
  q = torch.full((n + pad, 3), float('nan'), dtype=torch.float32, device='cuda')
  desc = mods._abi.BleQnetGroupedF32(pop._net, pop.members, mods._abi.POP_HEAD_Q, pop.member_stride, rows_per_member,
                                     max(obs.stride(0), 1099), obs.data_ptr(), scratch.data_ptr(), action.data_ptr(), q.data_ptr(), None, None)
  mods._lib.call('ble_qnet_forward_grouped_f32', ctypes.byref(desc), mods.dev.stream_ptr(obs.device))
  ld = floats // (2 * n)
  off = ((pop.num_layers - 1) & 1) * n * ld
  untouched = bool((action[n:] == 255).all() and q[n:].isnan().all() and scratch[floats:].isnan().all())
  return action[:n], q[:n], scratch[off:off + n * ld].view(n, ld)[:, :3 * pop.num_atoms], untouched


def _same(a, b):
  """Bitwise equality of two tensors of one dtype (NaN equals NaN of the same bits)."""
  if a.dtype == torch.float32:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
  return torch.equal(a, b)


# ---- 1. the grouped forward = each member's own forward, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize('layers,hidden,atoms', SHAPES)
def test_grouped_forward_is_each_members_own(mods, layers, hidden, atoms):
  nets = [_network(mods, layers, hidden, atoms, seed=p) for p in range(max(MEMBERS))]
  packed = nets[0].packed_host.size
  for stride in (1099, 1104):
    obs = _rows(N_MAX, stride)
    # each member's own forward over every row, once: by the batch-invariance contract a slice of it is the member's forward of the slice
    own = [_plain_forward(mods, net, obs) for net in nets]
    for members in MEMBERS:
      pop = mods.population.QNetworkPopulation.from_networks(nets[:members], member_stride=packed + 128)
      pop.images[:, packed:] = float('nan')                 # between images: never read
      for rows in ROWS:
        n = members * rows
        action, q, logits, untouched = _grouped_forward(mods, pop, rows, obs[:n])
        assert untouched, (members, rows, stride)
        for p in range(members):
          sl = slice(p * rows, (p + 1) * rows)
          for got, want, what in zip((action, q, logits), own[p], ('action', 'q_values', 'logits')):
            assert _same(got[sl], want[sl]), (what, members, rows, stride, p)
        assert not q.isnan().any() and not logits.isnan().any()


def test_grouped_forward_keeps_a_nan_inside_its_member(mods):
  nets = [_network(mods, 3, 256, 2, seed=p) for p in range(3)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  rows = 33
  obs = _rows(3 * rows, 1099).clone()
  clean = [t.clone() for t in _grouped_forward(mods, pop, rows, obs)[:3]]
  obs[rows:2 * rows, 7] = float('nan')                      # one feature of every row of member 1
  dirty = _grouped_forward(mods, pop, rows, obs)[:3]
  for got, want in zip(dirty, clean):
    assert _same(got[:rows], want[:rows]) and _same(got[2 * rows:], want[2 * rows:])
  assert dirty[1][rows:2 * rows].isnan().all()


def test_population_members_and_refusals(mods):
  nets = [_network(mods, 2, 64, 1, seed=p) for p in range(3)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  for p, net in enumerate(nets):
    got = pop.member(p)
    assert all(np.array_equal(a, b) for a, b in zip(got.kernels + got.biases, net.kernels + net.biases))
  pop.set_member(0, nets[2])
  assert np.array_equal(pop.member(0).kernels[0], nets[2].kernels[0])
  with pytest.raises(ValueError):
    mods.population.QNetworkPopulation.from_networks([nets[0], _network(mods, 2, 32, 1, seed=9)])
  with pytest.raises(ValueError):
    pop.set_member(1, _network(mods, 3, 64, 1, seed=9))
  with pytest.raises(ValueError):
    mods.population.VecPopulationAgent(pop, 4, head='actor')             # (one atom)
  agent = mods.population.VecPopulationAgent(pop, 4)
  assert agent.get_name() == 'Population[3 x DQNAgent]'
  with pytest.raises(AssertionError):
    agent.act(_rows(11, 1099))


# ---- 2. the actor head -----------------------------------------------------------------------------------------------------------------
def test_actor_head_is_each_members_greedy_act(mods):
  members, rows = 3, 33
  nets = [_network(mods, 3, 256, 2, seed=p) for p in range(members)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  obs = _rows(members * rows, 1104)
  n = members * rows
  value = torch.full((n,), float('nan'), dtype=torch.float32, device='cuda')
  probs = torch.full((n, 3), float('nan'), dtype=torch.float32, device='cuda')
  agent = mods.population.VecPopulationAgent(pop, rows, head='actor')
  action = agent.act(obs, value=value, probs=probs)
  bare = agent.act(obs)                                       # value and probs are optional
  assert torch.equal(bare, action)
  for p, net in enumerate(nets):
    sl = slice(p * rows, (p + 1) * rows)
    v, pr = torch.empty(rows, dtype=torch.float32, device='cuda'), torch.empty(rows, 3, dtype=torch.float32, device='cuda')
    a = mods.actor_critic.VecActorCriticAgent(net, deterministic=True).act(obs[sl], value=v, probs=pr)
    assert torch.equal(action[sl], a) and _same(value[sl], v) and _same(probs[sl], pr), p


# ---- 3. eval_population_vec ------------------------------------------------------------------------------------------------------------
def test_eval_population_vec_is_eval_agent_vec_per_member(mods):
  nets = [_network(mods, 2, 64, 1, seed=p) for p in range(3)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  suite = mods.suites.EvaluationSuite([0, 1, 2, 3], 30)
  own = [mods.eval_lib.eval_agent_vec(mods.qnet.VecQNetworkAgent(pop.member(p)), suite) for p in range(3)]
  together = mods.eval_lib.eval_population_vec(pop, suite)
  assert together == own                                     # (dataclass equality: every field of every EvaluationResult)
  assert [r.seed for r in together[1]] == [0, 1, 2, 3] and all(r.final_timestep > 0 for m in together for r in m)
  assert mods.eval_lib.eval_population_vec(pop, suite, batch_size=6) == own         # two seeds a batch
  assert mods.eval_lib.eval_population_vec(pop, suite, capture_graph=False) == own


# ---- 4. and 5. the evolution strategy's kernels -----------------------------------------------------------------------------------------
def _inside_mask(mods, net):
  """bool [packed]: the slots of the packed image that hold a parameter."""
  ones = mods.qnet.QNetwork([np.ones_like(k) for k in net.kernels], [np.ones_like(b) for b in net.biases], net.num_atoms)
  return torch.from_numpy(ones.packed_host == 1.0).cuda()


def _device_eps(es, streams, generation):
  """eps_i in the packed layout, i < streams, read back through the gradient kernel: one-hot w, sigma = 1 and a power-of-two number
  of streams make -streams * grad = eps_i exactly."""
  assert es.streams & (es.streams - 1) == 0 and streams <= es.streams
  sigma, es.sigma = es.sigma, 1.0
  out = []
  for i in range(streams):
    es.generation.fill_(generation)
    w = torch.zeros(es.streams, dtype=torch.float32, device='cuda')
    w[i] = 1.0
    out.append((-float(es.streams)) * es.estimate(w).clone())
  es.sigma = sigma
  es.generation.fill_(generation)
  return torch.stack(out)


def _pack_flat(mods, net, flat):
  ks, bs = es_host.unflatten(flat, net.kernels, net.biases)
  return mods.qnet.QNetwork(ks, bs, net.num_atoms).packed_host


@pytest.mark.parametrize('layers,hidden,atoms', [(2, 64, 1), (1, 0, 1)])
@pytest.mark.parametrize('members,antithetic', [(8, True), (3, False)])
def test_perturbation(mods, layers, hidden, atoms, members, antithetic):
  net = _network(mods, layers, hidden, atoms, seed=4)
  seed, generation, sigma = 0x1234567890ABCDEF, 2 ** 32 + 3, 0.02
  es = mods.evolution.ESTrainer(net, members, sigma=sigma, seed=seed, antithetic=antithetic)
  es.generation.fill_(generation)
  es.population.images.fill_(float('nan'))
  images = es.perturb().images
  packed = es.population.packed_floats
  inside = _inside_mask(mods, net)
  assert not images[:, :packed].isnan().any()
  assert (images[:, :packed][:, ~inside].view(torch.int32) == 0).all()                  # the padding is +0.0f
  assert int(es.generation.item()) == generation                                         # (perturb does not advance it)
  # against the twin: pack(theta +- sigma eps) of the logical parameters
  theta = es_host.flatten(net.kernels, net.biases)
  eps = es_host.noise(seed, generation, es.streams, theta.size)
  want = np.stack([_pack_flat(mods, net, row) for row in es_host.population(theta, sigma, eps, antithetic)])
  bound = np.stack([_pack_flat(mods, net, 2.0 ** -22 * (np.abs(theta) + sigma * np.abs(e))) for e in eps])
  bound = np.repeat(bound, 2, axis=0) if antithetic else bound
  got = images[:, :packed].cpu().numpy()
  exact = np.mean(got.view(np.uint32) == want.view(np.uint32))
  print(f'images against the twin: {exact:.5f} bitwise, worst |diff| / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-30)):.3g}')
  # eps is within one float32 step of the twin's (the normal-deviate tolerance), sigma eps and the sum round once each: an image differs
  # by at most 2^-22 (|theta| + sigma |eps|), and 99.9 % of the slots not at all
  assert exact >= 0.999 and np.all(np.abs(got - want) <= bound)
  # given the device's own eps (through the gradient kernel) the images are theta +- fl(sigma eps), bit for bit
  reader = mods.evolution.ESTrainer(net, 8, sigma=sigma, seed=seed)
  dev_eps = _device_eps(reader, es.streams, generation)
  steps = rd.f32_steps(dev_eps[:, inside].cpu().numpy(), np.stack([_pack_flat(mods, net, e) for e in eps])[:, inside.cpu().numpy()])
  assert steps.max() <= 1 and np.mean(steps == 0) >= 0.999
  th = es.weights
  for i in range(es.streams):
    s = sigma * dev_eps[i]
    plus, minus = th + s, th - s
    if antithetic:
      assert _same(images[2 * i, :packed], plus) and _same(images[2 * i + 1, :packed], minus), i
    else:
      assert _same(images[i, :packed], plus), i
  if antithetic:      # eps_0 does not depend on the population's size
    two = mods.evolution.ESTrainer(net, 2, sigma=sigma, seed=seed)
    two.generation.fill_(generation)
    assert _same(two.perturb().images[:2], images[:2])
    other = mods.evolution.ESTrainer(net, 2, sigma=sigma, seed=seed)
    other.generation.fill_(generation + 1)
    assert (other.perturb().images[0, :packed] != images[0, :packed])[inside].float().mean() > 0.99       # generations differ


def test_gradient(mods):
  net = _network(mods, 2, 64, 1, seed=5)
  seed, generation, sigma, pairs = 77, 5, 0.03, 64
  es = mods.evolution.ESTrainer(net, 2 * pairs, sigma=sigma, seed=seed)
  inside = _inside_mask(mods, net)
  eps = _device_eps(es, pairs, generation)                   # [64, packed]; -64 grad of a one-hot w
  assert (eps[:, ~inside] == 0.0).all()                       # (-64 x the gradient's +0.0f padding)
  twin = es_host.noise(seed, generation, 4, 512)             # logical parameters 0 .. 511: the first eight rows of layer 0's kernel
  for i in range(4):
    logical = mods.qnet_train.unpack(es._net, eps[i].cpu().numpy())['params']['Dense_0']['kernel'].ravel()[:512]
    assert rd.f32_steps(logical, twin[i]).max() <= 1
  w = torch.from_numpy(np.random.default_rng(2).standard_normal(pairs).astype(np.float32)).cuda()
  theta = es.weights.cpu().numpy()
  mask = inside.cpu().numpy()
  for wd in (0.0, 0.01):
    es.weight_decay = wd
    es.generation.fill_(generation)
    es.grad.fill_(float('nan'))
    grad = es.estimate(w).cpu().numpy()
    assert int(es.generation.item()) == generation + 1       # exactly one
    want = es_host.gradient(w.cpu().numpy(), eps.cpu().numpy(), sigma, wd, theta)
    assert np.array_equal(grad[mask].view(np.uint32), want[mask].view(np.uint32)), wd
    assert np.all(grad[~mask].view(np.uint32) == 0)          # the padding is +0.0f
  # a captured gradient call advances the generation on every replay, and estimates that generation's gradient
  es.weight_decay = 0.0
  es.generation.fill_(generation)
  graph, _ = mods.dev.capture(es.device, lambda: es.estimate(w))
  assert int(es.generation.item()) == generation             # (recording runs nothing)
  graph.replay()
  first = es.grad.clone()
  graph.replay()
  second = es.grad.clone()
  assert int(es.generation.item()) == generation + 2
  es.generation.fill_(generation + 1)
  assert _same(es.estimate(w), second) and not _same(first, second)
  es.generation.fill_(generation)
  assert _same(es.estimate(w), first)


# ---- 6. ble_qnet_apply_grad_f32 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layers,hidden,atoms', [(2, 64, 1), (8, 600, 51)])
def test_apply_grad_is_the_train_steps_optimiser(mods, layers, hidden, atoms):
  net = _network(mods, layers, hidden, atoms, seed=6)
  rng = np.random.default_rng(3)
  b = 32
  x = rng.random((2 * b, 1099), dtype=np.float32)
  batch = mods.qnet_train.TrainBatch.from_tensors(x[:b], x[b:], rng.standard_normal(b).astype(np.float32), np.full(b, 0.96, np.float32),
                                                  rng.integers(0, 3, b), 'cuda')
  whole = mods.qnet_train.QNetworkTrainer(net, lr=1e-3, eps=1e-6)
  split = mods.evolution.ESTrainer(net, 2, lr=1e-3, adam_eps=1e-6)          # (a QNetworkTrainer with apply_grad())
  for step in range(2):
    whole.train_on_batch(batch, apply_update=True)
    split.train_on_batch(batch, apply_update=False)
    split.apply_grad()
    for name in ('weights', 'weights_t', 'adam_m', 'adam_v', 'adam_step', 'grad'):
      assert _same(getattr(whole, name), getattr(split, name)), (name, step)
  assert int(split.adam_step.item()) == 2 and not _same(whole.weights, whole.target)


# ---- 7. the ES loop learns, deterministically ------------------------------------------------------------------------------------------
def _learn(mods, generations, state=None, before=0):
  theta0, target = learning_problem()
  shape = ([np.zeros((1099, 3), np.float32)], [np.zeros(3, np.float32)])
  net = mods.qnet.QNetwork(*es_host.unflatten(theta0, *shape), 1)
  goal = torch.from_numpy(mods.qnet.QNetwork(*es_host.unflatten(target, *shape), 1).packed_host).cuda()
  es = mods.evolution.ESTrainer(net, 64, sigma=0.05, lr=0.05, seed=0)
  if state is not None:
    es.load_state_dict(state)
  packed = es.population.packed_floats
  start = float(torch.linalg.vector_norm(torch.from_numpy(net.packed_host).cuda().double() - goal.double()))
  half = None
  for g in range(generations):
    images = es.perturb().images[:, :packed]
    es.update(-((images - goal) ** 2).sum(dim=1))
    if g + 1 == before:
      half = es.state_dict()
  return es, float(torch.linalg.vector_norm(es.weights.double() - goal.double())) / start, half


def test_es_learns_a_quadratic_deterministically(mods):
  """P = 64, sigma 0.05, lr 0.05, fitness -|W_p - W*|^2 on a (1, -, 1) network.  The twin (tests/test_es_host.py) is at 0.90 of the
  start after 60 generations -- 32 pairs in 3300 dimensions, and Adam moves a parameter by at most lr a step -- and at 0.15 after 600, so
  the run is 600 generations long; the quarter stands."""
  es, ratio, half = _learn(mods, LEARN_GENERATIONS, before=LEARN_GENERATIONS // 2)
  print(f'distance / start after {LEARN_GENERATIONS} generations: {ratio:.4f}')
  assert ratio < 0.25
  assert int(es.generation.item()) == LEARN_GENERATIONS == int(es.adam_step.item())
  again, ratio2, _ = _learn(mods, LEARN_GENERATIONS)
  resumed, ratio3, _ = _learn(mods, LEARN_GENERATIONS - LEARN_GENERATIONS // 2, state=half)
  for name in ('weights', 'weights_t', 'adam_m', 'adam_v', 'adam_step', 'generation'):
    assert _same(getattr(es, name), getattr(again, name)), name
    assert _same(getattr(es, name), getattr(resumed, name)), name
  assert _same(es.population.images, again.population.images) and ratio == ratio2 == ratio3
  handed = mods.qnet.VecQNetworkAgent(es.network())           # the centre leaves as a QNetwork
  assert handed.act(_rows(4, 1099)).shape == (4,)


# ---- 8. the loop -----------------------------------------------------------------------------------------------------------------------
def test_es_loop_one_generation(mods):
  members, per, steps, first_seed = 4, 2, 20, 11
  es = mods.evolution.ESTrainer(_network(mods, 2, 64, 1, seed=8), members, sigma=0.02, lr=1e-3, seed=3)
  before = es.weights.clone()
  stats = mods.train_lib.run_es_loop_vec(es, num_generations=1, seeds_per_member=per, max_episode_length=steps, first_seed=first_seed,
                                         eval_center_every=1)
  assert len(stats) == 1 and int(es.generation.item()) == 1 and not _same(es.weights, before)
  suite = mods.suites.EvaluationSuite([first_seed, first_seed + 1], steps)
  flights = [mods.eval_lib.eval_agent_vec(mods.qnet.VecQNetworkAgent(es.population.member(p)), suite) for p in range(members)]
  want = np.array([np.float32(np.mean([f.cumulative_reward for f in fl])) for fl in flights], np.float32)
  got = stats[0]['fitness'].cpu().numpy()
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
  assert stats[0]['mean_fitness'] == pytest.approx(float(want.astype(np.float64).mean()), rel=1e-6)
  assert stats[0]['max_fitness'] == float(want.max()) and stats[0]['min_fitness'] == float(want.min())
  flown = sum(f.final_timestep for fl in flights for f in fl)
  assert stats[0]['transitions'] == flown <= members * per * steps
  assert flown == members * per * steps - sum(steps - f.final_timestep for fl in flights for f in fl)
  assert np.isfinite(stats[0]['center_score'])
