"""Prioritized replay and Marco Polo exploration for a population of replay learners (csrc/ble_population_prio.h,
agents/qnet_train.py: VecPopulationPrioritizedReplayBuffer, agents/marco_polo.py: VecPopulationMarcoPoloExploration,
agents/population.py: PopulationQTrainer, train_lib.run_population_training_loop_vec).  The contract is 3t's: member p's part
of a grouped call holds the BYTES the single-learner entry point gives member p's own objects -- a solo VecPrioritizedReplayBuffer of its
R columns with its own tree and max priority, a solo VecMarcoPoloExploration(R, probability[p], seed[p]), a solo QNetworkTrainer /
DQNTrainer loaded from member_trainer_state(p) -- so every comparison below is bitwise and the references are the plain classes."""
import numpy as np
import pytest
import torch

import population_prio_host as pp
import prio_replay_host as ph

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  import types
  from balloon_learning_environment_amd import _abi, _lib, device, train_lib
  from balloon_learning_environment_amd.agents import dqn_agent, marco_polo, population, qnet, qnet_train
  from balloon_learning_environment_amd.env import balloon_env
  return types.SimpleNamespace(_abi=_abi, _lib=_lib, dev=device, train_lib=train_lib, dqn=dqn_agent, marco_polo=marco_polo,
                               population=population, qnet=qnet, qnet_train=qnet_train, balloon_env=balloon_env)


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


_BITS = {torch.float32: torch.int32, torch.float64: torch.int64}


def _same(a, b):
  """Bitwise equality of two tensors of one dtype (NaN equals NaN of the same bits)."""
  assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
  if a.dtype in _BITS:
    return torch.equal(a.contiguous().view(_BITS[a.dtype]), b.contiguous().view(_BITS[a.dtype]))
  return torch.equal(a, b)


def _counter(value):
  return torch.tensor([value], dtype=torch.int64, device='cuda')


def _flags(obj):
  """The flag word, read and cleared."""
  f = int(obj.err_flags.item())
  obj.err_flags.zero_()
  return f


def _trees_are_the_solos(rp, solos, what):
  for p, solo in enumerate(solos):
    assert _same(rp.tree[p], solo.tree), (what, p)
    assert _same(rp.max_priority[p:p + 1], solo.max_priority), (what, p)


def _rows_are_the_solos(grouped, plain, p, rows, r):
  """Rows [p B, (p + 1) B) of a grouped prioritized batch against member p's own: index (column + p R), return, discount, action, both
  observation rows, priority."""
  s = slice(p * rows, (p + 1) * rows)
  for k in ('state', 'next_state', 'ret', 'discount', 'action', 'priority'):
    assert _same(getattr(grouped, k)[s], getattr(plain, k)), (p, k)
  index = plain.index.clone()
  index[:, 1] = torch.where(index[:, 1] >= 0, index[:, 1] + p * r, index[:, 1])
  assert torch.equal(grouped.index[s], index), p


# ---- 1. the trees after every add -------------------------------------------------------------------------------------------------------
def _widen(mods, rp, gap):
  """Moves the buffer's trees into a tensor whose rows lie `gap` doubles apart (member_stride = 2 padded + gap), the gaps NaN: every
  call of the class then hands the raw entry points that stride.  Returns the wide tensor."""
  wide = torch.full((rp.members, 2 * rp.padded + gap), NAN, dtype=torch.float64, device='cuda')
  wide[:, :2 * rp.padded] = rp.tree
  rp.tree = wide[:, :2 * rp.padded]
  rp._tree = mods._abi.BleSumTreeGroupedF64(rp.members, rp.capacity * rp.rows_per_member, rp.padded, 2 * rp.padded + gap, wide.data_ptr(),
                                            rp.max_priority.data_ptr())
  return wide


@pytest.mark.parametrize('members,r,cap,n', [(3, 5, 6, 5), (2, 64, 8, 3), (2, 1025, 7, 5), (1, 65, 12, 5)])
def test_trees_after_every_add_are_the_solos(mods, members, r, cap, n):
  """3 T + n adds of a history with terminals and time-limit ends, two sample + set_priority rounds in between: after every call tree p
  and max_priority[p] are the solo buffer's of member p's columns and the host twin's; the NaN between the trees stays."""
  qt = mods.qnet_train
  steps, rows = 3 * cap + n, 16
  h = ph.history(steps, members * r, 40 + members, obs=False)
  obs = torch.rand(members * r, 1099, device='cuda')
  rp = qt.VecPopulationPrioritizedReplayBuffer(members, r, cap, n, 0.993)
  wide = _widen(mods, rp, 5)
  solos = [qt.VecPrioritizedReplayBuffer(r, cap, n, 0.993) for _ in range(members)]
  twin = pp.PopulationTrees(members, r, cap, n)
  seeds = qt.member_seeds([7, 2 ** 63 + 11, 9][:members], members, 'cuda')
  rng = np.random.default_rng(2)
  rounds = 0
  for s in range(steps):
    dev_step = {k: torch.from_numpy(h[k][s]).cuda() for k in ('action', 'reward', 'terminal', 'episode_end')}
    rp.add(obs, *[dev_step[k] for k in ('action', 'reward', 'terminal', 'episode_end')])
    for p, solo in enumerate(solos):
      cols = pp.member_columns(p, r)
      solo.add(obs[cols], *[dev_step[k][cols] for k in ('action', 'reward', 'terminal', 'episode_end')])
    twin.add(h, s)
    if s in (cap + n, 2 * cap + n):
      rounds += 1
      bt = rp.sample(rows, seeds, _counter(s))
      loss = torch.from_numpy((rng.random(members * rows) * 4).astype(np.float32)).cuda()
      weighted = rp.set_priority(bt, loss)
      assert (bt.index >= 0).all()
      for p, solo in enumerate(solos):
        own = solo.sample(rows, int(seeds[p].item()), _counter(s))
        _rows_are_the_solos(bt, own, p, rows, r)
        sl = slice(p * rows, (p + 1) * rows)
        assert _same(weighted[sl], solo.set_priority(own, loss[sl].clone())), (s, p)
        idx = own.index.cpu().numpy()
        assert not twin.trees[p].set_priority((idx[:, 0] % cap) * r + idx[:, 1], loss[sl].cpu().numpy())
      assert _flags(rp) == 0 and all(_flags(solo) == 0 for solo in solos)
    _trees_are_the_solos(rp, solos, s)
    assert np.array_equal(rp.tree.cpu().numpy(), twin.nodes()), s
    assert np.array_equal(rp.max_priority.cpu().numpy(), twin.max_priority()), s
  assert rounds == 2 and (twin.max_priority() > 1.0).all()
  assert torch.isnan(wide[:, 2 * rp.padded:]).all()                   # the doubles between the trees were never written
  assert (rp.tree[:, 1] > 0).all()
  lv = rp.leaf_priorities()
  assert lv.shape == (members, cap, r) and np.array_equal(lv.cpu().numpy(), np.stack([t.leaf_view() for t in twin.trees]))
  # member_buffer(p): the solo of member p's columns, tree and maximum copied in
  for p, solo in enumerate(solos):
    copy = rp.member_buffer(p)
    for k in ('action', 'reward', 'terminal', 'episode_end', 'tree', 'max_priority', 'count'):
      assert _same(getattr(copy, k), getattr(solo, k)), (p, k)
    assert copy.cursor == solo.cursor == steps and copy.prioritized


# ---- 2. the grouped prioritized batch ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  return ph.build_replay_draws(tmp_path_factory.mktemp('rpd'))


@pytest.fixture(scope='module')
def draw_case(mods, draws):
  """pp.POP_DRAW_CASE on the device: 40 adds into 12 rows of 3 x 65 columns, the device trees equal to the twins', then the crafted
  priorities copied in and the solos taken.  The precondition -- for every member and row the query and its two fp64 neighbours walk to
  one leaf -- is asserted here for every batch size and counter of the case (on the CPU: test_population_prio_host.py)."""
  c = pp.POP_DRAW_CASE
  h = pp.pop_draw_case_history()
  fed, crafted = pp.pop_draw_case_trees(h)
  leaves = {}
  for b in c['batches']:
    for counter in c['counters']:
      for p in range(c['members']):
        leaf, split = pp.pop_draw_case_leaves(draws, crafted, p, b, counter)
        assert not split, (p, b, counter, split)
        leaves[p, b, counter] = leaf
  rp = mods.qnet_train.VecPopulationPrioritizedReplayBuffer(c['members'], c['rows'], c['capacity'], c['horizon'], 0.993)
  for s in range(c['steps']):
    rp.add(*[torch.from_numpy(h[k][s]).cuda() for k in ('obs', 'action', 'reward', 'terminal', 'episode_end')])
  assert np.array_equal(rp.tree.cpu().numpy(), fed.nodes())
  rp.tree.copy_(torch.from_numpy(crafted.nodes()))
  assert np.array_equal(rp.leaf_priorities().cpu().numpy(), np.stack([t.leaf_view() for t in crafted.trees]))
  solos = [rp.member_buffer(p) for p in range(c['members'])]
  return rp, solos, h, crafted, leaves


@pytest.mark.parametrize('counter', pp.POP_DRAW_CASE['counters'])
@pytest.mark.parametrize('b', pp.POP_DRAW_CASE['batches'])
def test_grouped_prioritized_batch_is_each_members_own(mods, draw_case, b, counter):
  rp, solos, h, crafted, leaves = draw_case
  c = pp.POP_DRAW_CASE
  members, r, cap = c['members'], c['rows'], c['capacity']
  seeds = mods.qnet_train.member_seeds(list(c['seeds']), members, 'cuda')
  ctr = _counter(counter)
  got = rp.sample(b, seeds, ctr)
  assert int(ctr.item()) == counter + 1                             # advanced once, not once per member
  assert got.batch_size == members * b and got.priority.shape == (members * b,)
  flags = 0
  for p, solo in enumerate(solos):
    own_ctr = _counter(counter)
    own = solo.sample(b, c['seeds'][p], own_ctr)
    assert int(own_ctr.item()) == counter + 1
    _rows_are_the_solos(got, own, p, b, r)
    flags |= _flags(solo)
    # ... and the twin's walk from the host's Philox uniforms
    idx = got.index[p * b:(p + 1) * b].cpu().numpy()
    assert ((idx[:, 1] >= p * r) & (idx[:, 1] < (p + 1) * r)).all()
    leaf = (idx[:, 0] % cap) * r + idx[:, 1] - p * r
    assert np.array_equal(leaf, leaves[p, b, counter]), p
    tree = crafted.trees[p]
    assert np.array_equal(got.priority[p * b:(p + 1) * b].cpu().numpy(), tree.nodes[tree.P + leaf].astype(np.float32))
    t, e = idx[:, 0], idx[:, 1]
    assert np.array_equal(got.state[p * b:(p + 1) * b, :1099].cpu().numpy(), h['obs'][t, e])
    assert np.array_equal(got.action[p * b:(p + 1) * b].cpu().numpy(), h['action'][t, e])
  assert _flags(rp) == flags == 0


# ---- 3. isolation -----------------------------------------------------------------------------------------------------------------------
def _small_ring(mods, members, r, cap, n, steps, blocked=None, seed=8):
  """A ring of `steps` adds of a random history; member `blocked`'s columns end (without a terminal) at every step."""
  h = ph.history(steps, members * r, seed)
  if blocked is not None:
    cols = pp.member_columns(blocked, r)
    h['terminal'][:, cols] = 0
    h['episode_end'][:, cols] = 1
  rp = mods.qnet_train.VecPopulationPrioritizedReplayBuffer(members, r, cap, n, 0.993)
  for s in range(steps):
    rp.add(*[torch.from_numpy(h[k][s]).cuda() for k in ('obs', 'action', 'reward', 'terminal', 'episode_end')])
  return rp


def test_a_member_with_an_empty_tree_fails_alone(mods):
  members, r, cap, n, rows = 3, 5, 12, 5, 33
  seeds = mods.qnet_train.member_seeds([7, 8, 9], members, 'cuda')
  clean_rp = _small_ring(mods, members, r, cap, n, 30)
  clean = clean_rp.sample(rows, seeds, _counter(1))
  clean = {k: getattr(clean, k).clone() for k in ('state', 'next_state', 'ret', 'discount', 'action', 'index', 'priority')}
  assert _flags(clean_rp) == 0
  rp = _small_ring(mods, members, r, cap, n, 30, blocked=1)
  assert not rp.tree[1].any() and (rp.tree[0, 1] > 0) and (rp.tree[2, 1] > 0)
  bt = rp.batch_buffers(rows)
  for t in (bt.state, bt.next_state, bt.ret, bt.discount, bt.priority):
    t.fill_(NAN)
  got = rp.sample(rows, seeds, _counter(1))
  assert _flags(rp) == mods._lib.FLAG_REPLAY_EMPTY
  s = slice(rows, 2 * rows)
  assert (got.index[s] == -1).all()
  for k in ('state', 'next_state', 'ret', 'discount', 'action', 'priority'):
    assert not getattr(got, k)[s].any(), k                          # (zeros, not the NaN the buffers held)
  for p in (0, 2):
    s = slice(p * rows, (p + 1) * rows)
    for k in clean:
      assert _same(getattr(got, k)[s], clean[k][s]), (p, k)
  # every member against its solo, the failed one and its flag included
  flags = 0
  for p in range(members):
    solo = rp.member_buffer(p)
    own = solo.sample(rows, 7 + p, _counter(1))
    _rows_are_the_solos(got, own, p, rows, r)
    flags |= _flags(solo)
  assert flags == mods._lib.FLAG_REPLAY_EMPTY
  # set_priority on that batch: member 1's rows are skipped and report 0, its tree stays empty
  loss = torch.rand(members * rows, device='cuda')
  solos = [rp.member_buffer(p) for p in range(members)]
  weighted = rp.set_priority(got, loss).clone()
  for p, solo in enumerate(solos):
    own = solo.sample(rows, 7 + p, _counter(1))
    sl = slice(p * rows, (p + 1) * rows)
    assert _same(weighted[sl], solo.set_priority(own, loss[sl].clone())), p
  _trees_are_the_solos(rp, solos, 'after set_priority')
  assert not rp.tree[1].any() and not weighted[rows:2 * rows].any() and _flags(rp) == 0


@pytest.mark.parametrize('steps', [0, 3, 5])
def test_an_entirely_empty_ring_behaves_as_the_plain_call(mods, steps):
  members, r, rows = 3, 5, 7
  rp = _small_ring(mods, members, r, 12, 5, steps)
  assert not rp.tree.any()
  seeds = mods.qnet_train.member_seeds(1, members, 'cuda')
  ctr = _counter(0)
  got = rp.sample(rows, seeds, ctr)
  assert int(ctr.item()) == 1 and (got.index == -1).all() and not got.priority.any()
  for p in range(members):
    solo = rp.member_buffer(p)
    _rows_are_the_solos(got, solo.sample(rows, 1 + p, _counter(0)), p, rows, r)
    assert _flags(solo) == mods._lib.FLAG_REPLAY_EMPTY
  with pytest.raises(RuntimeError):
    rp.check_errors()


# ---- 4. set_priority --------------------------------------------------------------------------------------------------------------------
SP_R, SP_T, SP_N = 40, 40, 2                                         # 1 600 leaves per member: a batch of 1 025 distinct ones fits


@pytest.fixture(scope='module')
def sp_rings(mods):
  """{P: (history steps, a ring of P x 40 columns after 45 adds)}; a test works on a copy (load_state_dict)."""
  out = {}
  for members in (2, 3):
    steps = SP_T + 5
    h = ph.history(steps, members * SP_R, 60 + members, obs=False)
    obs = torch.zeros(members * SP_R, 1099, device='cuda')
    rp = mods.qnet_train.VecPopulationPrioritizedReplayBuffer(members, SP_R, SP_T, SP_N, 0.993)
    for s in range(steps):
      rp.add(obs, *[torch.from_numpy(h[k][s]).cuda() for k in ('action', 'reward', 'terminal', 'episode_end')])
    out[members] = (steps, rp)
  return out


def _crafted_rows(members, b, hot, steps, seed):
  """index [P, B, 2] (member-local columns), priority and loss [P, B]: distinct leaves per member, then the special rows."""
  rng = np.random.default_rng(seed)
  index = np.zeros((members, b, 2), np.int64)
  for p in range(members):
    leaves = rng.permutation(SP_T * SP_R)[:b]
    row, col = leaves // SP_R, leaves % SP_R
    index[p, :, 0] = ph.newest_step(steps - 1, SP_T, row)
    index[p, :, 1] = col
  priority = (0.1 + 1.9 * rng.random((members, b))).astype(np.float32)
  loss = (4 * rng.random((members, b))).astype(np.float32)
  for p in range(members):
    priority[p, hot[p]] = 1e-6                                       # the largest importance weight of member p
  return index, priority, loss


@pytest.mark.parametrize('members,b,hot', [(3, 33, (0, 16, 32)), (2, 1025, (63, 64)), (2, 1025, (1024, 0))])
def test_set_priority_is_each_members_own(mods, sp_rings, members, b, hot):
  qt = mods.qnet_train
  steps, base = sp_rings[members]
  rp = qt.VecPopulationPrioritizedReplayBuffer(members, SP_R, SP_T, SP_N, 0.993)
  rp.load_state_dict(base.state_dict())
  assert _same(rp.tree, base.tree) and (rp.tree[:, 1] > 0).all()
  index, priority, loss = _crafted_rows(members, b, hot, steps, 70 + b)
  free = [i for i in range(2, 31) if all(i != x for x in hot)]       # rows for the special cases, none a hot row
  dup_a, dup_b, tri_a, tri_b, tri_c, same_0, same_1, fail_a, fail_b, foreign_0, foreign_1, nan_row, neg_row = free[:13]
  # a duplicate and a triple inside member 0: the later row wins
  index[0, dup_b] = index[0, dup_a]
  index[0, tri_b] = index[0, tri_c] = index[0, tri_a]
  # the same leaf number in members 0 and 1 in one call (a leaf no other row of either holds)
  held = lambda p: set(((index[p, :, 0] % SP_T) * SP_R + index[p, :, 1]).tolist())
  shared = min(set(range(SP_T * SP_R)) - held(0) - held(1))
  index[0, same_0] = index[1, same_1] = (ph.newest_step(steps - 1, SP_T, shared // SP_R), shared % SP_R)
  # failed rows; one would hold its member's largest weight (priority 0: w = 1e5)
  for p in range(members):
    index[p, fail_a] = index[p, fail_b] = -1
    priority[p, fail_a], priority[p, fail_b] = 0.0, 0.5
  # NaN and negative losses in member 1 only
  loss[1, nan_row], loss[1, neg_row] = NAN, -1.0
  before = rp.tree.clone()
  # the grouped batch (the index's column + p R); a row of member 0 in member 1's columns and one of member 1 in member 0's
  grouped_index = index.copy()
  for p in range(members):
    valid = grouped_index[p, :, 0] >= 0
    grouped_index[p, valid, 1] += p * SP_R
  grouped_index[0, foreign_0, 1] = SP_R + 3
  grouped_index[1, foreign_1, 1] = 3
  bt = qt.TrainBatch(members * b, 'cuda', True)
  bt.index.copy_(torch.from_numpy(grouped_index.reshape(-1, 2)))
  bt.priority.copy_(torch.from_numpy(priority.reshape(-1)))
  dloss = torch.from_numpy(loss.reshape(-1)).cuda()
  solos = [rp.member_buffer(p) for p in range(members)]
  weighted = rp.set_priority(bt, dloss).clone()
  flags = 0
  for p, solo in enumerate(solos):
    own = qt.TrainBatch(b, 'cuda', True)
    mine = grouped_index[p].copy()
    valid = mine[:, 0] >= 0
    mine[valid, 1] -= p * SP_R                                       # (the foreign rows fall outside [0, R) on either side)
    own.index.copy_(torch.from_numpy(mine))
    own.priority.copy_(torch.from_numpy(priority[p]))
    solo_weighted = solo.set_priority(own, torch.from_numpy(loss[p]).cuda())
    assert _same(weighted[p * b:(p + 1) * b], solo_weighted), p
    flags |= _flags(solo)
  _trees_are_the_solos(rp, solos, 'set_priority')
  assert _flags(rp) == flags == mods._lib.FLAG_REPLAY_PRIORITY
  # what the rows mean, stated once on the grouped result
  leaf = lambda p, row: rp.padded + (index[p, row, 0] % SP_T) * SP_R + index[p, row, 1]
  value = lambda p, row: float(np.sqrt(np.float32(loss[p, row]) + np.float32(1e-10)))
  assert rp.tree[0, leaf(0, dup_a)].item() == value(0, dup_b) and rp.tree[0, leaf(0, tri_a)].item() == value(0, tri_c)
  assert rp.tree[0, leaf(0, same_0)].item() == value(0, same_0) and rp.tree[1, leaf(1, same_1)].item() == value(1, same_1)
  assert leaf(0, same_0) == leaf(1, same_1) and value(0, same_0) != value(1, same_1)
  for p, row in ((0, foreign_0), (1, foreign_1), (1, nan_row), (1, neg_row)):
    assert rp.tree[p, leaf(p, row)].item() == before[p, leaf(p, row)].item(), (p, row)
  w = weighted.view(members, b)
  assert not w[:, fail_a].any() and not w[:, fail_b].any()
  for p in range(members):                                           # the hot row has weight 1: it reports its loss
    assert w[p, hot[p]].item() == loss[p, hot[p]]
  assert (rp.max_priority.cpu().numpy() >= 1.0).all() and len(set(rp.max_priority.tolist())) == members


# ---- 5. Marco Polo ----------------------------------------------------------------------------------------------------------------------
MP_STATE = ('phase_clock', 'walk_clock', 'exploratory_episode', 'exploratory_phase', 'target')


@pytest.mark.parametrize('start', [0, 2 ** 32 - 3])
def test_grouped_marco_polo_is_each_members_own(mods, start):
  """(P, R) = (3, 65), probabilities (0, 1, 0.5), 130 calls: both phase flips (80 and 40 steps) occur in the lanes no episode end
  reaches.  Actions and the five state tensors per slice after every call against solos built before the run; a state_dict resume."""
  mp = mods.marco_polo
  members, r, calls, resume_at = 3, 65, 130, 50
  n = members * r
  probs, seed = (0.0, 1.0, 0.5), (3, 2 ** 64 - 2, 17)
  seeds = mods.qnet_train.member_seeds(seed, members, 'cuda')
  g = torch.Generator(device='cuda').manual_seed(5)
  inputs = []
  for k in range(calls):
    begin = torch.ones(n, dtype=torch.uint8, device='cuda') if k == 0 else \
        (torch.rand(n, device='cuda', generator=g) < 0.004).to(torch.uint8)
    inputs.append((torch.rand(n, 4, device='cuda', generator=g), torch.randint(0, 3, (n,), dtype=torch.uint8, device='cuda', generator=g),
                   begin))
  grouped = mp.VecPopulationMarcoPoloExploration(members, r, probs, seeds)
  grouped.step.fill_(start)
  assert grouped.seeds.data_ptr() != seeds.data_ptr() and _same(grouped.seeds, seeds)
  solos = [grouped.member(p) for p in range(members)]
  for p, solo in enumerate(solos):
    assert (solo.num_envs, solo.probability, solo.seed) == (r, probs[p], seed[p]) and int(solo.step.item()) == start
  survivors = torch.ones(n, dtype=torch.bool, device='cuda')
  saw = {'explore': False, 'back': False}
  taken, checkpoint = [], None
  for k, (obs, agent, begin) in enumerate(inputs):
    if k == resume_at:
      checkpoint = grouped.state_dict()
    if k > 0:
      survivors &= ~begin.bool()
    got = grouped(obs, agent.clone(), begin)
    taken.append(got.clone())
    assert int(grouped.step.item()) == start + k + 1                # advanced once per call
    for p, solo in enumerate(solos):
      s = slice(p * r, (p + 1) * r)
      own = solo(obs[s], agent[s].clone(), begin[s])
      assert torch.equal(got[s], own), (k, p)
      for name in MP_STATE:
        assert _same(getattr(grouped, name)[s], getattr(solo, name)), (k, p, name)
      assert int(solo.step.item()) == start + k + 1
    lanes = survivors[r:2 * r] & grouped.exploratory_episode[r:2 * r].bool()
    phase = grouped.exploratory_phase[r:2 * r][lanes]
    if k == 100:
      saw['explore'] = bool(lanes.any()) and bool(phase.all())       # 80 RL steps, then the random walk
    if k == 125:
      saw['back'] = bool(lanes.any()) and not bool(phase.any())      # ... 40 steps of it, then RL again
  assert saw == {'explore': True, 'back': True}
  assert not grouped.exploratory_episode[:r].any() and grouped.exploratory_episode[r:2 * r].all()
  mixed = grouped.exploratory_episode[2 * r:]
  assert mixed.any() and not mixed.all()
  assert any(not torch.equal(t, a) for t, (_, a, _) in zip(taken, inputs))       # (the walk took some actions over)
  # resume: a fresh explorer of other probabilities and seeds, loaded from the checkpoint, repeats calls 50 .. 129
  fresh = mp.VecPopulationMarcoPoloExploration(members, r, 0.3, 99)
  fresh.load_state_dict(checkpoint)
  for k in range(resume_at, calls):
    obs, agent, begin = inputs[k]
    assert torch.equal(fresh(obs, agent.clone(), begin), taken[k]), k
  for name in MP_STATE + ('step', 'probability', 'seeds'):
    assert _same(getattr(fresh, name), getattr(grouped, name)), name
  with pytest.raises(ValueError):
    mp.VecPopulationMarcoPoloExploration(members, r, (0.0, 1.5, 0.5), seeds)
  with pytest.raises(ValueError):
    mp.VecPopulationMarcoPoloExploration(members, r, (0.0, 0.5), seeds)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------
def _network(mods, layers, hidden, atoms, seed):
  """An independently initialised network with non-zero biases."""
  params = mods.qnet.init_params('quantile', seed, layers, hidden, atoms)
  rng = np.random.default_rng(1000 + seed)
  for leaf in params['params'].values():
    leaf['bias'] = (rng.standard_normal(leaf['bias'].shape) * 1e-2).astype(np.float32)
  return mods.qnet.QNetwork.from_params(params, num_atoms=atoms)


def _trainer(mods, atoms, kind, members):
  nets = [_network(mods, 2, 64, atoms, seed=11 + p) for p in range(members)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  p = np.arange(members)
  tr = mods.population.PopulationQTrainer(pop, kind=kind, seed=5, lr=1e-3 * 1.5 ** p, kappa=0.25 + 0.25 * p)
  for q in range(members):                                           # a target that differs from the online image
    tr.target[q, :pop.packed_floats] = torch.from_numpy(_network(mods, 2, 64, atoms, seed=51 + q).packed_host).cuda()
  return pop, tr


def _solo_from_state(mods, tr, p):
  """A solo trainer that continues member p: built on another network, then loaded from member_trainer_state(p)."""
  other = _network(mods, tr.num_layers, tr.hidden_units, tr.num_atoms, seed=900 + p)
  solo = mods.qnet_train.QNetworkTrainer(other, seed=123) if tr.kind == 'quantile' else mods.dqn.DQNTrainer(other, seed=123)
  solo.load_state_dict(tr.member_trainer_state(p))
  return solo


def _solo_step(solo, own, rows):
  """One prioritized update of a solo trainer on its own buffer: QNetworkTrainer.train_step; for a DQNTrainer -- whose train_step refuses
  a prioritized buffer, JaxDQNAgent having no priority rule -- the same three single-learner calls in the same order."""
  if type(solo).__name__ == 'QNetworkTrainer':
    return solo.train_step(own, rows)
  batch = own.sample(rows, solo.seed, solo.counter)
  return own.set_priority(batch, solo.train_on_batch(batch))


def _state_equal(tr, solo, p, what):
  packed = tr.population.packed_floats
  for name, mine in (('weights', tr.images), ('target', tr.target), ('adam_m', tr.adam_m), ('adam_v', tr.adam_v), ('grad', tr.grad)):
    assert _same(mine[p, :packed], getattr(solo, name)), (what, p, name)
  assert int(tr.adam_step.item()) == int(solo.adam_step.item()) and int(tr.counter.item()) == int(solo.counter.item()), what


@pytest.fixture(scope='module')
def real_rings(mods):
  """{P: a VecPopulationPrioritizedReplayBuffer filled by 40 random-action steps of a real VecBalloonEnv of P x 32 balloons with a
  7-step episode limit (time-limit ends inside the ring)}; a test works on a copy (load_state_dict)."""
  out = {}
  for members in (1, 2):
    n = members * 32
    env = mods.balloon_env.VecBalloonEnv(n, seed=1)
    rp = mods.qnet_train.VecPopulationPrioritizedReplayBuffer(members, 32, 24, 5, 0.993)
    g = torch.Generator(device='cuda').manual_seed(1)
    obs = env.reset()
    clock = torch.zeros(n, dtype=torch.int32, device='cuda')
    for _ in range(40):
      act = torch.randint(0, 3, (n,), dtype=torch.uint8, device='cuda', generator=g)
      end_mask = (clock + 1 >= 7).to(torch.uint8)
      nxt, reward, terminal = env.step(act, end_mask=end_mask)
      end = terminal | end_mask
      rp.add(obs, act, reward, terminal, end)
      clock = torch.where(end.bool(), torch.zeros_like(clock), clock + 1)
      obs = nxt.clone()
    env.check_errors()
    out[members] = rp
  return out


def _copy_of(mods, rp):
  copy = mods.qnet_train.VecPopulationPrioritizedReplayBuffer(rp.members, rp.rows_per_member, rp.capacity, rp.update_horizon, rp.gamma)
  copy.load_state_dict(rp.state_dict())
  for k in rp._TENSORS:
    assert _same(getattr(copy, k), getattr(rp, k)), k
  assert copy.cursor == rp.cursor and int(copy.count.item()) == rp.cursor
  return copy


@pytest.mark.parametrize('members', [2, 1])
@pytest.mark.parametrize('kind,atoms', [('quantile', 51), ('dqn_mse', 1)])
def test_train_step_is_each_members_own_prioritized_update(mods, real_rings, kind, atoms, members):
  """sample -> grouped update -> set_priority against solo trainers from member_trainer_state(p) on member_buffer(p): three updates
  with a sync_target in between, eager and from a captured graph replayed twice -- weights, moments, trees, maxima, returned losses.
  One member: the plain prioritized train_step."""
  rows = 32
  results = {}
  for mode in ('eager', 'captured'):
    rp = _copy_of(mods, real_rings[members])
    assert (rp.tree[:, 1] > 0).all()
    pop, tr = _trainer(mods, atoms, kind, members)
    solos = [_solo_from_state(mods, tr, p) for p in range(members)]
    own = [rp.member_buffer(p) for p in range(members)]
    for u in range(3):
      loss = tr.capture(rp, rows) if (mode == 'captured' and u == 0) else tr.train_step(rp, rows)
      assert loss.shape == (members * rows,)
      for p in range(members):
        solo_loss = _solo_step(solos[p], own[p], rows)
        assert _same(loss.view(members, rows)[p], solo_loss), (mode, u, p)
        _state_equal(tr, solos[p], p, f'{mode} update {u}')
      _trees_are_the_solos(rp, own, f'{mode} update {u}')
      if u == 1:
        tr.sync_target()
        for s in solos:
          s.sync_target()
    tr.check_errors(); rp.check_errors()
    for s, o in zip(solos, own):
      s.check_errors(); o.check_errors()
    assert int(tr.counter.item()) == int(tr.adam_step.item()) == 3
    assert (rp.max_priority != 1.0).any() or kind != 'quantile'
    results[mode] = (pop.images.clone(), rp.tree.clone(), rp.max_priority.clone(), loss.clone())
  for a, b in zip(results['eager'], results['captured']):
    assert _same(a, b)
  assert not _same(results['eager'][1], real_rings[members].tree)    # (set_priority wrote the trees)
  # a plain prioritized buffer, or another member count, is refused as before
  with pytest.raises(ValueError, match='PopulationQTrainer samples a VecPopulationReplayBuffer'):
    tr.train_step(own[0], 16)
  if members == 2:
    with pytest.raises(ValueError, match='PopulationQTrainer samples a VecPopulationReplayBuffer'):
      tr.train_step(real_rings[1], 16)


# ---- 7. the loop ------------------------------------------------------------------------------------------------------------------------
def _loop_run(mods, capture_graph):
  members, r = 2, 32
  env = mods.balloon_env.VecBalloonEnv(members * r, seed=1)
  nets = [_network(mods, 2, 64, 51, seed=3 + p) for p in range(members)]
  pop = mods.population.QNetworkPopulation.from_networks(nets)
  tr = mods.population.PopulationQTrainer(pop, kind='quantile', lr=[1e-4, 3e-4], kappa=[1.0, 0.5], seed=[2, 77])
  rp = mods.qnet_train.VecPopulationPrioritizedReplayBuffer(members, r, 16, 5, 0.993)
  explorer = mods.marco_polo.VecPopulationMarcoPoloExploration(members, r, [1.0, 0.8], tr.seeds)
  # quantile.gin's recipe: prioritized replay, Marco Polo, epsilon 0.  90 steps: the exploratory episodes reach their random walk
  stats = mods.train_lib.run_population_training_loop_vec(
      env, tr, rp, num_iterations=1, steps_per_iteration=90, min_replay_history=r * 80, updates_per_step=2, target_update_period=12,
      epsilon=0.0, batch_size=16, capture_graph=capture_graph, exploration=explorer)
  return pop, tr, rp, explorer, stats


def test_loop_with_prioritized_replay_and_the_explorer_eager_captured_and_resumed(mods):
  pop, tr, rp, ex, stats = _loop_run(mods, False)
  pop_c, tr_c, rp_c, ex_c, stats_c = _loop_run(mods, True)
  s = stats[0]
  assert s['updates'] == 22 == int(tr.adam_step.item()) == int(tr.counter.item()) and s['transitions'] == 90 * 64
  assert all(np.isfinite(v) for v in s['member_mean_loss'])
  assert int(ex.step.item()) == 90 and ex.exploratory_phase.any() and ex.exploratory_episode[:32].all()
  assert (rp.max_priority != 1.0).all() and (rp.tree[:, 1] > 0).all()
  assert _same(pop.images, pop_c.images)
  np.testing.assert_equal(stats, stats_c)                            # (NaN, the mean return of no finished episode, equals NaN)
  for name in tr._TENSORS:
    assert _same(getattr(tr, name), getattr(tr_c, name)), name
  for name in rp._TENSORS:
    assert _same(getattr(rp, name), getattr(rp_c, name)), name
  for name in ex._STATE:
    assert _same(getattr(ex, name), getattr(ex_c, name)), name
  # the checkpoint: three more updates and explorer calls straight, and from fresh objects that loaded the state
  sd_tr, sd_rp, sd_ex = tr.state_dict(), rp.state_dict(), ex.state_dict()
  assert 'tree' in sd_rp and 'max_priority' in sd_rp and sd_rp['members'] == 2
  obs = torch.rand(64, 1099, device='cuda')
  begin = torch.zeros(64, dtype=torch.uint8, device='cuda')

  def more(trainer, replay, explorer):
    acts = []
    for u in range(3):
      trainer.train_step(replay, 16)
      if u == 0:
        trainer.sync_target()
      acts.append(explorer(obs, torch.ones(64, dtype=torch.uint8, device='cuda'), begin).clone())
    return acts
  straight = more(tr, rp, ex)
  fresh_pop = mods.population.QNetworkPopulation.from_networks([_network(mods, 2, 64, 51, seed=70 + p) for p in range(2)])
  fresh = mods.population.PopulationQTrainer(fresh_pop, kind='quantile', lr=1.0, kappa=9.0, seed=0)
  fresh.load_state_dict(sd_tr)
  fresh_rp = mods.qnet_train.VecPopulationPrioritizedReplayBuffer(2, 32, 16, 5, 0.993)
  fresh_rp.load_state_dict(sd_rp)
  fresh_ex = mods.marco_polo.VecPopulationMarcoPoloExploration(2, 32, 0.1, 1)
  fresh_ex.load_state_dict(sd_ex)
  resumed = more(fresh, fresh_rp, fresh_ex)
  assert all(torch.equal(a, b) for a, b in zip(straight, resumed)) and any((a != 1).any() for a in straight)
  assert _same(fresh_pop.images, pop.images)
  for name in rp._TENSORS:
    assert _same(getattr(fresh_rp, name), getattr(rp, name)), name
  for name in ex._STATE:
    assert _same(getattr(fresh_ex, name), getattr(ex, name)), name
  tr.check_errors(); rp.check_errors(); fresh.check_errors(); fresh_rp.check_errors()
  # a copy of member 1's parameters into member 0 leaves priorities and the explorer's state with the columns
  tree, phase = rp.tree.clone(), ex.exploratory_phase.clone()
  tr.copy_members(torch.tensor([1], device='cuda'), torch.tensor([0], device='cuda'))
  assert _same(pop.images[0], pop.images[1]) and _same(rp.tree, tree) and _same(ex.exploratory_phase, phase)


# ---- 8. two members learn the contextual bandit as two solo prioritized runs -----------------------------------------------------------
def test_two_members_learn_the_bandit_as_two_solo_prioritized_runs(mods, observations):
  """test_gpu_population_td.py's contextual bandit (every transition terminal; reward 1 for the right action, which is 0 or 2 as one
  observation feature is below or above its median) with DQN 'mse' and prioritized replay: two members at two learning rates, each on
  64 columns of one ring with its own tree, against two solo DQNTrainers on prioritized buffers of those columns (_solo_step) after
  120 updates of 128 rows, byte for byte; the best member clears the solo test's bar (greedy action right on >= 90 % of held-out states,
  mean |q - r| <= 0.2)."""
  qnet, qnet_train = mods.qnet, mods.qnet_train
  x = observations.cpu().numpy()
  std = np.where((x.min(axis=0) >= 0) & (x.max(axis=0) <= 1), x.std(axis=0), 0.0)
  col = int(np.argmax(std))
  label = np.where(x[:, col] > np.median(x[:, col]), 2, 0).astype(np.uint8)
  rng = np.random.default_rng(0)
  perm = rng.permutation(len(x))
  train_i, test_i = perm[:768], perm[768:]
  members, r, steps, rows, updates = 2, 64, 48, 128, 120
  n_env = members * r
  rp = qnet_train.VecPopulationPrioritizedReplayBuffer(members, r, steps, update_horizon=1, gamma=0.99)
  for s in range(steps):
    i = rng.choice(train_i, n_env)
    a = rng.integers(0, 3, n_env).astype(np.uint8)
    rew = (a == label[i]).astype(np.float32)
    rp.add(torch.from_numpy(x[i]).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(rew).cuda(),
           torch.ones(n_env, dtype=torch.uint8, device='cuda'))
  own = [rp.member_buffer(p) for p in range(members)]                # (before the population's updates write the trees)
  lrs = [1e-3, 3e-3]

  def nets():
    return [qnet.QNetwork.from_params(qnet.init_params('quantile', 7 + p, 2, 64, 1), num_atoms=1) for p in range(members)]
  pop = mods.population.QNetworkPopulation.from_networks(nets())
  tr = mods.population.PopulationQTrainer(pop, kind='dqn_mse', lr=lrs, update_horizon=1, gamma=0.99, seed=5)
  tr.capture(rp, rows)
  for _ in range(updates - 1):
    tr.train_step(rp, rows)
  tr.check_errors(); rp.check_errors()
  for p, net in enumerate(nets()):
    solo = mods.dqn.DQNTrainer(net, loss_type='mse', lr=float(np.float32(lrs[p])), update_horizon=1, gamma=0.99, seed=5 + p)
    for _ in range(updates):
      _solo_step(solo, own[p], rows)
    solo.check_errors(); own[p].check_errors()
    assert _same(pop.images[p, :pop.packed_floats], solo.weights), p
  _trees_are_the_solos(rp, own, 'bandit')
  truth = (np.arange(3)[None, :] == label[test_i][:, None]).astype(np.float64)
  agent = mods.population.VecPopulationAgent(pop, len(test_i))
  q = torch.empty(members * len(test_i), 3, dtype=torch.float32, device='cuda')
  held = torch.from_numpy(x[test_i]).cuda()
  act = agent.act(held.repeat(members, 1), q_values=q).cpu().numpy().reshape(members, -1)
  acc = [float((act[p] == label[test_i]).mean()) for p in range(members)]
  err = [float(np.abs(q.view(members, -1, 3)[p].cpu().numpy() - truth).mean()) for p in range(members)]
  print('prioritized bandit: accuracy per member', acc, 'mean |q - r| per member', err)
  best = int(np.argmax(acc))
  assert acc[best] >= 0.9, acc
  assert err[best] <= 0.2, err
