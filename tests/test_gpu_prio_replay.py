"""Prioritized n-step replay on the device (csrc/ble_replay.h, VecPrioritizedReplayBuffer) against the fp64 restatement
(prio_replay_host.py): the tree's contents bit for bit, the stratified draws, set_priority, and determinism of prioritized updates.

Past one wave and one 1024-thread pass: the tree after every add at 1 .. 2500 environments (adjacent zeroed and completed rows, a
power-of-two leaf count, either side of the workgroup's width); set_priority on crafted batches of 1 .. 3000 rows with the largest
weight in each wave position, duplicates across a wave and a pass, failed rows, bad losses and an empty tree; and the prioritized batch
row by row -- the leaf from the host's Philox uniforms, the window, return, discount, action and both observation rows."""
import numpy as np
import pytest
import torch

import prio_replay_host as ph
import train_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd import _lib
  from balloon_learning_environment_amd.agents import qnet, qnet_train
  return _lib, qnet, qnet_train


def _hist(steps, n_env, seed, term_p=0.08, end_p=0.05):
  rng = np.random.default_rng(seed)
  h = {'obs': rng.random((steps, n_env, 1099), dtype=np.float32), 'action': rng.integers(0, 3, (steps, n_env)).astype(np.uint8),
       'reward': rng.standard_normal((steps, n_env)).astype(np.float32),
       'terminal': (rng.random((steps, n_env)) < term_p).astype(np.uint8)}
  h['episode_end'] = np.maximum(h['terminal'], (rng.random((steps, n_env)) < end_p).astype(np.uint8))
  return h


def _add(rp, h, s):
  rp.add(*[torch.from_numpy(h[k][s]).cuda() for k in ('obs', 'action', 'reward', 'terminal', 'episode_end')])


def _host_add(tree, ring, h, s):
  ring['terminal'][s % tree.T] = h['terminal'][s]
  ring['episode_end'][s % tree.T] = h['episode_end'][s]
  tree.add(ring['terminal'], ring['episode_end'])


def _leaves(rp, bt):
  idx = bt.index.cpu().numpy()
  return np.where(idx[:, 0] >= 0, (idx[:, 0] % rp.capacity) * rp.num_envs + idx[:, 1], -1)


def test_tree_contents_and_set_priority_bit_for_bit(mods):
  """Adds that wrap the ring (terminals, time-limit ends), with sample + set_priority in between: the device tree equals the host's."""
  _lib, _, qnet_train = mods
  n_env, cap, n, steps = 8, 40, 5, 100
  h = _hist(steps, n_env, 0)
  rp = qnet_train.VecPrioritizedReplayBuffer(n_env, cap, n, 0.993)
  host = ph.SumTree(cap, n_env, n)
  ring = {'terminal': np.zeros((cap, n_env), np.uint8), 'episode_end': np.zeros((cap, n_env), np.uint8)}
  rng = np.random.default_rng(1)
  for s in range(steps):
    _add(rp, h, s)
    _host_add(host, ring, h, s)
    if s in (30, 55, 80):
      bt = rp.sample(16, seed=3)
      loss = torch.from_numpy((rng.random(16) * 4).astype(np.float32)).cuda()
      rp.set_priority(bt, loss)
      assert not host.set_priority(_leaves(rp, bt), loss.cpu().numpy())
      rp.check_errors()
    got = rp.tree.cpu().numpy()
    assert np.array_equal(got, host.nodes), s
    assert rp.max_priority.item() == host.max_priority
  lv = host.leaf_view()
  last = steps - 1
  for row in range(cap):                               # incomplete rows and windows that cross a time limit are 0
    t = last - ((last % cap) - row) % cap
    for e in range(n_env):
      if t + n > last or not ph.window_valid(ring['terminal'], ring['episode_end'], t, e, n):
        assert lv[row, e] == 0.0, (row, e)
      else:
        assert lv[row, e] > 0.0
  assert host.max_priority > 1.0


def test_stratified_draws_and_frequencies(mods):
  _lib, _, qnet_train = mods
  n_env, cap, n = 4, 16, 1
  h = _hist(40, n_env, 2, term_p=0.0, end_p=0.0)
  rp = qnet_train.VecPrioritizedReplayBuffer(n_env, cap, n, 0.993)
  for s in range(40):
    _add(rp, h, s)
  host = ph.SumTree(cap, n_env, n)
  host.nodes[:] = rp.tree.cpu().numpy()
  lv = host.leaf_view()
  valid = lv > 0
  rng = np.random.default_rng(3)
  lv[valid] = rng.integers(1, 20, int(valid.sum())).astype(np.float64) / 7.0           # crafted priorities
  host.rebuild()
  rp.tree.copy_(torch.from_numpy(host.nodes))
  # each row's leaf lies in its stratum of the host prefix sums
  prefix, total, b = host.prefix(), host.nodes[1], 64
  bt = rp.sample(b, seed=11)
  leaves = _leaves(rp, bt)
  assert (leaves >= 0).all()
  for i, leaf in enumerate(leaves):
    lo, hi = total * i / b, total * (i + 1) / b
    assert prefix[leaf] < hi and prefix[leaf + 1] > lo, (i, leaf)
  np.testing.assert_array_equal(bt.priority.cpu().numpy(), host.nodes[host.P + leaves].astype(np.float32))
  # frequencies over 4096 x 80 draws against p / sum p (chi-square)
  counts = np.zeros(host.leaves, np.int64)
  for _ in range(80):
    bt = rp.sample(4096, seed=12)
    counts += np.bincount(_leaves(rp, bt), minlength=host.leaves)
  p = host.nodes[host.P:host.P + host.leaves]
  assert counts[p == 0].sum() == 0
  expect = counts.sum() * p[p > 0] / p.sum()
  chi2 = float(((counts[p > 0] - expect) ** 2 / expect).sum())
  dof = int((p > 0).sum()) - 1
  assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)
  rp.check_errors()


def test_set_priority_rows(mods):
  """Duplicates (the later row wins), failed rows skipped, the max rising and never falling, the weighted loss, NaN flagged."""
  _lib, _, qnet_train = mods
  n_env, cap, n = 4, 16, 2
  h = _hist(30, n_env, 4, term_p=0.0, end_p=0.0)
  rp = qnet_train.VecPrioritizedReplayBuffer(n_env, cap, n, 0.993)
  for s in range(30):
    _add(rp, h, s)
  bt = rp.sample(8, seed=5)
  idx = bt.index.cpu().numpy()
  idx[3] = idx[1]                                      # a duplicate: row 3 wins over row 1
  idx[5] = -1                                          # a failed draw
  bt.index.copy_(torch.from_numpy(idx))
  bt.priority.copy_(torch.tensor([1.0, 0.5, 2.0, 0.25, 1.0, 0.0, 3.0, 1.5]))
  loss = torch.tensor([0.5, 9.0, 0.0, 16.0, 1.0, 7.0, 2.0, 0.1], device='cuda')
  keep = loss.clone()
  host = ph.SumTree(cap, n_env, n)
  host.nodes[:] = rp.tree.cpu().numpy()
  host.max_priority = rp.max_priority.item()
  out = rp.set_priority(bt, loss)
  leaves = np.where(idx[:, 0] >= 0, (idx[:, 0] % cap) * n_env + idx[:, 1], -1)
  assert not host.set_priority(leaves, keep.cpu().numpy())
  assert np.array_equal(rp.tree.cpu().numpy(), host.nodes)
  assert rp.max_priority.item() == host.max_priority == float(np.sqrt(np.float32(16.0) + np.float32(1e-10)))
  assert host.nodes[host.P + leaves[1]] == 4.0                                         # sqrt(16): row 3's value
  want = ph.weighted_loss(bt.priority.cpu().numpy(), keep.cpu().numpy(), idx[:, 0] >= 0)
  assert np.array_equal(out.cpu().numpy(), want)
  assert torch.equal(loss, keep)                                                        # the unweighted losses are untouched
  # a lower loss does not lower the max; NaN leaves the leaf and sets the flag
  rp.set_priority(bt, torch.full((8,), 0.01, device='cuda'))
  assert rp.max_priority.item() == 4.0
  before = rp.tree.clone()
  bad = torch.full((8,), 0.01, device='cuda')
  bad[0] = float('nan')
  rp.set_priority(bt, bad)
  assert rp.tree[rp.padded + int(leaves[0])].item() == before[rp.padded + int(leaves[0])].item()
  with pytest.raises(ValueError, match='non-finite or negative'):
    rp.check_errors()


def _trained(mods, obs_hist, updates, graph, resume_at=None):
  _lib, qnet, qnet_train = mods
  params = qnet.init_params('quantile', 7, 2, 64, 51)
  n_env, cap = 8, 40

  def fresh():
    tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(params), lr=1e-4, seed=9)
    rp = qnet_train.VecPrioritizedReplayBuffer(n_env, cap, 5, 0.993)
    return tr, rp
  tr, rp = fresh()
  for s in range(cap + 10):
    _add(rp, obs_hist, s)
  losses = []
  for u in range(updates):
    if resume_at is not None and u == resume_at:
      sd_t, sd_r = tr.state_dict(), rp.state_dict()
      tr, rp = fresh()
      tr.load_state_dict(sd_t)
      rp.load_state_dict(sd_r)
    if graph and u == 0:
      losses.append(tr.capture(rp, 32).clone())
    else:
      losses.append(tr.train_step(rp, 32).clone())
  tr.check_errors()
  rp.check_errors()
  return tr.weights.cpu().numpy(), rp.tree.cpu().numpy(), rp.max_priority.item(), torch.stack(losses).cpu().numpy()


def test_prioritized_updates_are_deterministic(mods):
  h = _hist(50, 8, 6)
  a = _trained(mods, h, 50, graph=False)
  b = _trained(mods, h, 50, graph=True)
  c = _trained(mods, h, 50, graph=False, resume_at=25)
  for x in (b, c):
    assert np.array_equal(a[0].view(np.uint32), x[0].view(np.uint32))
    assert np.array_equal(a[1], x[1]) and a[2] == x[2]
    assert np.array_equal(a[3].view(np.uint32), x[3].view(np.uint32))
  assert np.isfinite(a[3]).all() and a[2] > 1.0


# ------------------------------------------------------------------------------------------------- the tree at many environments
def _add_flags(rp, h, s, obs):
  rp.add(obs, *[torch.from_numpy(h[k][s]).cuda() for k in ('action', 'reward', 'terminal', 'episode_end')])


def _sync_host(rp):
  host = ph.SumTree(rp.capacity, rp.num_envs, rp.update_horizon)
  host.nodes[:] = rp.tree.cpu().numpy()
  host.max_priority = rp.max_priority.item()
  return host


@pytest.mark.parametrize('n_env,cap,n', [(1, 6, 5), (63, 6, 5), (65, 6, 5), (64, 8, 3), (1023, 4, 3), (1024, 4, 3), (1025, 4, 3),
                                         (2500, 6, 5)])
def test_tree_at_many_environments(mods, n_env, cap, n):
  """3 T + n adds (terminals ~8 %, time-limit ends ~5 %), two sample + set_priority rounds after the first wrap: after every add the
  whole device tree, padding included, and the max recorded priority equal the twin's.  With T = n + 1 the completed row is the one
  next to the zeroed row at every step; 1025 and 2500 environments need a second and a third strided pass per level."""
  _lib, _, qnet_train = mods
  steps, batch = 3 * cap + n, 33
  h = ph.history(steps, n_env, 100 + n_env, obs=False)
  obs = torch.full((n_env, 1099), 0.5, dtype=torch.float32, device='cuda')                  # (the tree does not read the observations)
  rp = qnet_train.VecPrioritizedReplayBuffer(n_env, cap, n, 0.993)
  host, ring = ph.SumTree(cap, n_env, n), ph.new_ring(cap, n_env)
  assert rp.padded == host.P and ((n_env, cap) != (64, 8) or host.P == host.leaves)         # (64 x 8: no padded leaves)
  rng = np.random.default_rng(n_env)
  rounds = 0
  for s in range(steps):
    _add_flags(rp, h, s, obs)
    ph.host_add(host, ring, h, s)
    assert np.array_equal(rp.tree.cpu().numpy(), host.nodes), ('after add', s)
    assert rp.max_priority.item() == host.max_priority
    if s in (cap + 1, 2 * cap + 2):
      bt = rp.sample(batch, seed=3)
      leaves = _leaves(rp, bt)
      flags = int(rp.err_flags.item())
      rp.err_flags.zero_()
      if host.nodes[1] > 0:                                     # every nonzero leaf is a valid window: no row fails
        assert (leaves >= 0).all() and flags == 0
        assert (host.nodes[host.P + leaves] > 0).all()
      else:
        assert (leaves == -1).all() and flags == _lib.FLAG_REPLAY_EMPTY
      loss = (rng.random(batch) * 4).astype(np.float32)
      rp.set_priority(bt, torch.from_numpy(loss).cuda())
      assert not host.set_priority(leaves, loss)
      rp.check_errors()
      assert np.array_equal(rp.tree.cpu().numpy(), host.nodes), ('after set_priority', s)
      assert rp.max_priority.item() == host.max_priority
      rounds += 1
  assert rounds == 2
  lv, last = host.leaf_view(), steps - 1
  for row in range(cap):                                        # incomplete rows and windows that cross a time limit are 0
    t = ph.newest_step(last, cap, row)
    ok = ph.windows_valid(ring['terminal'], ring['episode_end'], t, n) if t + n <= last else np.zeros(n_env, bool)
    assert np.array_equal(lv[row] > 0, ok), row
  assert np.array_equal(rp.leaf_priorities().cpu().numpy(), lv)


# ---------------------------------------------------------------------------------------------------- set_priority at large batches
_BIG = dict(n_env=65, cap=16, n=2, steps=30)
_MIN_ROWS = (0, 63, 64, 1023, 1024)


@pytest.fixture(scope='module')
def big(mods):
  """One buffer for every set_priority case: 65 environments, 16 steps, n = 2, no episode ends, 30 adds (the 14 complete rows hold
  910 nonzero leaves).  Each test reads the tree it finds into a fresh twin."""
  _lib, _, qnet_train = mods
  c = _BIG
  h = ph.history(c['steps'], c['n_env'], 4, term_p=0.0, end_p=0.0, obs=False)
  rp = qnet_train.VecPrioritizedReplayBuffer(c['n_env'], c['cap'], c['n'], 0.993)
  obs = torch.full((c['n_env'], 1099), 0.5, dtype=torch.float32, device='cuda')
  for s in range(c['steps']):
    _add_flags(rp, h, s, obs)
  last = c['steps'] - 1
  rows = [r for r in range(c['cap']) if ph.newest_step(last, c['cap'], r) + c['n'] <= last]
  complete = np.array([r * c['n_env'] + e for r in rows for e in range(c['n_env'])], np.int64)
  assert len(complete) == 910 and (rp.tree[rp.padded + torch.from_numpy(complete).cuda()] > 0).all()
  return rp, complete


def _craft(complete, b, min_row, seed, bad_rows=()):
  """A batch of b crafted rows over the complete leaves: index, priority and loss on the host, and the rows of each duplicate group
  (ascending; its leaf appears in no other row).  min_row holds the one smallest priority, 0.01; 5 % of the ordinary rows are failed
  draws, the last of which carries a priority of 0.001."""
  c = _BIG
  rng = np.random.default_rng(seed)
  perm = rng.permutation(complete)
  reserved, pool = perm[:3 + len(bad_rows)], perm[3 + len(bad_rows):]
  leaf = rng.choice(pool, b)
  groups = []
  if b >= 65:
    groups.append((63, 64))                                     # one row apart, across a wave boundary
  if b >= 1025:
    groups.append((0, 1024))                                    # the same thread, one strided pass apart
  if b >= 5:
    groups.append((1, 2 + b // 3, b - 3))
  for g, rows in enumerate(groups):
    leaf[list(rows)] = reserved[g]
  for k, r in enumerate(bad_rows):
    leaf[r] = reserved[3 + k]
  special = set(_MIN_ROWS) | {b - 1, min_row} | {r for rows in groups for r in rows} | set(bad_rows)
  ordinary = np.array([r for r in range(b) if r not in special], np.int64)
  failed = rng.choice(ordinary, max(1, round(0.05 * b)), replace=False) if b >= 8 else np.zeros(0, np.int64)
  leaf[failed] = -1
  priority = (0.25 + 3.75 * rng.random(b)).astype(np.float32)
  priority[min_row] = 0.01
  if len(failed):
    priority[failed.max()] = 0.001                              # would be the largest weight: a failed row is left out of the max
  loss = (rng.random(b) * 4).astype(np.float32)
  last = c['steps'] - 1
  index = np.full((b, 2), -1, np.int64)
  ok = leaf >= 0
  index[ok, 0] = ph.newest_step(last, c['cap'], leaf[ok] // c['n_env'])
  index[ok, 1] = leaf[ok] % c['n_env']
  assert (index[ok, 0] % c['cap'] * c['n_env'] + index[ok, 1] == leaf[ok]).all()
  return leaf, index, priority, loss, groups, failed


def _load(rp, b, index, priority, loss):
  bt = rp.batch_buffers(b)
  bt.index.copy_(torch.from_numpy(index))
  bt.priority.copy_(torch.from_numpy(priority))
  return bt, torch.from_numpy(loss).cuda()


def _leaf_value(l):
  return float(np.sqrt(np.float32(l) + np.float32(1e-10)))


@pytest.mark.parametrize('b,min_row', [(b, r) for b in (1, 64, 65, 1024, 1025, 3000) for r in sorted({r for r in _MIN_ROWS + (b - 1,) if r < b})])
def test_set_priority_at_large_batches(mods, big, b, min_row):
  """The largest importance weight (the one priority of 0.01) in row min_row: lane 0 of wave 0, the last lane of wave 0, wave 1,
  the last wave, the second strided pass, the last row.  The weighted losses equal the twin's bit for bit only if the max over all 16
  waves and all passes reaches every row; the tree and the max recorded priority equal the twin's; on a duplicate the later row wins."""
  _lib, _, _ = mods
  rp, complete = big
  leaf, index, priority, loss, groups, failed = _craft(complete, b, min_row, seed=1000 * b + min_row)
  assert (priority[leaf >= 0] >= 0.01).all() and (priority[leaf >= 0] == 0.01).sum() == 1
  assert b < 8 or (len(failed) >= 1 and (priority[failed] == 0.001).sum() == 1)
  host = _sync_host(rp)
  bt, loss_d = _load(rp, b, index, priority, loss)
  out = rp.set_priority(bt, loss_d)
  assert not host.set_priority(leaf, loss)
  tree = rp.tree.cpu().numpy()
  assert np.array_equal(tree, host.nodes)
  assert rp.max_priority.item() == host.max_priority
  for rows in groups:
    values = [_leaf_value(loss[r]) for r in rows]
    assert len(set(values)) == len(rows) and (leaf == leaf[rows[0]]).sum() == len(rows)
    assert tree[rp.padded + leaf[rows[0]]] == values[-1], rows
  want = ph.weighted_loss(priority, loss, leaf >= 0)
  got = out.cpu().numpy()
  assert np.array_equal(got, want), (np.flatnonzero(got != want)[:5], got[got != want][:5], want[got != want][:5])
  assert want[min_row] == loss[min_row] and not want[failed].any()
  assert np.array_equal(loss_d.cpu().numpy(), loss)
  assert int(rp.err_flags.item()) == 0


def test_set_priority_bad_losses_past_the_first_pass(mods, big):
  """B = 3000, a NaN loss in row 1500 and a negative one in row 2600 (the second and third strided passes): their leaves stay, every
  other leaf and ancestor is the twin's, and the flag is raised."""
  rp, complete = big
  b, bad_rows = 3000, (1500, 2600)
  leaf, index, priority, loss, _, _ = _craft(complete, b, 0, seed=77, bad_rows=bad_rows)
  loss[1500], loss[2600] = np.nan, -0.5
  host = _sync_host(rp)
  before = host.nodes[host.P + leaf[list(bad_rows)]].copy()
  assert (before > 0).all() and all((leaf == leaf[r]).sum() == 1 for r in bad_rows)
  bt, loss_d = _load(rp, b, index, priority, loss)
  out = rp.set_priority(bt, loss_d).cpu().numpy()
  assert host.set_priority(leaf, loss)
  tree = rp.tree.cpu().numpy()
  assert np.array_equal(tree[rp.padded + leaf[list(bad_rows)]], before)
  assert np.array_equal(tree, host.nodes)
  assert rp.max_priority.item() == host.max_priority
  want = ph.weighted_loss(priority, loss, leaf >= 0)
  fine = np.arange(b) != 1500
  assert np.array_equal(out[fine], want[fine]) and np.isnan(out[1500]) and out[2600] < 0
  with pytest.raises(ValueError, match='non-finite or negative'):
    rp.check_errors()
  assert int(rp.err_flags.item()) == 0                          # (check_errors clears what it reports)


def test_empty_tree_sample_and_set_priority(mods):
  """Fewer than n + 1 adds: no window is complete and the root is 0.  Every row of a draw fails; set_priority on it changes nothing."""
  _lib, _, qnet_train = mods
  c = _BIG
  h = ph.history(c['n'], c['n_env'], 5, term_p=0.0, end_p=0.0, obs=False)
  rp = qnet_train.VecPrioritizedReplayBuffer(c['n_env'], c['cap'], c['n'], 0.993)
  obs = torch.full((c['n_env'], 1099), 0.5, dtype=torch.float32, device='cuda')
  for s in range(c['n']):
    _add_flags(rp, h, s, obs)
  assert not rp.tree.cpu().numpy().any()
  b = 65
  bt = rp.batch_buffers(b)
  for t in (bt.state, bt.next_state, bt.ret, bt.discount, bt.priority, bt.weighted_loss):
    t.fill_(7.0)                                                # stale contents the draw must overwrite
  bt.action.fill_(2)
  assert int(rp.counter.item()) == 0
  assert rp.sample(b, seed=11) is bt
  assert (bt.index.cpu().numpy() == -1).all()
  for t in (bt.priority, bt.ret, bt.discount, bt.state, bt.next_state, bt.action):
    assert not t.cpu().numpy().any()
  assert int(rp.err_flags.item()) == _lib.FLAG_REPLAY_EMPTY
  assert int(rp.counter.item()) == 1
  before = rp.tree.cpu().numpy().copy()
  out = rp.set_priority(bt, torch.full((b,), float('nan'), device='cuda'))
  assert np.array_equal(rp.tree.cpu().numpy().view(np.uint64), before.view(np.uint64))
  assert rp.max_priority.item() == 1.0
  assert not out.cpu().numpy().any() and not np.isnan(out.cpu().numpy()).any()
  assert int(rp.err_flags.item()) == _lib.FLAG_REPLAY_EMPTY                               # and no priority flag
  with pytest.raises(RuntimeError):
    rp.check_errors()


# ------------------------------------------------------------------------------------------ the prioritized batch, row by row
@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  return ph.build_replay_draws(tmp_path_factory.mktemp('rpd'))


@pytest.fixture(scope='module')
def draw_case(mods):
  """ph.DRAW_CASE on the device: 40 adds into 12 rows of 65 environments (the ring wraps three times), the device tree equal to the
  twin's, then the crafted priorities copied in."""
  _lib, _, qnet_train = mods
  c = ph.DRAW_CASE
  h = ph.history(c['steps'], c['num_envs'], c['hist_seed'], distinct_rewards=True)
  rp = qnet_train.VecPrioritizedReplayBuffer(c['num_envs'], c['capacity'], c['horizon'], 0.993)
  for s in range(c['steps']):
    _add(rp, h, s)
  fed, tree = ph.draw_case_tree(h)
  assert np.array_equal(rp.tree.cpu().numpy(), fed.nodes)
  rp.tree.copy_(torch.from_numpy(tree.nodes))
  return rp, h, tree


@pytest.mark.parametrize('counter', ph.DRAW_CASE['counters'])
@pytest.mark.parametrize('b', ph.DRAW_CASE['batches'])
def test_prioritized_batch_row_by_row(mods, draws, draw_case, b, counter):
  """Row b's leaf is the twin's walk from q_b = seg b + u_b seg with the host's Philox uniform (every row's three candidate queries
  agree on one leaf, and it is a valid window -- asserted first); index, return, discount, action, both observation rows and the
  priority are those of that window in the history."""
  rp, h, tree = draw_case
  c = ph.DRAW_CASE
  n_env, cap, n, last = c['num_envs'], c['capacity'], c['horizon'], c['steps'] - 1
  q = tree.stratified_queries(draws(c['seed'], b, counter)[:, 0])
  cands = [tree.find_candidates(float(x)) for x in q]
  assert all(len(s) == 1 for s in cands)
  leaf = np.array([next(iter(s)) for s in cands], np.int64)
  tt, env = ph.newest_step(last, cap, leaf // n_env), leaf % n_env
  assert (tree.nodes[tree.P + leaf] > 0).all() and (last + 1 - cap <= tt).all() and (tt + n <= last).all()
  windows = [train_host.nstep(h['reward'], h['terminal'], h['episode_end'], int(t), int(e), n, 0.993) for t, e in zip(tt, env)]
  assert all(w is not None for w in windows)                    # no row needs a second draw
  ctr = torch.tensor([counter], dtype=torch.int64, device='cuda')
  bt = rp.sample(b, seed=c['seed'], counter=ctr)
  assert int(ctr.item()) == counter + 1 and int(rp.err_flags.item()) == 0
  idx = bt.index.cpu().numpy()
  assert np.array_equal(idx[:, 0], tt) and np.array_equal(idx[:, 1], env), np.flatnonzero((idx[:, 0] != tt) | (idx[:, 1] != env))[:5]
  assert np.array_equal(_leaves(rp, bt), leaf)
  m = np.array([w[0] for w in windows])
  ret, disc = np.array([w[1] for w in windows], np.float32), np.array([w[2] for w in windows], np.float32)
  assert np.array_equal(bt.ret.cpu().numpy().view(np.uint32), ret.view(np.uint32))
  assert np.array_equal(bt.discount.cpu().numpy().view(np.uint32), disc.view(np.uint32))
  assert np.array_equal(bt.action.cpu().numpy(), h['action'][tt, env])
  st, ns = bt.state.cpu().numpy(), bt.next_state.cpu().numpy()
  assert np.array_equal(st[:, :1099], h['obs'][tt, env]) and np.array_equal(ns[:, :1099], h['obs'][tt + m, env])
  assert not st[:, 1099:].any() and not ns[:, 1099:].any()
  assert np.array_equal(bt.priority.cpu().numpy(), tree.nodes[tree.P + leaf].astype(np.float32))
  assert b < 64 or ((m < n).any() and (disc == 0).any())        # (some windows end on a terminal)
