"""The acting and collecting half of training on the device against its NumPy twins (collect_host.py, DESIGN 3g "The two draw
contracts"), bit for bit:

 * ble_explore_kernel (qnet_train.explore): new actions and untouched lanes at n = 1 .. 65 537, six epsilons, three seeds, five steps
   either side of 2^32; batch invariance; the strict threshold; no byte written outside the tensor; the twin's laws on the device's
   own output; the Python wrapper refuses a tensor it would miswrite;
 * ble_replay_sample_kernel (VecReplayBuffer.sample): the window every batch row draws, the tries behind it, rows that fail next to
   rows that succeed, the flag, the counter; N = 1 .. 1000, capacities 6, 24, 40, horizons 5 and 1, spans 0 and 1, B = 1 .. 1025,
   counters either side of 2^32; max_tries = 3 through the C struct; a captured graph replayed three times;
 * run_training_loop_vec: the actions the replay ring holds are the twin's epsilon-greedy of the greedy actions, step by step.
"""
import ctypes

import numpy as np
import pytest
import torch

import collect_host
import train_host

pytestmark = pytest.mark.gpu

GAMMA = 0.993


@pytest.fixture(scope='module')
def qnet_train():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import qnet_train
  return qnet_train


# ---------------------------------------------------------------------------------------------------------------------- epsilon-greedy
def _explore(qnet_train, actions, epsilon, seed, step):
  t = torch.from_numpy(np.ascontiguousarray(actions, np.uint8)).cuda()
  assert qnet_train.explore(t, epsilon, seed, step) is t
  return t.cpu().numpy()


EPSILONS = (0.0, 2.0 ** -24, 0.01, 0.1, 0.5, 1.0)
SEEDS = (0, 3, 2 ** 40 + 5)
STEPS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 1025, 65537])
def test_explore_bit_for_bit(qnet_train, n):
  held = np.random.default_rng(n).integers(0, 3, n).astype(np.uint8)
  replaced = same = 0
  for seed in SEEDS:
    for step in STEPS:
      uf, random = collect_host.explore_draws(n, seed, step)
      for epsilon in EPSILONS:
        mask = uf < np.float32(epsilon)
        want = np.where(mask, random, held)
        got = _explore(qnet_train, held, epsilon, seed, step)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (n, seed, step, epsilon, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        replaced += int(mask.sum())
        same += int((mask & (random == held)).sum())
  if n >= 255:           # the cases tell "left alone" from "replaced by the value it held": both occur
    assert replaced > same > 0


def test_explore_batch_invariance(qnet_train):
  """The first m lanes of a launch of n are a launch of m: a lane's draw depends on its own index alone."""
  n, seed, step = 1025, 2 ** 40 + 5, 2 ** 32 + 1
  held = np.full(n, collect_host.SENTINEL, np.uint8)
  whole = _explore(qnet_train, held, 0.5, seed, step)
  for m in (1, 63, 64, 65, 256, 257, 1024):
    assert np.array_equal(_explore(qnet_train, held[:m], 0.5, seed, step), whole[:m]), m


def test_explore_strict_threshold(qnet_train):
  n, seed, step = 257, 3, 7
  held = np.full(n, collect_host.SENTINEL, np.uint8)
  uf, random = collect_host.explore_draws(n, seed, step)
  for j in (int(np.argmin(np.abs(uf - np.float32(0.3)))), int(np.argmin(uf)), 256):
    at, above = uf[j], np.nextafter(uf[j], np.float32(1.0))
    assert _explore(qnet_train, held, float(at), seed, step)[j] == collect_host.SENTINEL, 'uf == epsilon was replaced'
    assert _explore(qnet_train, held, float(above), seed, step)[j] == random[j]
  assert np.array_equal(_explore(qnet_train, held, 0.0, seed, step), held)
  assert np.array_equal(_explore(qnet_train, held, 1.0, seed, step), random)


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_explore_writes_inside_the_tensor_only(qnet_train, n):
  """A slice of a larger allocation with a guard byte either side: epsilon = 0 leaves every byte, epsilon = 1 the two guards."""
  buf = torch.full((n + 2,), 0xA5, dtype=torch.uint8, device='cuda')
  view = buf[1:n + 1]
  assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 1
  qnet_train.explore(view, 0.0, 3, 5)
  assert (buf.cpu().numpy() == 0xA5).all()
  qnet_train.explore(view, 1.0, 3, 5)
  got = buf.cpu().numpy()
  assert got[0] == 0xA5 and got[-1] == 0xA5
  assert np.array_equal(got[1:-1], collect_host.explore_draws(n, 3, 5)[1])


def test_explore_laws_on_the_device(qnet_train):
  collect_host.assert_explore_laws(lambda a, e, seed, step: _explore(qnet_train, a, e, seed, step), 'device')


def test_explore_refuses_what_it_would_miswrite(qnet_train):
  base = torch.full((16,), 7, dtype=torch.uint8, device='cuda')
  wide = torch.full((4,), 7, dtype=torch.int32, device='cuda')
  for bad in (base[::2], wide, base.view(8, 2).t()):
    with pytest.raises(ValueError):
      qnet_train.explore(bad, 1.0, 0, 0)
  assert (base.cpu().numpy() == 7).all() and (wide.cpu().numpy() == 7).all()


# ------------------------------------------------------------------------------------------------------------- the uniform replay draw
class _Ring:
  """A VecReplayBuffer whose tensors are written directly: terminal and episode_end as given, random observations, actions and
  rewards, count and cursor as given."""

  def __init__(self, qnet_train, terminal, episode_end, horizon, seed=0):
    self.capacity, self.n_env = terminal.shape
    self.horizon, self.terminal, self.episode_end = horizon, np.asarray(terminal, np.uint8), np.asarray(episode_end, np.uint8)
    self.rp = rp = qnet_train.VecReplayBuffer(self.n_env, self.capacity, horizon, GAMMA)
    g = torch.Generator(device='cuda').manual_seed(seed)
    rp.obs[:, :, :1099] = torch.rand(self.capacity, self.n_env, 1099, generator=g, device='cuda')
    rp.action.copy_(torch.randint(0, 3, rp.action.shape, generator=g, device='cuda', dtype=torch.uint8))
    rp.reward.copy_(torch.rand(rp.reward.shape, generator=g, device='cuda') * 4.0 - 1.0)
    rp.terminal.copy_(torch.from_numpy(self.terminal))
    rp.episode_end.copy_(torch.from_numpy(self.episode_end))
    self.reward, self.action = rp.reward.cpu().numpy(), rp.action.cpu().numpy()
    self._valid = {}

  def at(self, count):
    self.count = count
    self.rp.count.fill_(count)
    self.rp.cursor = count
    return self

  def valid(self):
    if self.count not in self._valid:
      self._valid[self.count] = collect_host.valid_windows(self.terminal, self.episode_end, self.count, self.capacity, self.horizon)
    return self._valid[self.count]

  def twin(self, batch, seed, counter, max_tries=collect_host.MAX_TRIES):
    return collect_host.uniform_draws(self.terminal, self.episode_end, self.count, self.capacity, self.horizon, batch, seed, counter,
                                      max_tries, valid=self.valid())

  def flag(self):
    """Whether BLE_FLAG_REPLAY_EMPTY is set (and nothing else); clears it."""
    from balloon_learning_environment_amd import _lib
    f = int(self.rp.err_flags.item())
    self.rp.err_flags.zero_()
    assert f in (0, _lib.FLAG_REPLAY_EMPTY), f
    return f != 0

  def check(self, bt, batch, seed, counter, max_tries=collect_host.MAX_TRIES):
    """The batch `bt` the device drew at (seed, counter) against the twin: index row by row, the flag, the contents of every row."""
    want, tries = self.twin(batch, seed, counter, max_tries)
    got = bt.index.cpu().numpy()
    assert got.shape == (batch, 2)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (self.n_env, self.capacity, self.horizon, self.count, batch, seed, counter, bad[:4].tolist(),
                           got[bad[:4]].tolist(), want[bad[:4]].tolist(), tries[bad[:4]].tolist())
    failed = want[:, 0] < 0
    assert self.flag() == bool(failed.any()), 'BLE_FLAG_REPLAY_EMPTY is set iff a row fails'
    ret, disc, act = bt.ret.cpu().numpy(), bt.discount.cpu().numpy(), bt.action.cpu().numpy()
    assert not ret[failed].any() and not disc[failed].any() and not act[failed].any()
    assert not bt.state[torch.from_numpy(failed).cuda()].any() and not bt.next_state[torch.from_numpy(failed).cuda()].any()
    lo_t, _ = collect_host.candidates(self.count, self.capacity, self.horizon)
    rows = (lo_t + np.arange(self.count - lo_t)) % self.capacity       # the steps held, oldest first
    reward, term, end = self.reward[rows], self.terminal[rows], self.episode_end[rows]
    ok = np.flatnonzero(~failed)
    m = np.zeros(batch, np.int64)
    for b in ok:
      t, e = want[b]
      m[b], r, d, _ = train_host.nstep(reward, term, end, t - lo_t, e, self.horizon, GAMMA)
      assert ret[b].view(np.uint32) == r.view(np.uint32) and disc[b].view(np.uint32) == d.view(np.uint32), (b, t, e)
    t, e = want[ok, 0], torch.from_numpy(want[ok, 1]).cuda()
    okd = torch.from_numpy(ok).cuda()
    assert np.array_equal(act[ok], self.action[t % self.capacity, want[ok, 1]])
    assert torch.equal(bt.state[okd], self.rp.obs[torch.from_numpy(t % self.capacity).cuda(), e])
    assert torch.equal(bt.next_state[okd], self.rp.obs[torch.from_numpy((t + m[ok]) % self.capacity).cuda(), e])
    return want, tries

  def sample_and_check(self, batch, seed, counter):
    c = torch.tensor([counter], dtype=torch.int64, device='cuda')
    bt = self.rp.sample(batch, seed, c)
    out = self.check(bt, batch, seed, counter)
    assert int(c.item()) == counter + 1, 'the sampler advances the counter by exactly one'
    return out


COUNTERS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5)


@pytest.mark.parametrize('capacity,horizon', [(6, 5), (24, 5), (40, 5), (6, 1), (40, 1)])
@pytest.mark.parametrize('n_env', [1, 3, 37, 64, 1000])
def test_uniform_draw_rings(qnet_train, n_env, capacity, horizon):
  """count = horizon (span 0: every row fails, the flag is set, the counter still advances), horizon + 1 (span 1), below the capacity (lo_t = 0) and past it (the ring has wrapped), B = 257 (two rows past 255)."""
  terminal, episode_end = collect_host.random_ring(np.random.default_rng(1000 * n_env + 10 * capacity + horizon), capacity, n_env, 0.05, 0.15)
  ring = _Ring(qnet_train, terminal, episode_end, horizon, seed=n_env)
  counts = (horizon, horizon + 1, max(capacity - 1, horizon + 1), capacity, capacity + capacity // 2 + 1, 3 * capacity + 2)
  for k, count in enumerate(counts):
    seed, counter = (11, 2 ** 40 + 5)[k % 2], COUNTERS[k % 4]
    want, tries = ring.at(count).sample_and_check(257, seed, counter)
    lo_t, span = collect_host.candidates(count, capacity, horizon)
    assert lo_t == max(count - capacity, 0)
    if span == 0:
      assert (want == -1).all() and not tries.any()
    if span >= 1:
      assert ((want[:, 0] >= lo_t) & (want[:, 0] + horizon <= count - 1) | (want[:, 0] == -1)).all()


@pytest.mark.parametrize('capacity,horizon,count', [(6, 5, 6), (6, 5, 11), (24, 5, 6), (40, 1, 2), (2, 1, 9)])
def test_uniform_draw_span_one(qnet_train, capacity, horizon, count):
  """A ring without episode ends at span 1, below the capacity and wrapped: the device's every row holds t = lo_t, at the first try,
  and every environment is drawn."""
  n_env = 3
  none = np.zeros((capacity, n_env), np.uint8)
  ring = _Ring(qnet_train, none, none, horizon, seed=count).at(count)
  lo_t, span = collect_host.candidates(count, capacity, horizon)
  assert span == 1 and lo_t == max(count - capacity, 0)
  c = torch.tensor([2 ** 32 - 1], dtype=torch.int64, device='cuda')
  got = ring.rp.sample(257, 11, c).index.cpu().numpy().copy()
  assert (got[:, 0] == lo_t).all() and set(got[:, 1].tolist()) == set(range(n_env))
  _, tries = ring.check(ring.rp.batch_buffers(257), 257, 11, 2 ** 32 - 1)
  assert (tries == 1).all() and int(c.item()) == 2 ** 32


@pytest.fixture(scope='module')
def rings(qnet_train):
  (easy, hard) = collect_host.easy_and_hard_ring()
  return _Ring(qnet_train, *easy, 5, seed=1).at(60), _Ring(qnet_train, *hard, 5, seed=2).at(60)


@pytest.mark.parametrize('batch', [1, 255, 256, 257, 1025])
def test_uniform_draw_batches_and_counters(rings, batch):
  """Every batch size at every counter, on the easy ring (retries) and the hard one (rows that fail beside rows that succeed)."""
  for ring in rings:
    for k, counter in enumerate(COUNTERS):
      ring.sample_and_check(batch, (11, 2 ** 40 + 5)[k % 2], counter)


def test_uniform_draw_retry_and_failure(rings):
  """B = 1025 at counter 2^32 + 5, seed 11.  The conditions are on the twin: a sampler without the retry or the failure path cannot
  pass by luck."""
  easy, hard = rings
  want, tries = easy.sample_and_check(1025, 11, 2 ** 32 + 5)
  print('easy ring: tries histogram', np.bincount(tries).tolist())
  assert (want >= 0).all() and (tries >= 3).sum() >= 20
  want, tries = hard.sample_and_check(1025, 11, 2 ** 32 + 5)
  failed = want[:, 0] < 0
  print('hard ring: failed rows', int(failed.sum()), 'tries histogram', np.bincount(tries).tolist())
  assert failed.sum() >= 10 and (~failed & (tries >= 10)).sum() >= 10 and tries.max() == 64
  border = failed[1:] != failed[:-1]
  assert border.sum() >= 10, 'failed rows sit next to rows that succeed'


def test_uniform_draw_max_tries_3(rings):
  """A smaller max_tries through the documented C struct (Python always passes 64)."""
  from balloon_learning_environment_amd import _lib
  from balloon_learning_environment_amd import device as dev
  _, hard = rings
  batch, seed, counter = 257, 11, 2 ** 32 - 1
  c = torch.tensor([counter], dtype=torch.int64, device='cuda')
  bt = hard.rp.batch_buffers(batch)
  st = hard.rp.struct(c)
  assert st.max_tries == 64
  st.max_tries = 3
  code = _lib.lib().ble_replay_sample_f32(ctypes.byref(st), ctypes.byref(bt.struct), seed, hard.rp.err_flags.data_ptr(),
                                          dev.stream_ptr(hard.rp.device))
  torch.cuda.synchronize()
  assert code == _lib.BLE_OK
  want, tries = hard.check(bt, batch, seed, counter, max_tries=3)
  assert int(c.item()) == counter + 1
  failed = want[:, 0] < 0
  assert tries.max() == 3 and failed.sum() >= 100 and (~failed).sum() >= 10
  full, _ = hard.twin(batch, seed, counter)
  assert ((full[:, 0] >= 0) & failed).sum() >= 50, 'rows that 64 tries would have served fail at 3'


def test_uniform_draw_graph_replay(rings):
  """A captured sample replayed three times draws the batches of counters c, c + 1, c + 2 (here across 2^32)."""
  from balloon_learning_environment_amd import device as dev
  easy, _ = rings
  batch, seed, start = 300, 2 ** 40 + 5, 2 ** 32 - 2
  c = torch.tensor([start], dtype=torch.int64, device='cuda')
  easy.check(easy.rp.sample(batch, seed, c), batch, seed, start)          # (eager once: the batch buffers are allocated here)
  graph, bt = dev.capture(easy.rp.device, lambda: easy.rp.sample(batch, seed, c))
  torch.cuda.synchronize()
  assert int(c.item()) == start + 1, 'recording runs nothing'
  seen = []
  for k in range(3):
    graph.replay()
    torch.cuda.synchronize()
    want, _ = easy.check(bt, batch, seed, start + 1 + k)
    assert int(c.item()) == start + 2 + k
    seen.append(want)
  assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# -------------------------------------------------------------------------------------------------------------------------- the loop
def test_training_loop_stores_the_twins_actions(qnet_train, monkeypatch):
  """One short real run: N = 64, a 5-step episode limit, epsilon 0.5, 2 x 5 steps.  The action row the replay ring holds for step s
  is collect_host.explore(the network's greedy actions of step s, 0.5, seed, s): the loop hands the kernel a fresh step every step."""
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.agents import qnet
  from balloon_learning_environment_amd.env import balloon_env
  greedy = []
  act = qnet_train.QNetworkTrainer.act

  def keeping(self, obs, out):
    result = act(self, obs, out)
    greedy.append(out.clone())
    return result
  monkeypatch.setattr(qnet_train.QNetworkTrainer, 'act', keeping)
  n, seed, steps = 64, 2 ** 33 + 3, 10
  env = balloon_env.VecBalloonEnv(n, seed=1)
  # (update horizon 2: a 5-step window never fits inside an episode that the limit ends at its 5th step)
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(qnet.init_params('quantile', 7, 2, 64, 51)), lr=1e-4, seed=2, update_horizon=2)
  rp = qnet_train.VecReplayBuffer(n, 16, update_horizon=2, gamma=GAMMA)
  stats = train_lib.run_training_loop_vec(env, tr, rp, num_iterations=2, steps_per_iteration=5, max_episode_length=5,
                                          min_replay_history=n * 7, updates_per_step=1, epsilon=0.5, seed=seed)
  assert [s['updates'] for s in stats] == [0, 4] and stats[1]['transitions'] == n * steps and len(greedy) == steps
  stored = rp.action.cpu().numpy()
  explored = 0
  for s in range(steps):
    want, mask, _, _ = collect_host.explore(greedy[s].cpu().numpy(), 0.5, seed, s)
    assert np.array_equal(stored[s], want), (s, np.flatnonzero(stored[s] != want)[:4].tolist())
    explored += int(mask.sum())
  assert 0 < explored < n * steps
  ends, terminal = rp.episode_end.cpu().numpy()[:steps], rp.terminal.cpu().numpy()[:steps]
  assert (ends[4] | terminal[:4].any(axis=0)).all(), 'the 5-step limit ends every episode that no terminal ended earlier'
  assert (ends[:4] == terminal[:4]).all()
