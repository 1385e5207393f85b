"""An fp64 NumPy restatement of the device's prioritized n-step replay (csrc/ble_replay.h): the sum tree over
capacity x num_envs windows, the insertion rule, the stratified walk from given uniforms, set_priority with the later row winning, the
max recorded priority and the reported (weighted) loss; the histories the replay tests feed both sides, and the replay's Philox
uniforms from a g++ build of the generator (replay_draws.cpp).  TEST TOOLING."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def window_valid(terminal, episode_end, t, env, n):
  """ble_train.h replay_window over the ring arrays [T, N]: no episode end before the first terminal among t .. t + n - 1."""
  cap = terminal.shape[0]
  for k in range(n):
    if terminal[(t + k) % cap, env]:
      return True
    if episode_end[(t + k) % cap, env]:
      return False
  return True


def windows_valid(terminal, episode_end, t, n):
  """window_valid for every environment at once: bool [N]."""
  cap = terminal.shape[0]
  valid = np.ones(terminal.shape[1], bool)
  undecided = np.ones(terminal.shape[1], bool)
  for k in range(n):
    term, end = terminal[(t + k) % cap] != 0, episode_end[(t + k) % cap] != 0
    valid &= ~(undecided & ~term & end)
    undecided &= ~(term | end)
  return valid


class SumTree:
  def __init__(self, capacity, num_envs, update_horizon):
    self.T, self.N, self.n = int(capacity), int(num_envs), int(update_horizon)
    self.leaves = self.T * self.N
    self.P = 1 << (self.leaves - 1).bit_length()
    self.nodes = np.zeros(2 * self.P)
    self.max_priority = 1.0
    self.count = 0

  def leaf_view(self):
    return self.nodes[self.P:self.P + self.leaves].reshape(self.T, self.N)

  def rebuild(self):
    """Every parent = left + right, from the leaves up (the tree is a pure function of its leaves), one level at a time."""
    lo = self.P >> 1
    while lo >= 1:
      self.nodes[lo:2 * lo] = self.nodes[2 * lo:4 * lo:2] + self.nodes[2 * lo + 1:4 * lo:2]
      lo >>= 1

  def rebuild_node_by_node(self):
    """rebuild() as its definition reads, one parent at a time: what the level-by-level form is held to."""
    for i in range(self.P - 1, 0, -1):
      self.nodes[i] = self.nodes[2 * i] + self.nodes[2 * i + 1]

  def add(self, terminal, episode_end):
    """After vector step s = count was written into the ring arrays [T, N]: zero row s % T, row (s - n) % T to the max (valid windows)."""
    s = self.count
    self.count += 1
    lv = self.leaf_view()
    lv[s % self.T] = 0.0
    if s >= self.n:
      lv[(s - self.n) % self.T] = np.where(windows_valid(terminal, episode_end, s - self.n, self.n), self.max_priority, 0.0)
    self.rebuild()

  def find(self, q):
    node = 1
    while node < self.P:
      left, right = self.nodes[2 * node], self.nodes[2 * node + 1]
      go_left = q < left
      if go_left and not left > 0:
        go_left = False
      elif not go_left and not right > 0:
        go_left = True
      if go_left:
        node = 2 * node
      else:
        q -= left
        node = 2 * node + 1
    return node - self.P

  def find_candidates(self, q):
    """The leaves of q and of its two fp64 neighbours.  The device evaluates seg * b + u * seg as one expression and may fuse one of
    the products; the twin rounds both, so the two queries can differ by one unit in the last place.  A row whose set has one member
    has the same leaf either way."""
    return {self.find(q), self.find(float(np.nextafter(q, -np.inf))), self.find(float(np.nextafter(q, np.inf)))}

  def stratified_queries(self, u):
    """q_b = seg b + u_b seg, both products rounded, for uniforms u [B]."""
    u = np.asarray(u, np.float64)
    seg = self.nodes[1] / len(u)
    return seg * np.arange(len(u), dtype=np.float64) + u * seg

  def stratified(self, u):
    """Leaves of the first (stratified) draws from uniforms u [B]: q = total (b + u_b) / B."""
    total, b = self.nodes[1], len(u)
    seg = total / b
    return np.array([self.find(seg * i + float(u[i]) * seg) for i in range(b)], np.int64)

  def prefix(self):
    """Prefix sums of the leaves (fp64): leaf i covers [prefix[i], prefix[i + 1])."""
    return np.concatenate([[0.0], np.cumsum(self.nodes[self.P:self.P + self.leaves])])

  def set_priority(self, leaves, loss):
    """Leaves in batch order (the later row wins), -1 skipped, non-finite / negative loss left unchanged; returns bad."""
    lv = self.nodes[self.P:]
    bad = False
    for leaf, l in zip(leaves, np.asarray(loss, np.float32)):
      if leaf < 0:
        continue
      if not (np.isfinite(l) and l >= 0):
        bad = True
        continue
      v = float(np.sqrt(np.float32(l) + np.float32(1e-10)))
      lv[leaf] = v
      self.max_priority = max(self.max_priority, v)
    self.rebuild()
    return bad


def weighted_loss(priority, loss, valid):
  """quantile_agent.py: w = 1 / sqrt(p + 1e-10), w /= max w (over the drawn rows), reported = w L (float32); 0 for failed rows."""
  p = np.asarray(priority, np.float32)
  w = np.float32(1.0) / np.sqrt(p + np.float32(1e-10))
  wmax = w[valid].max() if valid.any() else np.float32(0)
  return np.where(valid, (w / wmax) * np.asarray(loss, np.float32), np.float32(0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- shared test inputs
def history(steps, n_env, seed, term_p=0.08, end_p=0.05, obs=True, distinct_rewards=False):
  """A flight's worth of replay input [steps, n_env]: terminals at term_p, time-limit ends at end_p.  distinct_rewards: 100 s + env + U,
  so that a return names its window.  obs: random rows [steps, n_env, 1099], or none (the tree does not read them)."""
  rng = np.random.default_rng(seed)
  h = {'action': rng.integers(0, 3, (steps, n_env)).astype(np.uint8)}
  if distinct_rewards:
    h['reward'] = (np.arange(steps)[:, None] * 100 + np.arange(n_env)[None, :] + rng.random((steps, n_env))).astype(np.float32)
  else:
    h['reward'] = rng.standard_normal((steps, n_env)).astype(np.float32)
  h['terminal'] = (rng.random((steps, n_env)) < term_p).astype(np.uint8)
  h['episode_end'] = np.maximum(h['terminal'], (rng.random((steps, n_env)) < end_p).astype(np.uint8))
  if obs:
    h['obs'] = rng.random((steps, n_env, 1099), dtype=np.float32)
  return h


def host_add(tree, ring, h, s):
  """Vector step s of history h into the ring's flags and the twin."""
  ring['terminal'][s % tree.T] = h['terminal'][s]
  ring['episode_end'][s % tree.T] = h['episode_end'][s]
  tree.add(ring['terminal'], ring['episode_end'])


def new_ring(capacity, n_env):
  return {'terminal': np.zeros((capacity, n_env), np.uint8), 'episode_end': np.zeros((capacity, n_env), np.uint8)}


def newest_step(last, capacity, row):
  """The newest vector step held in ring row `row` after step `last` was added."""
  return last - ((last % capacity) - row) % capacity


# The batch-by-batch draw test (test_gpu_prio_replay.py) and the CPU check of its precondition (test_prio_replay_host.py).
DRAW_CASE = dict(num_envs=65, capacity=12, horizon=5, steps=40, hist_seed=21, craft_seed=22, seed=11,
                 batches=(1, 64, 300, 1025), counters=(0, 2 ** 32 + 3))


def draw_case_tree(h):
  """The twin after DRAW_CASE's adds of history h (every nonzero leaf a complete valid window), then crafted priorities k / 7 on the
  nonzero leaves.  Returns (tree before crafting, tree after)."""
  c = DRAW_CASE
  fed = SumTree(c['capacity'], c['num_envs'], c['horizon'])
  ring = new_ring(c['capacity'], c['num_envs'])
  for s in range(c['steps']):
    host_add(fed, ring, h, s)
  crafted = SumTree(c['capacity'], c['num_envs'], c['horizon'])
  crafted.nodes[:] = fed.nodes
  crafted.count, crafted.max_priority = fed.count, fed.max_priority
  lv = crafted.leaf_view()
  valid = lv > 0
  lv[valid] = np.random.default_rng(c['craft_seed']).integers(1, 20, int(valid.sum())).astype(np.float64) / 7.0
  crafted.rebuild()
  return fed, crafted


def build_replay_draws(directory):
  """Compiles replay_draws.cpp (g++, products and sums rounded apart) into `directory`; returns draw(seed, batch, counter, tries) ->
  float64 [batch, tries], the philox_uniform draws of the replay stream (seed, b, counter)."""
  so = os.path.join(str(directory), 'libreplay_draws.so')
  subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include',
                         os.path.join(_HERE, 'emul', 'ble_intrinsics.h'), '-o', so, os.path.join(_HERE, 'replay_draws.cpp')])
  lib = ctypes.CDLL(so)
  lib.replay_draws.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
  lib.replay_draws.restype = None

  def draw(seed, batch, counter, tries=1):
    u = np.empty((batch, tries))
    lib.replay_draws(seed, batch, counter, tries, u.ctypes.data)
    return u
  return draw
