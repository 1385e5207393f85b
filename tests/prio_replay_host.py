"""An fp64 NumPy restatement of the device's prioritized n-step replay (csrc/ble_replay.h): the sum tree over
capacity x num_envs windows, the insertion rule, the stratified walk from given uniforms, set_priority with the later row winning, the
max recorded priority and the reported (weighted) loss."""
import numpy as np


def window_valid(terminal, episode_end, t, env, n):
  """ble_train.h replay_window over the ring arrays [T, N]: no episode end before the first terminal among t .. t + n - 1."""
  cap = terminal.shape[0]
  for k in range(n):
    if terminal[(t + k) % cap, env]:
      return True
    if episode_end[(t + k) % cap, env]:
      return False
  return True


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
    """Every parent = left + right, from the leaves up (the tree is a pure function of its leaves)."""
    for i in range(self.P - 1, 0, -1):
      self.nodes[i] = self.nodes[2 * i] + self.nodes[2 * i + 1]

  def add(self, terminal, episode_end):
    """After vector step s = count was written into the ring arrays [T, N]: zero row s % T, row (s - n) % T to the max (valid windows)."""
    s = self.count
    self.count += 1
    lv = self.leaf_view()
    lv[s % self.T] = 0.0
    if s >= self.n:
      for e in range(self.N):
        lv[(s - self.n) % self.T, e] = self.max_priority if window_valid(terminal, episode_end, s - self.n, e, self.n) else 0.0
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
