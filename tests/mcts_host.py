"""The guided tree search as a host twin: select, backup and finish of ONE environment in Python floats (IEEE fp64, every
operation rounded once), written from the rules -- the issue's and include/ble_abi.h's prose -- and not from csrc/ble_mcts.h.

TEST TOOLING ONLY.  Node ids: 0 the root, 1 + r 3L + 3l + a the child under action a of slot l of round r."""
import math

import numpy as np

EMPTY, EXPAND, REVISIT = 0, 1, 2
STAY = 1
NINF32 = np.float32(-np.inf)
THIRD = np.float32(1.0) / np.float32(3.0)


def clean_prior(row):
  """A probs row as the pool keeps it: float32 [3]; a row with a non-finite or negative entry (or no row) is uniform."""
  if row is None:
    return np.full(3, THIRD, np.float32)
  row = np.asarray(row, np.float32)
  if not np.all(np.isfinite(row)) or np.any(row < 0):
    return np.full(3, THIRD, np.float32)
  return row.copy()


class Search:
  """One environment's pool.  Arrays over the cap = 1 + 3 L R ids, as the device keeps them."""

  def __init__(self, rounds, leaves, max_depth, c_puct, root_ok=True, root_prior=None):
    self.R, self.L, self.D, self.c = int(rounds), int(leaves), int(max_depth), float(c_puct)
    cap = 1 + 3 * self.L * self.R
    self.cap = cap
    self.parent = np.full(cap, -1, np.int32)
    self.first_child = np.zeros(cap, np.int32)
    self.depth = np.zeros(cap, np.int32)
    self.visits = np.zeros(cap, np.int32)
    self.pending = np.zeros(cap, np.int32)
    self.value_sum = np.zeros(cap, np.float64)
    self.g = np.zeros(cap, np.float64)
    self.prior = np.zeros((cap, 3), np.float32)
    self.prior[0] = clean_prior(root_prior)
    self.ok = np.zeros(cap, bool)
    self.ok[0] = bool(root_ok)
    self.g_lo, self.g_hi = math.inf, -math.inf
    self.born = 1                   # ids born so far
    self.leaf = np.zeros(self.L, np.int32)
    self.kind = np.zeros(self.L, np.int32)

  # -- selection
  def _score(self, node, a, child):
    visits, nv = float(self.visits[child]), float(self.visits[child] + self.pending[child])
    mean = float(self.value_sum[child]) / visits
    qn = 0.0
    if self.g_hi - self.g_lo > 0.0:
      qn = (mean - self.g_lo) / (self.g_hi - self.g_lo)
    qn = qn * (visits / nv)
    u = self.c * float(self.prior[node, a])
    u = u * math.sqrt(float(self.visits[node] + self.pending[node]))
    u = u / (1.0 + nv)
    return qn + u

  def _path(self, v):
    while v >= 0:
      yield v
      v = int(self.parent[v])

  def select(self):
    """The L descents of the next round -> (leaf [L], kind [L])."""
    for l in range(self.L):
      v, what = 0, EMPTY
      if self.ok[0]:
        while True:
          fc = int(self.first_child[v])
          if fc == 0:
            chosen = any(self.kind[k] == EXPAND and self.leaf[k] == v for k in range(l))
            what = EMPTY if chosen else (REVISIT if (not self.ok[v] or self.depth[v] == self.D) else EXPAND)
            break
          best, best_score = -1, 0.0
          for a in range(3):
            if self.visits[fc + a] == 0:
              continue                       # void
            score = self._score(v, a, fc + a)
            if best < 0 or score > best_score:
              best, best_score = fc + a, score
          if best < 0:                       # three void children: the node cannot grow (the root: nothing to count)
            what = EMPTY if v == 0 else REVISIT
            break
          v = best
      self.leaf[l], self.kind[l] = v, what
      for u in self._path(v):
        self.pending[u] += 3 if what == EXPAND else (1 if what == REVISIT else 0)
    return self.leaf.copy(), self.kind.copy()

  # -- backup
  def backup(self, acc, disc, ok, value=None, probs=None):
    """The round's 3L nodes as the expansion stored them (acc NaN: void), the network's value [3L] and probs [3L, 3] or None."""
    first = self.born
    for l in range(self.L):
      v, what = int(self.leaf[l]), int(self.kind[l])
      for a in range(3):
        c, j = first + 3 * l + a, 3 * l + a
        grown = what == EXPAND
        self.parent[c] = v if grown else -1
        self.depth[c] = self.depth[v] + 1 if grown else 0
        self.first_child[c] = 0
        self.prior[c] = clean_prior(None if probs is None else probs[j])
        self.ok[c] = bool(ok[j])
        if not grown or math.isnan(acc[j]):
          self.visits[c], self.value_sum[c], self.g[c] = 0, 0.0, math.nan
          continue
        v_c = float(np.float32(value[j])) if (value is not None and ok[j]) else 0.0
        tail = float(disc[j]) * v_c
        G = float(acc[j]) + tail
        self.g[c], self.visits[c], self.value_sum[c] = G, 1, G
        self.g_lo, self.g_hi = (G if G < self.g_lo else self.g_lo), (G if G > self.g_hi else self.g_hi)
        for u in self._path(v):
          self.visits[u] += 1
          self.value_sum[u] = float(self.value_sum[u]) + G
      if what == EXPAND:
        self.first_child[v] = first + 3 * l
      if what == REVISIT:
        G = float(self.g[v])
        for u in self._path(v):
          self.visits[u] += 1
          self.value_sum[u] = float(self.value_sum[u]) + G
    self.pending[:] = 0
    self.born = first + 3 * self.L

  # -- finish
  def _best_child(self, fc):
    best, best_n, best_q, q, n = -1, 0, NINF32, np.full(3, NINF32, np.float32), np.zeros(3, np.int32)
    for a in range(3):
      n[a] = self.visits[fc + a]
      if n[a] > 0:
        q[a] = np.float32(float(self.value_sum[fc + a]) / float(n[a]))
      if n[a] > 0 and (best < 0 or n[a] > best_n or (n[a] == best_n and q[a] > best_q)):
        best, best_n, best_q = a, n[a], q[a]
    return best, q, n

  def finish(self, segment):
    """-> dict(action, best_return, q [3], visits [3], best_plan [D * segment], pv_length)."""
    out = dict(action=STAY, best_return=np.float32(0.0), q=np.full(3, NINF32, np.float32), visits=np.zeros(3, np.int32),
               best_plan=np.full(self.D * segment, STAY, np.uint8), pv_length=0)
    if not self.ok[0]:
      return out
    out['best_return'] = NINF32
    v, path = 0, []
    while len(path) < self.D and self.first_child[v] != 0:
      a, q, n = self._best_child(int(self.first_child[v]))
      if v == 0:
        out['q'], out['visits'] = q, n
      if a < 0:
        break
      if v == 0:
        out['action'], out['best_return'] = a, q[a]
      path.append(a)
      v = int(self.first_child[v]) + a
    out['pv_length'] = len(path)
    out['best_plan'][:len(path) * segment] = np.repeat(np.array(path, np.uint8), segment)
    return out


def check_invariants(leaves, parent, visits, value_sum, g, rounds):
  """The two invariants of a pool after len(rounds) rounds, from its arrays alone.  rounds: [(leaf [L], kind [L])] per round.  The
  events of the search in backup order -- a non-void newborn c (g[c] not NaN) counts (c, g[c]), a REVISIT of v counts (v, g[v]) -- are
  replayed up the parent links: visits[node] is the number of events in its subtree (itself included; nothing is ever counted ON the
  root, only through it) and value_sum[node] their G added in that order, to the bit."""
  cap = len(parent)
  count, total = np.zeros(cap, np.int64), np.zeros(cap, np.float64)
  for r, (leaf, kind) in enumerate(rounds):
    for l in range(leaves):
      events = []
      if kind[l] == EXPAND:
        events = [1 + 3 * leaves * r + 3 * l + a for a in range(3)]
        events = [(int(parent[c]), c) for c in events if not math.isnan(g[c])]
      elif kind[l] == REVISIT:
        events = [(int(leaf[l]), int(leaf[l]))]
      for start, source in events:
        if source != start:                        # a newborn: itself first
          count[source] += 1
          total[source] = total[source] + g[source]
        u = start
        while u >= 0:
          count[u] += 1
          total[u] = total[u] + g[source]
          u = int(parent[u])
  born = 1 + 3 * leaves * len(rounds)
  assert np.array_equal(np.asarray(visits[:born], np.int64), count[:born]), (visits[:born], count[:born])
  assert np.array_equal(np.asarray(value_sum[:born], np.float64).view(np.uint64), total[:born].view(np.uint64))
  return count
