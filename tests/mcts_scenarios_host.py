"""The guided tree search in scenario winds as a host twin: the group step -- M scenario nodes to one G, one prior row, one
status -- and the backup of groups of ONE environment in Python floats (IEEE fp64, every operation rounded once), written from the rules
-- the issue's and include/ble_abi.h's prose -- and not from csrc/ble_mcts_scenarios.h.  Select and finish are mcts_host.Search's own:
the rules of a search do not change, a group's "status OK" is "not spent".

TEST TOOLING ONLY.  Node ids as in mcts_host; node (id, m) is scenario m of group id."""
import math

import numpy as np

import mcts_host
from mcts_host import EMPTY, EXPAND, REVISIT, THIRD  # noqa: F401  (re-exported for the tests)

FLY, CARRY, VOID = 0, 1, 2


def stopped(ok, acc):
  """A scenario node flies nothing more: its status is not OK or its acc is NaN."""
  return (not ok) or math.isnan(acc)


def group_spent(ok, acc):
  return all(stopped(ok[m], float(acc[m])) for m in range(len(acc)))


def group_values(acc, disc, ok, value=None):
  """[G_m]: acc_m + disc_m V_m, the product and the sum rounded once each; V_m = 0 without a guide and on a node that is not OK."""
  out = []
  for m in range(len(acc)):
    v_m = float(np.float32(value[m])) if (value is not None and ok[m]) else 0.0
    tail = float(disc[m]) * v_m
    out.append(float(acc[m]) + tail)
  return out


def group_g(acc, disc, ok, value, tail):
  """The group's G: the mean of the `tail` smallest G_m -- G_m ascending with -0 equal to +0, then m ascending --, summed in that order
  from 0.0 and divided once; NaN (void) if any G_m is not finite."""
  g = group_values(acc, disc, ok, value)
  if not all(math.isfinite(x) for x in g):
    return math.nan
  order = sorted(range(len(g)), key=lambda m: (g[m] + 0.0 if g[m] != 0.0 else 0.0, m))        # (-0.0 sorts as +0.0)
  total = 0.0
  for m in order[:int(tail)]:
    total = total + g[m]
  return total / float(int(tail))


def group_prior(ok, probs=None):
  """The group's prior row, float32 [3]: the mean of the probs rows of the nodes that are OK, m ascending, summed in double from 0.0,
  divided by their number once, rounded to float once; uniform without probs, without such a node, or if one of those rows has a
  non-finite or negative entry."""
  uniform = np.full(3, THIRD, np.float32)
  if probs is None:
    return uniform
  rows = [np.asarray(probs[m], np.float32) for m in range(len(ok)) if ok[m]]
  if not rows or any((not np.all(np.isfinite(row))) or np.any(row < 0) for row in rows):
    return uniform
  out = np.zeros(3, np.float32)
  for a in range(3):
    total = 0.0
    for row in rows:
      total = total + float(row[a])
    out[a] = np.float32(total / float(len(rows)))
  return out


def lane_rule(parent_ok, parent_acc, m, act):
  """What lane (m, act) of an EXPAND slot does, from its parent group (parent_acc None: the root, parent_ok [1] the environment's)."""
  if parent_acc is None:
    return FLY if parent_ok[0] else (CARRY if act == 0 else VOID)
  if not stopped(parent_ok[m], float(parent_acc[m])):
    return FLY
  return VOID if (group_spent(parent_ok, parent_acc) and act != 0) else CARRY


class Search(mcts_host.Search):
  """One environment's pool of groups.  self.ok[id]: the group is live (not spent).  group_g, group_status: [R, 3L] as the device keeps them."""

  def __init__(self, rounds, leaves, max_depth, c_puct, num, tail, root_ok=True, root_prior=None):
    super().__init__(rounds, leaves, max_depth, c_puct, root_ok, root_prior)
    self.M, self.tail = int(num), int(tail)
    self.group_g = np.zeros((self.R, 3 * self.L), np.float64)
    self.group_status = np.zeros((self.R, 3 * self.L), np.uint8)

  def backup(self, acc, disc, ok, value=None, probs=None):
    """The round's 3L M nodes as the expansion stored them, [3L, M] each (value [3L, M], probs [3L, M, 3] or None)."""
    first, r = self.born, (self.born - 1) // (3 * self.L)
    for l in range(self.L):
      v, what = int(self.leaf[l]), int(self.kind[l])
      grown = what == EXPAND
      for a in range(3):
        c, j = first + 3 * l + a, 3 * l + a
        self.parent[c] = v if grown else -1
        self.depth[c] = self.depth[v] + 1 if grown else 0
        self.first_child[c] = 0
        self.prior[c] = group_prior(ok[j], None if probs is None else probs[j])
        spent = group_spent(ok[j], acc[j])
        self.ok[c] = not spent
        self.group_status[r, j] = 1 if spent else 0
        G = group_g(acc[j], disc[j], ok[j], None if value is None else value[j], self.tail) if grown else math.nan
        self.group_g[r, j] = G
        if math.isnan(G):
          self.visits[c], self.value_sum[c], self.g[c] = 0, 0.0, math.nan
          continue
        self.g[c], self.visits[c], self.value_sum[c] = G, 1, G
        self.g_lo, self.g_hi = (G if G < self.g_lo else self.g_lo), (G if G > self.g_hi else self.g_hi)
        for u in self._path(v):
          self.visits[u] += 1
          self.value_sum[u] = float(self.value_sum[u]) + G
      if grown:
        self.first_child[v] = first + 3 * l
      if what == REVISIT:
        G = float(self.g[v])
        for u in self._path(v):
          self.visits[u] += 1
          self.value_sum[u] = float(self.value_sum[u]) + G
    self.pending[:] = 0
    self.born = first + 3 * self.L
