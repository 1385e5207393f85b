"""A population's prioritized replay on the host: P twins of prio_replay_host.SumTree over the column slices of ONE ring of
P * R columns, the grouped draw case of test_gpu_population_prio.py and the CPU check of its precondition
(test_population_prio_host.py).  TEST TOOLING."""
import ctypes

import numpy as np

import prio_replay_host as ph
from balloon_learning_environment_amd import _abi, _lib

FAKE = 0x100000          # a non-NULL, 16-byte aligned address (never dereferenced: the calls below have nothing to launch)


def member_columns(p, rows):
  return slice(p * rows, (p + 1) * rows)


class PopulationTrees:
  """Member p's tree is the solo twin of its column slice: leaf (t % T) R + r is the window of column p R + r."""

  def __init__(self, members, rows, capacity, horizon):
    self.P, self.R, self.T, self.n = int(members), int(rows), int(capacity), int(horizon)
    self.trees = [ph.SumTree(capacity, rows, horizon) for _ in range(self.P)]
    self.ring = ph.new_ring(capacity, self.P * self.R)

  def add(self, h, s):
    """Vector step s of history h [steps, P R] into the ring's flags and every member's twin."""
    self.ring['terminal'][s % self.T] = h['terminal'][s]
    self.ring['episode_end'][s % self.T] = h['episode_end'][s]
    for p, tree in enumerate(self.trees):
      cols = member_columns(p, self.R)
      tree.add(self.ring['terminal'][:, cols], self.ring['episode_end'][:, cols])

  def nodes(self):
    """[P, 2 padded]: what VecPopulationPrioritizedReplayBuffer.tree holds."""
    return np.stack([t.nodes for t in self.trees])

  def max_priority(self):
    return np.array([t.max_priority for t in self.trees])


def member_leaf(column, t, rows, capacity):
  """(member, leaf) of the window that starts at step t of ring column `column`."""
  p, r = divmod(int(column), int(rows))
  return p, (int(t) % int(capacity)) * int(rows) + r


def library_accepts(members, rows, capacity, horizon, leaves, padded, stride=None):
  """Whether the grouped entry points take these per-member tree sizes for a ring of members * rows columns: an empty batch, so nothing
  is launched and the answer is the argument check's alone."""
  rp = _abi.BleReplayF32(capacity, members * rows, horizon, 1104, 0.993, 64, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
  tr = _abi.BleSumTreeGroupedF64(members, leaves, padded, 2 * padded if stride is None else stride, FAKE, FAKE)
  bt = _abi.BleTrainBatchF32(0, 1104, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
  return _lib.lib().ble_replay_sample_prioritized_grouped_f32(ctypes.byref(rp), ctypes.byref(tr), FAKE, ctypes.byref(bt), FAKE, None, None) == 0


# The grouped draw test (test_gpu_population_prio.py) and the CPU check of its precondition, in the manner of ph.DRAW_CASE: 40 adds into
# 12 rows of 3 x 65 columns (the ring wraps three times), then crafted priorities k / 7, another draw of k per member.
POP_DRAW_CASE = dict(members=3, rows=65, capacity=12, horizon=5, steps=40, hist_seed=31, craft_seed=32, seeds=(11, 12, 13),
                     batches=(1, 33, 300), counters=(0, 2 ** 32 + 3))


def pop_draw_case_history():
  c = POP_DRAW_CASE
  return ph.history(c['steps'], c['members'] * c['rows'], c['hist_seed'], distinct_rewards=True)


def pop_draw_case_trees(h):
  """(the twins after the case's adds of history h, the twins with crafted priorities on the nonzero leaves)."""
  c = POP_DRAW_CASE
  fed = PopulationTrees(c['members'], c['rows'], c['capacity'], c['horizon'])
  for s in range(c['steps']):
    fed.add(h, s)
  crafted = PopulationTrees(c['members'], c['rows'], c['capacity'], c['horizon'])
  for p, (src, dst) in enumerate(zip(fed.trees, crafted.trees)):
    dst.nodes[:] = src.nodes
    dst.count, dst.max_priority = src.count, src.max_priority
    lv = dst.leaf_view()
    valid = lv > 0
    lv[valid] = np.random.default_rng(c['craft_seed'] + p).integers(1, 20, int(valid.sum())).astype(np.float64) / 7.0
    dst.rebuild()
  return fed, crafted


def pop_draw_case_leaves(draw, crafted, p, b, counter):
  """Member p's rows of a draw of b rows per member: (leaves [b], the rows whose query and its two fp64 neighbours do NOT walk to one
  leaf).  The device evaluates seg * b + u * seg as one expression and may fuse either product; the plain and the grouped kernel are
  two compilations of that statement, so a row is comparable when all three queries agree."""
  c = POP_DRAW_CASE
  tree = crafted.trees[p]
  q = tree.stratified_queries(draw(c['seeds'][p], b, counter)[:, 0])
  cands = [tree.find_candidates(float(x)) for x in q]
  split = [i for i, s in enumerate(cands) if len(s) != 1]
  return np.array([min(s) for s in cands], np.int64), split
