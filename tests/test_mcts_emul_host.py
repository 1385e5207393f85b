"""The guided tree search without a GPU: the select, backup and finish lane functions of csrc/ble_mcts.h, built for the host
(tests/emul/mcts_emul.cpp), against the float64 twin written from the rules (tests/mcts_host.py), on whole searches over synthetic edges:
an edge is a table entry (reward, status, void) keyed by its path, so nothing is flown.  Integers and bits, no tolerance."""
import math

import numpy as np
import pytest

import mcts_host
from mcts_host import EMPTY, EXPAND, REVISIT, STAY
from emul import mcts_emul

GAMMA = 0.993
NAN = float('nan')


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _edge(seed, path, kind):
  """The table: what flying `path` (a tuple of actions) ends in -> (reward of its last edge, status, void)."""
  rng = np.random.default_rng([seed, len(path), *path])
  reward = float(rng.integers(0, 2)) * 0.5 if kind == 'ties' else float(rng.uniform(-1.0, 1.0))
  if kind == 'equal':
    return 0.25, 0, False
  return reward, (2 if rng.random() < 0.2 else 0), bool(rng.random() < 0.15)


def _network(rng, rows, kind):
  """(value [rows] f32, probs [rows, 3] f32) of random weights: some rows non-finite or negative."""
  value = rng.standard_normal(rows).astype(np.float32)
  probs = rng.random((rows, 3)).astype(np.float32)
  probs /= probs.sum(1, keepdims=True)
  for j in range(rows):
    if rng.random() < 0.12:
      probs[j, rng.integers(0, 3)] = [NAN, np.inf, -0.25][rng.integers(0, 3)]
  if kind == 'equal':
    value[:] = 0.5
  return value, probs


class _Run:
  """One search, the emulation and the twin in step.  counts: how often each kind of slot and a void child occurred."""

  def __init__(self, R, L, D, c_puct, seed, kind='random', guide=True, source_status=0, root_prior=None, void_root=False):
    self.R, self.L, self.D, self.seed, self.kind_of, self.guide, self.void_root = R, L, D, seed, kind, guide, void_root
    self.emul = mcts_emul.Pool(R, L, D, c_puct, source_status, root_prior)
    self.twin = mcts_host.Search(R, L, D, c_puct, source_status == 0, root_prior)
    self.rng = np.random.default_rng(seed)
    self.paths, self.node = {0: ()}, {0: (0.0, 1.0)}          # id -> path, id -> (acc, disc)
    self.rounds, self.counts = [], {EMPTY: 0, EXPAND: 0, REVISIT: 0, 'void': 0}
    self.sanitised = 0

  def round(self, r):
    L = self.L
    leaf, kind = self.emul.select(r)
    want_leaf, want_kind = self.twin.select()
    assert np.array_equal(kind, want_kind) and np.array_equal(leaf, want_leaf), (r, leaf, kind, want_leaf, want_kind)
    assert np.array_equal(self.emul.pending[:1 + 3 * L * r], self.twin.pending[:1 + 3 * L * r])
    acc, disc, status = np.full(3 * L, NAN), np.ones(3 * L), np.zeros(3 * L, np.uint8)
    for l in range(L):
      self.counts[int(kind[l])] += 1
      if kind[l] != EXPAND:
        continue
      assert leaf[l] in self.paths and leaf[l] not in [leaf[k] for k in range(l) if kind[k] == EXPAND]
      for a in range(3):
        path = self.paths[int(leaf[l])] + (a,)
        reward, st, void = _edge(self.seed, path, self.kind_of)
        void = void or self.void_root
        p_acc, p_disc = self.node[int(leaf[l])]
        j, c = 3 * l + a, 1 + 3 * L * r + 3 * l + a
        term = p_disc * reward
        acc[j], disc[j], status[j] = (NAN if void else p_acc + term), p_disc * GAMMA, st
        self.counts['void'] += int(void)
        if not void:
          self.paths[c], self.node[c] = path, (acc[j], disc[j])
    value, probs = _network(self.rng, 3 * L, self.kind_of) if self.guide else (None, None)
    self.emul.backup(r, acc, disc, status, value, probs)
    self.twin.backup(acc, disc, status == 0, value, probs)
    self.rounds.append((leaf, kind))
    born = 1 + 3 * L * (r + 1)
    for name in ('parent', 'first_child', 'depth', 'visits', 'pending'):
      assert np.array_equal(getattr(self.emul, name)[:born], getattr(self.twin, name)[:born]), (r, name)
    for name in ('value_sum', 'g', 'prior'):
      assert np.array_equal(_bits(getattr(self.emul, name)[:born]), _bits(getattr(self.twin, name)[:born])), (r, name)
    assert np.array_equal(_bits(self.emul.g_range), _bits(np.array([self.twin.g_lo, self.twin.g_hi])))
    # the two invariants, from the emulation's arrays alone
    mcts_host.check_invariants(L, self.emul.parent[:born], self.emul.visits, self.emul.value_sum, self.emul.g, self.rounds)
    # a row with a non-finite or negative entry became uniform, every other row is kept to the bit
    if probs is not None:
      for j in range(3 * L):
        bad = not np.all(np.isfinite(probs[j])) or np.any(probs[j] < 0)
        want = np.full(3, mcts_host.THIRD, np.float32) if bad else probs[j]
        assert np.array_equal(_bits(self.emul.prior[born - 3 * L + j]), _bits(want))
        self.sanitised += int(bad)

  def run(self):
    for r in range(self.R):
      self.round(r)
    return self

  def finish(self, segment=2):
    got, want = self.emul.finish(segment), self.twin.finish(segment)
    assert got['action'] == want['action'] and got['pv_length'] == want['pv_length']
    assert np.array_equal(got['best_plan'], want['best_plan']) and np.array_equal(got['visits'], want['visits'])
    assert np.array_equal(_bits(got['q']), _bits(want['q'])) and _bits(np.float32(got['best_return'])) == _bits(np.float32(want['best_return']))
    return got


@pytest.mark.parametrize('kind', ['random', 'ties'])
@pytest.mark.parametrize('guide', [True, False])
@pytest.mark.parametrize('D', [2, 4])
@pytest.mark.parametrize('L', [1, 3])
def test_whole_searches_equal_the_twin(L, D, guide, kind):
  totals = {EMPTY: 0, EXPAND: 0, REVISIT: 0, 'void': 0}
  sanitised = 0
  for seed in range(8):
    for c_puct in (1.25, 0.0):
      run = _Run(6, L, D, c_puct, 1000 * L + 10 * D + seed, kind, guide).run()
      got = run.finish(segment=1 + seed % 3)
      segment = 1 + seed % 3
      # the principal variation: pv_length edges, each repeated over its segment, then STAY
      assert 0 <= got['pv_length'] <= D and np.all(got['best_plan'][got['pv_length'] * segment:] == STAY)
      if got['pv_length'] > 0:
        assert got['best_plan'][0] == got['action'] and got['visits'][got['action']] == got['visits'].max()
        assert np.all(got['best_plan'][:got['pv_length'] * segment].reshape(-1, segment) == got['best_plan'][:got['pv_length'] * segment:segment, None])
      for k in totals:
        totals[k] += run.counts[k]
      sanitised += run.sanitised
  # every kind of slot and a void child occurred (an EMPTY slot needs a second descent in the round)
  assert totals[EXPAND] > 0 and totals[REVISIT] > 0 and totals['void'] > 0, totals
  assert L == 1 or totals[EMPTY] > 0, totals
  assert not guide or sanitised > 0


def test_ties_go_to_the_lower_action():
  """Equal rewards, equal values, uniform priors: g_hi == g_lo, every score of a level is one number, and the descent takes action 0."""
  run = _Run(4, 1, 3, 1.25, 7, 'equal', guide=False)
  run.round(0)
  run.round(1)
  assert run.rounds[1][0][0] == 1 and run.rounds[1][1][0] == EXPAND         # the root's child under action 0
  # the score itself: equal inputs, equal bits; a larger prior, a larger score
  a = mcts_emul.score(1.5, 3, 0, 0.0, 1.0, 1.25, np.float32(1 / 3), 9)
  assert a == mcts_emul.score(1.5, 3, 0, 0.0, 1.0, 1.25, np.float32(1 / 3), 9) and a < mcts_emul.score(1.5, 3, 0, 0.0, 1.0, 1.25, np.float32(0.5), 9)
  # finish: equal visits -> the larger q; equal q as well -> the lower action
  pool = mcts_emul.Pool(1, 1, 2, 1.0)
  pool.select(0)
  pool.backup(0, [1.0, 2.0, 2.0], [1.0] * 3, [0, 0, 0])
  got = pool.finish(1)
  assert got['action'] == 1 and got['visits'].tolist() == [1, 1, 1] and got['best_return'] == 2.0 and got['pv_length'] == 1
  pool = mcts_emul.Pool(1, 1, 2, 1.0)
  pool.select(0)
  pool.backup(0, [3.0, 3.0, 3.0], [1.0] * 3, [0, 0, 0])
  assert pool.finish(1)['action'] == 0


def test_one_hot_root_prior_leads_the_first_expansions():
  for hot in range(3):
    prior = np.zeros(3, np.float32)
    prior[hot] = 1.0
    run = _Run(4, 1, 3, 1.25, 11 + hot, 'equal', guide=False, root_prior=prior)
    for r in range(3):
      run.round(r)
    assert run.rounds[0][0][0] == 0 and run.rounds[1][0][0] == 1 + hot      # the root, then its child under the hot action
    assert run.emul.parent[run.rounds[2][0][0]] == 1 + hot                  # then a child of that child


def test_without_exploration_the_search_descends_by_value():
  """c_puct = 0: the score is Qn alone, so round 1 grows the root's child of the largest G (ties to the lower action)."""
  for seed in range(12):
    run = _Run(3, 1, 3, 0.0, 300 + seed, 'random', guide=True)
    run.round(0)
    g = run.emul.g[1:4].copy()
    if np.all(np.isnan(g)):
      continue
    run.round(1)
    leaf, kind = run.rounds[1]
    alive = [a for a in range(3) if not math.isnan(g[a])]
    best = max(alive, key=lambda a: (g[a], -a))
    assert leaf[0] == 1 + best and kind[0] in (EXPAND, REVISIT)
    # what the node cannot do decides the kind: a dead node is revisited
    assert (kind[0] == REVISIT) == (run.emul.status[0, best] != 0)


def test_dead_root_and_all_void_root():
  dead = _Run(3, 2, 2, 1.25, 5, 'random', guide=True, source_status=2).run()
  assert dead.counts[EMPTY] == 6 and dead.counts[EXPAND] == 0 and dead.counts[REVISIT] == 0
  got = dead.finish(segment=3)
  assert got['action'] == STAY and np.all(got['best_plan'] == STAY) and got['pv_length'] == 0
  assert _bits(np.float32(got['best_return'])) == 0 and np.all(got['visits'] == 0) and np.all(np.isneginf(got['q']))       # +0.0f
  void = _Run(3, 2, 2, 1.25, 6, 'random', guide=True, void_root=True).run()
  assert void.counts[EXPAND] == 1 and void.counts['void'] == 3 and void.counts[EMPTY] == 5
  got = void.finish(segment=3)
  assert got['action'] == STAY and np.all(got['best_plan'] == STAY) and got['pv_length'] == 0
  assert np.isneginf(got['best_return']) and np.all(got['visits'] == 0) and np.all(np.isneginf(got['q']))


def test_pv_length_and_padding():
  """A search deep enough to reach max_depth: the variation is followed to a node without children and padded with STAY."""
  run = _Run(6, 3, 2, 1.25, 42, 'equal', guide=False).run()
  got = run.finish(segment=4)
  assert got['pv_length'] == 2 and len(got['best_plan']) == 8
  assert np.all(got['best_plan'][:4] == got['action']) and np.all(got['best_plan'][4:] == got['best_plan'][4])
  shallow = _Run(1, 1, 4, 1.25, 42, 'equal', guide=False).run()
  got = shallow.finish(segment=2)
  assert got['pv_length'] == 1 and np.all(got['best_plan'][2:] == STAY) and np.all(got['best_plan'][:2] == got['action'])
