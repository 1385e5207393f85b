"""The guided tree search in scenario winds without a GPU: the group functions of csrc/ble_mcts_scenarios.h, built for the host
(tests/emul/mcts_scenarios_emul.cpp), against the float64 twin written from the rules (tests/mcts_scenarios_host.py) -- first the group
step alone on hand-made and random groups, then whole searches over synthetic edges in test_mcts_emul_host.py's manner: an edge is a
table entry (reward, status) keyed by (path, m), so nothing is flown.  Select and finish are the plain search's own emulation and twin
(imported, not copied), fed the groups' status.  Integers and bits, no tolerance."""
import math

import numpy as np
import pytest

import mcts_host
import mcts_scenarios_host as twin_lib
from mcts_scenarios_host import EMPTY, EXPAND, REVISIT, FLY, CARRY, VOID, THIRD
from emul import mcts_scenarios_emul as emul_lib

GAMMA = 0.993
NAN, INF = float('nan'), float('inf')
KINDS = (EMPTY, EXPAND, REVISIT, 'void', 'stopped_in_live', 'spent')


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_group(acc, disc, status, value, probs, tail):
  """The emulation's group step against the twin's, to the bit -> (G, prior, spent)."""
  ok = [s == 0 for s in status]
  g, prior, spent = emul_lib.group(acc, disc, status, value, probs, tail)
  want_g = twin_lib.group_g(acc, disc, ok, value, tail)
  want_prior = twin_lib.group_prior(ok, probs)
  assert _bits(np.float64(g)) == _bits(np.float64(want_g)) or (math.isnan(g) and math.isnan(want_g)), (g, want_g)
  assert np.array_equal(_bits(prior), _bits(want_prior)), (prior, want_prior)
  assert spent == int(twin_lib.group_spent(ok, acc))
  return g, prior, spent


# ---------------------------------------------------------------------------------------------------------------- the group step
def test_ties_with_signed_zeros_and_equal_values():
  """-0.0 and +0.0 are one key, equal G_m go by m: the sum takes them in m order, which the sign of a zero sum shows."""
  ones, live = [1.0] * 3, [0, 0, 0]
  g, _, _ = _same_group([-0.0, 0.0, 5.0], ones, live, None, None, 1)
  assert _bits(np.float64(g)) == _bits(np.float64(0.0 + -0.0))               # m = 0 first: 0.0 + (-0.0) = +0.0
  g, _, _ = _same_group([0.0, -0.0, -0.0], ones, live, None, None, 3)
  assert _bits(np.float64(g)) == 0
  g, _, _ = _same_group([-0.0, -0.0, 1.0], ones, live, None, None, 2)
  assert _bits(np.float64(g)) == 0                                           # the sum starts from +0.0
  # equal G_m at different m, a tail that cuts between them: the same number whichever is taken, and the twin agrees on the order
  g, _, _ = _same_group([2.0, 1.0, 1.0, 3.0], [1.0] * 4, [0] * 4, None, None, 1)
  assert g == 1.0
  g, _, _ = _same_group([2.0, 1.0, 1.0, 3.0], [1.0] * 4, [0] * 4, None, None, 3)
  assert g == 4.0 / 3.0
  # tail = M: the expectation; tail = 1: the worst case; a sum whose order matters in the last bit
  acc = [0.1, 1e16, -1e16, 0.3]
  g, _, _ = _same_group(acc, [1.0] * 4, [0] * 4, None, None, 4)
  assert g == (((0.0 + -1e16) + 0.1) + 0.3 + 1e16) / 4.0
  assert _same_group(acc, [1.0] * 4, [0] * 4, None, None, 1)[0] == -1e16


def test_values_enter_live_nodes_only():
  acc, disc = [1.0, 2.0, 3.0], [0.5, 0.25, 0.125]
  # a stopped node (status not OK) keeps its return whatever the network says of it: NaN and Inf there are ignored
  for junk in (NAN, INF, -INF, 7.0):
    g, _, spent = _same_group(acc, disc, [0, 2, 0], [1.0, junk, 1.0], None, 3)
    assert g == ((1.0 + 0.5) + 2.0 + (3.0 + 0.125)) / 3.0 and spent == 0
  # on a live node a non-finite value voids the group
  for junk in (NAN, INF, -INF):
    g, _, spent = _same_group(acc, disc, [0, 2, 0], [1.0, 1.0, junk], None, 1)
    assert math.isnan(g) and spent == 0
  # a node whose acc is NaN, an acc that is infinite: void
  assert math.isnan(_same_group([1.0, NAN, 3.0], disc, [0, 0, 0], None, None, 1)[0])
  assert math.isnan(_same_group([1.0, -INF, 3.0], disc, [0, 0, 0], None, None, 1)[0])
  # spent: all stopped (a terminal, a NaN acc); void: all NaN
  g, _, spent = _same_group([1.0, 2.0], [1.0, 1.0], [2, 3], [5.0, 5.0], None, 2)
  assert g == 1.5 and spent == 1
  g, _, spent = _same_group([NAN, NAN], [1.0, 1.0], [0, 0], None, None, 2)
  assert math.isnan(g) and spent == 1
  g, _, spent = _same_group([1.0, NAN], [1.0, 1.0], [2, 0], None, None, 1)
  assert math.isnan(g) and spent == 1


def test_prior_is_the_mean_of_the_live_rows():
  rows = np.array([[0.2, 0.3, 0.5], [0.6, 0.3, 0.1], [0.1, 0.1, 0.8]], np.float32)
  acc, disc = [1.0, 2.0, 3.0], [1.0] * 3
  _, prior, _ = _same_group(acc, disc, [0, 0, 0], [0.0] * 3, rows, 3)
  want = np.float32((rows.astype(np.float64)[0] + rows.astype(np.float64)[1] + rows.astype(np.float64)[2]) / 3.0)
  assert np.array_equal(_bits(prior), _bits(want))
  # a stopped node's row does not count, be it garbage
  bad = rows.copy()
  bad[1] = [NAN, -1.0, INF]
  _, prior, _ = _same_group(acc, disc, [0, 2, 0], [0.0] * 3, bad, 3)
  assert np.array_equal(_bits(prior), _bits(np.float32((rows.astype(np.float64)[0] + rows.astype(np.float64)[2]) / 2.0)))
  # a contributing row with a NaN or a negative entry, no contributing row, no guide: uniform
  uniform = _bits(np.full(3, THIRD, np.float32))
  for entry in (NAN, -0.25, INF):
    bad = rows.copy()
    bad[2, 1] = entry
    assert np.array_equal(_bits(_same_group(acc, disc, [0, 0, 0], [0.0] * 3, bad, 3)[1]), uniform)
  assert np.array_equal(_bits(_same_group(acc, disc, [2, 2, 3], [0.0] * 3, rows, 3)[1]), uniform)
  assert np.array_equal(_bits(_same_group(acc, disc, [0, 0, 0], None, None, 3)[1]), uniform)


@pytest.mark.parametrize('M', [1, 2, 3, 8, 16])
def test_random_groups_equal_the_twin(M):
  rng = np.random.default_rng(100 + M)
  seen = dict(void=0, spent=0, stopped_in_live=0, live=0, bad_row=0, zero_tie=0)
  for case in range(300):
    acc = rng.choice([-0.0, 0.0, 0.25, -0.5, 1.0], M) if case % 3 == 0 else rng.uniform(-2, 2, M)
    disc = GAMMA ** rng.integers(0, 12, M)
    status = np.where(rng.random(M) < (0.8 if case % 7 == 0 else 0.25), 2, 0).astype(np.uint8)
    acc = np.where(rng.random(M) < (0.9 if case % 11 == 0 else 0.03), NAN, acc)
    value = rng.choice([0.0, -0.0, 0.5], M).astype(np.float32) if case % 3 == 0 else rng.standard_normal(M).astype(np.float32)
    value = np.where(rng.random(M) < 0.06, rng.choice([NAN, INF, -INF], M), value).astype(np.float32)
    probs = rng.random((M, 3)).astype(np.float32)
    probs /= probs.sum(1, keepdims=True)
    for m in range(M):
      if rng.random() < 0.08:
        probs[m, rng.integers(0, 3)] = [NAN, INF, -0.25][rng.integers(0, 3)]
    guided = case % 4 != 0
    for tail in sorted({1, min(2, M), M}):
      g, _, spent = _same_group(acc, disc, status, value if guided else None, probs if guided else None, tail)
    stopped = [twin_lib.stopped(status[m] == 0, acc[m]) for m in range(M)]
    seen['void'] += math.isnan(g)
    seen['spent'] += spent
    seen['stopped_in_live'] += (not spent) and any(stopped)
    seen['live'] += not math.isnan(g)
    seen['bad_row'] += guided and any((not np.all(np.isfinite(probs[m]))) or np.any(probs[m] < 0) for m in range(M) if status[m] == 0)
    seen['zero_tie'] += sum(float(x) == 0.0 for x in acc) >= 2
  assert all(v > 0 for k, v in seen.items() if not (M == 1 and k in ('stopped_in_live', 'zero_tie'))), seen


def test_lane_rule_is_the_scenario_trees():
  """The expand's rule per lane, the emulation's (tree_scenario_lane) against the twin's prose."""
  rng = np.random.default_rng(5)
  seen = set()
  for _ in range(200):
    M = int(rng.integers(1, 5))
    status = np.where(rng.random(M) < 0.4, 2, 0).astype(np.uint8)
    acc = np.where(rng.random(M) < 0.2, NAN, rng.uniform(-1, 1, M))
    for m in range(M):
      for act in range(3):
        got = emul_lib.lane_rule(status, acc, m, act)
        assert got == twin_lib.lane_rule(status == 0, acc, m, act)
        seen.add(got)
  for root_status in (0, 2):
    for act in range(3):
      got = emul_lib.lane_rule([root_status], None, 0, act)
      assert got == twin_lib.lane_rule([root_status == 0], None, 0, act) == (FLY if root_status == 0 else (CARRY if act == 0 else VOID))
  assert seen == {FLY, CARRY, VOID}


# ---------------------------------------------------------------------------------------------------------------- whole searches
def _edge(seed, path, m, harsh):
  """The table: what flying `path` (a tuple of actions) in scenario m ends in -> (reward of its last edge, status)."""
  rng = np.random.default_rng([seed, m, len(path), *path])
  reward = float(rng.integers(-1, 2)) * 0.5 if seed % 3 == 0 else float(rng.uniform(-1.0, 1.0))        # (some tables tie, zeros included)
  return reward, (2 if rng.random() < (0.55 if harsh else 0.2) else 0)


def _void_edge(seed, path):
  """Whether the table makes the whole child group under `path` void (an edge that flew nothing in any scenario)."""
  return bool(np.random.default_rng([seed, 77, len(path), *path]).random() < 0.1)


def _network(rng, rows, M):
  """(value [rows, M] f32, probs [rows, M, 3] f32) of random weights: some values non-finite, some rows non-finite or negative."""
  value = rng.standard_normal((rows, M)).astype(np.float32)
  value = np.where(rng.random((rows, M)) < 0.05, rng.choice([NAN, INF, -INF], (rows, M)), value).astype(np.float32)
  probs = rng.random((rows, M, 3)).astype(np.float32)
  probs /= probs.sum(2, keepdims=True)
  for j in range(rows):
    for m in range(M):
      if rng.random() < 0.08:
        probs[j, m, rng.integers(0, 3)] = [NAN, INF, -0.25][rng.integers(0, 3)]
  return value, probs


class _Run:
  """One search over groups, the emulation and the twin in step.  counts: how often each kind of slot and of group occurred."""

  def __init__(self, R, L, D, M, tail, c_puct, seed, guide=True, source_status=0):
    self.R, self.L, self.D, self.M, self.seed, self.guide = R, L, D, M, seed, guide
    self.emul = emul_lib.Pool(R, L, D, c_puct, M, tail, source_status)
    self.twin = twin_lib.Search(R, L, D, c_puct, M, tail, source_status == 0)
    self.rng = np.random.default_rng(seed)
    self.root_status = source_status
    self.paths = {0: ()}                         # id -> path
    self.node = {}                               # id -> (acc [M], disc [M], status [M]) of a non-void group
    self.rounds, self.counts = [], {k: 0 for k in KINDS}
    self.edge = _edge

  def round(self, r):
    L, M = self.L, self.M
    leaf, kind = self.emul.select(r)
    want_leaf, want_kind = self.twin.select()
    assert np.array_equal(kind, want_kind) and np.array_equal(leaf, want_leaf), (r, leaf, kind, want_leaf, want_kind)
    assert np.array_equal(self.emul.pending[:1 + 3 * L * r], self.twin.pending[:1 + 3 * L * r])
    # what the expansion stores: a slot that does not grow holds the source's words with acc NaN
    acc, disc = np.full((3 * L, M), NAN), np.ones((3 * L, M))
    status = np.full((3 * L, M), self.root_status, np.uint8)
    for l in range(L):
      self.counts[int(kind[l])] += 1
      v = int(leaf[l])
      if kind[l] == REVISIT and v in self.node:
        assert v != 0
      if kind[l] != EXPAND:
        continue
      assert v in self.paths and v not in [leaf[k] for k in range(l) if kind[k] == EXPAND]
      if v == 0:
        p_status, p_acc, p_disc = np.zeros(M, np.uint8), np.zeros(M), np.ones(M)
        assert self.root_status == 0
      else:
        p_acc, p_disc, p_status = self.node[v]
        assert not twin_lib.group_spent(p_status == 0, p_acc), 'a spent group is never EXPAND'
      for a in range(3):
        path, j = self.paths[v] + (a,), 3 * l + a
        void = _void_edge(self.seed, path)
        for m in range(M):
          rule = FLY if v == 0 else emul_lib.lane_rule(p_status, p_acc, m, a)
          assert v == 0 or rule == twin_lib.lane_rule(p_status == 0, p_acc, m, a)
          assert rule != VOID
          if rule == FLY:
            reward, st = self.edge(self.seed, path, m, self.seed % 2 == 1)
            term = p_disc[m] * reward
            acc[j, m], disc[j, m], status[j, m] = p_acc[m] + term, p_disc[m] * GAMMA, st
          else:                                  # a stopped node of a live group: carried on unchanged under every action
            acc[j, m], disc[j, m], status[j, m] = p_acc[m], p_disc[m], p_status[m]
        if void:
          acc[j, :] = NAN
        self.paths[1 + 3 * L * r + j] = path
    value, probs = _network(self.rng, 3 * L, M) if self.guide else (None, None)
    self.emul.backup(r, acc, disc, status, value, probs)
    self.twin.backup(acc, disc, status == 0, value, probs)
    self.rounds.append((leaf, kind))
    born = 1 + 3 * L * (r + 1)
    for name in ('parent', 'first_child', 'depth', 'visits', 'pending'):
      assert np.array_equal(getattr(self.emul, name)[:born], getattr(self.twin, name)[:born]), (r, name)
    for name in ('value_sum', 'g', 'prior'):
      assert np.array_equal(_bits(getattr(self.emul, name)[:born]), _bits(getattr(self.twin, name)[:born])), (r, name)
    assert np.array_equal(_bits(self.emul.g_range), _bits(np.array([self.twin.g_lo, self.twin.g_hi])))
    assert np.array_equal(_bits(self.emul.group_g[r]), _bits(self.twin.group_g[r])), r
    assert np.array_equal(self.emul.status[r], self.twin.group_status[r]), r
    # visits[group] = the non-void groups in its subtree plus the revisits in it; value_sum their G in backup order (from the arrays alone)
    mcts_host.check_invariants(L, self.emul.parent[:born], self.emul.visits, self.emul.value_sum, self.emul.g, self.rounds)
    for l in range(L):
      for a in range(3):
        j, c = 3 * l + a, born - 3 * L + 3 * l + a
        g = self.emul.group_g[r, j]
        assert _bits(np.float64(g)) == _bits(np.float64(self.emul.g[c])) or (math.isnan(g) and math.isnan(self.emul.g[c]))
        if math.isnan(g):
          assert self.emul.visits[c] == 0
          self.counts['void'] += int(kind[l] == EXPAND)
          self.paths.pop(c, None)
          continue
        self.node[c] = (acc[j].copy(), disc[j].copy(), status[j].copy())
        stopped = [twin_lib.stopped(status[j, m] == 0, acc[j, m]) for m in range(M)]
        assert self.emul.status[r, j] == int(all(stopped))
        self.counts['spent'] += int(all(stopped))
        self.counts['stopped_in_live'] += int(any(stopped) and not all(stopped))

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


SEEDS = range(24)


@pytest.mark.parametrize('guide', [True, False])
@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('shape', [(3, 2, 3), (6, 4, 2)])
def test_whole_searches_equal_the_twin(shape, M, guide):
  R, L, D = shape
  totals = {k: 0 for k in KINDS}
  for seed in SEEDS:
    for c_puct in (1.25, 0.0):
      run = _Run(R, L, D, M, 1 + seed % M, c_puct, 1000 * L + 10 * D + seed, guide).run()
      got = run.finish(segment=1 + seed % 3)
      assert 0 <= got['pv_length'] <= D
      for k in totals:
        totals[k] += run.counts[k]
  # every kind occurred (with M = 1 a stopped node IS a spent group: there is no stopped node inside a live one)
  assert all(totals[k] > 0 for k in KINDS if not (M == 1 and k == 'stopped_in_live')), totals


def test_spent_groups_are_revisited_never_expanded():
  """A table in which every scenario ends at once: the root's children are spent, every later slot is a REVISIT of one of them (or
  EMPTY), and the revisit adds the group's own G."""
  run = _Run(4, 2, 3, 3, 2, 1.25, 3, guide=False)
  run.edge = lambda seed, path, m, harsh: (_edge(seed, path, m, harsh)[0], 2)
  run.run()
  assert run.counts[EXPAND] == 1 and run.counts[REVISIT] > 0 and run.counts['spent'] + run.counts['void'] == 3
  assert all(k != EXPAND for _, kind in run.rounds[1:] for k in kind)
  got = run.finish()
  assert got['visits'].sum() == run.emul.visits[0]


def test_dead_root():
  dead = _Run(3, 2, 2, 3, 3, 1.25, 5, guide=True, source_status=2).run()
  assert dead.counts[EMPTY] == 6 and dead.counts[EXPAND] == 0 and dead.counts[REVISIT] == 0
  assert np.all(dead.emul.status == 1) and np.all(np.isnan(dead.emul.group_g))          # the source's words with acc NaN: spent, void
  got = dead.finish(segment=3)
  assert got['action'] == mcts_host.STAY and np.all(got['best_plan'] == mcts_host.STAY) and got['pv_length'] == 0
  assert _bits(np.float32(got['best_return'])) == 0 and np.all(got['visits'] == 0) and np.all(np.isneginf(got['q']))       # +0.0f
