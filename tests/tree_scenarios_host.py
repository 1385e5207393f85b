"""NumPy twin of the beam search in scenario winds, written from the definitions there and not from the kernels: which
scenario nodes fly, which are carried and which are void; and the level loop -- the risk score of every group, the order of the groups,
the cut to the beam, the finish on the scores.  Built on the twins of its two halves (tree_host: order, select, finish; scenario_host:
the risk score).  Everything is a comparison, an integer or one fp64 sum in a stated order: the device's answers bit for bit.
TEST TOOLING."""
import numpy as np

import scenario_host
import tree_host

FLY, CARRY, VOID = 0, 1, 2


def stopped(status, acc):
  """A scenario node is stopped when its status is not OK or its acc is NaN."""
  return status != 0 or acc != acc


def lane(status, acc, m, act):
  """What the child of scenario node m under action act is, from the parent group's status [M] and acc [M] (acc None: level 1 -- the M
  nodes are the environment itself, status[0] its byte, acc 0).  A live node flies.  A stopped node is carried on unchanged under every
  action -- unless the whole group is spent (all M stopped): then a = 0 carries and a = 1, 2 are void (the copy with acc = NaN)."""
  if acc is None:
    group = [stopped(int(status[0]), 0.0)]
    mine = group[0]
  else:
    group = [stopped(int(s), float(a)) for s, a in zip(status, acc)]
    mine = group[m]
  if not mine:
    return FLY
  return VOID if (all(group) and act != 0) else CARRY


def level(ret, tail, beam):
  """ret [n, C, M] float32 -> (score [n, C] float32, parent int32 [n, min(C, beam)]): every group's risk score -- NaN with any
  non-finite scenario return --, the groups ordered by it as tree_host orders returns."""
  score = scenario_host.risk_scores(ret, tail)
  return score, tree_host.select(score, beam)


def finish(score, choice, depth, segment, source_ok, want_q=True):
  """The finish on the last level's scores alone (ret := score): best_return is the best group's score, q the best score under each
  first action, visits the groups whose score is not NaN."""
  return tree_host.finish(score, choice, depth, segment, source_ok, None, want_q)


def search(returns_by_level, tail, beam, segment, source_ok):
  """A whole search over given returns: returns_by_level[d - 1] is level d's [n, C_d, M] (the device's own, or crafted).
  -> (scores per level, parents per level, finish tuple)."""
  scores, parents = [], []
  for ret in returns_by_level:
    s, p = level(ret, tail, beam)
    scores.append(s)
    parents.append(p)
  depth = len(returns_by_level)
  return scores, parents, finish(scores[-1], parents, depth, segment, source_ok)
