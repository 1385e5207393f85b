"""NumPy twin of the beam search's select and finish, written from the definition there and not from the kernels: the order
of a level's children, the cut to the beam, the walk back through the choice lists, the per-action values and the two special answers
(a source that is not OK, no finite key).  Everything is a comparison of floats or an integer: the device's answers are reproduced bit
for bit.  TEST TOOLING."""
import numpy as np

STAY = 1


def level_sizes(depth, beam):
  """[(P_{d-1}, C_d)] for d = 1 .. depth."""
  out, parents = [], 1
  for _ in range(depth):
    out.append((parents, 3 * parents))
    parents = min(3 * parents, beam)
  return out


def order(ret):
  """The children of one environment, best first: a finite return before a non-finite one, the return descending (-0 == +0), c
  ascending."""
  ret = np.asarray(ret, np.float32)
  finite = np.isfinite(ret)
  value = np.where(finite, ret, np.float32(0.0)).astype(np.float64) + 0.0
  return np.lexsort((np.arange(len(ret)), -value, ~finite))


def select(ret, beam):
  """ret [n, C] -> the first min(C, beam) children of every environment in order: int32 [n, min(C, beam)] (parent and choice alike)."""
  ret = np.asarray(ret, np.float32)
  keep = min(ret.shape[1], beam)
  return np.stack([order(r)[:keep] for r in ret]).astype(np.int32)


def path(choice, e, c, depth):
  """The actions (a_1 .. a_depth) of child c of level `depth` of environment e.  choice[d - 1]: level d's list, [n, >= P_d]."""
  actions = []
  for d in range(depth, 0, -1):
    actions.append(c % 3)
    if d > 1:
      c = int(choice[d - 2][e][c // 3])
  return actions[::-1]


def finish(ret, choice, depth, segment, source_ok, score=None, want_q=True):
  """ret [n, C] float32 (NaN: void), score [n, C] or None (the keys: ret), source_ok [n] bool, choice: per level [n, .].
  -> (best_plan [depth * segment, n] u8, action [n] u8, best_return [n] f32, q [n, 3] f32, visits [n, 3] i32)."""
  ret = np.asarray(ret, np.float32)
  key = ret if score is None else np.asarray(score, np.float32)
  n, C = ret.shape
  best_plan = np.full((depth * segment, n), STAY, np.uint8)
  best_return = np.zeros(n, np.float32)
  q = np.full((n, 3), -np.inf, np.float32)
  visits = np.zeros((n, 3), np.int32)
  for e in range(n):
    o = order(key[e])
    if not source_ok[e]:
      best_return[e] = np.float32(0.0)
    elif not np.isfinite(key[e, o[0]]):
      best_return[e] = -np.inf
    else:
      best_return[e] = key[e, o[0]]
      best_plan[:, e] = np.repeat(path(choice, e, int(o[0]), depth), segment)
    if want_q:
      roots = np.array([path(choice, e, c, depth)[0] for c in range(C)])
      for a in range(3):
        mine = o[roots[o] == a]                                      # this action's children, best first
        visits[e, a] = int((~np.isnan(ret[e, mine])).sum())
        if len(mine) and np.isfinite(key[e, mine[0]]):
          q[e, a] = key[e, mine[0]]
  return best_plan, best_plan[0].copy(), best_return, q, visits
