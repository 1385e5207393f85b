"""A population's prioritized replay without a GPU: the precondition of the grouped draw case of
test_gpu_population_prio.py, from replay_draws.cpp's uniforms and the twin; and member p's leaf numbering and window validity over ONE
ring of P * R columns stated in NumPy against the solo twin on its column slice, with the per-member tree sizes the library accepts."""
import numpy as np
import pytest

import population_prio_host as pp
import prio_replay_host as ph
import train_host


@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  return ph.build_replay_draws(tmp_path_factory.mktemp('rpd'))


@pytest.fixture(scope='module')
def case():
  h = pp.pop_draw_case_history()
  return (h,) + pp.pop_draw_case_trees(h)


def test_draw_case_sizes_are_the_library_s(case):
  c = pp.POP_DRAW_CASE
  _, fed, _ = case
  tree = fed.trees[0]
  assert (tree.leaves, tree.P) == (c['capacity'] * c['rows'], 1024)
  args = (c['members'], c['rows'], c['capacity'], c['horizon'])
  assert pp.library_accepts(*args, tree.leaves, tree.P)
  assert pp.library_accepts(*args, tree.leaves, tree.P, stride=2 * tree.P + 3)
  # not the whole ring's sizes, not another padding, not trees that overlap
  assert not pp.library_accepts(*args, c['members'] * tree.leaves, 4096)
  assert not pp.library_accepts(*args, tree.leaves, 2048) and not pp.library_accepts(*args, tree.leaves, 512)
  assert not pp.library_accepts(*args, tree.leaves, tree.P, stride=2 * tree.P - 1)


@pytest.mark.parametrize('counter', pp.POP_DRAW_CASE['counters'])
@pytest.mark.parametrize('b', pp.POP_DRAW_CASE['batches'])
def test_draw_case_precondition(draws, case, b, counter):
  """For every member and row, the query and its two fp64 neighbours walk to one leaf, a nonzero one whose window is complete and valid
  (no row needs a second draw); the members' trees, seeds and therefore leaves differ."""
  c = pp.POP_DRAW_CASE
  h, _, crafted = case
  r, cap, n, last = c['rows'], c['capacity'], c['horizon'], c['steps'] - 1
  assert pp.library_accepts(c['members'], r, cap, n, crafted.trees[0].leaves, crafted.trees[0].P)
  seen = []
  for p in range(c['members']):
    leaf, split = pp.pop_draw_case_leaves(draws, crafted, p, b, counter)
    assert not split, (p, split)
    tree = crafted.trees[p]
    assert (tree.nodes[tree.P + leaf] > 0).all()
    tt, col = ph.newest_step(last, cap, leaf // r), p * r + leaf % r
    assert (last + 1 - cap <= tt).all() and (tt + n <= last).all()
    assert all(train_host.nstep(h['reward'], h['terminal'], h['episode_end'], int(t), int(e), n, 0.993) is not None for t, e in zip(tt, col))
    seen.append(leaf)
  assert not np.array_equal(crafted.trees[0].nodes, crafted.trees[1].nodes) and not np.array_equal(crafted.trees[1].nodes, crafted.trees[2].nodes)
  assert b == 1 or not (np.array_equal(seen[0], seen[1]) or np.array_equal(seen[1], seen[2]))


@pytest.mark.parametrize('members,rows,capacity,horizon', [(3, 5, 6, 5), (2, 64, 8, 3), (1, 65, 12, 5)])
def test_member_leaf_numbering_and_validity_are_the_twins_on_the_slice(members, rows, capacity, horizon):
  """The grouped rule written over the WHOLE ring -- column c is member c // R's, its window at step t leaf (t % T) R + c % R, entered
  at that member's max priority when replay_window holds at column c -- against the solo twin fed member p's column slice."""
  assert pp.library_accepts(members, rows, capacity, horizon, capacity * rows, 1 << (capacity * rows - 1).bit_length())
  steps = 3 * capacity + horizon
  h = ph.history(steps, members * rows, 5, obs=False)
  pop = pp.PopulationTrees(members, rows, capacity, horizon)
  whole = np.zeros((members, capacity * rows))
  rng = np.random.default_rng(6)
  for s in range(steps):
    pop.add(h, s)
    term, end = pop.ring['terminal'], pop.ring['episode_end']
    for c in range(members * rows):
      p, zeroed = pp.member_leaf(c, s, rows, capacity)
      whole[p, zeroed] = 0.0
      if s >= horizon:
        _, done = pp.member_leaf(c, s - horizon, rows, capacity)
        whole[p, done] = pop.trees[p].max_priority if ph.window_valid(term, end, s - horizon, c, horizon) else 0.0
    if s % 7 == 6:                                       # a set_priority round in member s % P only: the others' leaves stay
      p = s % members
      tree = pop.trees[p]
      leaves = rng.choice(np.flatnonzero(tree.nodes[tree.P:] > 0), 4)
      loss = (rng.random(4) * 9).astype(np.float32)
      tree.set_priority(leaves, loss)
      whole[p, leaves] = np.sqrt(loss + np.float32(1e-10)).astype(np.float64)
    for p, tree in enumerate(pop.trees):
      assert np.array_equal(whole[p], tree.nodes[tree.P:tree.P + tree.leaves]), (s, p)
      # windows_valid on the whole ring at member p's columns is windows_valid on the slice
      if s >= horizon:
        cols = pp.member_columns(p, rows)
        assert np.array_equal(ph.windows_valid(term, end, s - horizon, horizon)[cols],
                              ph.windows_valid(term[:, cols], end[:, cols], s - horizon, horizon))
  assert len({t.max_priority for t in pop.trees}) == members or members == 1      # (each member's own maximum)
