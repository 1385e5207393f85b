"""Guided tree search in scenario winds on the device: ble_mcts_expand_scenarios_f32 and ble_mcts_backup_scenarios_f32 with
ble_mcts_select_f32 and ble_mcts_finish_f32 on the groups' view of the pool, through VecSimulator.mcts_search(scenarios=) and
VecScenarioMCTSAgent.

The reference of a scenario node is the look-ahead in scenario winds itself: a node of a non-void group reached by (a_1 .. a_d) must
hold, BIT FOR BIT, the return, steps_flown and final words rollout_plans(scenarios=) gives the plan a_1 x segment, .., a_d x segment in
its scenario, and in every array what the exhaustive scenario tree (tree_search(scenarios=), itself held to scenario_wind + step on a
copy) holds at that path.  The selections, the statistics, the groups' G, status and priors and the finish are held to the float64 twin
(mcts_scenarios_host.py) on the device's own acc, disc, status, values and probabilities.  No tolerance anywhere: bits or integers."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import mcts_host
import mcts_scenarios_host as twin_lib
import test_gpu_scenarios as tgs
import test_gpu_tree_scenarios as tts
import tree_host
from balloon_learning_environment_amd import _abi, _lib, device as dev, train_lib, vec_state
from balloon_learning_environment_amd.agents import actor_critic, expert_iteration, mcts_agent, qnet
from balloon_learning_environment_amd.env import balloon_env
from balloon_learning_environment_amd.eval import eval_lib, suites
from mcts_host import EMPTY, EXPAND, REVISIT

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
GAMMA = 0.993
FINAL_FIELDS = tgs.FINAL_FIELDS
RINGS = tts.RINGS
DEAD, BURST = tts.DEAD, tts.BURST
_dev, _same_words, _guard, _assert_guarded = tgs._dev, tts._same_words, tts._guard, tts._assert_guarded


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _critic(seed=1):
  net = qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', seed=seed, num_layers=2, hidden_units=64), num_atoms=2)
  return actor_critic.VecActorCriticAgent(net, deterministic=True)


def _pool_host(pool):
  """The pool's node arrays as [R, n, 3L, M] host arrays, the groups' as [R, n, 3L], and the statistics."""
  torch.cuda.synchronize()
  M = pool.num_scenarios
  shape = (pool.rounds, pool.sim.n, 3 * pool.leaves, M)
  out = {name: getattr(pool, name).cpu().numpy().reshape(shape) for name in ('acc', 'disc', 'flown', 'ret')}
  out['status'] = pool.node_state['status'].cpu().numpy().reshape(shape)
  out['group_g'], out['group_status'] = pool.group_g.cpu().numpy(), pool.group_status.cpu().numpy()
  out.update({name: t.cpu().numpy() for name, t in pool.statistics().items()})
  return out


def _path(parent, c):
  path = []
  while c > 0:
    path.append((c - 1) % 3)
    c = int(parent[c])
  return tuple(reversed(path))


def _groups_by_depth(host, pool):
  """{depth: [(e, id, path)]} of the non-void groups (acc not NaN in all M nodes), which are exactly the groups with a G."""
  n = pool.sim.n
  acc = host['acc'].transpose(1, 0, 2, 3).reshape(n, -1, pool.num_scenarios)            # [n, cap - 1, M]: id c at row c - 1
  void = np.isnan(acc).all(-1)
  assert np.array_equal(np.isnan(acc).any(-1), void)                                     # a group is void in all its nodes or in none
  assert np.array_equal(void, np.isnan(host['g'][:, 1:])) and np.all(host['visits'][:, 1:][void] == 0)
  nodes = {}
  for e in range(n):
    for c in np.nonzero(~void[e])[0] + 1:
      path = _path(host['parent'][e], int(c))
      assert len(path) == host['depth'][e, c] and 1 <= len(path) <= pool.max_depth
      nodes.setdefault(len(path), []).append((e, int(c), path))
  return nodes, int((~void).sum())


def _assert_nodes_are_their_plans(src, scn, pool, segment, repeat):
  """Every node of every non-void group against rollout_plans(scenarios=) of its path's plan in its scenario (ret, steps_flown, the final
  words) and against the exhaustive scenario tree's node at that path (every state array, acc, disc, flown, ret)
  -> (non-void groups, scenario nodes that are not OK, groups in which some but not all nodes are not OK)."""
  n, M = src.n, scn.num
  host = _pool_host(pool)
  nodes, alive = _groups_by_depth(host, pool)
  assert not any(e in np.nonzero(src.state['status'].cpu().numpy() != 0)[0] for group in nodes.values() for e, _, _ in group)
  terminal = mixed = 0
  scenario = torch.arange(M, device=DEVICE)
  for d, group in sorted(nodes.items()):
    paths = sorted({p for _, _, p in group})
    k_of = {p: k for k, p in enumerate(paths)}
    plans = np.repeat(np.array(paths, np.uint8).T, segment, 0)             # [d * segment, K]
    plans = np.ascontiguousarray(np.broadcast_to(plans[:, None, :], (d * segment, n, len(paths))))
    want = src.rollout_plans(_dev(plans), gamma=GAMMA, action_repeat=repeat, scenarios=scn, want_final=True)
    at = (_dev(np.array([pool.node_index(c, e) for e, c, _ in group], np.int64))[:, None] * M + scenario).view(-1)
    plan = (_dev(np.array([e * len(paths) + k_of[p] for e, _, p in group], np.int64))[:, None] * M + scenario).view(-1)
    _same_words(pool.ret[at], want.returns.view(-1)[plan], (d, 'ret'))
    _same_words(pool.flown[at], want.steps_flown.view(-1)[plan], (d, 'flown'))
    for f, name in enumerate(FINAL_FIELDS):
      _same_words(pool.node_state[name][at], want.final[f].reshape(-1)[plan], (d, 'final', name))
    # every array: the exhaustive tree of depth d holds all 3^d paths in its last level (child c of environment e: tree_host.path)
    tree = src.tree_search(d, 3 ** (d - 1), segment=segment, action_repeat=repeat, gamma=GAMMA, scenarios=scn)
    torch.cuda.synchronize()
    choice, C = tree.buffers.choice.cpu().numpy(), 3 ** d
    child = [{tuple(tree_host.path(choice, e, c, d)): c for c in range(C)} for e in range(n)]
    leaf = (_dev(np.array([e * C + child[e][p] for e, _, p in group], np.int64))[:, None] * M + scenario).view(-1)
    bf = tree.buffers
    for name in _abi.FIELD_NAMES:
      _same_words(pool.node_state[name][at], tree.leaves.state[name][leaf], (d, name))
    for name in ('acc', 'disc', 'flown', 'ret'):
      _same_words(getattr(pool, name)[at], getattr(bf, name)[d & 1][leaf], (d, name))
    bad = (pool.node_state['status'][at] != 0).view(-1, M).sum(1)
    terminal += int(bad.sum().item())
    mixed += int(((bad > 0) & (bad < M)).sum().item())
  return alive, terminal, mixed


# ------------------------------------------------------------------------------------------------ 1: a node is its plan's look-ahead
@pytest.mark.parametrize('segment', [1, 3])
def test_every_node_equals_the_scenario_rollout_of_its_path(segment):
  R, L, D, M = 3, 2, 3, 3
  src, _ = tts._five(600 + segment)
  scn = src.fit_wind_scenarios(M, seed=33)
  src.rollout_flags.zero_()
  before = _guard(src, scn)
  flags = int(src.err_flags.item())
  got = src.mcts_search(R, L, D, segment=segment, gamma=GAMMA, scenarios=scn, risk_tail=2)
  _assert_guarded(src, scn, before, 'the source')
  assert int(src.err_flags.item()) == flags
  pool = got.pool
  assert pool.num_scenarios == M and pool.acc.numel() == R * src.n * 3 * L * M and tuple(pool.group_g.shape) == (R, src.n, 3 * L)
  assert pool.arenas[0].n == src.n * 3 * L * M and pool.arenas[0].leaves_per_env == 3 * L * M
  alive, terminal, _ = _assert_nodes_are_their_plans(src, scn, pool, segment, 1)
  host = _pool_host(pool)
  print(f'segment {segment}: non-void groups {alive} of {src.n * 3 * L * R}, scenario nodes not OK {terminal}')
  assert alive > 3 * src.n and terminal >= 3 * M
  # the source that is not OK grew nothing and answers STAY, +0.0f; the one that bursts has three spent children, revisited
  assert np.isnan(host['acc'][:, DEAD]).all() and int(got.action[DEAD].item()) == 1
  assert _bits(got.best_return.cpu().numpy())[DEAD] == 0 and int(got.pv_length[DEAD].item()) == 0
  assert np.all(host['group_status'][0, BURST, :3] == 1) and np.all(host['flown'][0, BURST, :3] == 1)
  assert host['first_child'][BURST, 1:4].tolist() == [0, 0, 0] and host['visits'][BURST, 1:4].sum() > 3
  # really flown: the scenarios of a live group end elsewhere than each other
  x = pool.node_state['x'].view(R, src.n, 3 * L, M)[0, 0, :3].cpu().numpy()
  assert all(len(set(_bits(x[a]).tolist())) == M for a in range(3))


def test_every_node_with_a_runtime_vehicle_and_per_environment_seeds():
  """The VehicleRt, EnvSeed instantiation (and, with seed=, VehicleRt, ScalarSeed): edges of segment 2 x action_repeat 2."""
  n, M, R, L, D = 3, 2, 3, 2, 3
  for fit in (dict(seeds=_dev(np.array([101, 102, 103], np.int64))), dict(seed=33)):
    src, _ = tgs._source(n, tts.VEHICLE_SEED, RINGS[2:], vehicle=tts.VEHICLE)
    src.state['status'][DEAD] = 1
    scn = src.fit_wind_scenarios(M, **fit)
    before = _guard(src, scn)
    got = src.mcts_search(R, L, D, segment=2, action_repeat=2, gamma=GAMMA, scenarios=scn)
    _assert_guarded(src, scn, before, 'the source')
    alive, _, _ = _assert_nodes_are_their_plans(src, scn, got.pool, 2, 2)
    assert alive >= 2 * 3 * 2
  # the vehicle is really flown: the default vehicle's nodes are other nodes
  ret = got.pool.ret.clone()
  src.set_vehicle()
  other = src.mcts_search(R, L, D, segment=2, action_repeat=2, gamma=GAMMA, scenarios=scn)
  torch.cuda.synchronize()
  assert not torch.equal(other.pool.ret[:3 * M].view(torch.int32), ret[:3 * M].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 2: the search equals the twin
def _host_of(t):
  if isinstance(t, dict):
    return {k: v.cpu().numpy() for k, v in t.items()}
  return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _assert_search_equals_the_twin(src, got, trace, c_puct, tail, segment):
  """-> counts of the slot kinds and of the kinds of group."""
  pool = got.pool
  host = _pool_host(pool)
  n, M, L3 = src.n, pool.num_scenarios, 3 * pool.leaves
  source_ok = src.state['status'].cpu().numpy() == 0
  trace = [tuple(_host_of(t) for t in rec) for rec in trace]
  assert [rec[0] for rec in trace] == list(range(pool.rounds)) and all(len(rec) == 8 for rec in trace)
  out = {name: getattr(got, name).cpu().numpy() for name in ('action', 'q', 'visits', 'best_return', 'best_plan', 'pv_length')}
  seen = {EMPTY: 0, EXPAND: 0, REVISIT: 0, 'void': 0, 'spent': 0, 'stopped_in_live': 0, 'dead_valued': 0, 'mean_prior': 0}
  for e in range(n):
    twin = twin_lib.Search(pool.rounds, pool.leaves, pool.max_depth, c_puct, M, tail, source_ok[e])
    rounds = []
    for r, leaf, kind, stats, value, probs, group_g, group_status in trace:
      want_leaf, want_kind = twin.select()
      assert np.array_equal(leaf[e], want_leaf) and np.array_equal(kind[e], want_kind), (e, r, leaf[e], kind[e], want_leaf, want_kind)
      for k in kind[e]:
        seen[int(k)] += 1
      rows = slice(e * L3 * M, (e + 1) * L3 * M)
      acc, disc, ok = host['acc'][r, e], host['disc'][r, e], host['status'][r, e] == 0
      v = None if value is None else value[rows].reshape(L3, M)
      p = None if probs is None else probs[rows].reshape(L3, M, 3)
      twin.backup(acc, disc, ok, v, p)
      born = twin.born
      for name in ('parent', 'first_child', 'depth', 'visits', 'pending'):
        assert np.array_equal(stats[name][e, :born], getattr(twin, name)[:born]), (e, r, name)
      for name in ('value_sum', 'g', 'prior'):
        assert np.array_equal(_bits(stats[name][e, :born]), _bits(getattr(twin, name)[:born])), (e, r, name)
      assert np.array_equal(_bits(stats['g_range'][e]), _bits(np.array([twin.g_lo, twin.g_hi])))
      assert np.array_equal(_bits(group_g[r, e]), _bits(twin.group_g[r])), (e, r)
      assert np.array_equal(group_status[r, e], twin.group_status[r]), (e, r)
      rounds.append((leaf[e], kind[e]))
      mcts_host.check_invariants(pool.leaves, stats['parent'][e, :born], stats['visits'][e], stats['value_sum'][e], stats['g'][e], rounds)
      for l in range(pool.leaves):
        if kind[e][l] != EXPAND:
          continue
        assert leaf[e][l] == 0 or twin.ok[leaf[e][l]], 'a spent group was expanded'
        for j in range(3 * l, 3 * l + 3):
          stopped = [twin_lib.stopped(ok[j, m], acc[j, m]) for m in range(M)]
          seen['void'] += int(np.isnan(group_g[r, e, j]))
          seen['spent'] += int(all(stopped) and not np.isnan(group_g[r, e, j]))
          seen['stopped_in_live'] += int(any(stopped) and not all(stopped))
          if v is not None and not np.isnan(group_g[r, e, j]):
            seen['dead_valued'] += int((~ok[j]).sum())
            seen['mean_prior'] += int(ok[j].sum() > 1)
          if M == 1 and not np.isnan(group_g[r, e, j]):          # one scenario, tail 1: the group's G is its node's own acc + disc V
            v_c = float(v[j, 0]) if (v is not None and ok[j, 0]) else 0.0
            tail_term = float(disc[j, 0]) * v_c
            assert _bits(group_g[r, e, j:j + 1])[0] == _bits(np.array([float(acc[j, 0]) + tail_term]))[0], (e, r, j)
    want = twin.finish(segment)
    assert out['action'][e] == want['action'] and out['pv_length'][e] == want['pv_length'], e
    assert np.array_equal(out['best_plan'][:, e], want['best_plan']) and np.array_equal(out['visits'][e], want['visits']), e
    assert np.array_equal(_bits(out['q'][e]), _bits(want['q'])), e
    assert _bits(out['best_return'][e:e + 1])[0] == _bits(np.float32(want['best_return']).reshape(1))[0], e
  return seen


N, R, L, D = 65, 4, 3, 3


@pytest.fixture(scope='module')
def many():
  """65 environments, 3 L M 65 lanes a round: with M = 8 a few full workgroups and a partial one.  Environment 7 is not OK, environment
  9 bursts in its first step in every scenario (its root's children are spent)."""
  src, _ = tgs._source(N, 610, [RINGS[e % len(RINGS)] for e in range(N)])
  src.state['status'][7] = 2
  src.state['mols_air'][9] += 30000.0
  return src


@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('M, tail', [(1, 1), (8, 1), (8, 3), (8, 8)])
def test_the_search_equals_the_twin(many, M, tail, guided):
  src = many
  scn = src.fit_wind_scenarios(M, seed=7)
  critic = _critic() if guided else None
  buffers = src.mcts_buffers(R, L, D, 2, guide=guided, num_scenarios=M)
  if guided:
    assert tuple(buffers.obs.shape) == (N * 3 * L * M, 1099) and tuple(buffers.probs.shape) == (N * 3 * L * M, 3)
    critic.act(buffers.obs, out=buffers.guide_action, value=buffers.value, probs=buffers.probs)
  for c_puct in (1.25, 0.0):
    trace = []
    got = src.mcts_search(R, L, D, segment=2, gamma=GAMMA, c_puct=c_puct, scenarios=scn, risk_tail=tail, buffers=buffers,
                          guide_fn=critic.act if guided else None, trace=trace)
    assert got.pool is buffers
    seen = _assert_search_equals_the_twin(src, got, trace, c_puct, tail, 2)
    print(f'M {M} tail {tail} guided {guided} c_puct {c_puct}:', seen)
    assert seen[EXPAND] > N and seen[EMPTY] > 0 and seen[REVISIT] > 0 and seen['spent'] >= 3
    assert not guided or M == 1 or seen['mean_prior'] > N
    action, best = got.action.cpu().numpy(), got.best_return.cpu().numpy()
    assert action[7] == 1 and _bits(best)[7] == 0 and np.all(got.best_plan.cpu().numpy()[:, 7] == 1) and got.pv_length.cpu().numpy()[7] == 0
    live = np.delete(np.arange(N), 7)
    assert np.isfinite(best[live]).all() and np.all(got.pv_length.cpu().numpy()[live] >= 1)
    assert np.array_equal(_bits(got.q.cpu().numpy()[live, action[live]]), _bits(best[live]))
  if guided:      # the last round's rows are what the guide was asked: its values and probabilities on that round's slice as it lies
    rows = N * 3 * L * M
    value, probs = torch.empty(rows, device=DEVICE), torch.empty(rows, 3, device=DEVICE)
    critic.act(src.observe_leaves(buffers.arenas[R - 1]), out=torch.empty(rows, dtype=torch.uint8, device=DEVICE), value=value, probs=probs)
    _same_words(value, trace[-1][4], 'value')
    _same_words(probs, trace[-1][5], 'probs')


# ------------------------------------------------------------------------------------------------ 3: stopped and spent
def _drive(src, scn, bf, c_puct, tail, after_expand=None, guide_fn=None):
  """mcts_search's own sequence of calls, with a hook between a round's expand and its backup -> [(leaf, kind) per round] (host)."""
  lib, stream = _lib.lib(), dev.stream_ptr(src.device)
  pool, groups, status = ctypes.byref(bf._struct), ctypes.byref(bf._group_struct), src.state['status'].data_ptr()
  b, gen = src._scenario_structs(scn)
  rounds = []
  with torch.cuda.device(src.device):
    for r in range(bf.rounds):
      _lib.check(lib.ble_mcts_select_f32(groups, r, float(c_puct), status, None, stream), 'select')
      ex = _abi.BleMctsExpand(r, 1, vec_state.SUBSTEPS, 0, GAMMA, src.grid.data_ptr(), src.grid_env_stride)
      _lib.check(lib.ble_mcts_expand_scenarios_f32(ctypes.byref(src._struct), pool, ctypes.byref(ex), ctypes.byref(b), ctypes.byref(gen),
                                                   src.rollout_flags.data_ptr(), stream), 'expand')
      if after_expand is not None:
        after_expand(r)
      _lib.check(lib.ble_mcts_backup_scenarios_f32(pool, r, scn.num, tail, None, None, bf.group_status.data_ptr(), bf.group_g.data_ptr(),
                                                   stream), 'backup')
      torch.cuda.synchronize()
      rounds.append((bf.leaf.cpu().numpy().copy(), bf.kind.cpu().numpy().copy()))
    fin = _abi.BleMctsFinish(status, bf.best_plan.data_ptr(), bf.action.data_ptr(), bf.best_return.data_ptr(), bf.q.data_ptr(),
                             bf.root_visits.data_ptr(), bf.pv_length.data_ptr())
    _lib.check(lib.ble_mcts_finish_f32(groups, ctypes.byref(fin), stream), 'finish')
  torch.cuda.synchronize()
  return rounds


def test_stopped_nodes_inside_live_groups_and_spent_groups():
  """test_stopped_nodes_inside_live_and_spent_groups' edits, made to the root's children between round 0's expand and its backup: in
  environment 0 a node of the a = 0 group stops and the whole a = 1 group stops; in environment 3 an acc of the a = 2 group is NaN."""
  Rr, Ll, Dd, M, tail = 4, 3, 3, 3, 2
  src, _ = tts._five(620)
  scn = src.fit_wind_scenarios(M, seed=33)
  n = src.n
  bf = src.mcts_buffers(Rr, Ll, Dd, 2, num_scenarios=M)
  one, group, nan = bf.node_index(1, 0, 1), bf.node_index(2, 0, 0), bf.node_index(3, 3, 0)

  def edit(r):
    if r == 0:
      bf.node_state['status'][one] = 2
      bf.node_state['status'][group:group + M] = 2
      bf.acc[nan] = float('nan')
  rounds = _drive(src, scn, bf, 1.25, tail, edit)
  host = _pool_host(bf)
  words = {name: t.cpu().numpy() for name, t in bf.node_state.items()}
  words.update(acc=bf.acc.cpu().numpy(), disc=bf.disc.cpu().numpy(), flown=bf.flown.cpu().numpy())
  # the groups as the backup saw them
  assert host['group_status'][0, 0, :3].tolist() == [0, 1, 0] and np.isfinite(host['group_g'][0, 0, :3]).all()
  assert np.isnan(host['group_g'][0, 3, 2]) and host['visits'][3, 3] == 0 and host['group_status'][0, 3, 2] == 0
  seen = dict(carried=0, flown=0, revisits=0)
  for r, (leaf, kind) in enumerate(rounds):
    for e in range(n):
      for l in range(Ll):
        v, what = int(leaf[e, l]), int(kind[e, l])
        assert not (e == 0 and v == 2 and what == EXPAND), 'the spent group was expanded'
        assert not (e == 3 and v == 3), 'the void group was selected'
        assert not (e == DEAD and what != EMPTY)
        seen['revisits'] += int(e == 0 and v == 2 and what == REVISIT)
        if not (e == 0 and v == 1 and what == EXPAND):
          continue
        # the live group with a stopped scenario: its node m = 1 is carried on unchanged under all three actions, the others fly
        for a in range(3):
          child = bf.node_index(1 + 3 * Ll * r + 3 * l + a, 0)
          for m in range(M):
            for name, w in words.items():
              if m == 1:
                parent = bf.node_index(1, 0, m)
                assert w[child * M + m:child * M + m + 1].tobytes() == w[parent:parent + 1].tobytes(), (name, a, m)
            seen['carried' if m == 1 else 'flown'] += 1
            if m != 1:
              assert words['flown'][child * M + m] > words['flown'][bf.node_index(1, 0, m)] > 0
          assert host['group_status'][r, 0, 3 * l + a] == 0 and np.isfinite(host['group_g'][r, 0, 3 * l + a])
  print('stopped and spent:', seen)
  assert seen['carried'] == 3 and seen['flown'] == 6 and seen['revisits'] > 0
  # the revisits added the spent group's own G, nothing else: its visits are 1 + revisits, its value_sum that many G
  assert host['visits'][0, 2] == 1 + seen['revisits'] and host['first_child'][0, 2] == 0
  total = 0.0
  for _ in range(1 + seen['revisits']):
    total = total + float(host['g'][0, 2])
  assert _bits(host['value_sum'][0, 2:3])[0] == _bits(np.array([total]))[0]
  # a root that is not OK answers STAY, +0.0f
  assert int(bf.action[DEAD].item()) == 1 and _bits(bf.best_return.cpu().numpy())[DEAD] == 0 and np.all(bf.best_plan.cpu().numpy()[:, DEAD] == 1)
  # and the whole edited search is the twin's on the device's own arrays
  for e in range(n):
    twin = twin_lib.Search(Rr, Ll, Dd, 1.25, M, tail, e != DEAD)
    for r, (leaf, kind) in enumerate(rounds):
      want_leaf, want_kind = twin.select()
      assert np.array_equal(leaf[e], want_leaf) and np.array_equal(kind[e], want_kind), (e, r)
      twin.backup(host['acc'][r, e], host['disc'][r, e], host['status'][r, e] == 0)
    assert np.array_equal(host['visits'][e], twin.visits) and np.array_equal(_bits(host['value_sum'][e]), _bits(twin.value_sum)), e
    assert np.array_equal(_bits(host['group_g'][:, e]), _bits(twin.group_g)) and np.array_equal(host['group_status'][:, e], twin.group_status)


# ------------------------------------------------------------------------------------------------ 4: housekeeping
def test_flags_go_to_their_own_word_and_nothing_is_written():
  src, _ = tts._five(630)
  src.wind_noise(7)                                  # (allocates the harmonic cache: it must stay as it is)
  scn = src.fit_wind_scenarios(3, seed=4)
  critic = _critic()
  src.rollout_flags.zero_()
  before = _guard(src, scn)
  flags = int(src.err_flags.item())
  src.mcts_search(3, 2, 3, segment=2, gamma=GAMMA, scenarios=scn, guide_fn=critic.act)
  _assert_guarded(src, scn, before, 'a guided search')
  assert int(src.err_flags.item()) == flags
  src.rollout_flags.zero_()
  src.state['upwelling_infrared'][3] = 1e-3          # outside total_absorptivity's range: the flag of the imagined flights, not the real one's
  src.mcts_search(2, 1, 2, segment=1, gamma=GAMMA, scenarios=scn)
  torch.cuda.synchronize()
  assert int(src.rollout_flags.item()) & _lib.FLAG_ABSORPTIVITY and int(src.err_flags.item()) == flags
  src.check_errors()                                 # a flight that never happened raises nothing


def test_batch_invariance_with_per_environment_seeds():
  Rr, Ll, Dd, M = 3, 2, 3, 3
  src, _ = tgs._source(5, 640, (17, 3, 120, 1, 0), env_offset=3)
  src.episode[2] += 2
  seeds = np.array([101, 102, 103, 104, 105], np.int64)

  def search(sim, which):
    scn = sim.fit_wind_scenarios(M, seeds=_dev(seeds[which]))
    out = sim.mcts_search(Rr, Ll, Dd, segment=2, gamma=GAMMA, scenarios=scn, risk_tail=2)
    torch.cuda.synchronize()
    return out

  batch = search(src, slice(None))
  for e in (0, 2, 4):
    alone = search(tgs._clone_env(src, e, offset=0), slice(e, e + 1))
    for name in ('action', 'best_plan', 'best_return', 'q', 'visits', 'pv_length'):
      a, b = getattr(alone, name), getattr(batch, name)
      _same_words(a, (b[:, e:e + 1] if name == 'best_plan' else b[e:e + 1]).contiguous(), (e, name))
    for name, t in alone.pool.statistics().items():
      _same_words(t, batch.pool.statistics()[name][e:e + 1].contiguous(), (e, name))
    _same_words(alone.pool.group_g, batch.pool.group_g[:, e:e + 1].contiguous(), (e, 'group_g'))
    _same_words(alone.pool.ret.view(Rr, 1, -1), batch.pool.ret.view(Rr, 5, -1)[:, e:e + 1].contiguous(), (e, 'ret'))


KW = dict(num_rounds=3, leaves_per_round=2, max_depth=3, segment=2, num_scenarios=3, risk_tail=2, seed=5)


def test_act_is_the_public_composition_and_a_captured_decision_replays():
  n = 9
  env = tgs._env(n)
  sim = env.arena.sim
  sim.state['status'][2] = 2                         # one environment is not OK: it gets STAY
  agent = env.planner(search='mcts', wind='scenarios', **KW)
  assert type(agent) is mcts_agent.VecScenarioMCTSAgent and agent.get_name() == 'ScenarioMCTSAgent'
  assert agent.SEEDED and agent.WINDS == ('scenarios',)
  action = agent.act(None).clone()
  plan, best = (t.clone() for t in agent.plan())
  q, visits = (t.clone() for t in agent.action_values())
  probs = agent.visit_probs().cpu().numpy()
  scn = sim.fit_wind_scenarios(3, seed=5)
  want = sim.mcts_search(3, 2, 3, segment=2, gamma=agent.gamma, scenarios=scn, risk_tail=2)
  for a, b, name in ((action, want.action, 'action'), (plan, want.best_plan, 'best_plan'), (best, want.best_return, 'best_return'),
                     (q, want.q, 'q'), (visits, want.visits, 'visits')):
    _same_words(a, b, name)
  assert int(action[2].item()) == 1 and bool(torch.isfinite(best).all())
  assert np.all((np.abs(probs.sum(1) - 1) < 1e-6) | (probs.sum(1) == 0)) and probs[2].sum() == 0
  # a captured decision replays to the eager one, bit for bit
  stats = agent.buffers.statistics()
  group_g = agent.buffers.group_g.clone()
  graph = dev.capture(env.device, lambda: agent.act(None))[0]
  for t in (agent.action, agent.best_return, agent.q, agent.buffers.group_g, agent.buffers.value_sum):
    t.fill_(7)
  graph.replay()
  torch.cuda.synchronize()
  for a, b, name in ((agent.action, action, 'action'), (agent.best_plan, plan, 'best_plan'), (agent.best_return, best, 'best_return'),
                     (agent.q, q, 'q'), (agent.visits, visits, 'visits'), (agent.buffers.group_g, group_g, 'group_g')):
    _same_words(a, b, ('graph', name))
  for name, t in agent.buffers.statistics().items():
    _same_words(t, stats[name], ('graph', name))
  # the environment's own pass-through is the same search (its scenario streams are keyed by the env's seed)
  scn = sim.fit_wind_scenarios(3, seed=env.arena._seed)
  best = sim.mcts_search(3, 2, 3, segment=2, scenarios=scn, risk_tail=1).best_return.clone()
  got = env.mcts_search(3, 2, 3, segment=2, wind='scenarios', num_scenarios=3, risk_tail=1)
  _same_words(got.best_return, best, 'env.mcts_search')
  assert got.pool.num_scenarios == 3
  env.check_errors()


def test_evaluation_is_finite_and_batch_invariant():
  suite = suites.EvaluationSuite([11, 12, 13], 8)
  make = lambda: mcts_agent.VecScenarioMCTSAgent(3, 2, 2, num_scenarios=3, risk_tail=2, segment=2)
  alone = eval_lib.eval_agent_vec(make(), suite, batch_size=1)
  batch = eval_lib.eval_agent_vec(make(), suite, batch_size=3)
  for a, b in zip(alone, batch):
    assert dataclasses.asdict(a) == dataclasses.asdict(b), (a, b)
    assert np.isfinite(a.cumulative_reward) and np.isfinite(a.time_within_radius)
  assert [r.seed for r in batch] == [11, 12, 13]


@pytest.mark.parametrize('max_depth', [2, 1])
def test_one_iteration_of_expert_iteration_with_the_learner_as_guide(max_depth):
  n, steps = 4, 4
  env = balloon_env.VecBalloonEnv(n, seed=1)
  learner = expert_iteration.SoftBCTrainer(qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', 2, 2, 64), num_atoms=2), lr=1e-3,
                                           seed=5, temperature=0.5, value_coef=0.5)
  planner = env.planner(search='mcts', wind='scenarios', num_rounds=3, leaves_per_round=2, max_depth=max_depth, segment=2, num_scenarios=3,
                        risk_tail=2, guide=learner)
  assert isinstance(planner, mcts_agent.VecScenarioMCTSAgent) and planner.guide is learner
  buffer = expert_iteration.VecPlanLabelBuffer(n, steps)
  stats = train_lib.run_exit_loop_vec(env, learner, planner, buffer, num_iterations=1, beta=0.5, epochs=1, batch_size=8,
                                      max_episode_length=960, capture_graph=False)
  assert len(stats) == 1
  q, visits = planner.action_values()
  assert bool(torch.isfinite(q[visits > 0]).all()) and bool(torch.isneginf(q[visits == 0]).all()) and int((visits > 0).sum().item()) > 0
  assert torch.equal(buffer.target_q[steps - 1].view(n, 3), q)
  if max_depth == 1:                                 # every visit of a child is the child's own G or a revisit of it: q is that G
    action, best = planner.action.long(), planner.best_return
    _same_words(q[torch.arange(n, device=DEVICE), action].contiguous(), best, 'q[action]')
  env.check_errors()


def test_refusals():
  with pytest.raises(ValueError, match='num_scenarios'):
    mcts_agent.VecScenarioMCTSAgent(4, 2, 3, num_scenarios=17)
  with pytest.raises(ValueError, match='num_scenarios'):
    mcts_agent.VecScenarioMCTSAgent(4, 2, 3, num_scenarios=0)
  with pytest.raises(ValueError, match='risk_tail'):
    mcts_agent.VecScenarioMCTSAgent(4, 2, 3, num_scenarios=4, risk_tail=5)
  with pytest.raises(ValueError, match='risk_tail'):
    mcts_agent.VecScenarioMCTSAgent(4, 2, 3, num_scenarios=4, risk_tail=0)
  with pytest.raises(TypeError):
    mcts_agent.VecScenarioMCTSAgent(4, 2, 3)         # num_scenarios has no default
  with pytest.raises(ValueError, match='256'):
    mcts_agent.VecScenarioMCTSAgent(33, 8, 3, num_scenarios=2)
  with pytest.raises(ValueError, match='bind'):
    mcts_agent.VecScenarioMCTSAgent(4, 2, 3, num_scenarios=2).act(None)
  with pytest.raises(ValueError, match="VecScenarioBeamSearchAgent's tree"):          # the plain agent still refuses the wind
    mcts_agent.VecMCTSAgent(4, 2, 3, wind='scenarios')
  env = tgs._env(3, steps=0)
  sim = env.arena.sim
  scn = sim.fit_wind_scenarios(2)
  with pytest.raises(ValueError, match='three winds'):
    sim.mcts_search(2, 1, 2, scenarios=scn, belief=sim.fit_wind_belief())
  with pytest.raises(ValueError, match='three winds'):
    sim.mcts_search(2, 1, 2, scenarios=scn, noise_seed=1)
  with pytest.raises(ValueError, match='risk_tail'):
    sim.mcts_search(2, 1, 2, scenarios=scn, risk_tail=3)
  with pytest.raises(ValueError, match='risk_tail'):
    sim.mcts_search(2, 1, 2, risk_tail=1)
  with pytest.raises(ValueError, match='buffers'):
    sim.mcts_search(2, 1, 2, scenarios=scn, buffers=sim.mcts_buffers(2, 1, 2, num_scenarios=3))          # buffers of another M
  with pytest.raises(ValueError, match='buffers'):
    sim.mcts_search(2, 1, 2, scenarios=scn, buffers=sim.mcts_buffers(2, 1, 2))
  with pytest.raises(ValueError, match='buffers'):
    sim.mcts_search(2, 1, 2, buffers=sim.mcts_buffers(2, 1, 2, num_scenarios=2))
  with pytest.raises(ValueError, match='num_scenarios'):
    sim.mcts_buffers(2, 1, 2, num_scenarios=17)
  with pytest.raises(ValueError, match="'scenarios'.*num_scenarios"):
    env.mcts_search(2, 1, 2, wind='scenarios')
  with pytest.raises(ValueError, match='num_scenarios'):
    env.planner(search='mcts', wind='scenarios', num_rounds=2, leaves_per_round=1, max_depth=2)
  fleet = balloon_env.VecBalloonEnv(3, seed=1, vehicles=[{}, {'envelope_mass': 75.0}], vehicle_index=[0, 1, 0], auto_reset=False)
  with pytest.raises(ValueError, match='fleet'):
    fleet.planner(search='mcts', wind='scenarios', num_rounds=2, leaves_per_round=1, max_depth=2, num_scenarios=2)
  with pytest.raises(ValueError, match='fleet'):
    fleet.arena.sim.mcts_search(2, 1, 2, scenarios=scn)
  with pytest.raises(ValueError, match='fleet'):
    fleet.arena.sim.mcts_buffers(2, 1, 2, num_scenarios=2)
