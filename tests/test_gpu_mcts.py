"""Guided tree search on the device: ble_mcts_select_f32, ble_mcts_expand_f32, ble_mcts_backup_f32 and ble_mcts_finish_f32
through VecSimulator.mcts_search and VecMCTSAgent.

The reference of a node is the look-ahead itself: a non-void node reached by the actions (a_1 .. a_d) must hold, BIT FOR BIT, the state
words, the return and the steps_flown ble_rollout_leaves_f32 gives the plan a_1 x segment, .., a_d x segment flown from the same
environment in the same wind.  The selections, the statistics and the finish are held to the float64 twin (mcts_host.py) on the device's
own acc, disc, status, values and probabilities.  No tolerance anywhere: every comparison is on bits or integers."""
import numpy as np
import pytest
import torch

import mcts_host
from balloon_learning_environment_amd import _abi, _lib, device as dev, vec_state
from balloon_learning_environment_amd.agents import actor_critic, mcts_agent, qnet
from test_gpu_leaves import RT_DEAD, _assert_untouched, _five_with_a_vehicle, _parent, _snapshot
from test_gpu_tree import _env, _same_words, _winds, _with_terminals

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
GAMMA = 0.993
N, R, L, D = 65, 4, 2, 3            # 3 L 65 = 390 lanes: six full wavefronts and a partial one
DEAD = 1


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _critic(seed=1):
  net = qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', seed=seed, num_layers=2, hidden_units=64), num_atoms=2)
  return actor_critic.VecActorCriticAgent(net, deterministic=True)


def _pool_host(pool):
  """The pool's node arrays as [R, n, 3L] host arrays and its statistics."""
  torch.cuda.synchronize()
  n, shape = pool.sim.n, (pool.rounds, pool.sim.n, 3 * pool.leaves)
  out = {name: getattr(pool, name).cpu().numpy().reshape(shape) for name in ('acc', 'disc', 'flown', 'ret')}
  out['status'] = pool.node_state['status'].cpu().numpy().reshape(shape)
  out.update({name: t.cpu().numpy() for name, t in pool.statistics().items()})
  assert out['parent'].shape == (n, pool.cap)
  return out


def _path(parent, c):
  """The actions from the root to node c of one environment: a node's action is (id - 1) % 3."""
  path = []
  while c > 0:
    path.append((c - 1) % 3)
    c = int(parent[c])
  return tuple(reversed(path))


def _assert_nodes_are_their_plans(src, pool, segment, repeat, kw):
  """Every non-void pool node against rollout_plans(leaves=) of its path's plan -> (non-void nodes, nodes that went terminal)."""
  n = src.n
  host = _pool_host(pool)
  ret = host['ret'].transpose(1, 0, 2).reshape(n, -1)                      # [n, cap - 1]: node id c at column c - 1
  alive = ~np.isnan(ret)
  nodes = {}                                                               # depth -> [(e, c, path)]
  for e in range(n):
    for c in np.nonzero(alive[e])[0] + 1:
      path = _path(host['parent'][e], int(c))
      assert len(path) == host['depth'][e, c] and 1 <= len(path) <= pool.max_depth
      nodes.setdefault(len(path), []).append((e, int(c), path))
  assert not alive[np.nonzero(src.state['status'].cpu().numpy() != 0)[0]].any()          # a dead source grows nothing
  terminal = 0
  for d, group in sorted(nodes.items()):
    paths = sorted({p for _, _, p in group})
    k_of = {p: k for k, p in enumerate(paths)}
    plans = np.repeat(np.array(paths, np.uint8).T, segment, 0)             # [d * segment, K]
    plans = np.ascontiguousarray(np.broadcast_to(plans[:, None, :], (d * segment, n, len(paths))))
    arena = src.leaf_arena(len(paths))
    want = src.rollout_plans(_dev(plans), gamma=GAMMA, action_repeat=repeat, leaves=arena, **kw)
    at = _dev(np.array([pool.node_index(c, e) for e, c, _ in group], np.int64))
    leaf = _dev(np.array([e * len(paths) + k_of[p] for e, _, p in group], np.int64))
    for name in _abi.FIELD_NAMES:
      _same_words(pool.node_state[name][at], arena.state[name][leaf], (d, name))
    _same_words(pool.ret[at], want.returns.view(-1)[leaf], (d, 'ret'))
    _same_words(pool.flown[at], want.steps_flown.view(-1)[leaf], (d, 'flown'))
    terminal += int((pool.node_state['status'][at] != 0).sum().item())
  # a void node's ret is NaN and nothing counts it
  assert np.all(host['visits'][:, 1:][~alive] == 0) and np.all(np.isnan(host['g'][:, 1:][~alive]))
  return int(alive.sum()), terminal


# ------------------------------------------------------------------------------------------------ 1, 2: a node is its plan's look-ahead
@pytest.mark.parametrize('segment', [1, 3])
@pytest.mark.parametrize('wind', ['forecast', 'noise', 'belief'])
def test_every_node_equals_the_rollout_of_its_path(wind, segment):
  src, _, _ = _parent(N, 300 + segment)
  _with_terminals(src, dead=DEAD)
  kw = _winds(src, wind)
  got = src.mcts_search(R, L, D, segment=segment, gamma=GAMMA, **kw)
  alive, terminal = _assert_nodes_are_their_plans(src, got.pool, segment, 1, kw)
  print(f'{wind} segment {segment}: non-void nodes {alive} of {N * 3 * L * R}, went terminal inside an edge {terminal}')
  assert alive > N and terminal > 0


@pytest.mark.parametrize('wind', ['forecast', 'noise', 'belief'])
def test_every_node_with_a_runtime_vehicle_equals_the_rollout_of_its_path(wind):
  """ble_mcts_expand_kernel's VehicleRt instantiations, 30 lanes: edges of segment 2 x action_repeat 2."""
  src, _ = _five_with_a_vehicle()
  kw = _winds(src, wind)
  before = _snapshot(src)
  got = src.mcts_search(R, L, D, segment=2, action_repeat=2, gamma=GAMMA, **kw)
  _assert_untouched(src, before, 'the source')
  alive, terminal = _assert_nodes_are_their_plans(src, got.pool, 2, 2, kw)
  assert alive > 5 and terminal > 0                                        # (the night environment ends inside its first edge)
  assert np.all(np.isnan(_pool_host(got.pool)['ret'][:, RT_DEAD]))


# ------------------------------------------------------------------------------------------------ 3, 5: the search equals the twin
def _assert_search_equals_the_twin(src, got, trace, c_puct, segment, root_prior):
  pool = got.pool
  host = _pool_host(pool)
  n, cap = src.n, pool.cap
  source_ok = src.state['status'].cpu().numpy() == 0

  def host_of(t):
    if isinstance(t, dict):
      return {k: v.cpu().numpy() for k, v in t.items()}
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t
  trace = [tuple(host_of(t) for t in rec) for rec in trace]
  assert [rec[0] for rec in trace] == list(range(pool.rounds))
  out = {name: getattr(got, name).cpu().numpy() for name in ('action', 'q', 'visits', 'best_return', 'best_plan', 'pv_length')}
  kinds = np.zeros(3, np.int64)
  dead_valued = 0
  for e in range(n):
    twin = mcts_host.Search(pool.rounds, pool.leaves, pool.max_depth, c_puct, source_ok[e], None if root_prior is None else root_prior[e])
    rounds = []
    for r, leaf, kind, stats, value, probs in trace:
      want_leaf, want_kind = twin.select()
      assert np.array_equal(leaf[e], want_leaf) and np.array_equal(kind[e], want_kind), (e, r, leaf[e], kind[e], want_leaf, want_kind)
      kinds += np.bincount(kind[e], minlength=3)
      rows = slice(e * 3 * pool.leaves, (e + 1) * 3 * pool.leaves)
      ok = host['status'][r, e] == 0
      twin.backup(host['acc'][r, e], host['disc'][r, e], ok, None if value is None else value[rows], None if probs is None else probs[rows])
      born = twin.born
      for name in ('parent', 'first_child', 'depth', 'visits', 'pending'):
        assert np.array_equal(stats[name][e, :born], getattr(twin, name)[:born]), (e, r, name)
      for name in ('value_sum', 'g', 'prior'):
        assert np.array_equal(_bits(stats[name][e, :born]), _bits(getattr(twin, name)[:born])), (e, r, name)
      assert np.array_equal(_bits(stats['g_range'][e]), _bits(np.array([twin.g_lo, twin.g_hi])))
      rounds.append((leaf[e], kind[e]))
      mcts_host.check_invariants(pool.leaves, stats['parent'][e, :born], stats['visits'][e], stats['value_sum'][e], stats['g'][e], rounds)
      if value is not None:                       # a node that is not OK keeps its return: V = 0
        first = born - 3 * pool.leaves
        for j in np.nonzero(~ok & ~np.isnan(host['acc'][r, e]))[0]:
          assert _bits(stats['g'][e, first + j:first + j + 1])[0] == _bits(host['acc'][r, e, j:j + 1])[0]
          dead_valued += 1
    want = twin.finish(segment)
    assert out['action'][e] == want['action'] and out['pv_length'][e] == want['pv_length'], e
    assert np.array_equal(out['best_plan'][:, e], want['best_plan']) and np.array_equal(out['visits'][e], want['visits']), e
    assert np.array_equal(_bits(out['q'][e]), _bits(want['q'])), e
    assert _bits(out['best_return'][e:e + 1])[0] == _bits(np.float32(want['best_return']).reshape(1))[0], e
  assert cap == 1 + 3 * L * R
  return kinds, dead_valued


@pytest.mark.parametrize('c_puct', [1.25, 0.0])
def test_the_search_equals_the_twin(c_puct):
  src, rng, _ = _parent(N, 31)
  _with_terminals(src, dead=7)
  root_prior = rng.dirichlet(np.ones(3), N).astype(np.float32)
  root_prior[5] = [0.5, np.nan, 0.5]                                       # a row the pool makes uniform
  trace = []
  got = src.mcts_search(R, L, D, segment=2, gamma=GAMMA, c_puct=c_puct, belief=src.fit_wind_belief(), root_prior=_dev(root_prior), trace=trace)
  kinds, _ = _assert_search_equals_the_twin(src, got, trace, c_puct, 2, root_prior)
  print('c_puct', c_puct, 'slots: EMPTY, EXPAND, REVISIT =', kinds.tolist())
  assert kinds[mcts_host.EXPAND] > 0 and kinds[mcts_host.EMPTY] > 0
  action, best = got.action.cpu().numpy(), got.best_return.cpu().numpy()
  assert action[7] == 1 and best[7] == 0.0 and np.all(got.best_plan.cpu().numpy()[:, 7] == 1) and got.pv_length.cpu().numpy()[7] == 0
  live = np.delete(np.arange(N), 7)
  assert np.isfinite(best[live]).all() and np.all(got.pv_length.cpu().numpy()[live] >= 1)
  assert np.array_equal(_bits(got.q.cpu().numpy()[live, action[live]]), _bits(best[live]))


def test_the_guided_search_equals_the_twin_and_observes_its_round_slices():
  src, _, _ = _parent(N, 32)
  _with_terminals(src, dead=7)
  critic = _critic()
  buffers = src.mcts_buffers(R, L, D, 2, guide=True)
  critic.act(buffers.obs, out=buffers.guide_action, value=buffers.value, probs=buffers.probs)
  trace = []
  belief = src.fit_wind_belief()
  got = src.mcts_search(R, L, D, segment=2, gamma=GAMMA, belief=belief, guide_fn=critic.act, buffers=buffers, trace=trace)
  assert got.pool is buffers
  kinds, dead_valued = _assert_search_equals_the_twin(src, got, trace, 1.25, 2, None)
  print('guided slots: EMPTY, EXPAND, REVISIT =', kinds.tolist(), 'dead nodes valued 0:', dead_valued)
  assert dead_valued > 0 and kinds[mcts_host.REVISIT] > 0
  # the values moved the statistics: some G is not its node's return
  host = _pool_host(buffers)
  g, acc = host['g'][:, 1:], host['acc'].transpose(1, 0, 2).reshape(N, -1)
  assert int((~np.isnan(g) & (_bits(g) != _bits(acc))).sum()) > N
  # every round's slice of the pool, observed as it lies, is the observation of a leaf arena filled with the same states
  for r in range(R):
    view = buffers.arenas[r]
    assert view.n == N * 3 * L and view.leaves_per_env == 3 * L
    arena = src.leaf_arena(3 * L)
    for name, t in arena.state.items():
      t.copy_(view.state[name])
    _same_words(src.observe_leaves(view), src.observe_leaves(arena), ('round', r))
  # the last round's rows are what the guide was asked: its values and probabilities on that observation
  value, probs, acts = torch.empty(N * 3 * L, device=DEVICE), torch.empty(N * 3 * L, 3, device=DEVICE), torch.empty(N * 3 * L, dtype=torch.uint8, device=DEVICE)
  critic.act(src.observe_leaves(buffers.arenas[R - 1]), out=acts, value=value, probs=probs)
  _same_words(value, trace[-1][4], 'value')
  _same_words(probs, trace[-1][5], 'probs')


# ------------------------------------------------------------------------------------------------ 4: housekeeping
def test_flags_go_to_their_own_word_and_nothing_is_written():
  env = _env(N, seed=5)
  sim = env.arena.sim
  obs = sim.observe(env._noise_now(), append=False).clone()
  for wind in mcts_agent.WINDS:
    agent = env.planner(search='mcts', num_rounds=R, leaves_per_round=L, max_depth=D, segment=2, wind=wind, guide=_critic())
    assert isinstance(agent, mcts_agent.VecMCTSAgent) and agent.get_name() == 'MCTSAgent'
    before = _snapshot(sim)
    flags = int(sim.err_flags.item())
    agent.act(obs)
    _assert_untouched(sim, before, wind)
    assert int(sim.err_flags.item()) == flags == 0
    probs = agent.visit_probs().cpu().numpy()
    assert probs.shape == (N, 3) and np.all((np.abs(probs.sum(1) - 1) < 1e-6) | (probs.sum(1) == 0))
  # an upwelling IR outside total_absorptivity's range (test_gpu_rollout.py's device): the flag of the imagined flights, not the real one's
  sim.rollout_flags.zero_()
  sim.state['upwelling_infrared'][3] = 1e-3
  env.planner(search='mcts', num_rounds=2, leaves_per_round=1, max_depth=2, segment=1, wind='forecast').act(None)
  torch.cuda.synchronize()
  assert int(sim.rollout_flags.item()) & _lib.FLAG_ABSORPTIVITY and int(sim.err_flags.item()) == 0
  sim.check_errors()                                # a flight that never happened raises nothing


# ------------------------------------------------------------------------------------------------ 6: a captured decision
def test_graph_equals_eager_and_no_counter_moves():
  n, decisions = N, 3
  runs = {}
  for mode in ('eager', 'graph'):
    env = _env(n, seed=9)
    agent = env.planner(search='mcts', num_rounds=R, leaves_per_round=L, max_depth=D, segment=2, guide=_critic())
    actions = torch.ones(n, dtype=torch.uint8, device=DEVICE)
    obs = env.arena.sim.observe(env._noise_now(), append=False).clone()

    def body():
      agent.act(obs, out=actions)
      env._step_eager(actions, obs_out=obs)
    if mode == 'eager':                                  # two decisions on one state: the same bytes, nothing carried between them
      agent.act(obs)
      first = {k: getattr(agent, k).clone() for k in ('action', 'q', 'visits', 'best_return', 'best_plan')}
      stats = agent.buffers.statistics()
      agent.act(obs)
      for k, t in first.items():
        _same_words(getattr(agent, k), t, k)
      for k, t in agent.buffers.statistics().items():
        _same_words(t, stats[k], k)
    body()                                               # (lazy allocations happen here, in both modes)
    graph = dev.capture(env.device, body)[0] if mode == 'graph' else None
    log = []
    for _ in range(decisions):
      graph.replay() if graph is not None else body()
      torch.cuda.synchronize()
      log.append((actions.cpu().numpy().copy(), _bits(agent.best_return.cpu().numpy()).copy(), _bits(agent.q.cpu().numpy()).copy(),
                  agent.visits.cpu().numpy().copy(), agent.best_plan.cpu().numpy().copy(), obs.cpu().numpy().copy()))
    runs[mode] = log
    env.check_errors()
  for d, (a, b) in enumerate(zip(runs['eager'], runs['graph'])):
    for x, y in zip(a, b):
      assert np.array_equal(x, y), d


# ------------------------------------------------------------------------------------------------ 7: batch invariance
def test_batch_invariance():
  n, e = 5, 3
  src, _, _ = _parent(n, 41, per_env=True)
  one = vec_state.VecSimulator(1, DEVICE, env_offset=e)
  for name, t in one.state.items():
    t.copy_(src.state[name][e:e + 1])
  one.set_grid(src.grid[e:e + 1].cpu().numpy(), per_env=True)
  one._allocate_history(True)
  for name, t in one._gp.items():
    t.copy_(src._gp[name][e:e + 1])
  one._obs_reset.copy_(src._obs_reset[e:e + 1])
  make = lambda: mcts_agent.VecMCTSAgent(num_rounds=R, leaves_per_round=L, max_depth=D, segment=2, wind='belief')
  batch, alone = make().bind(src), make().bind(one)
  batch.act(None)
  alone.act(None)
  torch.cuda.synchronize()
  for name in ('action', 'q', 'visits', 'best_return', 'best_plan'):
    a, b = getattr(alone, name), getattr(batch, name)
    _same_words(a, (b[:, e:e + 1] if name == 'best_plan' else b[e:e + 1]).contiguous(), name)
  for name, t in alone.buffers.statistics().items():
    _same_words(t, batch.buffers.statistics()[name][e:e + 1].contiguous(), name)


def test_refusals():
  with pytest.raises(ValueError, match='256'):
    mcts_agent.VecMCTSAgent(num_rounds=33, leaves_per_round=8, max_depth=3)
  with pytest.raises(ValueError, match='960'):
    mcts_agent.VecMCTSAgent(4, 2, max_depth=121, segment=4, action_repeat=2)
  with pytest.raises(ValueError, match="VecScenarioBeamSearchAgent's tree"):
    mcts_agent.VecMCTSAgent(4, 2, 3, wind='scenarios')
  with pytest.raises(ValueError, match='wind'):
    mcts_agent.VecMCTSAgent(4, 2, 3, wind='gp')
  with pytest.raises(ValueError, match='c_puct'):
    mcts_agent.VecMCTSAgent(4, 2, 3, c_puct=float('nan'))
  with pytest.raises(ValueError, match='sampling agent'):
    mcts_agent.VecMCTSAgent(4, 2, 3, guide=actor_critic.VecActorCriticAgent(_critic().network, deterministic=False))
  with pytest.raises(ValueError, match='bind'):
    mcts_agent.VecMCTSAgent(4, 2, 3).act(None)
  env = _env(3, steps=0)
  with pytest.raises(ValueError, match='two winds'):
    env.arena.sim.mcts_search(2, 1, 2, noise_seed=1, belief=env.arena.fit_wind_belief())
  with pytest.raises(ValueError, match='buffers'):
    env.arena.sim.mcts_search(2, 1, 2, buffers=env.arena.sim.mcts_buffers(3, 1, 2))
  with pytest.raises(ValueError, match='scenarios'):
    env.mcts_search(2, 1, 2, wind='scenarios')
  from balloon_learning_environment_amd.env import balloon_env
  fleet = balloon_env.VecBalloonEnv(3, seed=1, vehicles=[{}, {'envelope_mass': 75.0}], vehicle_index=[0, 1, 0], auto_reset=False)
  with pytest.raises(ValueError, match='a fleet \\(set_fleet\\) has no look-ahead kernel'):
    fleet.planner(search='mcts', num_rounds=2, leaves_per_round=1, max_depth=2)
  with pytest.raises(ValueError, match='max_depth: the budget'):            # the budget of a search has no default
    env.planner(search='mcts', num_rounds=2, leaves_per_round=1)
  with pytest.raises(TypeError):
    mcts_agent.VecMCTSAgent()
  with pytest.raises(ValueError, match='fleet'):
    fleet.arena.sim.mcts_search(2, 1, 2)
  got = env.mcts_search(2, 1, 2, wind='truth')
  assert tuple(got.visits.shape) == (3, 3) and tuple(got.best_plan.shape) == (2 * 4, 3)
