"""Plan by beam search on the device: ble_tree_expand_f32, ble_tree_select_f32 and ble_tree_finish_f32 through
VecSimulator.tree_search and VecBeamSearchAgent.

The reference of a node is the look-ahead itself: a non-void node reached by the actions (a_1 .. a_d) must hold, BIT FOR BIT, the state
words, the return and the steps_flown ble_rollout_leaves_f32 gives the plan a_1 x segment, .., a_d x segment flown from the same
environment in the same wind.  The selections and the finish are held to the NumPy twin (tree_host.py) on the device's own returns.
No tolerance anywhere: every comparison is on bits or integers."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import tree_host
from balloon_learning_environment_amd import _abi, _lib, device as dev, vec_state
from balloon_learning_environment_amd.agents import actor_critic, beam_agent, qnet
from balloon_learning_environment_amd.env import balloon_env
from balloon_learning_environment_amd.eval import eval_lib, suites
from test_gpu_leaves import RT_DEAD, RT_NIGHT, _assert_untouched, _five_with_a_vehicle, _parent, _snapshot

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
GAMMA = 0.993
NOISE_SEED = 5


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_words(a, b, what):
  assert a.dtype == b.dtype and a.shape == b.shape, what
  bad = torch.nonzero(a.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8))
  assert bad.numel() == 0, (what, bad[:4].tolist())


def _with_terminals(src, dead):
  """The device of test_terminals_freeze_a_plan_and_a_dead_source_flies_nothing: the night environments get a battery of 23 Wh, which the
  night load drains inside a plan; environment `dead` is not OK."""
  night = (src.state['solar_charging'] == 0) & (src.state['status'] == 0)
  src.state['battery_charge'][night] = 23.0
  src.state['status'][dead] = 2
  src.state['last_command'][dead] = 2
  return int(night.sum().item())


def _winds(src, wind):
  return dict(noise_seed=NOISE_SEED if wind == 'noise' else None, belief=src.fit_wind_belief() if wind == 'belief' else None)


# ------------------------------------------------------------------------------------------------ 1: one level equals the rollout
@pytest.mark.parametrize('segment', [1, 3])
@pytest.mark.parametrize('wind', ['forecast', 'noise', 'belief'])
def test_one_level_equals_the_rollout(wind, segment):
  n = 65                                          # 3 x 65 lanes: three full wavefronts and a partial one
  src, _, _ = _parent(n, 300 + segment)
  _with_terminals(src, dead=1)
  kw = _winds(src, wind)
  plans = np.broadcast_to(np.arange(3, dtype=np.uint8), (segment, n, 3))
  want_arena = src.leaf_arena(3)
  want = src.rollout_plans(_dev(plans), gamma=GAMMA, leaves=want_arena, **kw)
  before = _snapshot(src)
  got = src.tree_search(1, 1, segment=segment, gamma=GAMMA, action_values=True, **kw)
  _assert_untouched(src, before, 'the source')
  assert got.leaves.n == 3 * n and got.leaves.leaves_per_env == 3
  flown = want.steps_flown.cpu().numpy()
  void = np.zeros((n, 3), bool)
  void[flown[:, 0] == 0, 1:] = True               # a dead source: the a = 0 child carries it on, the other two stand for nothing
  assert void[1].tolist() == [False, True, True]
  live = _dev(~void)
  for name in _abi.FIELD_NAMES:
    _same_words(got.leaves.state[name].view(n, 3), want_arena.state[name].view(n, 3), name)      # (a void node is the same copy)
  _same_words(got.returns[live], want.returns[live], 'returns')
  assert bool(torch.isnan(got.returns[~live]).all())
  _same_words(got.steps_flown, want.steps_flown, 'steps_flown')
  # the finish on one level: the twin on the device's returns
  ret = got.returns.cpu().numpy()
  ok = src.state['status'].cpu().numpy() == 0
  plan, action, best, q, visits = tree_host.finish(ret, [], 1, segment, ok)
  assert np.array_equal(got.best_plan.cpu().numpy(), plan) and np.array_equal(got.action.cpu().numpy(), action)
  assert np.array_equal(_bits(got.best_return.cpu().numpy()), _bits(best))
  assert np.array_equal(_bits(got.q.cpu().numpy()), _bits(q)) and np.array_equal(got.visits.cpu().numpy(), visits)
  assert action[1] == 1 and best[1] == 0.0 and visits[1].tolist() == [1, 0, 0]
  print(f'{wind} segment {segment}: plans that went terminal {int(((flown > 0) & (flown < segment)).sum())} of {3 * n}')


@pytest.mark.parametrize('wind', ['forecast', 'noise', 'belief'])
def test_one_level_with_a_runtime_vehicle_equals_the_rollout(wind):
  """ble_tree_expand_kernel's VehicleRt instantiations, 15 lanes: one level of edges of segment 2 x action_repeat 2 against the leaf
  rollout flown with the same vehicle (which test_gpu_leaves.py holds to stepped copies)."""
  n, segment, repeat = 5, 2, 2
  src, _ = _five_with_a_vehicle()
  kw = _winds(src, wind)
  plans = np.broadcast_to(np.arange(3, dtype=np.uint8), (segment, n, 3))
  want_arena = src.leaf_arena(3)
  want = src.rollout_plans(_dev(plans), gamma=GAMMA, action_repeat=repeat, leaves=want_arena, **kw)
  before = _snapshot(src)
  got = src.tree_search(1, 1, segment=segment, action_repeat=repeat, gamma=GAMMA, **kw)
  _assert_untouched(src, before, 'the source')
  assert got.leaves.n == 3 * n and got.leaves.leaves_per_env == 3
  void = np.zeros((n, 3), bool)
  void[RT_DEAD, 1:] = True                        # a dead source: the a = 0 child carries it on, the other two stand for nothing
  live = _dev(~void)
  for name in _abi.FIELD_NAMES:
    _same_words(got.leaves.state[name].view(n, 3), want_arena.state[name].view(n, 3), (wind, name))      # (a void node is the same copy)
  _same_words(got.returns[live], want.returns[live], 'returns')
  assert bool(torch.isnan(got.returns[~live]).all())
  _same_words(got.steps_flown, want.steps_flown, 'steps_flown')
  flown = want.steps_flown.cpu().numpy()
  assert np.all(flown[RT_DEAD] == 0) and np.all((flown[RT_NIGHT] > 0) & (flown[RT_NIGHT] < segment * repeat))      # it ends inside the edge
  assert np.all(np.delete(flown, [RT_NIGHT, RT_DEAD], 0) == segment * repeat)


# ------------------------------------------------------------------------------------------------ 2: the exhaustive tree is the enumeration
def _six_environments():
  """Six environments with per-environment grids: three that fly in the dark and three in daylight, picked from a batch of 64."""
  big, rng, _ = _parent(64, 77, steps=4)
  night = torch.nonzero((big.state['solar_charging'] == 0) & (big.state['status'] == 0)).view(-1)
  day = torch.nonzero((big.state['solar_charging'] > 0) & (big.state['status'] == 0)).view(-1)
  assert night.numel() >= 3 and day.numel() >= 3, (night.numel(), day.numel())
  pick = torch.cat([night[:3], day[:3]])
  src = vec_state.VecSimulator(6, DEVICE)
  for name, t in src.state.items():
    t.copy_(big.state[name][pick])
  src.set_grid(rng.uniform(-12.0, 12.0, (6,) + vec_state.GRID_SHAPE).astype(np.float32), per_env=True)
  return src


def test_the_exhaustive_tree_is_the_enumeration():
  n, D, segment, B = 6, 3, 2, 27
  src = _six_environments()
  dead = 4
  assert _with_terminals(src, dead) >= 3
  # the enumeration: plan k = 9 a_1 + 3 a_2 + a_3, each action over its segment
  digits = np.array([[k // 9, (k // 3) % 3, k % 3] for k in range(27)], np.uint8)                 # [27, D]
  plans = np.ascontiguousarray(np.broadcast_to(np.repeat(digits.T, segment, 0)[:, None, :], (D * segment, n, 27)))
  enum_arena = src.leaf_arena(27)
  enum = src.rollout_plans(_dev(plans), gamma=GAMMA, leaves=enum_arena)
  before = _snapshot(src)
  got = src.tree_search(D, B, segment=segment, gamma=GAMMA)
  _assert_untouched(src, before, 'the source')
  torch.cuda.synchronize()
  enum_flown, enum_ret = enum.steps_flown.cpu().numpy(), enum.returns.cpu().numpy()
  assert np.any((enum_flown > 0) & (enum_flown < D * segment)), 'no plan ends strictly inside the horizon'
  assert np.all(enum_flown[dead] == 0)
  choice = got.buffers.choice.cpu().numpy()
  ret, flown = got.returns.cpu().numpy(), got.steps_flown.cpu().numpy()
  assert ret.shape == (n, 27)
  # every non-void leaf is the look-ahead of its own path
  ks = np.array([[int(np.dot(tree_host.path(choice, e, c, D), [9, 3, 1])) for c in range(27)] for e in range(n)])
  live = ~np.isnan(ret)
  index = _dev(ks).long()
  for name in _abi.FIELD_NAMES:
    want = torch.gather(enum_arena.state[name].view(n, 27), 1, index)
    _same_words(got.leaves.state[name].view(n, 27)[_dev(live)], want[_dev(live)], name)
  assert np.array_equal(_bits(ret[live]), _bits(np.take_along_axis(enum_ret, ks, 1)[live]))
  assert np.array_equal(flown[live], np.take_along_axis(enum_flown, ks, 1)[live])
  for e in range(n):
    assert sorted(set(ks[e].tolist())) == list(range(27))                                         # nothing was cut: every plan has its leaf
    # the non-void returns, the a = 0 chains among them, cover the returns of all 27 plans
    assert set(_bits(enum_ret[e]).tolist()) <= set(_bits(ret[e][live[e]]).tolist()), e
  assert live[dead].sum() == 1 and not live.all() and live.sum() > n
  # the best plan is the enumeration's best, and flying it earns its return
  best = np.array([enum_ret[e, tree_host.order(enum_ret[e])[0]] for e in range(n)], np.float32)
  assert np.array_equal(_bits(got.best_return.cpu().numpy()), _bits(best))
  assert np.all(got.best_plan.cpu().numpy()[:, dead] == 1) and best[dead] == 0.0
  again = src.rollout_plans(got.best_plan.view(D * segment, n, 1).contiguous(), gamma=GAMMA)
  assert np.array_equal(_bits(again.returns.cpu().numpy()[:, 0]), _bits(got.best_return.cpu().numpy()))
  assert np.array_equal(got.action.cpu().numpy(), got.best_plan.cpu().numpy()[0])
  print('plans ending inside the horizon:', int(((enum_flown > 0) & (enum_flown < D * segment)).sum()), 'void leaves:', int((~live).sum()))


# ------------------------------------------------------------------------------------------------ 3: pruning
def test_pruning_equals_the_twin():
  n, D, segment, B = 65, 4, 2, 4
  src, _, _ = _parent(n, 31)
  _with_terminals(src, dead=7)
  trace = []
  got = src.tree_search(D, B, segment=segment, gamma=GAMMA, belief=src.fit_wind_belief(), action_values=True, trace=trace)
  torch.cuda.synchronize()
  choice = got.buffers.choice.cpu().numpy()
  sizes = tree_host.level_sizes(D, B)
  assert [c for _, c in sizes] == [3, 9, 12, 12] and len(trace) == D
  lists = []
  for (level, ret, parent), (_, C) in zip(trace, sizes):
    assert tuple(ret.shape) == (n, C)
    want = tree_host.select(ret.cpu().numpy(), B)
    keep = want.shape[1]
    assert np.array_equal(parent.cpu().numpy()[:, :keep], want), level
    assert np.array_equal(choice[level - 1][:, :keep], want), level
    lists.append(want)
  ret = got.returns.cpu().numpy()
  assert np.array_equal(_bits(ret), _bits(trace[-1][1].cpu().numpy()))
  ok = src.state['status'].cpu().numpy() == 0
  plan, action, best, q, visits = tree_host.finish(ret, lists, D, segment, ok)
  assert np.array_equal(got.best_plan.cpu().numpy(), plan) and np.array_equal(got.action.cpu().numpy(), action)
  assert np.array_equal(_bits(got.best_return.cpu().numpy()), _bits(best))
  assert np.array_equal(_bits(got.q.cpu().numpy()), _bits(q)) and np.array_equal(got.visits.cpu().numpy(), visits)
  assert np.isfinite(best).all() and best[7] == 0.0 and np.all(plan[:, 7] == 1)
  live = ok & np.isfinite(best)
  assert np.array_equal(_bits(q[live, action[live]]), _bits(best[live]))                        # the chosen action's value is the best return
  # the best plan's return is what the look-ahead gives that plan
  again = src.rollout_plans(got.best_plan.view(D * segment, n, 1).contiguous(), gamma=GAMMA, belief=src.fit_wind_belief())
  assert np.array_equal(_bits(again.returns.cpu().numpy()[:, 0]), _bits(best))
  print('actions', np.bincount(action, minlength=3), 'void nodes at the last level', int(np.isnan(ret).sum()))


# ------------------------------------------------------------------------------------------------ 4: the truth
def _env(n, seed=3, wind_noise=True, steps=3):
  env = balloon_env.VecBalloonEnv(n, seed=seed, wind_noise=wind_noise, auto_reset=False)
  env.reset()
  rng = np.random.default_rng(seed)
  for a in rng.integers(0, 3, (steps, n)).astype(np.uint8):
    env.step(_dev(a))
  return env


def test_the_chosen_plan_is_real():
  n = 65
  env = _env(n, seed=8)
  agent = env.planner(search='beam', beam_width=4, depth=3, segment=2, wind='truth')
  assert isinstance(agent, beam_agent.VecBeamSearchAgent)
  agent.act(None)
  best_plan, best_return = (t.clone() for t in agent.plan())
  # the environment's own pass-through is the same search, in every wind it names
  for wind in ('truth', 'forecast', 'belief'):
    other = env.planner(search='beam', beam_width=4, depth=3, segment=2, wind=wind)
    other.act(None)
    tree = env.tree_search(3, 4, segment=2, wind=wind, gamma=other.gamma)
    _same_words(tree.best_return, other.best_return.clone(), wind)
    _same_words(tree.best_plan, other.best_plan.clone(), wind)
  _same_words(env.tree_search(3, 4, segment=2, wind='truth').best_return, best_return, 'truth')
  H = agent.horizon
  rewards = torch.stack([env.step(best_plan[h].contiguous())[1] for h in range(H)]).cpu().numpy()
  acc, disc = np.zeros(n, np.float64), 1.0
  for t in range(H):                                     # the kernel's order: the product and the sum rounded separately
    term = disc * rewards[t].astype(np.float64)
    acc += term
    disc *= agent.gamma
  print('best_return', best_return.cpu().numpy()[:8], 'flown', acc.astype(np.float32)[:8])
  assert np.array_equal(_bits(acc.astype(np.float32)), _bits(best_return.cpu().numpy()))
  env.check_errors()


# ------------------------------------------------------------------------------------------------ 5: housekeeping
def test_flags_go_to_their_own_word_and_nothing_is_written():
  env = _env(65, seed=5)
  sim = env.arena.sim
  for wind in beam_agent.WINDS:
    agent = env.planner(search='beam', beam_width=4, depth=3, segment=2, wind=wind, action_values=True)
    before = _snapshot(sim)
    flags = int(sim.err_flags.item())
    agent.act(None)
    _assert_untouched(sim, before, wind)
    assert int(sim.err_flags.item()) == flags
  # an upwelling IR outside total_absorptivity's range (test_gpu_rollout.py's device): the flag of the imagined flights, not the real one's
  sim.rollout_flags.zero_()
  sim.state['upwelling_infrared'][3] = 1e-3
  env.planner(search='beam', beam_width=4, depth=2, segment=1, wind='forecast').act(None)
  torch.cuda.synchronize()
  assert int(sim.rollout_flags.item()) & _lib.FLAG_ABSORPTIVITY and int(sim.err_flags.item()) == flags
  sim.check_errors()                                # a flight that never happened raises nothing


@pytest.mark.parametrize('wind', ['forecast', 'belief'])
def test_batch_invariance(wind):
  n, D, segment, B = 65, 3, 2, 4
  src, _, _ = _parent(n, 41, per_env=True)
  _with_terminals(src, dead=2)
  batch = src.tree_search(D, B, segment=segment, gamma=GAMMA, action_values=True, **_winds(src, wind))
  torch.cuda.synchronize()
  for e in (0, 2, 33, 64):
    one = vec_state.VecSimulator(1, DEVICE, env_offset=e)
    for name, t in one.state.items():
      t.copy_(src.state[name][e:e + 1])
    one.set_grid(src.grid[e:e + 1].cpu().numpy(), per_env=True)
    one._allocate_history(True)
    for name, t in one._gp.items():
      t.copy_(src._gp[name][e:e + 1])
    one._obs_reset.copy_(src._obs_reset[e:e + 1])
    alone = one.tree_search(D, B, segment=segment, gamma=GAMMA, action_values=True, **_winds(one, wind))
    torch.cuda.synchronize()
    for name in ('action', 'best_plan', 'best_return', 'q', 'visits', 'returns', 'steps_flown'):
      a, b = getattr(alone, name), getattr(batch, name)
      b = b[:, e:e + 1] if name == 'best_plan' else b[e:e + 1]
      _same_words(a, b, (wind, e, name))
    assert np.array_equal(alone.buffers.choice.cpu().numpy()[:, 0], batch.buffers.choice.cpu().numpy()[:, e])


def test_graph_equals_eager():
  n, decisions = 65, 3
  runs = {}
  for mode in ('eager', 'graph'):
    env = _env(n, seed=9)
    agent = env.planner(search='beam', beam_width=4, depth=3, segment=2, action_values=True)
    actions = torch.ones(n, dtype=torch.uint8, device=DEVICE)
    obs = torch.empty(n, 1099, dtype=torch.float32, device=DEVICE)

    def body():
      agent.act(None, out=actions)
      env._step_eager(actions, obs_out=obs)
    body()                                               # (lazy allocations happen here, in both modes)
    graph = dev.capture(env.device, body)[0] if mode == 'graph' else None
    log = []
    for _ in range(decisions):
      graph.replay() if graph is not None else body()
      torch.cuda.synchronize()
      log.append((actions.cpu().numpy().copy(), _bits(agent.best_return.cpu().numpy()).copy(), _bits(agent.q.cpu().numpy()).copy(),
                  obs.cpu().numpy().copy()))
    runs[mode] = log
    env.check_errors()
  for d, (a, b) in enumerate(zip(runs['eager'], runs['graph'])):
    for x, y in zip(a, b):
      assert np.array_equal(x, y), d


# ------------------------------------------------------------------------------------------------ 6: a leaf value
def test_the_leaf_value_is_the_public_composition():
  n = 5
  env = _env(n, seed=7)
  sim = env.arena.sim
  net = qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', 0, 2, 64), num_atoms=2)
  critic = actor_critic.VecActorCriticAgent(net)
  agent = env.planner(search='beam', beam_width=4, depth=3, segment=2, wind='belief', leaf_value=critic, action_values=True)
  agent.act(None)
  res = agent.result
  torch.cuda.synchronize()
  C = res.leaves.leaves_per_env
  assert C == 12 and tuple(res.returns.shape) == (n, C)
  obs = sim.observe_leaves(res.leaves)
  values, acts = torch.empty(n * C, device=DEVICE), torch.empty(n * C, dtype=torch.uint8, device=DEVICE)
  critic.act(obs, out=acts, value=values)
  score = torch.full((n, C), 55.0, device=DEVICE)
  bs = _abi.BlePlanBootstrap(n, C, 0, agent.gamma, res.returns.data_ptr(), res.steps_flown.data_ptr(), res.leaves.state['status'].data_ptr(),
                             values.data_ptr(), score.data_ptr())
  _lib.check(_lib.lib().ble_plan_bootstrap_f32(ctypes.byref(bs), dev.stream_ptr(torch.device(DEVICE))), 'ble_plan_bootstrap_f32')
  torch.cuda.synchronize()
  _same_words(agent.score, score, 'the finish keys')
  ret, keys = res.returns.cpu().numpy(), score.cpu().numpy()
  assert int((_bits(ret) != _bits(keys)).sum()) > 0, 'the critic moved no key'
  choice = res.buffers.choice.cpu().numpy()
  lists = [choice[d][:, :min(c, 4)] for d, (_, c) in enumerate(tree_host.level_sizes(3, 4))]
  plan, action, best, q, visits = tree_host.finish(ret, lists, 3, 2, sim.state['status'].cpu().numpy() == 0, score=keys)
  assert np.array_equal(res.best_plan.cpu().numpy(), plan) and np.array_equal(res.action.cpu().numpy(), action)
  assert np.array_equal(_bits(res.best_return.cpu().numpy()), _bits(best))
  assert np.array_equal(_bits(res.q.cpu().numpy()), _bits(q)) and np.array_equal(res.visits.cpu().numpy(), visits)


# ------------------------------------------------------------------------------------------------ 7: evaluation
def test_evaluation_is_finite_and_batch_invariant():
  suite = suites.EvaluationSuite([11, 12, 13], 8)
  make = lambda: beam_agent.VecBeamSearchAgent(beam_width=4, depth=2, segment=2)
  alone = eval_lib.eval_agent_vec(make(), suite, batch_size=1)
  batch = eval_lib.eval_agent_vec(make(), suite, batch_size=3)
  for a, b in zip(alone, batch):
    assert dataclasses.asdict(a) == dataclasses.asdict(b), (a, b)
    assert np.isfinite(a.cumulative_reward) and np.isfinite(a.time_within_radius)
  assert [r.seed for r in batch] == [11, 12, 13]
  assert make().get_name() == 'BeamSearchAgent'


def test_refusals():
  with pytest.raises(ValueError, match='256'):
    beam_agent.VecBeamSearchAgent(beam_width=257)
  with pytest.raises(ValueError, match='960'):
    beam_agent.VecBeamSearchAgent(depth=121, segment=4, action_repeat=2)
  with pytest.raises(ValueError, match='scenarios'):
    beam_agent.VecBeamSearchAgent(wind='scenarios')
  with pytest.raises(ValueError, match='wind'):
    beam_agent.VecBeamSearchAgent(wind='gp')
  with pytest.raises(ValueError, match='bind'):
    beam_agent.VecBeamSearchAgent().act(None)
  env = _env(3, steps=0)
  with pytest.raises(ValueError, match='truth'):
    beam_agent.VecBeamSearchAgent(wind='truth').bind(env.arena.sim, seeds=torch.zeros(3, dtype=torch.int64, device=DEVICE))
  with pytest.raises(ValueError, match='search'):
    env.planner(search='mcts')
  with pytest.raises(ValueError, match='two winds'):
    env.arena.sim.tree_search(2, 4, noise_seed=1, belief=env.arena.fit_wind_belief())
  with pytest.raises(ValueError, match='buffers'):
    env.arena.sim.tree_search(2, 4, buffers=env.arena.sim.tree_buffers(3, 4))
  fleet = balloon_env.VecBalloonEnv(3, seed=1, vehicles=[{}, {'envelope_mass': 75.0}], vehicle_index=[0, 1, 0], auto_reset=False)
  with pytest.raises(ValueError, match='fleet'):
    fleet.planner(search='beam')
  with pytest.raises(ValueError, match='fleet'):
    fleet.arena.sim.tree_search(2, 4)
  assert type(env.planner()).__name__ == 'VecLookaheadAgent'          # the default search is the sampler
