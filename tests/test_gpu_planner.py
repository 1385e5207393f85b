"""The planner on the device: ble_plan_sample_u8, ble_plan_select_f32 and agents.lookahead_agent.VecLookaheadAgent.

References.  The sampler and the selection: the NumPy twin written from DESIGN 3k (tests/plan_host.py), bit for bit -- the sampler is
integer arithmetic, the selection an order on float32 values.  The agent: the composition it claims to be -- twin plans ->
env.lookahead(plans, wind=...) -> twin selection, iteration after iteration, decision after decision -- all outputs bitwise; and, with
wind='truth', the flight itself: the plan the agent chose, flown with env.step, earns the return the agent expected (the float64
discounted sum of the rewards in the kernel's order, rounded once: bit for bit).  There is no tolerance in this file."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import plan_host
from balloon_learning_environment_amd import _abi, _lib, device as dev
from balloon_learning_environment_amd.agents import lookahead_agent
from balloon_learning_environment_amd.env import balloon_env
from balloon_learning_environment_amd.eval import eval_lib, suites

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)


def _gpu_sample(n, K, H, segment, iteration, decision, seed=0, env_seed=None, env_offset=0, counts=None, best_plan=None):
  counter = _dev(np.array([decision & (2 ** 64 - 1)], np.uint64).view(np.int64))
  env_seed_t = None if env_seed is None else _dev(np.asarray(env_seed, np.uint64).view(np.int64))
  counts_t = None if counts is None else _dev(np.asarray(counts, np.uint16).view(np.int16))
  best = _dev(np.full((H, n), 1, np.uint8) if best_plan is None else best_plan)
  plans = torch.full((H, n, K), 9, dtype=torch.uint8, device=DEVICE)
  ps = _abi.BlePlanSample(n, K, H, segment, iteration, seed & (2 ** 64 - 1), dev.ptr(env_seed_t), env_offset, counter.data_ptr(),
                          dev.ptr(counts_t), best.data_ptr(), plans.data_ptr())
  _lib.check(_lib.lib().ble_plan_sample_u8(ctypes.byref(ps), dev.stream_ptr(torch.device(DEVICE))), 'ble_plan_sample_u8')
  torch.cuda.synchronize()
  return plans.cpu().numpy()


def _gpu_select(ret, plans, iteration, elite, segment, best_return=None, best_plan=None, counter=None):
  H, n, K = plans.shape
  S = -(-H // segment)
  ret_t, plans_t = _dev(np.asarray(ret, np.float32)), _dev(plans)
  br = _dev(np.full(n, 123.0, np.float32) if best_return is None else np.asarray(best_return, np.float32))
  bp = _dev(np.full((H, n), 7, np.uint8) if best_plan is None else best_plan)
  bk = torch.full((n,), 77, dtype=torch.int32, device=DEVICE)
  act = torch.full((n,), 9, dtype=torch.uint8, device=DEVICE)
  counts = torch.full((n, S, 3), -1, dtype=torch.int16, device=DEVICE)
  sel = _abi.BlePlanSelect(n, K, H, segment, iteration, elite, 0, ret_t.data_ptr(), plans_t.data_ptr(), br.data_ptr(), bk.data_ptr(),
                           bp.data_ptr(), act.data_ptr(), counts.data_ptr(), dev.ptr(counter))
  _lib.check(_lib.lib().ble_plan_select_f32(ctypes.byref(sel), dev.stream_ptr(torch.device(DEVICE))), 'ble_plan_select_f32')
  torch.cuda.synchronize()
  return (br.cpu().numpy(), bk.cpu().numpy(), bp.cpu().numpy(), act.cpu().numpy(),
          counts.cpu().numpy().view(np.uint16) if elite >= 1 else None)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_selection(got, want, what):
  assert np.array_equal(_bits(got[0]), _bits(want[0])), what
  for g, w, name in zip(got[1:4], want[1:4], ('best_k', 'best_plan', 'action')):
    assert np.array_equal(g, w), (what, name)
  assert (got[4] is None) == (want[4] is None) and (got[4] is None or np.array_equal(got[4], want[4])), (what, 'elite_counts')


# ---------------------------------------------------------------------------------------------- 1, 2: the sampler
@pytest.mark.parametrize('K', [1, 3, 5, 64, 67, 130])
def test_sampler_against_the_twin(K):
  rng = np.random.default_rng(K)
  for n, H, segment, env_offset in ((65, 7, 3, 0), (3, 1, 1, 1000), (130, 7, 1, 2 ** 33), (1, 1, 3, 5)):
    S = -(-H // segment)
    prev = rng.integers(0, 3, (H, n)).astype(np.uint8)
    decision = int(rng.integers(0, 2 ** 40))
    got = _gpu_sample(n, K, H, segment, 0, decision, seed=17, env_offset=env_offset, best_plan=prev)
    assert np.array_equal(got, plan_host.sample(n, K, H, segment, 0, decision, seed=17, env_offset=env_offset, best_plan=prev)), (n, H, segment)
    counts = rng.integers(0, 9, (n, S, 3)).astype(np.uint16)
    got = _gpu_sample(n, K, H, segment, 1, decision, seed=17, env_offset=env_offset, counts=counts, best_plan=prev)
    assert np.array_equal(got, plan_host.sample(n, K, H, segment, 1, decision, seed=17, env_offset=env_offset, counts=counts)), (n, H, segment)
    seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    got = _gpu_sample(n, K, H, segment, 1, decision, env_seed=seeds, counts=counts, best_plan=prev)
    assert np.array_equal(got, plan_host.sample(n, K, H, segment, 1, decision, env_seed=seeds, counts=counts)), (n, H, segment)


def test_sampler_batch_invariance():
  rng = np.random.default_rng(2)
  n, H, segment = 65, 7, 3
  seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64)
  prev = rng.integers(0, 3, (H, n)).astype(np.uint8)
  counts = rng.integers(0, 9, (n, 3, 3)).astype(np.uint16)
  for iteration in (0, 1):
    batch = _gpu_sample(n, 67, H, segment, iteration, 4, env_seed=seeds, counts=counts, best_plan=prev)
    for e in (0, 17, 64):
      alone = _gpu_sample(1, 67, H, segment, iteration, 4, env_seed=seeds[e:e + 1], counts=counts[e:e + 1], best_plan=prev[:, e:e + 1])
      assert np.array_equal(alone[:, 0], batch[:, e]), (iteration, e)
    few = _gpu_sample(n, 5, H, segment, iteration, 4, env_seed=seeds, counts=counts, best_plan=prev)
    assert np.array_equal(few, batch[:, :, :5]), iteration
  # one seed for the batch: environment e of a shard at env_offset is environment env_offset + e of the whole
  whole = _gpu_sample(n, 5, H, segment, 0, 9, seed=3)
  assert np.array_equal(_gpu_sample(3, 5, H, segment, 0, 9, seed=3, env_offset=40), whole[:, 40:43])


# ---------------------------------------------------------------------------------------------- 3: the selection
def _crafted(K, rng):
  base = rng.integers(0, 6, K).astype(np.float32) * np.float32(0.25)             # many exact ties
  rows = [base.copy(), np.zeros(K, np.float32),                                   # (all 0: an environment that is not OK)
          np.full(K, np.nan, np.float32), np.full(K, np.inf, np.float32), rng.standard_normal(K).astype(np.float32)]
  r = base.copy(); r[::3] = np.nan; rows.append(r)
  r = base.copy(); r[0] = np.inf; r[-1] = -np.inf; rows.append(r)
  r = base.copy(); r[K // 2] = np.float32(7.0); rows.append(r)
  r = base.copy(); r[-1] = np.float32(7.0); rows.append(r)                        # the best plan is the last one
  r = np.zeros(K, np.float32); r[::2] = np.float32(-0.0); rows.append(r)
  r = -base - np.float32(1.0); r[-1] = np.nan; rows.append(r)
  return np.stack(rows)


@pytest.mark.parametrize('K', [1, 63, 64, 65, 130, 1024])
def test_select_against_the_twin(K):
  rng = np.random.default_rng(K)
  H, segment = 7, 3
  ret = _crafted(K, rng)
  n = len(ret)
  plans = rng.integers(0, 3, (H, n, K)).astype(np.uint8)
  plans[:, :, 0] = 1                                                              # slot 0 is STAY, as the sampler leaves it
  for elite in sorted({0, 1, min(8, K), K}):
    got = _gpu_select(ret, plans, 0, elite, segment)
    _same_selection(got, plan_host.select(ret, plans, 0, elite, segment), (K, elite, 0))
    assert got[3][1] == 1 and got[1][1] == 0            # all returns 0: k = 0, STAY
    assert got[3][2] == 1 and got[1][2] == -1           # all NaN: STAY
    top = np.array([np.float32(r[np.isfinite(r)].max()) if np.isfinite(r).any() else np.float32(0.0) for r in ret])
    for name, inc in (('below', np.nextafter(top, np.float32(-np.inf))), ('equal', top), ('above', np.nextafter(top, np.float32(np.inf))),
                      ('nan', np.full(n, np.nan, np.float32))):
      prev = rng.integers(0, 3, (H, n)).astype(np.uint8)
      got = _gpu_select(ret, plans, 1, elite, segment, best_return=inc, best_plan=prev)
      _same_selection(got, plan_host.select(ret, plans, 1, elite, segment, best_return=inc, best_plan=prev), (K, elite, name))
      if name == 'equal':
        assert (got[1] == -1).all() and np.array_equal(got[2], prev)             # a tie keeps the incumbent


def test_select_advances_the_counter_once():
  counter = _dev(np.array([2 ** 32 - 1], np.int64))
  ret = np.zeros((130, 5), np.float32)
  _gpu_select(ret, np.ones((3, 130, 5), np.uint8), 0, 0, 1, counter=counter)
  assert int(counter.item()) == 2 ** 32


# ---------------------------------------------------------------------------------------------- the agent
def _env(n, seed=3, wind_noise=True, steps=3):
  env = balloon_env.VecBalloonEnv(n, seed=seed, wind_noise=wind_noise, auto_reset=False)
  env.reset()
  rng = np.random.default_rng(seed)
  for a in rng.integers(0, 3, (steps, n)).astype(np.uint8):
    env.step(_dev(a))
  return env


def _compose(env, agent, decision, prev_plan):
  """One decision as the composition of the twin and env.lookahead: (best_return, best_k, best_plan, action)."""
  n, K, H = env.num_envs, agent.num_plans, agent.horizon
  best_return, best_plan, counts = None, None, None
  for it in range(agent.iterations):
    plans = plan_host.sample(n, K, H, agent.segment, it, decision, seed=agent.seed, counts=counts, best_plan=prev_plan)
    ret = env.lookahead(_dev(plans), gamma=agent.gamma, action_repeat=agent.action_repeat, wind=agent.wind).returns
    torch.cuda.synchronize()
    last = it + 1 == agent.iterations
    best_return, best_k, best_plan, action, counts = plan_host.select(ret.cpu().numpy(), plans, it, 0 if last else agent.elite, agent.segment,
                                                                      best_return=best_return, best_plan=best_plan)
  return best_return, best_k, best_plan, action


@pytest.mark.parametrize('wind', ['forecast', 'belief', 'truth'])
def test_act_equals_the_composition(wind):
  n = 65
  env = _env(n)
  env.arena.sim.state['status'][2] = 2                       # one environment is not OK: it flies nothing and gets STAY
  agent = env.planner(num_plans=67, horizon=7, segment=3, action_repeat=2, wind=wind, iterations=2, elite=8, seed=5)
  prev = np.full((7, n), 1, np.uint8)
  rng = np.random.default_rng(1)
  for decision in range(3):
    action = agent.act(None).clone()
    torch.cuda.synchronize()
    got = (agent.best_return.cpu().numpy(), agent.best_k.cpu().numpy(), agent.best_plan.cpu().numpy(), action.cpu().numpy(), None)
    want = _compose(env, agent, decision, prev) + (None,)
    _same_selection(got, want, (wind, decision))
    assert int(agent.counter.item()) == decision + 1
    assert got[3][2] == 1 and got[0][2] == 0.0
    assert np.isfinite(got[0]).all()
    print(wind, decision, 'actions', np.bincount(got[3], minlength=3), 'best_k >= 0:', int((got[1] >= 0).sum()))
    prev = got[2]
    # (a step that is not the agent's choice everywhere: the warm start must follow the agent's plan, not the flight)
    env.step(_dev(np.where(rng.random(n) < 0.5, got[3], 1).astype(np.uint8)))
  env.check_errors()


@pytest.mark.parametrize('n', [3, 130])
def test_the_chosen_plan_is_real(n):
  env = _env(n, seed=8)
  H = 8
  agent = env.planner(num_plans=16, horizon=H, segment=2, wind='truth', iterations=1, seed=n)
  agent.act(None)
  best_plan, best_return = (t.clone() for t in agent.plan())
  returns = agent.returns.clone()
  rewards = torch.stack([env.step(best_plan[h].contiguous())[1] for h in range(H)]).cpu().numpy()
  acc, disc = np.zeros(n, np.float64), 1.0
  for t in range(H):                                     # the kernel's order: the product and the sum rounded separately
    term = disc * rewards[t].astype(np.float64)
    acc += term
    disc *= agent.gamma
  print('best_return', best_return.cpu().numpy()[:8], 'flown', acc.astype(np.float32)[:8])
  assert np.array_equal(_bits(acc.astype(np.float32)), _bits(best_return.cpu().numpy()))
  assert bool((best_return[:, None] >= returns[:, :3]).all())
  env.check_errors()


def test_elitism():
  n = 65
  env = _env(n, seed=4)
  one = env.planner(num_plans=16, horizon=8, segment=2, iterations=1, seed=6)
  two = env.planner(num_plans=16, horizon=8, segment=2, iterations=2, elite=4, seed=6)
  one.act(None); two.act(None)
  torch.cuda.synchronize()
  r1, r2, k2 = one.best_return.cpu().numpy(), two.best_return.cpu().numpy(), two.best_k.cpu().numpy()
  print('environments the second iteration improved:', int((k2 >= 0).sum()), 'of', n)
  assert (r2 >= r1).all()
  assert np.array_equal(_bits(r2[k2 == -1]), _bits(r1[k2 == -1]))
  assert np.array_equal(two.best_plan.cpu().numpy()[:, k2 == -1], one.best_plan.cpu().numpy()[:, k2 == -1])


def _tensors(d, prefix=''):
  for key, v in d.items():
    if isinstance(v, torch.Tensor):
      yield prefix + str(key), v
    elif isinstance(v, dict):
      yield from _tensors(v, prefix + str(key) + '.')


def test_act_writes_nothing_of_the_environment():
  env = _env(65, seed=5)
  sim = env.arena.sim
  for wind in lookahead_agent.WINDS:
    agent = env.planner(num_plans=5, horizon=4, wind=wind, iterations=2)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _tensors(env.state_dict())}
    flags = int(sim.err_flags.item())
    agent.act(None)
    torch.cuda.synchronize()
    after = dict(_tensors(env.state_dict()))
    assert sorted(before) == sorted(after) and 'arena.sim.state.x' in before, sorted(before)[:5]
    for name in before:
      assert torch.equal(before[name], after[name]), (wind, name)
    assert int(sim.err_flags.item()) == flags


def test_graph_equals_eager():
  n, decisions = 65, 6
  runs = {}
  for mode in ('eager', 'graph'):
    env = _env(n, seed=9)
    agent = env.planner(num_plans=8, horizon=4, segment=2, iterations=2, elite=3, seed=2)
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
      log.append((actions.cpu().numpy().copy(), _bits(agent.best_return.cpu().numpy()).copy(), int(agent.counter.item()), obs.cpu().numpy().copy()))
    runs[mode] = log
    env.check_errors()
  for d, (a, b) in enumerate(zip(runs['eager'], runs['graph'])):
    assert a[2] == b[2] == d + 2
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), d


def test_evaluator_flies_the_agent_seed_by_seed():
  suite = suites.EvaluationSuite([11, 12, 13], 6)
  make = lambda: lookahead_agent.VecLookaheadAgent(num_plans=8, horizon=4, wind='belief')
  batch = eval_lib.eval_agent_vec(make(), suite)
  alone = eval_lib.eval_agent_vec(make(), suite, batch_size=1)
  eager = eval_lib.eval_agent_vec(make(), suite, capture_graph=False)
  for a, b, c in zip(batch, alone, eager):
    assert dataclasses.asdict(a) == dataclasses.asdict(b) == dataclasses.asdict(c), (a, b, c)
  assert [r.seed for r in batch] == [11, 12, 13]
  assert make().get_name() == 'LookaheadAgent'


def test_refusals():
  with pytest.raises(ValueError, match='1024'):
    lookahead_agent.VecLookaheadAgent(num_plans=1025)
  with pytest.raises(ValueError, match='960'):
    lookahead_agent.VecLookaheadAgent(horizon=481, action_repeat=2)
  with pytest.raises(ValueError, match='wind'):
    lookahead_agent.VecLookaheadAgent(wind='gp')
  with pytest.raises(ValueError, match='bind'):
    lookahead_agent.VecLookaheadAgent().act(None)
  env = _env(3, steps=0)
  seeds = torch.zeros(3, dtype=torch.int64, device=DEVICE)
  with pytest.raises(ValueError, match='truth'):
    lookahead_agent.VecLookaheadAgent(wind='truth').bind(env.arena.sim, seeds=seeds)
  fleet = balloon_env.VecBalloonEnv(3, seed=1, vehicles=[{}, {'envelope_mass': 75.0}], vehicle_index=[0, 1, 0], auto_reset=False)
  with pytest.raises(ValueError, match='fleet'):
    fleet.planner()
  # state_dict round trip: the counter and the warm start
  agent = env.planner(num_plans=5, horizon=4)
  agent.act(None)
  saved = agent.state_dict()
  first = agent.act(None).clone()
  agent.load_state_dict(saved)
  assert torch.equal(agent.act(None), first) and int(agent.counter.item()) == 2


# ---------------------------------------------------------------------------------------------- what the four planners share
SHELL_CASES = {
    'sampler': dict(search='sample', num_plans=5, horizon=4, iterations=2),
    'sampler in scenarios': dict(search='sample', num_plans=5, horizon=4, iterations=2, wind='scenarios', num_scenarios=2),
    'beam': dict(search='beam', beam_width=2, depth=2),
    'scenario beam': dict(search='beam', beam_width=2, depth=2, wind='scenarios', num_scenarios=2),
    'guided search': dict(search='mcts', num_rounds=2, leaves_per_round=1, max_depth=2),
}


@pytest.mark.parametrize('case', list(SHELL_CASES))
def test_the_planner_shell(case):
  """What VecPlanner owns, held for every planner at a batch of 3 with one environment that is not OK: __call__ is act, out= is
  returned and holds the same bytes, a second bind of the same simulator (and seeds) allocates nothing, wind='truth' refuses a seed
  per environment, and the fleet refusal names the class."""
  kw = dict(SHELL_CASES[case], segment=2, action_repeat=1)
  n = 3
  env = _env(n)
  sim = env.arena.sim
  sim.state['status'][1] = 2                                 # not OK: the frozen path
  obs = sim.observe(append=False)
  agent = env.planner(**kw)
  cls = type(agent)
  noise_seed = lambda: env.arena._seed
  seeded = 'scenarios' in kw.get('wind', '') or kw['search'] == 'sample'       # the agents whose streams bind(seeds=) keys
  seeds = torch.arange(n, dtype=torch.int64, device=DEVICE)
  for s in (None, seeds):
    rebind = lambda: agent.bind(sim, seeds=s, noise_seed=noise_seed)           # (the sampler's run restarts: counter 0 every time)
    called = rebind()(obs).clone()
    acted = rebind().act(obs).clone()
    buf = torch.full((n,), 7, dtype=torch.uint8, device=DEVICE)
    assert rebind().act(obs, out=buf) is buf
    torch.cuda.synchronize()
    print(case, 'seeds' if s is not None else 'no seeds', 'actions', called.cpu().numpy())
    assert called.cpu().numpy().tobytes() == acted.cpu().numpy().tobytes() == buf.cpu().numpy().tobytes()
    assert int(called[1]) == 1                               # STAY where nothing is flown
    held = [agent.action] + [w.slab for w in (agent._belief, agent._scenarios) if w is not None]
    assert len(held) == 2                                    # every case here fits a belief or scenarios
    before = [t.data_ptr() for t in held]
    rebind()
    after = [agent.action] + [w.slab for w in (agent._belief, agent._scenarios) if w is not None]
    assert [t.data_ptr() for t in after] == before and all(a is b for a, b in zip(after, held))
  if not seeded:                                             # seeds that key nothing are no new binding either
    agent.bind(sim, noise_seed=noise_seed)
    assert agent.action.data_ptr() == before[0]
  env.check_errors()
  shape = {k: v for k, v in kw.items() if k not in ('search', 'wind', 'num_scenarios')}
  if 'truth' in cls.WINDS:
    with pytest.raises(ValueError, match='truth'):
      cls(wind='truth', **shape).bind(sim, seeds=seeds)
  fleet = balloon_env.VecBalloonEnv(n, seed=1, vehicles=[{}, {'envelope_mass': 75.0}], vehicle_index=[0, 1, 0], auto_reset=False)
  with pytest.raises(ValueError, match=cls.__name__ + r': a fleet \(set_fleet\) has no look-ahead kernel'):
    fleet.planner(**kw)
