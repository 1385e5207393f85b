"""A learned terminal value for the planner: ble_rollout_leaves_f32, ble_observe_leaves_f32 and ble_plan_bootstrap_f32
through VecSimulator.leaf_arena / rollout_plans(leaves=) / observe_leaves and VecLookaheadAgent(leaf_value=), on the device.

Leaf states.  The reference of a leaf is a copy of its environment stepped with its plan's actions by the transition kernel itself:
plan by plan the source's state_dict() is loaded into a second VecSimulator of the same n and env_offset and flown -- step_n in the
forecast and in the noise (whose streams are keyed by the environment's index, which is why the copies keep theirs, as in
test_gpu_rollout.py), belief_wind at the copy's state + step(noise_uv=that) in the belief.  Every array of the leaf arena must equal
the copy's BIT FOR BIT, last_command and the safety layers' words included.

Leaf observations.  The reference is ble_observe_f32 itself: a simulator of n K environments in the arena's state, with the parent's
ring repeated K times, observed with append=False and no carried factor; bit for bit on every live leaf.  And the feature oracle, which
is fed the parent's recorded rows and then the leaf's row, within test_gpu_observe.py's own rule (1e-5 on every entry, the pattern of
unreachable levels and the discrete features exact), unwidened and with no leaf excluded.

The bootstrap and the agent are held to the NumPy twins (leaves_host.py, plan_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import leaves_host
import plan_host
from balloon_learning_environment_amd import _abi, _lib, device as dev, vec_state
from balloon_learning_environment_amd.agents import actor_critic, lookahead_agent, qnet
from balloon_learning_environment_amd.env import balloon_env
from test_gpu_observe import check as check_features

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
SHAPES = [(1, 1), (3, 5), (4, 64), (1, 257), (257, 1)]          # (n, K); the last two cross the step workgroup of 256 lanes
H, SEGMENT = 6, 2
NOISE_SEED = 19


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _parent(n, seed, steps=8, per_env=False, carry=True, record=None):
  """A simulator `steps` agent steps into its episodes that has observed after every one of them, with a random measured-minus-forecast
  term: (sim, rng, field).  record: a list that receives (state dict, noise) after every observation."""
  rng = np.random.default_rng(seed)
  sim = vec_state.VecSimulator(n, DEVICE)
  field = rng.uniform(-12.0, 12.0, ((n,) if per_env else ()) + vec_state.GRID_SHAPE).astype(np.float32)
  sim.set_grid(field, per_env=per_env)
  sim.reset_device(seed)
  for _ in range(steps):
    sim.step(_dev(rng.integers(0, 3, n).astype(np.uint8)))
    noise = (rng.standard_normal((n, 2)) * 1.5).astype(np.float32)
    sim.observe(_dev(noise), carry_factor=carry)
    if record is not None:
      record.append((sim.get_state(), noise))
  sim.check_errors()
  return sim, rng, field


def _tensors(d, prefix=''):
  for key, v in d.items():
    if isinstance(v, torch.Tensor):
      yield prefix + str(key), v
    elif isinstance(v, dict):
      yield from _tensors(v, prefix + str(key) + '.')


def _snapshot(sim):
  """Everything of a simulator a look-ahead must leave alone: state, episode counters, grid, flags, the WindGP history (ring, carried
  factor, counts, pending restarts) and the per-episode cache, as clones."""
  torch.cuda.synchronize()
  snap = {k: v.clone() for k, v in _tensors(sim.state_dict())}
  snap['episode_cache'] = sim.episode_cache.clone()
  return snap


def _assert_untouched(sim, before, what):
  after = _snapshot(sim)
  assert sorted(before) == sorted(after)
  for name in before:
    a, b = before[name], after[name]
    assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (what, name)


# ------------------------------------------------------------------------------------------------ 1: the leaves are a stepped copy's state
def _stepped_copies(src, plans, repeat, wind, belief):
  """{field: tensor [n, K]} of the copies' states after their plans, flown plan by plan in a simulator of the source's n and offset."""
  h, n, k_plans = plans.shape
  sd = src.state_dict()
  ref = vec_state.VecSimulator(n, DEVICE, env_offset=src.env_offset)
  out = {name: torch.empty(n, k_plans, dtype=t.dtype, device=src.device) for name, t in src.state.items()}
  for k in range(k_plans):
    ref.load_state_dict(sd)
    actions = _dev(np.repeat(plans[:, :, k], repeat, axis=0))
    if wind == 'belief':
      for a in actions:
        ref.step(a.contiguous(), noise_uv=ref.belief_wind(belief))
    else:
      r, t = torch.zeros(actions.shape, device=DEVICE), torch.zeros(actions.shape, dtype=torch.uint8, device=DEVICE)
      ref.step_n(actions, r, t, noise_seed=NOISE_SEED if wind == 'noise' else None)
    for name in out:
      out[name][:, k] = ref.state[name]
  ref.err_flags.zero_()
  return out


@pytest.mark.parametrize('repeat', [1, 3])
@pytest.mark.parametrize('wind', ['forecast', 'noise', 'belief'])
@pytest.mark.parametrize('n, k', SHAPES)
def test_leaf_states_are_a_stepped_copys_state(n, k, wind, repeat):
  src, rng, _ = _parent(n, 1000 + 10 * n + k)
  # a plan that goes terminal: the night load drains 23 Wh inside the second agent step (test_gpu_rollout.py); a source that is not OK
  night = (src.state['solar_charging'] == 0) & (src.state['status'] == 0)
  src.state['battery_charge'][night] = 23.0
  dead = 1 if n >= 3 else None
  if dead is not None:
    src.state['status'][dead] = 2
    src.state['last_command'][dead] = 2
  plans = rng.integers(0, 3, (H, n, k)).astype(np.uint8)
  belief = src.fit_wind_belief() if wind == 'belief' else None
  kw = dict(gamma=0.993, action_repeat=repeat, noise_seed=NOISE_SEED if wind == 'noise' else None, belief=belief, want_rewards=True,
            want_final=True)
  before = _snapshot(src)
  plain = src.rollout_plans(_dev(plans), **kw)
  arena = src.leaf_arena(k)
  for t in arena.state.values():          # (nothing of the arena is what the call should write)
    t.fill_(77)
  got = src.rollout_plans(_dev(plans), leaves=arena, **kw)
  assert got.leaves is arena and plain.leaves is None and len(got) == 4
  _assert_untouched(src, before, 'the source')
  for name, a, b in zip(got._fields, got, plain):          # ret, steps_flown, reward, final_state: the non-leaf entry's bits
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
  want = _stepped_copies(src, plans, repeat, wind, belief)
  torch.cuda.synchronize()
  for name in _abi.FIELD_NAMES:
    a, b = arena.state[name].view(n, k), want[name]
    assert a.dtype == b.dtype
    bad = torch.nonzero(a.view(torch.uint8) != b.contiguous().view(torch.uint8))
    assert bad.numel() == 0, (name, bad[:4].tolist())
  flown = got.steps_flown.cpu().numpy()
  status = arena.state['status'].view(n, k).cpu().numpy()
  assert np.all(status[flown < H * repeat] != 0)          # a plan that stopped early left a terminal leaf
  print(f'n {n} K {k} {wind} x{repeat}: plans that went terminal {int(((flown > 0) & (flown < H * repeat)).sum())}, dead sources '
        f'{int((flown == 0).all(1).sum())}, of {n * k}')
  if dead is not None:
    assert np.all(flown[dead] == 0) and np.all(status[dead] == 2)
    assert np.all(arena.state['last_command'].view(n, k)[dead].cpu().numpy() == 2)          # the source's own: it flew nothing
  if n >= 257:
    assert np.any((flown > 0) & (flown < H * repeat)), 'no plan went terminal'
  # the arena is a state like any other: the look-ahead flies from it
  again = arena.rollout_plans(torch.ones(1, n * k, 1, dtype=torch.uint8, device=DEVICE))
  torch.cuda.synchronize()
  assert np.array_equal(again.steps_flown.cpu().numpy()[:, 0] == 1, status.reshape(-1) == 0)


VEHICLE = {'payload_mass': 95.0, 'battery_capacity_wh': 2800.0}          # test_gpu_rollout.py's run-time vehicle
RT_NIGHT, RT_DEAD = 0, 4


def _five_with_a_vehicle(seed=77):
  """Five environments that fly a run-time vehicle (the VehicleRt instantiations), picked with their rings from a batch of 64:
  environment RT_NIGHT flies in the dark on a battery of 23 Wh, which the night load of 183.7 W drains in 45 strides of 10 s, inside the
  third agent step; three fly in daylight; environment RT_DEAD is not OK.  (sim, rng)"""
  big, rng, field = _parent(64, seed, steps=4)
  night = torch.nonzero((big.state['solar_charging'] == 0) & (big.state['status'] == 0)).view(-1)
  day = torch.nonzero((big.state['solar_charging'] > 0) & (big.state['status'] == 0)).view(-1)
  assert night.numel() >= 1 and day.numel() >= 4, (night.numel(), day.numel())
  pick = torch.cat([night[:1], day[:4]])
  src = vec_state.VecSimulator(5, DEVICE)
  for name, t in src.state.items():
    t.copy_(big.state[name][pick])
  src.set_grid(field)
  src.set_vehicle(**VEHICLE)
  src._allocate_history(True)
  for name, t in src._gp.items():
    t.copy_(big._gp[name][pick])
  src._obs_reset.copy_(big._obs_reset[pick])
  src.state['battery_charge'][RT_NIGHT] = 23.0
  src.state['status'][RT_DEAD] = 2
  src.state['last_command'][RT_DEAD] = 2
  return src, rng


@pytest.mark.parametrize('wind', ['forecast', 'noise', 'belief'])
def test_leaf_states_with_a_runtime_vehicle_are_a_stepped_copys_state(wind):
  """The leaf rollouts' VehicleRt instantiations, 15 lanes: every array of the arena against copies stepped with the same vehicle."""
  n, k, h, repeat = 5, 3, 2, 2                     # four agent steps: the night environment ends inside them
  src, rng = _five_with_a_vehicle()
  plans = rng.integers(0, 3, (h, n, k)).astype(np.uint8)
  belief = src.fit_wind_belief() if wind == 'belief' else None
  kw = dict(gamma=0.993, action_repeat=repeat, noise_seed=NOISE_SEED if wind == 'noise' else None, belief=belief, want_rewards=True,
            want_final=True)
  before = _snapshot(src)
  plain = src.rollout_plans(_dev(plans), **kw)
  arena = src.leaf_arena(k)
  for t in arena.state.values():
    t.fill_(77)
  got = src.rollout_plans(_dev(plans), leaves=arena, **kw)
  _assert_untouched(src, before, 'the source')
  for name, a, b in zip(got._fields, got, plain):          # ret, steps_flown, reward, final_state: the non-leaf entry's bits
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
  want = _stepped_copies(src, plans, repeat, wind, belief)
  torch.cuda.synchronize()
  for name in _abi.FIELD_NAMES:
    a, b = arena.state[name].view(n, k), want[name]
    assert a.dtype == b.dtype
    bad = torch.nonzero(a.view(torch.uint8) != b.contiguous().view(torch.uint8))
    assert bad.numel() == 0, (wind, name, bad[:4].tolist())
  flown = got.steps_flown.cpu().numpy()
  status = arena.state['status'].view(n, k).cpu().numpy()
  assert np.all(flown[RT_DEAD] == 0) and np.all(status[RT_DEAD] == 2)
  assert np.all((flown[RT_NIGHT] > 0) & (flown[RT_NIGHT] < h * repeat)) and np.all(status[RT_NIGHT] != 0)          # out of power inside the plan
  live = [e for e in range(n) if e not in (RT_NIGHT, RT_DEAD)]
  assert np.all(flown[live] == h * repeat) and np.all(status[live] == 0)
  # the vehicle is really flown: the default vehicle's leaves are other leaves
  src.set_vehicle()
  default_arena = src.leaf_arena(k)
  src.rollout_plans(_dev(plans), leaves=default_arena, **kw)
  assert not torch.equal(default_arena.state['pressure'].view(n, k)[live], arena.state['pressure'].view(n, k)[live])


def test_leaves_refusals():
  src, rng, _ = _parent(3, 5, steps=2)
  plans = torch.ones(H, 3, 5, dtype=torch.uint8, device=DEVICE)
  arena = src.leaf_arena(5)
  scn = src.fit_wind_scenarios(2, seed=1)
  with pytest.raises(ValueError, match='scenario'):
    src.rollout_plans(plans, scenarios=scn, leaves=arena)
  with pytest.raises(ValueError, match='leaf arena'):
    src.rollout_plans(plans, leaves=src.leaf_arena(4))
  with pytest.raises(ValueError, match='leaf arena'):
    src.rollout_plans(plans, leaves=vec_state.VecSimulator(15, DEVICE))
  other, _, _ = _parent(3, 6, steps=1)
  with pytest.raises(ValueError, match='leaf arena'):
    other.observe_leaves(arena)
  env = balloon_env.VecBalloonEnv(3, seed=2, auto_reset=False)
  env.reset()
  ro = env.lookahead(plans, wind='forecast', want_leaves=True)
  assert ro.leaves is not None and ro.leaves.n == 15 and env.lookahead(plans, wind='forecast').leaves is None
  assert env.lookahead(plans, wind='belief', want_leaves=True).leaves is ro.leaves          # kept per K
  with pytest.raises(ValueError, match='scenarios'):
    env.lookahead(plans, wind='scenarios', want_leaves=True)


# ------------------------------------------------------------------------------------------------ 2: the leaves' observation
def _observe_twin(parent, arena, k):
  """ble_observe_f32 (append=False, refit) on a simulator of n K environments in the arena's state with the parent's ring, K times."""
  twin = vec_state.VecSimulator(arena.n, DEVICE)
  for name, t in twin.state.items():
    t.copy_(arena.state[name])
  twin.set_vehicle(**parent.vehicle)
  per_env = parent.grid_env_stride != 0
  twin.set_grid(parent.grid.repeat_interleave(k, 0) if per_env else parent.grid, per_env=per_env)
  twin._allocate_history(False)
  for name, t in twin._gp.items():
    t.copy_(parent._gp[name].repeat_interleave(k, 0))
  twin._obs_reset.copy_(parent._obs_reset.repeat_interleave(k, 0))
  return twin.observe(append=False, carry_factor=False)


def _observe_case(n, k, steps, h=H, repeat=1, per_env=False):
  parent, rng, _ = _parent(n, 2000 + 10 * n + k + steps, steps=steps, per_env=per_env)
  assert 'chol' in parent._gp and int(parent._gp['n_chol'].min().item()) > 0          # a parent that carries a factor
  assert int(parent._gp['count'].max().item()) == steps
  if n >= 3:
    mask = torch.zeros(n, dtype=torch.uint8, device=DEVICE)
    mask[2] = 1
    parent.reset_observation_history(mask)          # a pending restart: an empty history for that parent's leaves
    parent._gp['count'][1] = 0                      # ... and a parent whose ring holds nothing
  plans = rng.integers(0, 3, (h, n, k)).astype(np.uint8)
  arena = parent.leaf_arena(k)
  parent.rollout_plans(_dev(plans), gamma=0.993, action_repeat=repeat, leaves=arena)
  if n * k > 1:
    arena.state['status'][::7] = 2                  # dead leaves, whatever else they hold
  before = _snapshot(parent)
  flags = int(parent.err_flags.item())
  obs = torch.full((n * k, _lib.OBS_DIM), float('nan'), device=DEVICE)
  assert parent.observe_leaves(arena, out=obs) is obs
  _assert_untouched(parent, before, 'the parent')          # ring, chol, n_chol, count, pending restarts: byte for byte
  assert int(parent.err_flags.item()) == flags
  want = _observe_twin(parent, arena, k)
  torch.cuda.synchronize()
  live = (arena.state['status'] == 0).cpu().numpy()
  got, want = obs.cpu().numpy(), want.cpu().numpy()
  assert live.any() and (n * k == 1 or not live[0])
  assert np.all(_bits(got[~live]) == 0), 'a dead leaf: +0.0f in all 1099 entries'
  bad = np.argwhere(_bits(got[live]) != _bits(want[live]))
  assert bad.size == 0, bad[:4].tolist()
  assert np.isfinite(got).all()
  return parent, arena, got, live


@pytest.mark.parametrize('steps', [8, 130])          # 130 fills the ring of 128 and wraps it
@pytest.mark.parametrize('n, k', SHAPES)
def test_leaf_observation_equals_observe(n, k, steps):
  _observe_case(n, k, steps)


def test_leaf_observation_with_the_whole_ring_outside_the_window():
  """121 agent steps ahead (H = 11, action_repeat = 11): 6 h 3 min after the parent's newest observation."""
  parent, arena, got, live = _observe_case(3, 5, 8, h=11, repeat=11)
  ahead = arena.state['time_elapsed_s'].view(3, 5) - parent.state['time_elapsed_s'][:, None]
  full = (ahead == 121 * 180).cpu().numpy().reshape(-1) & live
  assert full.any()
  assert full[:5].any()          # (parent 0: a ring of 8 observations, none pending)
  # no observation in the window: the deviation feature (16, 19, ...) is 0 at every level (wind_gp.py:166-168), as with no history
  assert np.all(got[full][:, 16::3] == 0.0)
  near = parent.observe_leaves(parent.rollout_plans(_dev(np.ones((1, 3, 5), np.uint8)), leaves=arena).leaves).cpu().numpy()
  assert np.any(near[:5, 16::3] != 0.0)          # ... and one step ahead the same parent's window is not empty


def test_leaf_observation_with_per_environment_grids():
  parent, arena, got, live = _observe_case(3, 5, 8, per_env=True)
  assert parent.grid_env_stride != 0 and arena.grid is None


def test_leaf_observation_equals_the_oracle():
  import features_oracle
  n, k = 3, 5
  record = []
  parent, rng, field = _parent(n, 4242, steps=8, record=record)
  plans = rng.integers(0, 3, (H, n, k)).astype(np.uint8)
  arena = parent.leaf_arena(k)
  parent.rollout_plans(_dev(plans), gamma=0.993, leaves=arena)
  obs = parent.observe_leaves(arena).cpu().numpy()
  assert int(parent.rollout_flags.item()) == 0
  leaf = arena.get_state()

  def row_of(state, j):
    row = {f: float(state[f][j]) for f in helpers.STATE_FLOATS}
    for f in ('center_lat_deg', 'center_lng_deg', 'upwelling_infrared', 'alpha'):
      row[f] = float(state[f][j])
    for f in ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s', 'start_unix'):
      row[f] = int(state[f][j])
    return row
  compared, worst = 0, 0.0
  for e in range(n):
    fo = features_oracle.FeatureOracle(field, float(record[0][0]['alpha'][e]))
    for state, noise in record:
      fo.observe(row_of(state, e), noise[e].astype(np.float64))
    for p in range(k):
      j = e * k + p
      if leaf['status'][j] != 0:
        continue
      fo.row = row_of(leaf, j)          # the balloon arrived here having measured nothing on the way
      err = check_features(obs[j], fo.features(), f'leaf {j} of parent {e}')
      compared, worst = compared + 1, max(worst, float(err.max()))
  print(f'leaf observation vs the oracle: {compared} of {n * k} leaves compared, none excluded, worst |diff| {worst:.3g}')
  assert compared >= n * k - 2


# ------------------------------------------------------------------------------------------------ 3: the bootstrap
def _gpu_bootstrap(ret, steps, status, value, gamma, alias):
  n, k = ret.shape
  ret_t, steps_t, status_t, value_t = _dev(ret), _dev(steps), _dev(status.reshape(-1)), _dev(value.reshape(-1))
  score = ret_t if alias else torch.full((n, k), 55.0, device=DEVICE)
  b = _abi.BlePlanBootstrap(n, k, 0, gamma, ret_t.data_ptr(), steps_t.data_ptr(), status_t.data_ptr(), value_t.data_ptr(), score.data_ptr())
  _lib.check(_lib.lib().ble_plan_bootstrap_f32(ctypes.byref(b), dev.stream_ptr(torch.device(DEVICE))), 'ble_plan_bootstrap_f32')
  torch.cuda.synchronize()
  return score.cpu().numpy()


@pytest.mark.parametrize('n', [1, 65])
@pytest.mark.parametrize('k', [1, 64, 65, 1024])
def test_bootstrap_against_the_twin(n, k):
  rng = np.random.default_rng(100 * n + k)
  special = np.array([0.0, -0.0, 1e-42, -1e-42, np.inf, -np.inf, np.nan, 3.5, -120.0], np.float32)
  total = n * k
  ret = (rng.standard_normal(total) * 30.0).astype(np.float32)
  steps = rng.choice(np.array([0, 1, 24, 960], np.int32), total)
  status = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), total)
  value = np.where(rng.random(total) < 0.6, rng.choice(special, total), (rng.standard_normal(total) * 80.0).astype(np.float32)).astype(np.float32)
  # every (steps, special value) pair on a live and on a dead leaf, as far as the batch reaches
  grid = [(s, v, st) for s in (0, 1, 24, 960) for v in special for st in (0, 2)]
  for i, (s, v, st) in enumerate(grid[:total]):
    steps[i], value[i], status[i] = s, v, st
  shape = (n, k)
  for gamma in (0.0, 0.993, 1.0):
    want = leaves_host.bootstrap(ret.reshape(shape), steps.reshape(shape), status.reshape(shape), value.reshape(shape), gamma)
    for alias in (False, True):
      got = _gpu_bootstrap(ret.reshape(shape).copy(), steps.reshape(shape), status, value, gamma, alias)
      bad = np.argwhere(_bits(got) != _bits(want))
      assert bad.size == 0, (gamma, alias, bad[:4].tolist())
  dead = status.reshape(shape) != 0
  assert np.array_equal(_bits(want[dead]), _bits(ret.reshape(shape)[dead]))          # whatever the value's bits


# ------------------------------------------------------------------------------------------------ 4: the agent
def _env(n, seed=3, steps=3):
  env = balloon_env.VecBalloonEnv(n, seed=seed, wind_noise=True, auto_reset=False)
  env.reset()
  rng = np.random.default_rng(seed)
  for a in rng.integers(0, 3, (steps, n)).astype(np.uint8):
    env.step(_dev(a))
  return env


def _critic(seed=1, deterministic=True):
  net = qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', seed=seed, num_layers=2, hidden_units=64), num_atoms=2)
  return actor_critic.VecActorCriticAgent(net, deterministic=deterministic)


def test_without_a_leaf_value_the_agent_is_todays():
  n = 5
  kw = dict(num_plans=8, horizon=H, segment=SEGMENT, iterations=2, elite=3, seed=4)
  envs = [_env(n, seed=6), _env(n, seed=6)]
  agents = [envs[0].planner(**kw), envs[1].planner(leaf_value=None, **kw)]
  assert agents[1].leaves is None
  for decision in range(5):
    acts = [a.act(None).clone() for a in agents]
    torch.cuda.synchronize()
    assert torch.equal(acts[0], acts[1]), decision
    assert torch.equal(agents[0].plans, agents[1].plans) and torch.equal(agents[0].best_plan, agents[1].best_plan), decision
    assert torch.equal(agents[0].best_return.view(torch.int32), agents[1].best_return.view(torch.int32)), decision
    for env, a in zip(envs, acts):
      env.step(a)


@pytest.mark.parametrize('iterations', [1, 2])
@pytest.mark.parametrize('wind', ['forecast', 'belief'])
def test_the_bootstrapped_agent_equals_the_twin_chain(wind, iterations):
  n, k = 4, 8
  env = _env(n, seed=7)
  sim = env.arena.sim
  critic = _critic()
  agent = env.planner(num_plans=k, horizon=H, segment=SEGMENT, wind=wind, iterations=iterations, elite=3, seed=9, action_values=True,
                      leaf_value=critic)
  prev = np.full((H, n), 1, np.uint8)
  values = torch.empty(n * k, device=DEVICE)
  moved = 0
  for decision in range(2):
    action = agent.act(None).clone()
    torch.cuda.synchronize()
    got_returns = agent.returns.cpu().numpy().copy()
    best_return, best_plan, counts = None, None, None
    for it in range(iterations):
      plans = plan_host.sample(n, k, H, SEGMENT, it, decision, seed=agent.seed, counts=counts, best_plan=prev)
      ro = env.lookahead(_dev(plans), gamma=agent.gamma, wind=wind, want_leaves=True)          # the plain returns and the leaves
      obs = sim.observe_leaves(ro.leaves)
      critic.act(obs, value=values)                                                              # the device's own values
      torch.cuda.synchronize()
      status = ro.leaves.state['status'].cpu().numpy()
      score = leaves_host.bootstrap(ro.returns.cpu().numpy(), ro.steps_flown.cpu().numpy(), status, values.cpu().numpy(), agent.gamma)
      moved += int((_bits(score) != _bits(ro.returns.cpu().numpy())).sum())
      last = it + 1 == iterations
      best_return, best_k, best_plan, want_action, counts = plan_host.select(score, plans, it, 0 if last else agent.elite, SEGMENT,
                                                                             best_return=best_return, best_plan=best_plan)
    assert np.array_equal(_bits(got_returns), _bits(score)), (decision, 'returns')
    assert np.array_equal(action.cpu().numpy(), want_action), (decision, 'action')
    assert np.array_equal(_bits(agent.best_return.cpu().numpy()), _bits(best_return)), (decision, 'best_return')
    assert np.array_equal(agent.best_plan.cpu().numpy(), best_plan), (decision, 'best_plan')
    q, _ = agent.action_values()
    q, a = q.cpu().numpy(), action.cpu().numpy()
    assert np.array_equal(_bits(q[np.arange(n), a]), _bits(agent.best_return.cpu().numpy())), decision
    prev = best_plan
    env.step(action)
  assert moved > 0, 'the value never moved a score'
  env.check_errors()


def test_a_captured_bootstrapped_decision_replays_the_eager_one():
  n, k = 4, 8
  env = _env(n, seed=8)
  agent = env.planner(num_plans=k, horizon=H, segment=SEGMENT, wind='belief', iterations=2, elite=3, seed=2, leaf_value=_critic(seed=2))
  out = torch.ones(n, dtype=torch.uint8, device=DEVICE)
  agent.act(None, out=out)
  saved = agent.state_dict()
  agent.act(None, out=out)
  torch.cuda.synchronize()
  eager = (out.clone(), agent.returns.clone(), agent.best_return.clone(), agent.best_plan.clone(), agent.leaf_obs.clone())
  graph, _ = dev.capture(env.device, lambda: agent.act(None, out=out))
  agent.load_state_dict(saved)
  out.fill_(9); agent.returns.fill_(0); agent.leaf_obs.fill_(0)
  graph.replay()
  torch.cuda.synchronize()
  for a, b in zip(eager, (out, agent.returns, agent.best_return, agent.best_plan, agent.leaf_obs)):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
  assert int(agent.counter.item()) == 2


def test_a_trainer_serves_its_live_weights_through_act_greedy():
  """A trainer as leaf_value is read through act_greedy -- its step counter stays -- and scores as the agent of its network does."""
  from balloon_learning_environment_amd.agents import imitation
  n, k = 4, 8
  env = _env(n, seed=11)
  trainer = imitation.BCTrainer(qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', seed=3, num_layers=2, hidden_units=64),
                                                          num_atoms=2))
  kw = dict(num_plans=k, horizon=H, segment=SEGMENT, wind='forecast', seed=5)
  by_trainer = env.planner(leaf_value=trainer, **kw)
  by_agent = env.planner(leaf_value=actor_critic.VecActorCriticAgent(trainer.network()), **kw)
  assert by_trainer._leaf_fn == trainer.act_greedy
  step = trainer.act_step.clone()
  a, b = by_trainer.act(None).clone(), by_agent.act(None).clone()
  torch.cuda.synchronize()
  assert torch.equal(a, b) and torch.equal(by_trainer.returns.view(torch.int32), by_agent.returns.view(torch.int32))
  assert torch.equal(trainer.act_step, step)


def test_leaf_value_refusals():
  with pytest.raises(ValueError, match='scenarios'):
    lookahead_agent.VecLookaheadAgent(wind='scenarios', leaf_value=_critic())
  with pytest.raises(ValueError, match='sampling'):
    lookahead_agent.VecLookaheadAgent(leaf_value=_critic(deterministic=False))
  with pytest.raises(ValueError, match='act_greedy'):
    lookahead_agent.VecLookaheadAgent(leaf_value=object())
