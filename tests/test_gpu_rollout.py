"""ble_rollout_f32 / VecSimulator.rollout_plans / VecBalloonEnv.lookahead against the existing transition kernels.

The reference of every case is ble_step_n_f32 itself: for plan k the source's state_dict() is loaded into a second VecSimulator of the
same n and env_offset (environment indices and episode counters, the key of the noise field, are preserved) and flown with
plans[:, :, k], every entry repeated action_repeat times, under the same noise seed.  Rewards, steps_flown (from the reference's
terminals) and the final (x, y, pressure, battery charge) must agree BIT FOR BIT; the return must lie within one float32 ulp of the
float64 host sum of gamma^t r_t over the reference's rewards, accumulated in the kernel's order (term = disc * r; acc += term;
disc *= gamma) and rounded to float32 once -- at most 960 float64 terms, so the sum itself carries ~1e-13 relative and the bound is
the final rounding.  Parity with the fp64 oracle follows transitively: ble_step_n_f32 is held to it by tests/test_gpu_parity.py, and
this file holds the rollout to ble_step_n_f32 exactly.

One reference simulator per case flies all K plans one after the other; sources are a few agent steps into a random rollout so that
the environments differ."""
import numpy as np
import pytest
import torch

from balloon_learning_environment_amd import _lib, device as dev, vec_state
from balloon_learning_environment_amd.env import balloon_env

pytestmark = pytest.mark.gpu

FINAL_FIELDS = ('x', 'y', 'pressure', 'battery_charge')


def _fly(sim, actions, noise_seed):
  """step_n over `actions` [T, n] (numpy): (rewards [T, n] f32, terminals [T, n] u8) device tensors."""
  a = torch.from_numpy(np.ascontiguousarray(actions, np.uint8)).to(sim.device)
  r = torch.zeros(a.shape, dtype=torch.float32, device=sim.device)
  t = torch.zeros(a.shape, dtype=torch.uint8, device=sim.device)
  sim.step_n(a, r, t, noise_seed=noise_seed)
  return r, t


def _source(n, seed, env_offset=0, per_env=False, noise_seed=None, vehicle=None, warm=4, advance_episodes=False):
  """A simulator `warm` random agent steps into its episodes: (sim, rng)."""
  rng = np.random.default_rng(seed)
  sim = vec_state.VecSimulator(n, 'cuda:0', env_offset=env_offset)
  sim.set_grid(rng.uniform(-12.0, 12.0, ((n,) if per_env else ()) + vec_state.GRID_SHAPE).astype(np.float32), per_env=per_env)
  if vehicle:
    sim.set_vehicle(**vehicle)
  sim.reset_device(seed)
  if advance_episodes:          # episode counters 1 and 2 in one batch
    sim.reset_device(seed, mask=torch.from_numpy((np.arange(n) % 3 != 0).astype(np.uint8)).to(sim.device))
  _fly(sim, rng.integers(0, 3, (warm, n)), noise_seed)
  sim.check_errors()
  return sim, rng


def _reference(src, plans, action_repeat, noise_seed):
  """ble_step_n_f32 on a copy of the source, plan by plan: (rewards [T, n, K] f32, steps_flown [n, K] i32, final [4, n, K] f32)."""
  h, n, k_plans = plans.shape
  steps = h * action_repeat
  sd = src.state_dict()
  ok = (sd['state']['status'] == 0).cpu().numpy()
  ref = vec_state.VecSimulator(n, 'cuda:0', env_offset=src.env_offset)
  rewards = np.zeros((steps, n, k_plans), np.float32)
  flown = np.zeros((n, k_plans), np.int32)
  final = np.zeros((4, n, k_plans), np.float32)
  for k in range(k_plans):
    ref.load_state_dict(sd)
    r, t = _fly(ref, np.repeat(plans[:, :, k], action_repeat, axis=0), noise_seed)
    term = t.cpu().numpy() != 0
    rewards[:, :, k] = r.cpu().numpy()
    flown[:, k] = np.where(ok, np.where(term.any(0), term.argmax(0) + 1, steps), 0)
    final[:, :, k] = np.stack([ref.state[f].cpu().numpy() for f in FINAL_FIELDS])
  return rewards, flown, final


def _host_returns(rewards, gamma):
  acc, disc = np.zeros(rewards.shape[1:], np.float64), 1.0
  for t in range(rewards.shape[0]):
    term = disc * rewards[t].astype(np.float64)
    acc += term
    disc *= gamma
  return acc.astype(np.float32)


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def _compare(out, ref, gamma, what):
  rewards, flown, final = ref
  torch.cuda.synchronize()
  got_rewards, got_final = out.rewards.cpu().numpy(), out.final.cpu().numpy()
  assert np.array_equal(out.steps_flown.cpu().numpy(), flown), what
  bad = np.argwhere(_bits(got_rewards) != _bits(rewards))
  assert bad.size == 0, (what, 'rewards', bad[:4].tolist())
  bad = np.argwhere(_bits(got_final) != _bits(final))
  assert bad.size == 0, (what, 'final', bad[:4].tolist())
  want = _host_returns(rewards, gamma)
  got = out.returns.cpu().numpy()
  err = np.abs(got.astype(np.float64) - want.astype(np.float64))
  ulp = np.spacing(np.abs(want)).astype(np.float64)
  print(f'{what}: returns max |diff| {err.max():.3e} = {np.max(err / ulp):.2f} ulp, exact in {np.mean(got == want):.3f}')
  assert np.all(err <= ulp), (what, 'returns', float(np.max(err / ulp)))


def _check(src, plans, gamma, action_repeat, noise_seed, what):
  out = src.rollout_plans(torch.from_numpy(plans).to(src.device), gamma=gamma, action_repeat=action_repeat, noise_seed=noise_seed,
                          want_rewards=True, want_final=True)
  ref = _reference(src, plans, action_repeat, noise_seed)
  _compare(out, ref, gamma, what)
  assert out.returns.shape == plans.shape[1:] and out.returns.dtype == torch.float32 and out.steps_flown.dtype == torch.int32
  return out, ref


# name: (n, K, H, action_repeat, gamma, source arguments, noise seed)
CASES = {
    'n130_k3_h6_waves_straddle_environments': (130, 3, 6, 1, 0.993, {}, None),
    'n5_k64_a_wave_shares_one_environment': (5, 64, 4, 1, 0.9, {}, None),
    'n1_k1': (1, 1, 5, 1, 1.0, {}, None),
    'n3_k70_per_environment_grids': (3, 70, 3, 1, 0.993, {'per_env': True}, None),
    'noise_env_offset_1000_episodes_advanced': (70, 5, 5, 1, 0.993, {'env_offset': 1000, 'advance_episodes': True}, 77),
    'action_repeat_2': (40, 4, 3, 2, 0.95, {}, None),
    'action_repeat_2_noise': (40, 4, 3, 2, 0.95, {}, 12),
    'runtime_vehicle': (66, 3, 4, 1, 0.993, {'vehicle': {'payload_mass': 95.0, 'battery_capacity_wh': 2800.0}}, None),
    'runtime_vehicle_noise': (66, 3, 4, 1, 0.993, {'vehicle': {'payload_mass': 95.0, 'battery_capacity_wh': 2800.0}}, 5),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_rollout_equals_step_n_on_a_copy(case):
  n, k, h, repeat, gamma, source, noise_seed = CASES[case]
  src, rng = _source(n, 100 + sorted(CASES).index(case), noise_seed=noise_seed, **source)
  if source.get('advance_episodes'):
    assert set(src.episode.cpu().numpy().tolist()) == {1, 2}
  if source.get('per_env'):
    assert src.grid_env_stride != 0
  plans = rng.integers(0, 3, (h, n, k)).astype(np.uint8)
  out, _ = _check(src, plans, gamma, repeat, noise_seed, case)
  assert int(src.rollout_flags.item()) == 0
  if noise_seed is not None:          # the noise is really flown: the forecast alone gives other rewards
    calm = src.rollout_plans(torch.from_numpy(plans).to(src.device), gamma=gamma, action_repeat=repeat, want_rewards=True)
    assert not torch.equal(calm.rewards, out.rewards)
  else:
    bare = src.rollout_plans(torch.from_numpy(plans).to(src.device), gamma=gamma, action_repeat=repeat)
    assert bare.rewards is None and bare.final is None and torch.equal(bare.returns, out.returns)


def test_terminals_freeze_a_plan_and_a_dead_source_flies_nothing():
  n, k, h = 48, 4, 6
  src, rng = _source(n, 31)
  dead = 3
  night = (src.state['solar_charging'] == 0) & (src.state['status'] == 0)
  night[dead] = False
  assert 0 < int(night.sum().item()) < n - 1
  # the night load, 183.7 W, drains 0.51 Wh per 10 s stride: 23 Wh last 45 strides, so the battery runs out inside agent step 2 of 0 .. 5
  src.state['battery_charge'][night] = 23.0
  src.state['status'][dead] = 1
  plans = rng.integers(0, 3, (h, n, k)).astype(np.uint8)
  out, (rewards, flown, final) = _check(src, plans, 0.993, 1, None, 'terminals')
  assert np.any((flown >= 2) & (flown <= h - 1)), 'no reference terminal at a step in [1, H - 2]'
  assert np.any(flown[np.arange(n) != dead] == h), 'no survivor'
  inside = np.argwhere((flown >= 2) & (flown <= h - 1))
  for e, p in inside[:8]:
    assert np.all(rewards[flown[e, p]:, e, p] == 0.0) and rewards[flown[e, p] - 1, e, p] != 0.0
  assert np.all(flown[dead] == 0) and np.all(rewards[:, dead] == 0.0)
  assert np.all(out.returns.cpu().numpy()[dead] == 0.0)
  for j, f in enumerate(FINAL_FIELDS):          # a dead source: its state as it lies
    assert np.all(_bits(final[j, dead]) == _bits(src.state[f][dead:dead + 1].cpu().numpy()))


def _tensors(d, prefix=''):
  for key, v in d.items():
    if isinstance(v, torch.Tensor):
      yield prefix + str(key), v
    elif isinstance(v, dict):
      yield from _tensors(v, prefix + str(key) + '.')


def _snapshot(sim):
  snap = dict(_tensors(sim.state_dict()))
  snap.update(episode_cache=sim.episode_cache.clone(), noise_cache=sim._noise_cache.clone())
  return snap


def test_no_side_effects_and_flags_of_its_own():
  n, k, h, noise_seed = 20, 9, 4, 9
  src, rng = _source(n, 41, noise_seed=noise_seed)
  src.wind_noise(noise_seed)
  assert src._noise_cache is not None and bool((src._noise_cache != 0).any())
  # an upwelling IR outside total_absorptivity's range: every plan of environment 2 raises BLE_FLAG_ABSORPTIVITY -- and its per-episode
  # cache entry no longer matches, a miss the rollout recomputes and must not store
  src.state['upwelling_infrared'][2] = 1e-3
  torch.cuda.synchronize()
  before = _snapshot(src)
  assert {'state.x', 'state.last_command', 'episode', 'err_flags', 'active_slots', 'grid'} <= set(before)
  plans = torch.from_numpy(rng.integers(0, 3, (h, n, k)).astype(np.uint8)).to(src.device)
  for seed in (noise_seed, None):
    src.rollout_plans(plans, gamma=0.993, noise_seed=seed, want_rewards=True, want_final=True)
  torch.cuda.synchronize()
  after = _snapshot(src)
  assert sorted(before) == sorted(after)
  for name in before:
    assert before[name].dtype == after[name].dtype and torch.equal(before[name], after[name]), name
  assert int(src.rollout_flags.item()) & _lib.FLAG_ABSORPTIVITY
  assert int(src.err_flags.item()) == 0
  src.check_errors()                       # a flight that never happened raises nothing
  assert int(src.rollout_flags.item()) != 0      # ... and check_errors() leaves the rollout's word alone


def test_graph_capture_replays_on_the_advanced_state():
  n, k, h, noise_seed = 70, 5, 4, 5
  src, rng = _source(n, 51, noise_seed=noise_seed)
  plans = torch.from_numpy(rng.integers(0, 3, (h, n, k)).astype(np.uint8)).to(src.device)
  kwargs = dict(gamma=0.99, noise_seed=noise_seed, want_rewards=True, want_final=True)
  first = src.rollout_plans(plans, **kwargs)
  torch.cuda.synchronize()
  out = vec_state.Rollout(*[torch.zeros_like(t) for t in first])
  graph, _ = dev.capture(src.device, lambda: src.rollout_plans(plans, out=out, **kwargs))
  _fly(src, rng.integers(0, 3, (1, n)), noise_seed)          # the source moves on one agent step
  graph.replay()
  eager = src.rollout_plans(plans, **kwargs)
  torch.cuda.synchronize()
  for name, a, b, c in zip(out._fields, out, eager, first):
    assert torch.equal(a, b), name
    assert name == 'steps_flown' or not torch.equal(a, c), name          # (the state the graph read is the new one)


def test_env_lookahead_predicts_the_rewards_step_returns():
  n, steps = 6, 4
  rng = np.random.default_rng(61)
  env = balloon_env.VecBalloonEnv(n, seed=3, wind_noise=True, auto_reset=False)
  env.reset()
  for a in rng.integers(0, 3, (5, n)).astype(np.uint8):
    env.step(torch.from_numpy(a).cuda())
  plans = torch.from_numpy(rng.integers(0, 3, (steps, n, 1)).astype(np.uint8)).cuda()
  truth = env.lookahead(plans, want_rewards=True)
  forecast = env.lookahead(plans, wind='forecast', want_rewards=True)
  arena = env.arena.lookahead(plans, 0.993, 1, env.arena._seed, want_rewards=True)
  torch.cuda.synchronize()
  assert torch.equal(arena.rewards, truth.rewards) and torch.equal(arena.returns, truth.returns)
  flown = torch.stack([env.step(plans[t, :, 0].contiguous())[1] for t in range(steps)])
  torch.cuda.synchronize()
  assert torch.equal(truth.rewards[:, :, 0], flown)
  assert not torch.equal(forecast.rewards, truth.rewards)
  want = _host_returns(flown.cpu().numpy()[:, :, None], 0.993)
  err = np.abs(truth.returns.cpu().numpy().astype(np.float64) - want)
  assert np.all(err <= np.spacing(np.abs(want)))
  env.check_errors()
  with pytest.raises(ValueError, match='truth'):
    env.lookahead(plans, wind='gp')
  calm = balloon_env.VecBalloonEnv(n, seed=3, wind_noise=False, auto_reset=False)
  calm.reset()
  a, b = calm.lookahead(plans, want_rewards=True), calm.lookahead(plans, wind='forecast', want_rewards=True)
  assert torch.equal(a.rewards, b.rewards)          # without wind noise the truth IS the forecast


def test_a_fleet_is_refused():
  src, rng = _source(4, 71)
  src.set_fleet([{}, {'envelope_mass': 75.0}])
  with pytest.raises(ValueError, match='fleet'):
    src.rollout_plans(torch.zeros(2, 4, 3, dtype=torch.uint8, device=src.device))
