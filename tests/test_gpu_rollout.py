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
the environments differ.

Step length and horizon.  The cases named substeps_* fly agent steps of 1, 2 and 60 strides (RolloutArgs.substeps reaches agent_step in
both kernels; a rollout that flew 18 strides whatever it was told would give other rewards than step_n(substeps=)).  The cases named
h960 / h320 / h120 fly BLE_ROLLOUT_MAX_STEPS = 960 agent steps: the reward offset advances by n K 960 times, the discount is multiplied
960 times, and the plans cross two sunsets, two sunrises and the 48 h end of the forecast's time axis.  Random plans alone never end a
flight (the safety layers see to that: 300 environments x 960 steps in the fp64 oracle, at a third, a fifth and a tenth of DOWN
actions, lost none), so the long cases give every environment that lies in the night (solar_charging == 0) a battery of 300 Wh, as
test_terminals_freeze_a_plan_and_a_dead_source_flies_nothing gives 23 Wh: 98 minutes of the night load of 183.7 W, so those whose sun
does not rise first run out of power at agent step 34 of 180 s (11 of 600 s), and the day's environments fly on.  The three
conditions are asserted from the reference's own terminals (see the note above the cases)."""
import numpy as np
import pytest
import torch

from balloon_learning_environment_amd import _lib, device as dev, vec_state
from balloon_learning_environment_amd.env import balloon_env

pytestmark = pytest.mark.gpu

FINAL_FIELDS = ('x', 'y', 'pressure', 'battery_charge')


def _fly(sim, actions, noise_seed, substeps=18):
  """step_n over `actions` [T, n] (numpy): (rewards [T, n] f32, terminals [T, n] u8) device tensors."""
  a = torch.from_numpy(np.ascontiguousarray(actions, np.uint8)).to(sim.device)
  r = torch.zeros(a.shape, dtype=torch.float32, device=sim.device)
  t = torch.zeros(a.shape, dtype=torch.uint8, device=sim.device)
  sim.step_n(a, r, t, substeps=substeps, noise_seed=noise_seed)
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


def _reference(src, plans, action_repeat, noise_seed, substeps=18, want_alive=False):
  """ble_step_n_f32 on a copy of the source, plan by plan: (rewards [T, n, K] f32, steps_flown [n, K] i32, final [4, n, K] f32); with
  want_alive a fourth entry, alive [n, K] bool: the reference's status is OK after the last step."""
  h, n, k_plans = plans.shape
  steps = h * action_repeat
  sd = src.state_dict()
  ok = (sd['state']['status'] == 0).cpu().numpy()
  ref = vec_state.VecSimulator(n, 'cuda:0', env_offset=src.env_offset)
  rewards = np.zeros((steps, n, k_plans), np.float32)
  flown = np.zeros((n, k_plans), np.int32)
  final = np.zeros((4, n, k_plans), np.float32)
  alive = np.zeros((n, k_plans), bool)
  for k in range(k_plans):
    ref.load_state_dict(sd)
    r, t = _fly(ref, np.repeat(plans[:, :, k], action_repeat, axis=0), noise_seed, substeps)
    term = t.cpu().numpy() != 0
    rewards[:, :, k] = r.cpu().numpy()
    flown[:, k] = np.where(ok, np.where(term.any(0), term.argmax(0) + 1, steps), 0)
    final[:, :, k] = np.stack([ref.state[f].cpu().numpy() for f in FINAL_FIELDS])
    alive[:, k] = ref.state['status'].cpu().numpy() == 0
  return (rewards, flown, final, alive) if want_alive else (rewards, flown, final)


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
  rewards, flown, final = ref[:3]
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


def _check(src, plans, gamma, action_repeat, noise_seed, what, substeps=18, want_alive=False):
  out = src.rollout_plans(torch.from_numpy(plans).to(src.device), gamma=gamma, action_repeat=action_repeat, noise_seed=noise_seed,
                          substeps=substeps, want_rewards=True, want_final=True)
  ref = _reference(src, plans, action_repeat, noise_seed, substeps, want_alive)
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
SEEDS = {case: 100 + i for i, case in enumerate(sorted(CASES))}          # (the seeds these nine have always had)

# Step length and horizon: an eighth field of extras -- substeps (default 18), seed, and low_battery (the long cases: the environments in
# the night get LOW_BATTERY_WH; see the docstring).
# substeps_*: 70 x 3 = 210 lanes, a block boundary inside an environment's plans; 60 strides is where the solar band widens (sun_band).
# h960 / h320 / h120: 960 agent steps.  22 x 3 = 66 lanes: one wave plus two lanes.  h960: 40 warm steps, so the last 40 of the 960 lie
# beyond the forecast's 48 h; gamma^960 = 1.2e-3, every term still counts.  h320: the sum carries no decay.  h120: 960 steps of 10
# minutes, 160 h.  The seeds' own counts (plans that fly all 960 steps / end at a step strictly inside (1, 959) / are alive after step
# 960) are printed by every run of a long case; NOT YET RECORDED HERE: no MI355X run of these cases exists.  What the fp64 oracle gives
# for 1 200 host-sampled initial states under the same treatment (a third of the actions DOWN): 48 % lie in the night; of those 85 - 88 %
# end, all at agent step 34 or 35 of 180 s (11 of 600 s), the others see the sun first and survive; every environment of the day is alive
# after 960 steps.  Groups of 22 drawn from them miss a condition in 0 - 1 of 20 000 draws, groups of 8 in 1.5 % (no or only night
# environments, or every night one saved by the sunrise); a seed that does is replaced, the condition is not.
_VEHICLE = {'vehicle': {'payload_mass': 95.0, 'battery_capacity_wh': 2800.0}}
CASES.update({
    'substeps_1': (70, 3, 3, 1, 0.993, {}, None, {'substeps': 1, 'seed': 120}),
    'substeps_2': (70, 3, 3, 1, 0.993, {}, None, {'substeps': 2, 'seed': 121}),
    'substeps_60': (70, 3, 3, 1, 0.993, {}, None, {'substeps': 60, 'seed': 122}),
    'substeps_1_noise': (70, 3, 3, 1, 0.993, {}, 21, {'substeps': 1, 'seed': 123}),
    'substeps_60_noise': (70, 3, 3, 1, 0.993, {}, 22, {'substeps': 60, 'seed': 124}),
    'substeps_60_runtime_vehicle': (66, 3, 2, 1, 0.993, _VEHICLE, None, {'substeps': 60, 'seed': 125}),
    'h960_full_horizon': (22, 3, 960, 1, 0.993, {'warm': 40}, None, {'seed': 140, 'low_battery': True}),
    'h320_repeat_3': (22, 3, 320, 3, 1.0, {}, None, {'seed': 141, 'low_battery': True}),
    'h320_repeat_3_noise': (22, 3, 320, 3, 1.0, {}, 33, {'seed': 142, 'low_battery': True}),
    'h120_repeat_8_substeps_60': (8, 9, 120, 8, 1.0, {}, None, {'substeps': 60, 'seed': 143, 'low_battery': True}),
})
LOW_BATTERY_WH = 300.0
MAX_STEPS = 960


def _long_counts(flown, alive, case, seed):
  """The three counts the long cases' conditions are about, from the reference's terminals and final status."""
  full, inside = flown == MAX_STEPS, (flown > 2) & (flown < MAX_STEPS - 1)          # (the terminal's step index is flown - 1)
  counts = int(full.sum()), int(inside.sum()), int((alive & full).sum())
  print(f'{case} seed {seed}: of {flown.size} plans {counts[0]} fly all {MAX_STEPS} steps, {counts[1]} end at a step inside (1, {MAX_STEPS - 1}), '
        f'{counts[2]} are alive after step {MAX_STEPS}; steps flown by those that end {sorted(set(flown[~full].tolist()))}')
  return counts


def _run_case(case, seed=None):
  """One of CASES, flown and checked; the long cases return their three counts.  seed: another source than the case's own (a seed scan)."""
  n, k, h, repeat, gamma, source, noise_seed, *extras = CASES[case]
  extras = extras[0] if extras else {}
  substeps = extras.get('substeps', 18)
  seed = extras.get('seed', SEEDS.get(case)) if seed is None else seed
  src, rng = _source(n, seed, noise_seed=noise_seed, **source)
  if source.get('advance_episodes'):
    assert set(src.episode.cpu().numpy().tolist()) == {1, 2}
  if source.get('per_env'):
    assert src.grid_env_stride != 0
  if extras.get('low_battery'):
    src.state['battery_charge'][(src.state['solar_charging'] == 0) & (src.state['status'] == 0)] = LOW_BATTERY_WH
  plans = rng.integers(0, 3, (h, n, k)).astype(np.uint8)
  out, ref = _check(src, plans, gamma, repeat, noise_seed, case, substeps, want_alive=True)
  assert int(src.rollout_flags.item()) == 0
  if noise_seed is not None:          # the noise is really flown: the forecast alone gives other rewards
    calm = src.rollout_plans(torch.from_numpy(plans).to(src.device), gamma=gamma, action_repeat=repeat, substeps=substeps, want_rewards=True)
    assert not torch.equal(calm.rewards, out.rewards)
  else:
    bare = src.rollout_plans(torch.from_numpy(plans).to(src.device), gamma=gamma, action_repeat=repeat, substeps=substeps)
    assert bare.rewards is None and bare.final is None and torch.equal(bare.returns, out.returns)
  if substeps != 18:                  # the step length is really flown: 18 strides give another flight
    other = src.rollout_plans(torch.from_numpy(plans).to(src.device), gamma=gamma, action_repeat=repeat, noise_seed=noise_seed,
                              want_rewards=True, want_final=True)
    assert not torch.equal(other.final, out.final) and not torch.equal(other.rewards, out.rewards)
  if h * repeat == MAX_STEPS:         # the long cases' conditions, from the reference's own terminals and state, never from the rollout
    rewards, flown, _, alive = ref
    full, inside, survivors = _long_counts(flown, alive, case, seed)
    assert full >= 1, 'no plan flies all 960 steps'
    assert inside >= 1, 'no reference terminal at a step strictly inside (1, 959)'
    assert survivors >= 1, 'no survivor of 960 steps: no live lane crossed sunset, sunrise and the 48 h end of the forecast'
    e, p = np.argwhere(flown < MAX_STEPS)[0]
    assert np.all(rewards[flown[e, p]:, e, p] == 0.0) and rewards[flown[e, p] - 1, e, p] != 0.0
    return full, inside, survivors


@pytest.mark.parametrize('case', sorted(CASES))
def test_rollout_equals_step_n_on_a_copy(case):
  _run_case(case)


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


def test_more_than_960_steps_are_refused():
  src, rng = _source(2, 72)
  for h, repeat in ((961, 1), (481, 2)):
    with pytest.raises(ValueError, match='960'):
      src.rollout_plans(torch.zeros(h, 2, 1, dtype=torch.uint8, device=src.device), action_repeat=repeat)
  src.rollout_plans(torch.zeros(480, 2, 1, dtype=torch.uint8, device=src.device), action_repeat=2)
  torch.cuda.synchronize()


def test_a_fleet_is_refused():
  src, rng = _source(4, 71)
  src.set_fleet([{}, {'envelope_mass': 75.0}])
  with pytest.raises(ValueError, match='fleet'):
    src.rollout_plans(torch.zeros(2, 4, 3, dtype=torch.uint8, device=src.device))
