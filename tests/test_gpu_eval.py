"""Evaluation on the device: ble_eval_accumulate_f32, the per-environment seeds and eval_lib.eval_agent_vec.

 * the bookkeeping against a line-by-line host restatement of eval_lib.py:157-190 on F13's states and rewards, and a burst;
 * eval_agent_vec against an eager host-driven loop over the same seeded batch (with and without a captured graph);
 * seed independence: a seed flies the same flight in any batch at any position, and the first episode of
   VecBalloonEnv(1, seed=s, per_env_fields=True, auto_reset=False);
 * the scalar-seed reset and noise are unchanged by the seeded forms.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
RADIUS_M = 50_000.0


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd import _abi, _lib, vec_state
  from balloon_learning_environment_amd.agents import station_seeker_agent
  from balloon_learning_environment_amd.eval import eval_lib, suites
  return dict(_abi=_abi, _lib=_lib, vec_state=vec_state, ssa=station_seeker_agent, eval_lib=eval_lib, suites=suites)


class _Acc:
  def __init__(self, m, n):
    z = lambda dt: torch.zeros(n, dtype=dt, device='cuda')
    self.reward, self.within, self.final, self.done, self.status = z(torch.float64), z(torch.int32), z(torch.int32), z(torch.uint8), z(torch.uint8)
    self.struct = m['_abi'].BleEvalAcc(self.reward.data_ptr(), self.within.data_ptr(), self.final.data_ptr(), self.done.data_ptr(),
                                       self.status.data_ptr())

  def call(self, m, sim, reward, t, max_steps, path=None):
    code = m['_lib'].lib().ble_eval_accumulate_f32(ctypes.byref(sim._struct), reward.data_ptr(), ctypes.byref(self.struct), RADIUS_M, t,
                                                   max_steps, 0 if path is None else path.data_ptr(), sim.n,
                                                   torch.cuda.current_stream().cuda_stream)
    m['_lib'].check(code, 'ble_eval_accumulate_f32')

  def host(self):
    return [t.cpu().numpy() for t in (self.reward, self.within, self.final, self.done, self.status)]


class _HostLoop:
  """eval_lib.py:157-190, line by line, on per-step values pulled to the host."""

  def __init__(self, n):
    self.total = [0.0] * n; self.within = [0] * n; self.final = [0] * n; self.done = [False] * n; self.status = [0] * n

  def add(self, i, reward32, x32, y32, status, t, max_steps):
    if self.done[i]:
      return
    self.total[i] += float(reward32)
    self.within[i] += (float(x32) * float(x32) + float(y32) * float(y32)) ** 0.5 <= RADIUS_M
    self.final[i] = t + 1
    if status != 0:
      self.status[i] = int(status); self.done[i] = True
    if t + 1 == max_steps:
      self.done[i] = True


def test_bookkeeping_on_f13(mods):
  g = helpers.golden('f13_station_seeker')
  n = int(g['n_flown'])
  sim = mods['vec_state'].VecSimulator(1)
  acc = _Acc(mods, 1)
  host = _HostLoop(1)
  reward = torch.zeros(1, dtype=torch.float32, device='cuda')
  path = torch.zeros(n, 1, 6, dtype=torch.float32, device='cuda')
  for i in range(n):
    row = helpers.feature_row(g, 0, i + 1)                     # the post-step state of step i
    sim.set_state({k: np.array([v]) for k, v in row.items()})
    r32 = np.float32(g['reward'][0, i])
    reward.fill_(float(r32))
    acc.call(mods, sim, reward, i, n, path[i])
    st = sim.get_state()
    host.add(0, r32, st['x'][0], st['y'][0], int(st['status'][0]), i, n)
    soc = np.float32(float(st['battery_charge'][0]) / 3058.56)                 # BalloonState.battery_soc, the default capacity
    np.testing.assert_array_equal(path[i, 0].cpu().numpy(), np.array([st['x'][0], st['y'][0], st['pressure'][0], st['superpressure'][0],
                                                                      st['time_elapsed_s'][0], soc], np.float32))
  got = acc.host()
  assert got[0][0] == host.total[0]
  assert got[1][0] == host.within[0] and got[2][0] == host.final[0] == n and got[3][0] == 1 and got[4][0] == 0
  ref = float(np.sum(g['reward'][0, :n]))
  assert abs(got[0][0] - ref) <= n * 2.0 ** -24 * abs(ref)
  print(f'F13 bookkeeping: reward {got[0][0]:.6f} (reference fp64 {ref:.6f}), {got[1][0]} of {n} steps within 50 km')


def test_burst_stops_counting(mods):
  g = helpers.golden('f13_station_seeker')
  sim = mods['vec_state'].VecSimulator(3)
  row = helpers.feature_row(g, 0, 10)
  sim.set_state({k: np.full(3, v) for k, v in row.items()})
  acc = _Acc(mods, 3)
  reward = torch.full((3,), 0.5, dtype=torch.float32, device='cuda')
  k, T = 5, 12
  for t in range(T):
    if t == k:
      sim.state['status'][1] = 2                                # BURST after step k
      sim.state['status'][2] = 3                                # ZEROPRESSURE
    acc.call(mods, sim, reward, t, T)
  total, within, final, done, status = acc.host()
  assert list(final) == [T, k + 1, k + 1] and list(done) == [1, 1, 1] and list(status) == [0, 2, 3]
  assert list(total) == [0.5 * T, 0.5 * (k + 1), 0.5 * (k + 1)]
  ev = mods['eval_lib']
  lib_res = ev.EvaluationResult(seed=0, cumulative_reward=float(total[1]), time_within_radius=within[1] / final[1], out_of_power=False,
                                envelope_burst=bool(status[1] == 2), zeropressure=False, final_timestep=int(final[1]), flight_path=[])
  assert lib_res.envelope_burst and lib_res.final_timestep == k + 1


def _eager_loop(m, seeds, T):
  """The reference for eval_agent_vec: VecSimulator calls and VecStationSeekerAgent, per-step pulls accumulated on the host."""
  from balloon_learning_environment_amd.env import generative_wind_field
  n = len(seeds)
  sim = m['vec_state'].VecSimulator(n)
  env_seed = torch.tensor(seeds, dtype=torch.int64, device='cuda')
  sim.episode.zero_()
  sim.reset_device_seeded(env_seed)
  sampler = generative_wind_field.GenerativeWindFieldSampler(device='cuda:0')
  sim.set_grid(sampler.decode(sampler.sample_latents_seeded(env_seed, sim.episode)), per_env=True)
  agent = m['ssa'].VecStationSeekerAgent(err_flags=sim.err_flags)
  noise = sim.wind_noise_seeded(env_seed)
  action = agent.act(sim.observe(noise, live_only=True)).clone()
  host = _HostLoop(n)
  actions, rewards = [], []
  for t in range(T):
    reward, _ = sim.step(action, noise)
    noise = sim.wind_noise_seeded(env_seed)
    action = agent.act(sim.observe(noise, live_only=True)).clone()
    st = sim.get_state()
    r = reward.cpu().numpy()
    actions.append(action.cpu().numpy()); rewards.append(r.copy())
    for i in range(n):
      host.add(i, r[i], st['x'][i], st['y'][i], int(st['status'][i]), t, T)
  sim.check_errors()
  return host, np.array(actions), np.array(rewards)


def _key(r):
  return (r.seed, r.cumulative_reward, r.time_within_radius, r.out_of_power, r.envelope_burst, r.zeropressure, r.final_timestep)


def test_eval_agent_vec_matches_eager_loop(mods):
  m = mods
  seeds, T = list(range(500, 756)), 120
  host, actions, rewards = _eager_loop(m, seeds, T)
  suite = m['suites'].EvaluationSuite(seeds, T)
  for capture in (False, True):
    agent = m['ssa'].VecStationSeekerAgent()
    log = []
    if not capture:                            # (a recording callable: a Python list cannot be filled inside a replayed graph)
      def rec(obs):
        a = agent.act(obs)
        log.append(a.clone())
        return a
      res = m['eval_lib'].eval_agent_vec(rec, suite, capture_graph=False)
      np.testing.assert_array_equal(torch.stack(log[1:]).cpu().numpy(), actions)
    else:
      res = m['eval_lib'].eval_agent_vec(agent, suite, capture_graph=True, calculate_flight_path=True)
      assert all(len(r.flight_path) == r.final_timestep for r in res)
    assert [r.seed for r in res] == seeds
    for i, r in enumerate(res):
      assert r.cumulative_reward == host.total[i], (capture, i)
      assert r.final_timestep == host.final[i] and r.time_within_radius == host.within[i] / host.final[i]
      assert (r.out_of_power, r.envelope_burst, r.zeropressure) == (host.status[i] == 1, host.status[i] == 2, host.status[i] == 3)
      live = np.arange(T) < host.final[i]
      assert r.cumulative_reward == float(sum(float(v) for v in rewards[live, i]))
  print(f'eval_agent_vec: 256 seeds x {T} steps bit-identical to the eager loop, with and without a captured graph; '
        f'mean reward {np.mean(host.total):.3f}')


def _shared_field_sampler(field):
  from balloon_learning_environment_amd.env import grid_wind_field_sampler

  class Fixed(grid_wind_field_sampler.GridWindFieldSampler):
    @property
    def field_shape(self):
      return grid_wind_field_sampler.FieldShape()

    def sample_field(self, key, date_time=None):
      return field
  return Fixed()


def test_seed_independence(mods):
  m = mods
  from balloon_learning_environment_amd.env import grid_based_wind_field
  field = helpers.fixture_field(helpers.golden('f13_station_seeker'))
  wf = grid_based_wind_field.GridBasedWindField(_shared_field_sampler(field), 'cuda:0')
  wf.set_field(field)
  seeds, T = [7 * s + 3 for s in range(64)], 96
  perm = list(np.random.default_rng(0).permutation(64))
  agent = m['ssa'].VecStationSeekerAgent()
  ev = lambda ss, **kw: m['eval_lib'].eval_agent_vec(agent, m['suites'].EvaluationSuite(ss, T), **kw)
  one = {r.seed: _key(r) for r in ev(seeds, wind_field=wf)}
  permuted = {r.seed: _key(r) for r in ev([seeds[j] for j in perm], wind_field=wf)}
  split = {r.seed: _key(r) for r in ev(seeds, wind_field=wf, batch_size=63)}          # batches of 63 and 1
  assert one == permuted == split
  # the generative field, one per seed: a permuted batch flies the same
  gen_one = {r.seed: _key(r) for r in ev(seeds)}
  gen_perm = {r.seed: _key(r) for r in ev([seeds[j] for j in perm])}
  assert gen_one == gen_perm
  print(f'seed independence: 64 seeds, shared field: one batch == permuted == 63 + 1; generative fields: one batch == permuted')


def test_seed_contract_against_vec_balloon_env(mods):
  """Seed s of an evaluation flies the first episode of VecBalloonEnv(1, seed=s, per_env_fields=True, auto_reset=False)."""
  m = mods
  from balloon_learning_environment_amd.env import balloon_env
  seeds, T = [11, 4242, 90001, 3], 60
  agent = m['ssa'].VecStationSeekerAgent()
  ev = m['eval_lib'].VecEvaluator(len(seeds), agent, T, capture_graph=False)
  ev.launch(seeds)
  res = ev.results(seeds)
  field_diffs = []
  for j, s in enumerate(seeds):
    env = balloon_env.VecBalloonEnv(1, seed=s, per_env_fields=True, auto_reset=False)
    obs = env.reset()
    sampler = env.arena.wind_field._wind_field_sampler
    lat_env = sampler.sample_latents_keyed(torch.zeros(1, dtype=torch.int64, device='cuda'), env.arena.sim.episode[:1], s)
    lat_eval = sampler.sample_latents_seeded(torch.tensor([s], dtype=torch.int64, device='cuda'), torch.ones(1, dtype=torch.int32, device='cuda'))
    assert torch.equal(lat_env, lat_eval)
    field_diff = float((env.arena._grids[0] - ev.grids[j]).abs().max())
    field_diffs.append(field_diff)
    assert field_diff == 0.0, (s, field_diff)     # the decoder's GEMMs give this row the same bits at batch sizes 4 and 1
    host = _HostLoop(1)
    a = agent.act(obs).clone()
    for t in range(T):
      obs, reward, _ = env.step(a)
      a = agent.act(obs).clone()
      st = env.arena.sim.get_state()
      host.add(0, reward.cpu().numpy()[0], st['x'][0], st['y'][0], int(st['status'][0]), t, T)
    assert res[j].cumulative_reward == host.total[0] and res[j].final_timestep == host.final[0]
    assert res[j].time_within_radius == host.within[0] / host.final[0]
  print(f'seed contract: {len(seeds)} seeds: latents, decoded fields and {T}-step flights equal to VecBalloonEnv(1, seed=s)')


def test_scalar_seed_paths_unchanged(mods):
  m = mods
  vs = m['vec_state']
  n = 5
  sim = vs.VecSimulator(n)
  sim.set_grid(helpers.fixture_field(helpers.golden('f13_station_seeker')))
  sim.reset_device(1234)
  before = sim.get_state()
  noise_before = sim.wind_noise(1234).clone()
  seeds = torch.tensor([1234, 5, 1234, 77, 2 ** 40 + 9], dtype=torch.int64, device='cuda')
  sim.episode.zero_()
  sim.reset_device_seeded(seeds)
  seeded_state = sim.get_state()
  seeded_noise = sim.wind_noise_seeded(seeds).clone()
  sim.episode.zero_()
  sim.reset_device(1234)
  after = sim.get_state()
  for k in before:
    np.testing.assert_array_equal(before[k], after[k], err_msg=k)
  assert torch.equal(noise_before, sim.wind_noise(1234))
  sim.check_errors()
  # each seeded environment is environment 0 of a one-environment simulator reset with its seed
  for i, s in enumerate(seeds.tolist()):
    one = vs.VecSimulator(1)
    one.set_grid(helpers.fixture_field(helpers.golden('f13_station_seeker')))
    one.reset_device(s)
    st = one.get_state()
    for k in st:
      assert st[k][0] == seeded_state[k][i], (i, k)
    assert torch.equal(one.wind_noise(s)[0], seeded_noise[i]), i


def test_live_observation_skips_terminated_lanes(mods):
  """ble_observe_live_f32: a lane whose status is not OK keeps its history and observation row; the others are observed bit for bit as
  by ble_observe_f32."""
  vs = mods['vec_state']
  n = 6
  seeds = torch.tensor([21, 22, 23, 24, 25, 26], dtype=torch.int64, device='cuda')
  field = helpers.fixture_field(helpers.golden('f13_station_seeker'))
  sims = [vs.VecSimulator(n) for _ in range(2)]
  obs = []
  for sim in sims:
    sim.set_grid(field)
    sim.reset_device_seeded(seeds)
    obs.append(sim.observe(sim.wind_noise_seeded(seeds)).clone())
    sim.step(torch.full((n,), 2, dtype=torch.uint8, device='cuda'), sim.wind_noise_seeded(seeds))
  sims[1].state['status'][[1, 4]] = torch.tensor([2, 1], dtype=torch.uint8, device='cuda')
  sims[0].state['status'][[1, 4]] = torch.tensor([2, 1], dtype=torch.uint8, device='cuda')
  full = sims[0].observe(sims[0].wind_noise_seeded(seeds))
  out = obs[1].clone()
  count_before = sims[1]._gp['count'].clone()
  live = sims[1].observe(sims[1].wind_noise_seeded(seeds), out=out, live_only=True)
  for sim in sims:
    sim.check_errors()
  keep = [0, 2, 3, 5]
  assert torch.equal(live[keep], full[keep])
  assert torch.equal(live[[1, 4]], obs[1][[1, 4]])                 # untouched rows
  after = sims[1]._gp['count']
  assert torch.equal(after[[1, 4]], count_before[[1, 4]]) and bool((after[keep] == count_before[keep] + 1).all())


def test_eval_agent_vec_reports_a_terminated_flight(mods):
  """A flight that terminates mid-way is reported (final_timestep, the terminal flag) and the rest of the batch flies on: the lane is
  not observed again, so its frozen clock adds nothing to its WindGP window and nothing raises."""
  m = mods
  seeds, T, k = [31, 32, 33, 34], 150, 9          # lane 2 bursts after step k - 1
  agent = m['ssa'].VecStationSeekerAgent()
  ev = m['eval_lib'].VecEvaluator(len(seeds), None, T, capture_graph=False, calculate_flight_path=True)
  rewards, calls = [], [0]

  def policy(obs):
    if calls[0] >= 1:
      rewards.append(ev.sim.reward.clone())       # the reward of step calls - 1
    if calls[0] == k:
      ev.sim.state['status'][2] = 2               # BURST, as the transition would write it
    calls[0] += 1
    return agent.act(obs)
  ev.agent = policy
  ev.launch(seeds)
  res = ev.results(seeds)
  assert [r.final_timestep for r in res] == [T, T, k, T]
  assert res[2].envelope_burst and not res[2].out_of_power and not res[2].zeropressure
  assert not any(r.envelope_burst or r.out_of_power or r.zeropressure for r in (res[0], res[1], res[3]))
  assert len(res[2].flight_path) == k
  r = torch.stack(rewards).cpu().numpy()
  assert res[2].cumulative_reward == float(sum(float(v) for v in r[:k, 2]))
  assert res[0].cumulative_reward == float(sum(float(v) for v in r[:, 0]))
  # the other flights are the ones a batch without the burst flies
  ref = m['eval_lib'].eval_agent_vec(agent, m['suites'].EvaluationSuite(seeds, T), capture_graph=True)
  for i in (0, 1, 3):
    assert _key(res[i]) == _key(ref[i]), i
  print(f'terminated flight: seed {seeds[2]} reported at final_timestep {k} (burst), the other {len(seeds) - 1} fly on unchanged')


def test_serial_eval_agent(mods):
  """eval_agent, the reference's serial loop, over a BalloonEnv with the reference-shaped StationSeekerAgent."""
  from balloon_learning_environment_amd.env import balloon_env
  m = mods
  env = balloon_env.BalloonEnv(seed=0)
  agent = m['ssa'].StationSeekerAgent(3, (1099,))
  res = m['eval_lib'].eval_agent(agent, env, m['suites'].EvaluationSuite([5, 6], 12), calculate_flight_path=True)
  assert [r.seed for r in res] == [5, 6]
  for r in res:
    assert r.final_timestep == 12 and len(r.flight_path) == 12
    assert 0.0 <= r.time_within_radius <= 1.0 and r.cumulative_reward > 0.0
    assert [p.time_elapsed.total_seconds() for p in r.flight_path] == [180.0 * (i + 1) for i in range(12)]
    assert 0.0 < r.flight_path[-1].battery_soc <= 1.0 + 1e-6          # (a full battery: the float32 charge may round above 3058.56 Wh)
  again = m['eval_lib'].eval_agent(agent, env, m['suites'].EvaluationSuite([5], 12), calculate_flight_path=False)
  assert _key(again[0]) == _key(res[0]) and again[0].flight_path == []
