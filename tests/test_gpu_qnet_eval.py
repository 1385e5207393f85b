"""A learned policy in the evaluation loop: eval_agent_vec with VecQNetworkAgent (a Perciatelli44-shaped QR-DQN network of the
reference's initialisation), and the reference-shaped QuantileAgent / Perciatelli44 in the serial loops.

 * captured and uncaptured evaluations are bit-identical; a permuted batch and a 63 + 1 split fly the same flights;
 * seed s flies what a host-driven loop over VecBalloonEnv(1, seed=s, per_env_fields=True, auto_reset=False) with QuantileAgent
   flies: the seed contract with the network in the loop;
 * eval_agent (the serial loop) with Perciatelli44(params=...) on BalloonEnv.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import perciatelli44, qnet, quantile_agent
  from balloon_learning_environment_amd.eval import eval_lib, suites
  params = qnet.init_params('quantile', 44, 8, 600, 51)
  return dict(qnet=qnet, qa=quantile_agent, p44=perciatelli44, eval_lib=eval_lib, suites=suites, params=params)


def _fixed_sampler(field):
  from balloon_learning_environment_amd.env import grid_wind_field_sampler

  class Fixed(grid_wind_field_sampler.GridWindFieldSampler):
    @property
    def field_shape(self):
      return grid_wind_field_sampler.FieldShape()

    def sample_field(self, key, date_time=None):
      return field
  return Fixed()


def _key(r):
  return (r.seed, r.cumulative_reward, r.time_within_radius, r.out_of_power, r.envelope_burst, r.zeropressure, r.final_timestep)


def test_eval_agent_vec_with_a_quantile_network(mods):
  m = mods
  agent = m['qnet'].VecQNetworkAgent(m['qnet'].QNetwork.from_params(m['params']))
  seeds, T = [13 * s + 1 for s in range(64)], 96
  suite = m['suites'].EvaluationSuite(seeds, T)
  log = []

  def rec(obs):                                     # uncaptured, recording every decision
    a = agent.act(obs)
    log.append(a.clone())
    return a
  eager = {r.seed: _key(r) for r in m['eval_lib'].eval_agent_vec(rec, suite, capture_graph=False)}
  captured = {r.seed: _key(r) for r in m['eval_lib'].eval_agent_vec(agent, suite, capture_graph=True)}
  assert eager == captured
  perm = list(np.random.default_rng(0).permutation(64))
  permuted = {r.seed: _key(r) for r in m['eval_lib'].eval_agent_vec(agent, m['suites'].EvaluationSuite([seeds[j] for j in perm], T))}
  assert captured == permuted
  # a 63 + 1 split, over one shared wind field as test_gpu_eval.test_seed_independence flies it (the generative fields are decoded
  # by library GEMMs, whose bits may change with the batch size)
  import helpers
  from balloon_learning_environment_amd.env import grid_based_wind_field
  field = helpers.fixture_field(helpers.golden('f13_station_seeker'))
  wf = grid_based_wind_field.GridBasedWindField(_fixed_sampler(field), 'cuda:0')
  wf.set_field(field)
  ev = lambda ss, **kw: {r.seed: _key(r) for r in m['eval_lib'].eval_agent_vec(agent, m['suites'].EvaluationSuite(ss, T), wind_field=wf,
                                                                               **kw)}
  one = ev(seeds)
  assert one == ev([seeds[j] for j in perm]) == ev(seeds, batch_size=63)
  counts = np.bincount(torch.stack(log).cpu().numpy().ravel(), minlength=3)
  assert (counts > 0).all(), counts                 # a real policy: every action is taken somewhere
  print(f'eval_agent_vec with a (8, 600, 51) network: 64 seeds x {T} steps: eager == captured == permuted; shared field: '
        f'one batch == permuted == 63 + 1; '
        f'actions {counts.tolist()}, mean reward {np.mean([v[1] for v in captured.values()]):.3f}')


def test_seed_contract_with_quantile_agent(mods):
  """Seed s of eval_agent_vec flies the first episode of VecBalloonEnv(1, seed=s, ...) driven by the serial QuantileAgent."""
  m = mods
  from balloon_learning_environment_amd.env import balloon_env
  network = m['qnet'].QNetwork.from_params(m['params'])
  seeds, T = [11, 4242, 90001], 60
  batch = seeds + [5, 6, 7, 8, 9]
  res = {r.seed: r for r in m['eval_lib'].eval_agent_vec(m['qnet'].VecQNetworkAgent(network),
                                                          m['suites'].EvaluationSuite(batch, T))}
  agent = m['qa'].QuantileAgent(3, [1099], params=network)
  for s in seeds:
    env = balloon_env.VecBalloonEnv(1, seed=s, per_env_fields=True, auto_reset=False)
    obs = env.reset()
    action = agent.begin_episode(obs)
    total, final, inside = 0.0, 0, 0
    for t in range(T):
      obs, reward, terminal = env.step(torch.tensor([action], dtype=torch.uint8, device='cuda'))
      action = agent.step(float(reward[0]), obs)
      st = env.arena.sim.get_state()
      total += float(reward.cpu().numpy()[0])
      inside += (float(st['x'][0]) ** 2 + float(st['y'][0]) ** 2) ** 0.5 <= 50_000.0
      final = t + 1
      if int(st['status'][0]) != 0:
        break
    assert res[s].cumulative_reward == total and res[s].final_timestep == final, s
    assert res[s].time_within_radius == inside / final
  print(f'seed contract with QuantileAgent: seeds {seeds} x {T} steps equal to VecBalloonEnv(1, seed=s)')


def test_serial_eval_agent_with_perciatelli44(mods, tmp_path):
  from balloon_learning_environment_amd.env import balloon_env
  m = mods
  env = balloon_env.BalloonEnv(seed=0)
  agent = m['p44'].Perciatelli44(3, [1099], params=m['params'])
  res = m['eval_lib'].eval_agent(agent, env, m['suites'].EvaluationSuite([5, 6], 12), calculate_flight_path=True)
  assert [r.seed for r in res] == [5, 6]
  for r in res:
    assert r.final_timestep == 12 and len(r.flight_path) == 12 and 0.0 <= r.time_within_radius <= 1.0
  path = tmp_path / 'p44.npz'
  agent.network.save_npz(path)
  again = m['eval_lib'].eval_agent(m['p44'].Perciatelli44(3, [1099], params_path=path), env, m['suites'].EvaluationSuite([6], 12),
                                   calculate_flight_path=False)
  assert _key(again[0]) == _key(res[1])
  with pytest.raises(NotImplementedError):
    agent.set_mode('train')
