"""Rates and scores of the learned terminal value, each beside the existing path it extends, in one process:

 * the rollout with and without leaves (rollout_plans(leaves=) beside rollout_plans()) at (N, K, H) = (4 096, 64, 24) and
   (65 536, 4, 24), in the forecast and in the belief;
 * the leaf observation per row (observe_leaves over 4 096 x 16 = 65 536 leaves) beside observe(append=False, carry_factor=False) per
   row on a simulator of 65 536 environments in the same states with the same rings: the same refit kernel on the same inputs;
 * one decision of VecLookaheadAgent with and without leaf_value at (4 096, 16, 24) and (4 096, 64, 24), wind='belief', and its parts
   (the critic over n K rows, ble_plan_bootstrap_f32) alone;
 * does it help: the network of §3o's run_exit_loop_vec budget (same seeds and hyperparameters, except value_coef = 0.5: §3o's run
   left the value column untrained), then on small_eval the planner at K = 16, wind='belief', H = 24 and H = 8, each with and without
   that network as leaf_value.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds); the loop and the evaluations by
the host clock around the whole call, one call each.  One JSON line per measurement.

  python profiles/leaf_rate.py [--quick] [--skip-scores] > profiles/leaf_rate.jsonl
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from balloon_learning_environment_amd import _abi, _lib, device as dev, train_lib  # noqa: E402
from balloon_learning_environment_amd.agents import actor_critic, expert_iteration, lookahead_agent, qnet  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402
from balloon_learning_environment_amd.eval import eval_lib, suites  # noqa: E402

LAYERS, HIDDEN = 3, 256
STRENGTH, TEMPERATURE, VALUE_COEF = 64, 0.25, 0.5


def timed(call, iters=21, warmup=5):
  """Microseconds of each of `iters` calls, by a pair of device events around every call: median, min and max."""
  for _ in range(warmup):
    call()
  torch.cuda.synchronize()
  pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
  for a, b in pairs:
    a.record()
    call()
    b.record()
  torch.cuda.synchronize()
  us = np.array([a.elapsed_time(b) * 1e3 for a, b in pairs])
  return {'median_us': float(np.median(us)), 'min_us': float(us.min()), 'max_us': float(us.max()), 'calls': iters}


def _actor_critic(seed=0):
  return qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', seed, LAYERS, HIDDEN), num_atoms=2)


def _env(n, steps):
  env = balloon_env.VecBalloonEnv(n, seed=0, auto_reset=False)
  obs = env.reset()
  g = torch.Generator(device='cuda').manual_seed(0)
  for _ in range(steps):
    obs, _, _ = env.step(torch.randint(0, 3, (n,), dtype=torch.uint8, device='cuda', generator=g))
  return env, obs, g


def rollout_rates(n, k, h):
  env, _, g = _env(n, 3)
  sim = env.arena.sim
  plans = torch.randint(0, 3, (h, n, k), dtype=torch.uint8, device='cuda', generator=g)
  out = (torch.empty(n, k, device='cuda'), torch.empty(n, k, dtype=torch.int32, device='cuda'), None, None)
  arena = sim.leaf_arena(k)
  belief = sim.fit_wind_belief()
  base = {'num_envs': n, 'num_plans': k, 'horizon': h}
  rows = []
  for wind, kw in (('forecast', {}), ('belief', {'belief': belief})):
    trio = [{'what': f'rollout_plans, {wind}', **base, **timed(lambda: sim.rollout_plans(plans, 0.993, out=out, **kw))},
            {'what': f'rollout_plans(leaves=), {wind}', **base, **timed(lambda: sim.rollout_plans(plans, 0.993, out=out, leaves=arena, **kw))},
            {'what': f'rollout_plans, {wind}, again', **base, **timed(lambda: sim.rollout_plans(plans, 0.993, out=out, **kw))}]
    trio[1]['vs_plain'] = trio[1]['median_us'] / trio[0]['median_us']
    trio[2]['vs_first'] = trio[2]['median_us'] / trio[0]['median_us']
    rows += trio
  return rows


def observe_rates(n, k, steps):
  env, _, g = _env(n, steps)
  sim = env.arena.sim
  plans = torch.randint(0, 3, (6, n, k), dtype=torch.uint8, device='cuda', generator=g)
  arena = sim.leaf_arena(k)
  sim.rollout_plans(plans, 0.993, leaves=arena)
  rows_n = n * k
  obs = torch.empty(rows_n, _lib.OBS_DIM, device='cuda')
  # the arena as a simulator of its own, with the parents' rings repeated K times: what observe() refits is what observe_leaves refits
  arena._allocate_history(False)
  for name, t in arena._gp.items():
    t.copy_(sim._gp[name].repeat_interleave(k, 0))
  base = {'rows': rows_n, 'num_envs': n, 'num_plans': k, 'observations_in_the_ring': int(sim._gp['count'].max().item())}
  rows = [{'what': 'observe(append=False, carry_factor=False)', **base, **timed(lambda: arena.observe(append=False, carry_factor=False, out=obs))},
          {'what': 'observe_leaves', **base, **timed(lambda: sim.observe_leaves(arena, out=obs))},
          {'what': 'observe(append=False, carry_factor=False), again', **base,
           **timed(lambda: arena.observe(append=False, carry_factor=False, out=obs))}]
  for r in rows:
    r['ns_per_row'] = r['median_us'] * 1e3 / rows_n
  rows[1]['vs_observe'] = rows[1]['median_us'] / rows[0]['median_us']
  rows[2]['vs_first'] = rows[2]['median_us'] / rows[0]['median_us']
  return rows


def decision_rates(n, k, h, steps):
  env, obs, _ = _env(n, steps)
  critic = actor_critic.VecActorCriticAgent(_actor_critic(1))
  kw = dict(num_plans=k, horizon=h, wind='belief')
  plain = env.planner(**kw)
  boot = env.planner(leaf_value=critic, **kw)
  base = {'num_envs': n, 'num_plans': k, 'horizon': h, 'wind': 'belief', 'critic': [LAYERS, HIDDEN, 2]}
  rows = [{'what': 'VecLookaheadAgent.act, no leaf value', **base, **timed(lambda: plain.act(obs))},
          {'what': 'VecLookaheadAgent.act, leaf_value', **base, **timed(lambda: boot.act(obs))},
          {'what': 'VecLookaheadAgent.act, no leaf value, again', **base, **timed(lambda: plain.act(obs))}]
  rows[1]['vs_plain'] = rows[1]['median_us'] / rows[0]['median_us']
  rows[2]['vs_first'] = rows[2]['median_us'] / rows[0]['median_us']
  sim = env.arena.sim
  stream = dev.stream_ptr(boot.device)
  bs = _abi.BlePlanBootstrap(n, k, 0, boot.gamma, boot.returns.data_ptr(), boot.steps_flown.data_ptr(), boot.leaves.state['status'].data_ptr(),
                             boot.leaf_values.data_ptr(), boot.returns.data_ptr())
  rows.append({'what': 'observe_leaves alone', **base, **timed(lambda: sim.observe_leaves(boot.leaves, out=boot.leaf_obs))})
  rows.append({'what': 'the critic over n K rows alone', **base,
               **timed(lambda: critic.act(boot.leaf_obs, out=boot.leaf_actions, value=boot.leaf_values))})
  rows.append({'what': 'ble_plan_bootstrap_f32 alone', **base, **timed(lambda: _lib.call('ble_plan_bootstrap_f32', ctypes.byref(bs), stream))})
  env.check_errors()
  return rows


def _score(agent):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  res = eval_lib.eval_agent_vec(agent, suites.get_eval_suite('small_eval'))
  torch.cuda.synchronize()
  return {'mean_cumulative_reward': float(np.mean([r.cumulative_reward for r in res])),
          'mean_time_within_radius': float(np.mean([r.time_within_radius for r in res])), 'flights': len(res),
          'eval_wall_s': time.perf_counter() - t0, 'runs': 1}


def value_scores(steps, n, iterations, epochs, batch):
  """§3o's run_exit_loop_vec budget with the value column trained (value_coef 0.5), then the planner with and without it."""
  planner_kw = dict(num_plans=16, horizon=24, wind='belief')
  env = balloon_env.VecBalloonEnv(n, seed=0)
  soft = expert_iteration.SoftBCTrainer(_actor_critic(1), lr=1e-3, temperature=TEMPERATURE, value_coef=VALUE_COEF)
  planner = env.planner(prior_strength=STRENGTH, action_values=True, **planner_kw)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = train_lib.run_exit_loop_vec(env, soft, planner, expert_iteration.VecPlanLabelBuffer(n, steps), num_iterations=iterations,
                                      beta=lambda i: 0.5 ** i, epochs=epochs, batch_size=batch)
  torch.cuda.synchronize()
  by = lambda key: [s[key] for s in stats]
  yield {'what': 'run_exit_loop_vec', 'steps': steps, 'num_envs': n, 'iterations': iterations, 'epochs': epochs, 'batch': batch, 'lr': 1e-3,
         'beta': '0.5 ** i', 'planner': planner_kw, 'prior_strength': STRENGTH, 'temperature': TEMPERATURE, 'value_coef': VALUE_COEF,
         'train_wall_s': time.perf_counter() - t0, 'loss_by_iteration': by('loss'), 'mean_best_return_by_iteration': by('mean_best_return')}
  value = actor_critic.VecActorCriticAgent(soft.network())
  for h in (24, 8):
    kw = dict(planner_kw, horizon=h)
    yield {'what': f'small_eval, the planner, H = {h}', 'planner': kw, **_score(lookahead_agent.VecLookaheadAgent(**kw))}
    yield {'what': f'small_eval, the planner with the trained value at its leaves, H = {h}', 'planner': kw,
           **_score(lookahead_agent.VecLookaheadAgent(leaf_value=value, **kw))}
  yield {'what': 'small_eval, greedy network after expert iteration (value_coef 0.5)', **_score(value)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small shapes and budgets')
  ap.add_argument('--skip-scores', action='store_true', help='the rates only')
  args = ap.parse_args()
  for n, k, h in (((256, 16, 8),) if args.quick else ((4096, 64, 24), (65536, 4, 24))):
    for row in rollout_rates(n, k, h):
      print(json.dumps(row), flush=True)
  for row in observe_rates(*((64, 16, 12) if args.quick else (4096, 16, 60))):
    print(json.dumps(row), flush=True)
  for n, k, h in (((256, 16, 8),) if args.quick else ((4096, 16, 24), (4096, 64, 24))):
    for row in decision_rates(n, k, h, 8 if args.quick else 60):
      print(json.dumps(row), flush=True)
  if not args.skip_scores:
    steps, n, iterations = (8, 256, 2) if args.quick else (32, 4096, 8)
    for row in value_scores(steps, n, iterations, 4, min(4096, steps * n)):
      print(json.dumps(row), flush=True)


if __name__ == '__main__':
  main()
