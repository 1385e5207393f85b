"""Rates and scores of expert iteration, each beside the existing path it extends, in one process:

 * one decision of VecLookaheadAgent with prior_strength = 64 and action_values = True (ble_plan_prior_u16 -> ble_plan_sample_prior_u8 ->
   rollout -> ble_plan_select_f32 -> ble_plan_action_values_f32) beside the same decision without either (today's calls), at
   (N, K, H) = (4 096, 64, 24) and (65 536, 4, 24), wind='forecast'; and the two added kernels alone;
 * one soft update (SoftBCTrainer.train_on_batch) beside one cloning update (BCTrainer.train_on_batch) of the same (3, 256, 2) network
   on B = 4 096 rows, eager and from the captured graph -- the two differ by the loss kernel;
 * does the loop help: 8 iterations of run_exit_loop_vec at (T, N) = (32, 4 096) with the planner at K = 16, H = 24, wind='belief',
   prior_strength = 64; then, on small_eval, that planner without a prior and with the trained network's prior, the network's greedy
   score, and the greedy score of a hard-label DAgger clone of the same planner, budget and seed.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds); the loop and the evaluations by
the host clock around the whole call (each ends in its own synchronisation), one call each.  One JSON line per measurement, each with
its run count.

  python profiles/exit_rate.py [--quick] > profiles/exit_rate.jsonl
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
from balloon_learning_environment_amd.agents import actor_critic, expert_iteration, imitation, lookahead_agent, qnet  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402
from balloon_learning_environment_amd.eval import eval_lib, suites  # noqa: E402

LAYERS, HIDDEN = 3, 256
PLANNER = dict(num_plans=16, horizon=24, wind='belief')
STRENGTH, TEMPERATURE = 64, 0.25


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


def decision_rates(n, k, h):
  env = balloon_env.VecBalloonEnv(n, seed=0, auto_reset=False)
  obs = env.reset()
  g = torch.Generator(device='cuda').manual_seed(0)
  for _ in range(3):
    obs, _, _ = env.step(torch.randint(0, 3, (n,), dtype=torch.uint8, device='cuda', generator=g))
  probs = torch.softmax(torch.randn(n, 3, device='cuda', generator=g), dim=1).contiguous()
  kw = dict(num_plans=k, horizon=h, wind='forecast')
  plain = env.planner(**kw)
  full = env.planner(prior_strength=STRENGTH, action_values=True, **kw)
  base = {'num_envs': n, 'num_plans': k, 'horizon': h, 'wind': 'forecast'}
  rows = [{'what': 'VecLookaheadAgent.act, no prior, no action values', **base, **timed(lambda: plain.act(obs))},
          {'what': 'VecLookaheadAgent.act, prior_strength 64, action_values', **base, **timed(lambda: full.act(obs, prior_probs=probs))},
          {'what': 'VecLookaheadAgent.act, no prior, no action values, again', **base, **timed(lambda: plain.act(obs))}]
  rows[1]['vs_plain'] = rows[1]['median_us'] / rows[0]['median_us']
  rows[2]['vs_first'] = rows[2]['median_us'] / rows[0]['median_us']
  stream = dev.stream_ptr(full.device)
  pr = _abi.BlePlanPrior(n, full.segments, STRENGTH, probs.data_ptr(), full.prior_counts.data_ptr())
  av = _abi.BlePlanActionValues(n, k, 0, full.returns.data_ptr(), full.plans.data_ptr(), full.q.data_ptr(), full.q_k.data_ptr(),
                                full.visits.data_ptr())
  rows.append({'what': 'ble_plan_prior_u16 alone', **base, **timed(lambda: _lib.call('ble_plan_prior_u16', ctypes.byref(pr), stream))})
  rows.append({'what': 'ble_plan_action_values_f32 alone', **base,
               **timed(lambda: _lib.call('ble_plan_action_values_f32', ctypes.byref(av), stream))})
  env.check_errors()
  return rows


def update_rates(b):
  rng = np.random.default_rng(2)
  x = rng.random((b, 1099), dtype=np.float32)
  act = rng.integers(0, 3, b)
  pb = actor_critic.PPOBatch.from_tensors(x, rng.standard_normal(b), act, np.full(b, -1.1), rng.standard_normal(b), 'cuda')
  sb = expert_iteration.SoftBatch.from_tensors(x, rng.standard_normal((b, 3)), rng.standard_normal(b), 'cuda')
  bc = imitation.BCTrainer(_actor_critic())
  soft = expert_iteration.SoftBCTrainer(_actor_critic(), temperature=TEMPERATURE)
  softv = expert_iteration.SoftBCTrainer(_actor_critic(), temperature=TEMPERATURE, label_smoothing=0.1, value_coef=0.5)
  base = {'shape': [LAYERS, HIDDEN, 2], 'batch': b}
  rows = [{'what': 'BCTrainer.train_on_batch eager (s = 0, c_v = 0)', **base, **timed(lambda: bc.train_on_batch(pb))},
          {'what': 'SoftBCTrainer.train_on_batch eager (s = 0, c_v = 0)', **base, **timed(lambda: soft.train_on_batch(sb))},
          {'what': 'SoftBCTrainer.train_on_batch eager (s = 0.1, c_v = 0.5)', **base, **timed(lambda: softv.train_on_batch(sb))},
          {'what': 'BCTrainer.train_on_batch eager, again', **base, **timed(lambda: bc.train_on_batch(pb))}]
  bc.capture(pb)
  soft.capture(sb)
  rows.append({'what': 'BCTrainer.train_step graph (s = 0, c_v = 0)', **base, **timed(lambda: bc.train_step(pb))})
  rows.append({'what': 'SoftBCTrainer.train_step graph (s = 0, c_v = 0)', **base, **timed(lambda: soft.train_step(sb))})
  rows[1]['vs_bc'] = rows[1]['median_us'] / rows[0]['median_us']
  rows[2]['vs_bc'] = rows[2]['median_us'] / rows[0]['median_us']
  rows[3]['vs_first'] = rows[3]['median_us'] / rows[0]['median_us']
  rows[5]['vs_bc'] = rows[5]['median_us'] / rows[4]['median_us']
  for t in (bc, soft, softv):
    t.check_errors()
  return rows


def _score(agent):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  res = eval_lib.eval_agent_vec(agent, suites.get_eval_suite('small_eval'))
  torch.cuda.synchronize()
  return {'mean_cumulative_reward': float(np.mean([r.cumulative_reward for r in res])),
          'mean_time_within_radius': float(np.mean([r.time_within_radius for r in res])), 'flights': len(res),
          'eval_wall_s': time.perf_counter() - t0, 'runs': 1}


def loop_scores(steps, n, iterations, epochs, batch):
  """Expert iteration and hard-label DAgger from the same near-uniform policy (init_params seed 1), environments (seed 0), planner,
  beta = 0.5 ** i, lr 1e-3 and budget; then small_eval."""
  budget = {'steps': steps, 'num_envs': n, 'iterations': iterations, 'epochs': epochs, 'batch': batch, 'lr': 1e-3, 'beta': '0.5 ** i',
            'planner': PLANNER, 'labels': steps * n * iterations}
  env = balloon_env.VecBalloonEnv(n, seed=0)
  soft = expert_iteration.SoftBCTrainer(_actor_critic(1), lr=1e-3, temperature=TEMPERATURE)
  planner = env.planner(prior_strength=STRENGTH, action_values=True, **PLANNER)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = train_lib.run_exit_loop_vec(env, soft, planner, expert_iteration.VecPlanLabelBuffer(n, steps), num_iterations=iterations,
                                      beta=lambda i: 0.5 ** i, epochs=epochs, batch_size=batch)
  torch.cuda.synchronize()
  exit_s = time.perf_counter() - t0
  env = balloon_env.VecBalloonEnv(n, seed=0)
  hard = imitation.BCTrainer(_actor_critic(1), lr=1e-3)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  dagger = train_lib.run_dagger_loop_vec(env, hard, env.planner(**PLANNER), actor_critic.VecRolloutBuffer(n, steps, 'cuda'),
                                         num_iterations=iterations, beta=lambda i: 0.5 ** i, epochs=epochs, batch_size=batch)
  torch.cuda.synchronize()
  dagger_s = time.perf_counter() - t0
  by = lambda rows, key: [s[key] for s in rows]
  yield {'what': 'run_exit_loop_vec', **budget, 'prior_strength': STRENGTH, 'temperature': TEMPERATURE, 'train_wall_s': exit_s,
         'updates': sum(by(stats, 'updates')), 'agreement_by_iteration': by(stats, 'agreement'), 'loss_by_iteration': by(stats, 'loss'),
         'mean_best_return_by_iteration': by(stats, 'mean_best_return'), 'time_within_radius_by_iteration': by(stats, 'time_within_radius')}
  yield {'what': 'run_dagger_loop_vec (hard labels)', **budget, 'train_wall_s': dagger_s, 'updates': sum(by(dagger, 'updates')),
         'agreement_by_iteration': by(dagger, 'agreement'), 'time_within_radius_by_iteration': by(dagger, 'time_within_radius')}
  policy = actor_critic.VecActorCriticAgent(soft.network())
  yield {'what': 'small_eval, the planner without a prior', 'planner': PLANNER, **_score(lookahead_agent.VecLookaheadAgent(**PLANNER))}
  yield {'what': 'small_eval, the planner with the trained network as its prior', 'planner': PLANNER, 'prior_strength': STRENGTH,
         **_score(expert_iteration.VecPriorPlannerAgent(policy, lookahead_agent.VecLookaheadAgent(prior_strength=STRENGTH, **PLANNER)))}
  yield {'what': 'small_eval, the planner with the untrained network as its prior', 'planner': PLANNER, 'prior_strength': STRENGTH,
         **_score(expert_iteration.VecPriorPlannerAgent(actor_critic.VecActorCriticAgent(_actor_critic(1)),
                                                        lookahead_agent.VecLookaheadAgent(prior_strength=STRENGTH, **PLANNER)))}
  yield {'what': 'small_eval, greedy network after expert iteration', **_score(policy)}
  yield {'what': 'small_eval, greedy hard-label DAgger clone', **_score(actor_critic.VecActorCriticAgent(hard.network()))}
  yield {'what': 'small_eval, the untrained network (greedy)', **_score(actor_critic.VecActorCriticAgent(_actor_critic(1)))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small shapes and budgets')
  args = ap.parse_args()
  for n, k, h in (((256, 16, 8),) if args.quick else ((4096, 64, 24), (65536, 4, 24))):
    for row in decision_rates(n, k, h):
      print(json.dumps(row), flush=True)
  for row in update_rates(4096):
    print(json.dumps(row), flush=True)
  steps, n, iterations = (8, 256, 2) if args.quick else (32, 4096, 8)
  for row in loop_scores(steps, n, iterations, 4, min(4096, steps * n)):
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
  main()
