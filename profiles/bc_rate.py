"""Rates of imitation beside the on-policy parts it shares its stages with, in one process:

 * one cloning update (BCTrainer.train_on_batch) beside one PPO update (PPOTrainer.train_on_batch) of the same (3, 256, 2) network on
   a given batch of B = 4 096 rows, eager and from the captured graph -- the two differ by the loss kernel;
 * BCTrainer.mix (ble_dagger_mix_u8 and the counter's advance) at n = 4 096 and 65 536;
 * one iteration of run_dagger_loop_vec at (T, N) = (32, 4 096), 1 epoch of B = 4 096, with the StationSeeker expert and with
   venv.planner(num_plans=64, horizon=24), split into collection (the same call with epochs = 0) and updates (the difference);
 * the greedy small_eval score of a clone of each expert after the budget stated in its line, next to the expert's own score, each
   with the wall time of its evaluation.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds); the loop and the evaluations by
the host clock around the whole call (each ends in its own synchronisation), the loop the median of 3 after a warm-up call, an
evaluation one call.  One JSON line per measurement, each with its run count.

  python profiles/bc_rate.py [--quick] > profiles/bc_rate.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from balloon_learning_environment_amd import train_lib  # noqa: E402
from balloon_learning_environment_amd.agents import actor_critic, imitation, lookahead_agent, qnet, station_seeker_agent  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402
from balloon_learning_environment_amd.eval import eval_lib, suites  # noqa: E402

LAYERS, HIDDEN = 3, 256
PLANNER = dict(num_plans=64, horizon=24)


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


def update_rates(b):
  rng = np.random.default_rng(2)
  x = rng.random((b, 1099), dtype=np.float32)
  act = rng.integers(0, 3, b)
  pb = actor_critic.PPOBatch.from_tensors(x, rng.standard_normal(b), act, np.full(b, -1.1), rng.standard_normal(b), 'cuda')
  ppo = actor_critic.PPOTrainer(_actor_critic())
  bc = imitation.BCTrainer(_actor_critic())
  bcv = imitation.BCTrainer(_actor_critic(), label_smoothing=0.1, value_coef=0.5)
  base = {'shape': [LAYERS, HIDDEN, 2], 'batch': b}
  rows = [{'what': 'PPOTrainer.train_on_batch eager', **base, **timed(lambda: ppo.train_on_batch(pb))},
          {'what': 'BCTrainer.train_on_batch eager (s = 0, c_v = 0)', **base, **timed(lambda: bc.train_on_batch(pb))},
          {'what': 'BCTrainer.train_on_batch eager (s = 0.1, c_v = 0.5)', **base, **timed(lambda: bcv.train_on_batch(pb))},
          {'what': 'PPOTrainer.train_on_batch eager, again', **base, **timed(lambda: ppo.train_on_batch(pb))}]
  ppo.capture(pb)
  bc.capture(pb)
  rows.append({'what': 'PPOTrainer.train_step graph', **base, **timed(lambda: ppo.train_step(pb))})
  rows.append({'what': 'BCTrainer.train_step graph (s = 0, c_v = 0)', **base, **timed(lambda: bc.train_step(pb))})
  rows[1]['vs_ppo'] = rows[1]['median_us'] / rows[0]['median_us']
  rows[2]['vs_ppo'] = rows[2]['median_us'] / rows[0]['median_us']
  rows[3]['vs_first'] = rows[3]['median_us'] / rows[0]['median_us']
  rows[5]['vs_ppo'] = rows[5]['median_us'] / rows[4]['median_us']
  for t in (ppo, bc, bcv):
    t.check_errors()
  return rows


def mix_rates(n):
  rng = np.random.default_rng(3)
  learner = torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)).cuda()
  expert = torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)).cuda()
  out, took = torch.zeros(n, dtype=torch.uint8, device='cuda'), torch.zeros(n, dtype=torch.uint8, device='cuda')
  tr = imitation.BCTrainer(_actor_critic())
  return {'what': 'BCTrainer.mix (ble_dagger_mix_u8 + the step advance)', 'n': n, **timed(lambda: tr.mix(learner, expert, 0.5, out, took))}


def _expert(name, env):
  return station_seeker_agent.VecStationSeekerAgent() if name == 'station_seeker' else env.planner(**PLANNER)


def loop_rates(name, steps, n, batch, reps):
  env = balloon_env.VecBalloonEnv(n, seed=0)
  tr = imitation.BCTrainer(_actor_critic(), lr=1e-3)
  ro = actor_critic.VecRolloutBuffer(n, steps, 'cuda')
  expert = _expert(name, env)

  def run(epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = train_lib.run_dagger_loop_vec(env, tr, expert, ro, num_iterations=1, beta=0.5, epochs=epochs, batch_size=batch)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, stats[0]['updates']
  run(1)                                                              # warm-up: allocations, the graph capture
  collect = float(np.median([run(0)[0] for _ in range(reps)]))
  whole = [run(1) for _ in range(reps)]
  total = float(np.median([w[0] for w in whole]))
  return {'what': 'run_dagger_loop_vec, one iteration', 'expert': name, 'shape': [LAYERS, HIDDEN, 2], 'steps': steps, 'num_envs': n,
          'batch': batch, 'epochs': 1, 'updates': whole[0][1], 'collect_s': collect, 'update_s': total - collect, 'total_s': total,
          'collect_env_steps_per_s': steps * n / collect, 'ms_per_update': 1e3 * (total - collect) / max(whole[0][1], 1), 'runs': reps}


def _score(agent):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  res = eval_lib.eval_agent_vec(agent, suites.get_eval_suite('small_eval'))
  torch.cuda.synchronize()
  return {'mean_cumulative_reward': float(np.mean([r.cumulative_reward for r in res])),
          'mean_time_within_radius': float(np.mean([r.time_within_radius for r in res])), 'flights': len(res),
          'eval_wall_s': time.perf_counter() - t0, 'runs': 1}


def clone_scores(name, steps, n, iterations, epochs, batch):
  """DAgger from init_params' near-uniform policy: `iterations` iterations of (steps, n), beta = 0.5 ** i, `epochs` epochs of `batch`
  rows, lr 1e-3; then the greedy clone and the expert through small_eval."""
  env = balloon_env.VecBalloonEnv(n, seed=0)
  tr = imitation.BCTrainer(_actor_critic(1), lr=1e-3)
  ro = actor_critic.VecRolloutBuffer(n, steps, 'cuda')
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = train_lib.run_dagger_loop_vec(env, tr, _expert(name, env), ro, num_iterations=iterations, beta=lambda i: 0.5 ** i, epochs=epochs,
                                        batch_size=batch)
  torch.cuda.synchronize()
  train_s = time.perf_counter() - t0
  budget = {'expert': name, 'steps': steps, 'num_envs': n, 'iterations': iterations, 'epochs': epochs, 'batch': batch, 'lr': 1e-3,
            'beta': '0.5 ** i', 'updates': sum(s['updates'] for s in stats), 'labels': steps * n * iterations}
  own = station_seeker_agent.VecStationSeekerAgent() if name == 'station_seeker' else lookahead_agent.VecLookaheadAgent(**PLANNER)
  yield {'what': 'small_eval, greedy clone', **budget, 'train_wall_s': train_s, 'agreement_by_iteration': [s['agreement'] for s in stats],
         'expert_share_by_iteration': [s['expert_share'] for s in stats], **_score(actor_critic.VecActorCriticAgent(tr.network()))}
  if name == 'station_seeker':
    yield {'what': 'small_eval, the untrained network (greedy)', **_score(actor_critic.VecActorCriticAgent(_actor_critic(1)))}
  yield {'what': 'small_eval, the expert itself', 'expert': name, **_score(own)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small loop shapes and budgets')
  args = ap.parse_args()
  for row in update_rates(4096):
    print(json.dumps(row), flush=True)
  for n in (4096, 65536):
    print(json.dumps(mix_rates(n)), flush=True)
  steps, n = (8, 256) if args.quick else (32, 4096)
  for name in ('station_seeker', 'planner'):
    print(json.dumps(loop_rates(name, steps, n, min(4096, steps * n), 3)), flush=True)
  for name, envs, iterations in (('station_seeker', n, 2 if args.quick else 8), ('planner', 256 if args.quick else 1024, 2 if args.quick else 6)):
    for row in clone_scores(name, steps, envs, iterations, 4, min(4096, steps * envs)):
      print(json.dumps(row), flush=True)


if __name__ == '__main__':
  main()
