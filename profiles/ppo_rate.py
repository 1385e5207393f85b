"""Rates of on-policy training beside the parts it is built from, in one process:

 * PPOTrainer.act (ble_ac_act_f32 and the step counter's advance) beside VecQNetworkAgent.act (ble_qnet_forward_f32) of the same
   (layers, hidden, 2) network at n = 4 096 and 65 536 -- the two differ by the head kernel and the counter;
 * one PPO minibatch update on a given batch of B = 4 096 rows beside DQNTrainer's update on a given batch of the same trunk -- the PPO
   update has no target pass;
 * generalised advantage estimation and the advantage normalisation at (T, N) = (32, 4 096) and (16, 65 536);
 * one iteration of run_ppo_loop_vec at those two shapes (4 epochs of B = 4 096), split into collection (the same call with
   epochs = 0: T closed-loop steps, the bootstrap act, GAE and the normalisation) and update (the difference).

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds); the loop by the host clock around
the whole call (it ends in its own synchronisation), the median of 3 after a warm-up call.  One JSON line per measurement.

  python profiles/ppo_rate.py [--quick] > profiles/ppo_rate.jsonl
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
from balloon_learning_environment_amd.agents import actor_critic, dqn_agent, qnet, qnet_train  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402

LAYERS, HIDDEN = 3, 256


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


def _actor_critic():
  return qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', 0, LAYERS, HIDDEN), num_atoms=2)


def act_rates(n):
  rng = np.random.default_rng(1)
  obs = torch.from_numpy(rng.random((n, 1099), dtype=np.float32)).cuda()
  actions = torch.zeros(n, dtype=torch.uint8, device='cuda')
  logp, value = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
  tr = actor_critic.PPOTrainer(_actor_critic())
  greedy = actor_critic.VecActorCriticAgent(_actor_critic())
  vec = qnet.VecQNetworkAgent(_actor_critic())
  base = {'shape': [LAYERS, HIDDEN, 2], 'n': n}
  rows = [{'what': 'VecQNetworkAgent.act (ble_qnet_forward_f32)', **base, **timed(lambda: vec.act(obs, out=actions))},
          {'what': 'PPOTrainer.act (ble_ac_act_f32 sampled + the step advance)', **base, **timed(lambda: tr.act(obs, actions, logp, value))},
          {'what': 'VecActorCriticAgent.act greedy (ble_ac_act_f32)', **base, **timed(lambda: greedy.act(obs, actions, logp, value))}]
  rows[1]['vs_forward'] = rows[1]['median_us'] / rows[0]['median_us']
  rows[2]['vs_forward'] = rows[2]['median_us'] / rows[0]['median_us']
  return rows


def update_rates(b):
  rng = np.random.default_rng(2)
  x, x2 = rng.random((b, 1099), dtype=np.float32), rng.random((b, 1099), dtype=np.float32)
  act = rng.integers(0, 3, b)
  ppo = actor_critic.PPOTrainer(_actor_critic())
  pb = actor_critic.PPOBatch.from_tensors(x, rng.standard_normal(b), act, np.full(b, -1.1), rng.standard_normal(b), 'cuda')
  dqn = dqn_agent.DQNTrainer(qnet.QNetwork.from_params(qnet.init_params('mlp', 0, LAYERS, HIDDEN)))
  db = qnet_train.TrainBatch.from_tensors(x, x2, rng.standard_normal(b), np.full(b, 0.9, np.float32), act, 'cuda')
  base = {'batch': b}
  rows = [{'what': 'DQNTrainer.train_on_batch eager', 'shape': [LAYERS, HIDDEN, 1], **base, **timed(lambda: dqn.train_on_batch(db))},
          {'what': 'PPOTrainer.train_on_batch eager', 'shape': [LAYERS, HIDDEN, 2], **base, **timed(lambda: ppo.train_on_batch(pb))}]
  ppo.capture(pb)
  rows.append({'what': 'PPOTrainer.train_step graph', 'shape': [LAYERS, HIDDEN, 2], **base, **timed(lambda: ppo.train_step(pb))})
  rows[1]['vs_dqn'] = rows[1]['median_us'] / rows[0]['median_us']
  ppo.check_errors()
  dqn.check_errors()
  return rows


def gae_rates(steps, n):
  rng = np.random.default_rng(3)
  ro = actor_critic.VecRolloutBuffer(n, steps, 'cuda')
  ro.reward.copy_(torch.from_numpy(rng.standard_normal((steps, n)).astype(np.float32)))
  ro.value.copy_(torch.from_numpy(rng.standard_normal((steps, n)).astype(np.float32)))
  ro.terminal.copy_(torch.from_numpy((rng.random((steps, n)) < 0.01).astype(np.uint8)))
  ro.episode_end.copy_(ro.terminal)
  boot = torch.zeros(n, device='cuda')
  gae = timed(lambda: ro.finish(boot, 0.993, 0.95, False))
  both = timed(lambda: ro.finish(boot, 0.993, 0.95, True))
  base = {'steps': steps, 'num_envs': n}
  return [{'what': 'GAE (boot_value copy + ble_gae_f32)', **base, **gae},
          {'what': 'GAE + advantage normalisation', **base, **both, 'normalisation_us': both['median_us'] - gae['median_us']}]


def loop_rates(steps, n, batch, reps):
  env = balloon_env.VecBalloonEnv(n, seed=0)
  tr = actor_critic.PPOTrainer(_actor_critic())
  ro = actor_critic.VecRolloutBuffer(n, steps, 'cuda')

  def run(epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = train_lib.run_ppo_loop_vec(env, tr, ro, num_iterations=1, epochs=epochs, batch_size=batch)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, stats[0]['updates']
  run(4)                                                              # warm-up: allocations, the graph capture
  collect = float(np.median([run(0)[0] for _ in range(reps)]))
  whole = [run(4) for _ in range(reps)]
  total = float(np.median([w[0] for w in whole]))
  return {'what': 'run_ppo_loop_vec, one iteration', 'shape': [LAYERS, HIDDEN, 2], 'steps': steps, 'num_envs': n, 'batch': batch, 'epochs': 4,
          'updates': whole[0][1], 'collect_s': collect, 'update_s': total - collect, 'total_s': total,
          'collect_env_steps_per_s': steps * n / collect, 'env_steps_per_s': steps * n / total,
          'ms_per_update': 1e3 * (total - collect) / max(whole[0][1], 1)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='the small shape only')
  args = ap.parse_args()
  shapes = ((32, 4096),) if args.quick else ((32, 4096), (16, 65536))
  for _, n in shapes:
    for row in act_rates(n):
      print(json.dumps(row), flush=True)
  for row in update_rates(4096):
    print(json.dumps(row), flush=True)
  for steps, n in shapes:
    for row in gae_rates(steps, n):
      print(json.dumps(row), flush=True)
  for steps, n in shapes:
    print(json.dumps(loop_rates(steps, n, 4096, 3)), flush=True)


if __name__ == '__main__':
  main()
