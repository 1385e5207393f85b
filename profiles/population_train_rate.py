"""Rates of training a population by gradient, a (3, 256, 2) network, all legs in one process:

 * the grouped PPO update (ble_qnet_ppo_step_grouped_f32) replayed from ONE captured graph at (P, B) = (1, 4 096), (16, 256), (64, 256)
   and (256, 64), each beside
     (a) P sequential captured ble_qnet_ppo_step_f32 updates of B rows (P trainers, P graphs, replayed back to back): the parent's path
         for the same work, and
     (b) one plain captured update of P * B rows (one network: not the same work, the same rows), timed twice -- the distance between
         its two timings is the run-to-run spread a ratio has to be read against;
   the sides alternate call by call (grouped, a, b, b again, grouped, ...), so a drift of the clocks falls on all of them alike;
 * the sampled grouped act (ble_ac_act_grouped_f32) at 65 536 rows, (P, R) = (256, 256), beside ble_ac_act_f32 at 65 536 rows;
 * one iteration of run_pbt_loop_vec at (P, R, T) = (16, 256, 32) on a VecBalloonEnv of 4 096 environments, 4 epochs of B = 256 rows per
   member, by the host clock around iterations that end in their own synchronisation.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds).  One JSON line per measurement.

  python profiles/population_train_rate.py [--quick] > profiles/population_train_rate.jsonl
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
from balloon_learning_environment_amd.agents import actor_critic, population, qnet  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402

LAYERS, HIDDEN = 3, 256
SHAPE = [LAYERS, HIDDEN, 2]


def emit(**row):
  print(json.dumps(row), flush=True)


def timed_alternating(calls, iters=21, warmup=5):
  """{name: stats} of the calls, run in turn `iters` times after `warmup` turns, a pair of device events around every single call."""
  for _ in range(warmup):
    for call in calls.values():
      call()
  torch.cuda.synchronize()
  pairs = {k: [] for k in calls}
  for _ in range(iters):
    for k, call in calls.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      call()
      b.record()
      pairs[k].append((a, b))
  torch.cuda.synchronize()
  out = {}
  for k, p in pairs.items():
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in p])
    out[k] = {'median_us': float(np.median(us)), 'min_us': float(us.min()), 'max_us': float(us.max()), 'calls': iters}
  return out


def network(seed=0):
  return qnet.QNetwork.from_params(actor_critic.init_params('actor_critic', seed, LAYERS, HIDDEN), num_atoms=2)


def fill(bt, rng):
  """Random rows in a batch's static buffers (the update's cost does not depend on the values)."""
  n = bt.state.shape[0]
  bt.state[:, :1099].copy_(torch.from_numpy(rng.random((n, 1099), dtype=np.float32)))
  bt.ret.copy_(torch.from_numpy(rng.standard_normal(n).astype(np.float32)))
  bt.action.copy_(torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)))
  bt.old_logp.copy_(torch.from_numpy((np.log(1 / 3) + 0.1 * rng.standard_normal(n)).astype(np.float32)))
  bt.advantage.copy_(torch.from_numpy(rng.standard_normal(n).astype(np.float32)))
  return bt


def update_legs(members, rows, rng):
  grouped = population.PopulationPPOTrainer(population.QNetworkPopulation(network(), members), lr=1e-4)
  gb = fill(population.PopulationPPOBatch(members, rows, 'cuda'), rng)
  grouped.capture(gb)
  solo = [actor_critic.PPOTrainer(network(), lr=1e-4) for _ in range(members)]
  sb = fill(actor_critic.PPOBatch(rows, 'cuda'), rng)               # (one batch serves the P trainers: its rows do not set the cost)
  for t in solo:
    t.capture(sb)
  plain = actor_critic.PPOTrainer(network(), lr=1e-4)
  pb = fill(actor_critic.PPOBatch(members * rows, 'cuda'), rng)
  plain.capture(pb)

  def sequential():
    for t in solo:
      t.train_step(sb)
  got = timed_alternating({'grouped': lambda: grouped.train_step(gb), 'sequential': sequential, 'plain': lambda: plain.train_step(pb),
                           'plain_again': lambda: plain.train_step(pb)})
  lay = grouped.workspace(rows)[1]
  for k, v in got.items():
    emit(leg='ppo_update', side=k, members=members, rows_per_member=rows, rows=members * rows, shape=SHAPE, slabs=int(lay.slabs),
         graphs_per_call=members if k == 'sequential' else 1, **v)
  g, s, b, b2 = (got[k]['median_us'] for k in ('grouped', 'sequential', 'plain', 'plain_again'))
  emit(leg='ppo_update', side='ratios', members=members, rows_per_member=rows, grouped_over_sequential=g / s, grouped_over_plain=g / b,
       plain_again_over_plain=b2 / b)


def act_legs(rng, members=256, rows=256):
  n = members * rows
  obs = torch.from_numpy(rng.random((n, 1099), dtype=np.float32)).cuda()
  out = torch.zeros(n, dtype=torch.uint8, device='cuda')
  logp, value = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
  grouped = population.PopulationPPOTrainer(population.QNetworkPopulation(network(), members))
  plain = actor_critic.PPOTrainer(network())
  got = timed_alternating({'grouped': lambda: grouped.act(obs, out, logp, value), 'plain': lambda: plain.act(obs, out, logp, value),
                           'plain_again': lambda: plain.act(obs, out, logp, value)})
  for k, v in got.items():
    emit(leg='sampled_act', side=k, members=members if k == 'grouped' else 1, rows=n, shape=SHAPE, **v)
  emit(leg='sampled_act', side='ratios', grouped_over_plain=got['grouped']['median_us'] / got['plain']['median_us'],
       plain_again_over_plain=got['plain_again']['median_us'] / got['plain']['median_us'])


def pbt_leg(members=16, rows=256, steps=32, iterations=3):
  env = balloon_env.VecBalloonEnv(members * rows, seed=0)
  tr = population.PopulationPPOTrainer(population.QNetworkPopulation(network(), members), lr=[1e-4 * 1.3 ** p for p in range(members)])
  ro = actor_critic.VecPopulationRolloutBuffer(members, rows, steps, 'cuda')
  pbt = train_lib.PBTController(members, 'cuda', ready_every=1)
  kw = dict(epochs=4, batch_size=256, ready_every=1, controller=pbt)
  train_lib.run_pbt_loop_vec(env, tr, ro, num_iterations=1, **kw)      # (the lazy allocations, the capture)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = train_lib.run_pbt_loop_vec(env, tr, ro, num_iterations=iterations, **kw)
  torch.cuda.synchronize()
  seconds = (time.perf_counter() - t0) / iterations
  emit(leg='pbt_iteration', members=members, rows_per_member=rows, horizon=steps, epochs=4, batch_rows_per_member=256, shape=SHAPE,
       updates_per_iteration=stats[-1]['updates'], seconds_per_iteration=seconds,
       transitions_per_second=members * rows * steps / seconds, iterations_timed=iterations)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='the two smallest update legs only')
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  emit(leg='device', name=torch.cuda.get_device_name(0), torch=torch.__version__)
  for members, rows in ((1, 4096), (16, 256)) if args.quick else ((1, 4096), (16, 256), (64, 256), (256, 64)):
    update_legs(members, rows, rng)
  if not args.quick:
    act_legs(rng)
    pbt_leg()


if __name__ == '__main__':
  main()
