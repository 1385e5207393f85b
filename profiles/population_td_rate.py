"""Rates of training a population of replay learners, all legs in one process, population_train_rate.py's method:

 * the grouped update (sample + ble_qnet_td_step_grouped_f32) replayed from ONE captured graph, an (8, 600, 51) network under the
   quantile loss and an (8, 600, 1) network under DQN's 'mse', each at (P, B) = (1, 32), (16, 32), (64, 32) and (16, 256), beside
     (a) P sequential captured plain updates of B rows (P trainers, P graphs of sample + ble_qnet_train_step_f32 /
         ble_qnet_td_step_f32, replayed back to back): the parent's path for the same work, and
     (b) one plain captured update of P * B rows (one network: not the same work, the same rows), timed twice -- the distance between
         its two timings is the run-to-run spread a ratio has to be read against;
   the sides alternate call by call (grouped, a, b, b again, grouped, ...), so a drift of the clocks falls on all of them alike;
 * the grouped sampler (ble_replay_sample_grouped_f32) at (P, R, B) = (16, 256, 32) beside 16 plain sampler calls of 32 rows, and the
   grouped epsilon-greedy (ble_qnet_explore_grouped_u8) at (16, 256) beside one plain call over the 4 096 rows; eager calls;
 * one iteration of run_population_training_loop_vec at (P, R) = (16, 256) on a VecBalloonEnv of 4 096 environments, the (8, 600, 51)
   quantile network, 8 steps of 64 grouped updates of 32 rows per member each, by the host clock around iterations that end in their
   own synchronisation.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds).  One JSON line per measurement.

  python profiles/population_td_rate.py [--quick] > profiles/population_td_rate.jsonl
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
from balloon_learning_environment_amd.agents import dqn_agent, population, qnet, qnet_train  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402
from profiles.population_train_rate import emit, timed_alternating  # noqa: E402

LAYERS, HIDDEN = 8, 600
KINDS = {'quantile': 51, 'dqn_mse': 1}                   # the loss kind and its network's atoms
COLUMNS = 16                                             # ring columns per member of the update legs (the cost is the batch's, not the ring's)


def network(atoms, seed=0):
  return qnet.QNetwork.from_params(qnet.init_params('quantile', seed, LAYERS, HIDDEN, atoms), num_atoms=atoms)


def fill(rp, rng, steps=24):
  """`steps` random vector steps in a ring, no episode ends (every window valid: the first draw is taken)."""
  n = rp.num_envs
  for _ in range(steps):
    rp.add(torch.from_numpy(rng.random((n, 1099), dtype=np.float32)).cuda(), torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)).cuda(),
           torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda(), torch.zeros(n, dtype=torch.uint8, device='cuda'))
  return rp


def solo_trainer(kind, atoms):
  if kind == 'quantile':
    return qnet_train.QNetworkTrainer(network(atoms), lr=1e-5)
  return dqn_agent.DQNTrainer(network(atoms), loss_type=kind[len('dqn_'):], lr=1e-5)


def update_legs(kind, members, rows, rng):
  atoms = KINDS[kind]
  grouped = population.PopulationQTrainer(population.QNetworkPopulation(network(atoms), members), kind=kind, lr=1e-5)
  grp = fill(qnet_train.VecPopulationReplayBuffer(members, COLUMNS, 32), rng)
  grouped.capture(grp, rows)
  srp = fill(qnet_train.VecReplayBuffer(COLUMNS, 32), rng)          # (one ring serves the P trainers: its contents do not set the cost)
  solo = [solo_trainer(kind, atoms) for _ in range(members)]
  for t in solo:
    t.capture(srp, rows)
  plain = solo_trainer(kind, atoms)
  prp = fill(qnet_train.VecReplayBuffer(COLUMNS, 32), rng)
  plain.capture(prp, members * rows)

  def sequential():
    for t in solo:
      t.train_step(srp, rows)
  got = timed_alternating({'grouped': lambda: grouped.train_step(grp, rows), 'sequential': sequential,
                           'plain': lambda: plain.train_step(prp, members * rows), 'plain_again': lambda: plain.train_step(prp, members * rows)})
  lay = grouped.workspace(rows)[1]
  shape = [LAYERS, HIDDEN, atoms]
  for k, v in got.items():
    emit(leg='td_update', kind=kind, side=k, members=members, rows_per_member=rows, rows=members * rows, shape=shape, slabs=int(lay.slabs),
         graphs_per_call=members if k == 'sequential' else 1, **v)
  g, s, b, b2 = (got[k]['median_us'] for k in ('grouped', 'sequential', 'plain', 'plain_again'))
  emit(leg='td_update', kind=kind, side='ratios', members=members, rows_per_member=rows, grouped_over_sequential=g / s,
       grouped_over_plain=g / b, plain_again_over_plain=b2 / b)
  for t in (grouped, plain, grp, srp, prp, *solo):
    t.check_errors()


def sampler_and_explore_legs(rng, members=16, columns=256, rows=32):
  grp = fill(qnet_train.VecPopulationReplayBuffer(members, columns, 32), rng)
  solo = [fill(qnet_train.VecReplayBuffer(columns, 32), rng, steps=6) for _ in range(2)]      # (two rings in turn serve the P calls)
  seeds = qnet_train.member_seeds(0, members, 'cuda')
  counter = torch.zeros(1, dtype=torch.int64, device='cuda')

  def sequential():
    for p in range(members):
      solo[p & 1].sample(rows, p, counter)
  got = timed_alternating({'grouped': lambda: grp.sample(rows, seeds, counter), 'sequential': sequential})
  for k, v in got.items():
    emit(leg='replay_sample', side=k, members=members, columns_per_member=columns, rows_per_member=rows, calls_per_call=members if k == 'sequential' else 1, **v)
  emit(leg='replay_sample', side='ratios', grouped_over_sequential=got['grouped']['median_us'] / got['sequential']['median_us'])
  n = members * columns
  actions = torch.zeros(n, dtype=torch.uint8, device='cuda')
  eps = torch.linspace(0.0, 0.4, members, device='cuda')
  got = timed_alternating({'grouped': lambda: qnet_train.explore_grouped(actions, eps, seeds, 3), 'plain': lambda: qnet_train.explore(actions, 0.2, 0, 3),
                           'plain_again': lambda: qnet_train.explore(actions, 0.2, 0, 3)})
  for k, v in got.items():
    emit(leg='explore', side=k, members=members if k == 'grouped' else 1, rows=n, **v)
  emit(leg='explore', side='ratios', grouped_over_plain=got['grouped']['median_us'] / got['plain']['median_us'],
       plain_again_over_plain=got['plain_again']['median_us'] / got['plain']['median_us'])


def loop_leg(members=16, columns=256, steps=8, iterations=3):
  env = balloon_env.VecBalloonEnv(members * columns, seed=0)
  tr = population.PopulationQTrainer(population.QNetworkPopulation(network(51), members), kind='quantile',
                                     lr=[2e-6 * 1.3 ** p for p in range(members)])
  rp = qnet_train.VecPopulationReplayBuffer(members, columns, 64)
  kw = dict(steps_per_iteration=steps, epsilon=[0.4 ** (1 + 7 * p / (members - 1)) for p in range(members)])
  train_lib.run_population_training_loop_vec(env, tr, rp, num_iterations=1, **kw)      # (the lazy allocations, the capture)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = train_lib.run_population_training_loop_vec(env, tr, rp, num_iterations=iterations, **kw)
  torch.cuda.synchronize()
  seconds = (time.perf_counter() - t0) / iterations
  emit(leg='loop_iteration', members=members, columns_per_member=columns, steps=steps, batch_rows_per_member=32, shape=[LAYERS, HIDDEN, 51],
       updates_per_iteration=stats[-1]['updates'], seconds_per_iteration=seconds, transitions_per_second=members * columns * steps / seconds,
       member_updates_per_second=members * stats[-1]['updates'] / seconds, iterations_timed=iterations)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='the two smallest update legs of each kind only')
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  emit(leg='device', name=torch.cuda.get_device_name(0), torch=torch.__version__)
  for kind in KINDS:
    for members, rows in ((1, 32), (16, 32)) if args.quick else ((1, 32), (16, 32), (64, 32), (16, 256)):
      update_legs(kind, members, rows, rng)
      torch.cuda.empty_cache()
  if not args.quick:
    sampler_and_explore_legs(rng)
    loop_leg()


if __name__ == '__main__':
  main()
