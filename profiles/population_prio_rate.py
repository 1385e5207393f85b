"""Rates of prioritized replay and Marco Polo exploration for a population of replay learners, all legs in one process,
population_td_rate.py's method:

 * the grouped prioritized train_step (grouped prioritized sample + ble_qnet_td_step_grouped_f32 + grouped set_priority) replayed from
   ONE captured graph, an (8, 600, 51) network under the quantile loss at (P, B) = (1, 32), (16, 32), (64, 32) and (16, 256), beside
     (a) P sequential captured plain prioritized train_steps of B rows (P QNetworkTrainers on a VecPrioritizedReplayBuffer, P graphs of
         sample + ble_qnet_train_step_f32 + set_priority, replayed back to back): the parent's path for the same work, and
     (b) the grouped UNIFORM train_step of the same shape (§3t's graph): what prioritization adds, timed twice -- the distance between
         its two timings is the run-to-run spread a ratio has to be read against;
   the sides alternate call by call, so a drift of the clocks falls on all of them alike;
 * the grouped tree add (ble_replay_tree_add_grouped_f64) per vector step at (P, R) = (16, 256), T = 32, beside 16 plain tree adds
   (ble_replay_tree_add_f64) of 256 columns; eager calls of the entry points (the ring copy of add() is left out on both sides);
 * the grouped explorer (ble_marco_polo_grouped_u8) at 16 x 256 = 4 096 rows beside the plain one over 4 096 rows; eager calls.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds).  One JSON line per measurement.

  python profiles/population_prio_rate.py [--quick] > profiles/population_prio_rate.jsonl
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from balloon_learning_environment_amd import _lib, device as dev  # noqa: E402
from balloon_learning_environment_amd.agents import marco_polo, population, qnet_train  # noqa: E402
from profiles.population_td_rate import COLUMNS, HIDDEN, LAYERS, fill, network  # noqa: E402
from profiles.population_train_rate import emit, timed_alternating  # noqa: E402

ATOMS = 51


def update_legs(members, rows, rng):
  def pop_trainer():
    return population.PopulationQTrainer(population.QNetworkPopulation(network(ATOMS), members), kind='quantile', lr=1e-5)
  grouped, uniform = pop_trainer(), pop_trainer()
  grp = fill(qnet_train.VecPopulationPrioritizedReplayBuffer(members, COLUMNS, 32), rng)
  urp = fill(qnet_train.VecPopulationReplayBuffer(members, COLUMNS, 32), rng)
  grouped.capture(grp, rows)
  uniform.capture(urp, rows)
  srp = fill(qnet_train.VecPrioritizedReplayBuffer(COLUMNS, 32), rng)      # (one ring serves the P trainers: its contents do not set the cost)
  solo = [qnet_train.QNetworkTrainer(network(ATOMS), lr=1e-5) for _ in range(members)]
  for t in solo:
    t.capture(srp, rows)

  def sequential():
    for t in solo:
      t.train_step(srp, rows)
  got = timed_alternating({'grouped_prioritized': lambda: grouped.train_step(grp, rows), 'sequential_prioritized': sequential,
                           'grouped_uniform': lambda: uniform.train_step(urp, rows),
                           'grouped_uniform_again': lambda: uniform.train_step(urp, rows)})
  shape = [LAYERS, HIDDEN, ATOMS]
  for k, v in got.items():
    emit(leg='prio_update', side=k, members=members, rows_per_member=rows, rows=members * rows, shape=shape,
         graphs_per_call=members if k == 'sequential_prioritized' else 1, **v)
  g, s, u, u2 = (got[k]['median_us'] for k in ('grouped_prioritized', 'sequential_prioritized', 'grouped_uniform', 'grouped_uniform_again'))
  emit(leg='prio_update', side='ratios', members=members, rows_per_member=rows, grouped_over_sequential=g / s, prioritized_over_uniform=g / u,
       uniform_again_over_uniform=u2 / u)
  for t in (grouped, uniform, grp, urp, srp, *solo):
    t.check_errors()


def tree_add_leg(rng, members=16, columns=256, capacity=32):
  grp = fill(qnet_train.VecPopulationPrioritizedReplayBuffer(members, columns, capacity), rng, steps=8)
  solo = [fill(qnet_train.VecPrioritizedReplayBuffer(columns, capacity), rng, steps=8) for _ in range(2)]      # (two rings in turn)
  stream = dev.stream_ptr(grp.device)
  g_rp, g_tr = grp.struct(grp.counter), grp._tree
  s_rp = [s.struct(s.counter) for s in solo]

  def grouped():
    _lib.call('ble_replay_tree_add_grouped_f64', ctypes.byref(g_rp), ctypes.byref(g_tr), stream)

  def sequential():
    for p in range(members):
      _lib.call('ble_replay_tree_add_f64', ctypes.byref(s_rp[p & 1]), ctypes.byref(solo[p & 1]._tree), stream)
  got = timed_alternating({'grouped': grouped, 'sequential': sequential})
  for k, v in got.items():
    emit(leg='tree_add', side=k, members=members, columns_per_member=columns, capacity=capacity,
         calls_per_call=members if k == 'sequential' else 1, **v)
  emit(leg='tree_add', side='ratios', grouped_over_sequential=got['grouped']['median_us'] / got['sequential']['median_us'])


def explorer_leg(members=16, columns=256):
  n = members * columns
  grouped = marco_polo.VecPopulationMarcoPoloExploration(members, columns, np.linspace(0.5, 1.0, members), 0)
  plain, again = marco_polo.VecMarcoPoloExploration(n, 0.8, 0), marco_polo.VecMarcoPoloExploration(n, 0.8, 1)
  obs = torch.rand(n, 1099, device='cuda')
  actions = torch.ones(n, dtype=torch.uint8, device='cuda')
  begin = torch.ones(n, dtype=torch.uint8, device='cuda')
  for ex in (grouped, plain, again):                       # every lane in its random walk: the longest path of the kernel
    ex(obs, actions, begin)
    ex.exploratory_episode.fill_(1)
    ex.exploratory_phase.fill_(1)
    ex.phase_clock.fill_(-1000)
  begin.zero_()
  got = timed_alternating({'grouped': lambda: grouped(obs, actions, begin), 'plain': lambda: plain(obs, actions, begin),
                           'plain_again': lambda: again(obs, actions, begin)})
  for k, v in got.items():
    emit(leg='marco_polo', side=k, members=members if k == 'grouped' else 1, rows=n, **v)
  emit(leg='marco_polo', side='ratios', grouped_over_plain=got['grouped']['median_us'] / got['plain']['median_us'],
       plain_again_over_plain=got['plain_again']['median_us'] / got['plain']['median_us'])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='the two smallest update legs only')
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  emit(leg='device', name=torch.cuda.get_device_name(0), torch=torch.__version__)
  for members, rows in ((1, 32), (16, 32)) if args.quick else ((1, 32), (16, 32), (64, 32), (16, 256)):
    update_legs(members, rows, rng)
    torch.cuda.empty_cache()
  tree_add_leg(rng)
  explorer_leg()


if __name__ == '__main__':
  main()
