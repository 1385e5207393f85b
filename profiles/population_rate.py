"""Rates of the population primitives, every leg beside the existing call in the same process, and that call timed again
afterwards (the distance between its two timings is the noise a ratio has to be read against):

 * ble_qnet_forward_grouped_f32 at (P, R) = (1, 65 536) beside ble_qnet_forward_f32 at 65 536 rows, a (3, 256, 1) network;
 * the grouped forward at (256, 256) and (2 048, 32) -- 65 536 rows each -- where every image (1.46 MB) serves 256 and 32 rows;
 * ble_es_perturb_f32 and ble_es_gradient_f32 (+ ble_qnet_apply_grad_f32) at P = 256;
 * one generation of run_es_loop_vec at P = 256, S = 16, 960 steps: the flight against the update;
 * a single-run report, not a gate: the small_eval score of the greedy centre after a stated ES budget from init_params' seed 0.

Device events around every single call, the median of 21 calls after 5 warm-up calls (microseconds); the generation by the host clock
around calls that end in their own synchronisation.  One JSON line per measurement.

  python profiles/population_rate.py [--quick] > profiles/population_rate.jsonl
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
from balloon_learning_environment_amd.agents import evolution, population, qnet  # noqa: E402
from balloon_learning_environment_amd.eval import eval_lib, suites  # noqa: E402

LAYERS, HIDDEN = 3, 256
SHAPE = [LAYERS, HIDDEN, 1]


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


def emit(**row):
  print(json.dumps(row), flush=True)


def _network(seed=0):
  return qnet.QNetwork.from_params(qnet.init_params('mlp', seed, LAYERS, HIDDEN))


def forward_rates(n):
  obs = torch.from_numpy(np.random.default_rng(1).random((n, 1099), dtype=np.float32)).cuda()
  out = torch.zeros(n, dtype=torch.uint8, device='cuda')
  plain = qnet.VecQNetworkAgent(_network())
  before = timed(lambda: plain.act(obs, out=out))
  emit(what='VecQNetworkAgent.act (ble_qnet_forward_f32)', shape=SHAPE, n=n, **before)
  legs = []
  for members in (1, 256, 2048):
    pop = population.QNetworkPopulation(_network(), members)
    agent = population.VecPopulationAgent(pop, n // members)
    t = timed(lambda: agent.act(obs, out=out))
    legs.append((members, t))
    del agent, pop
    torch.cuda.empty_cache()
  after = timed(lambda: plain.act(obs, out=out))
  emit(what='VecQNetworkAgent.act (ble_qnet_forward_f32), timed again', shape=SHAPE, n=n, **after,
       vs_first=after['median_us'] / before['median_us'])
  image_mb = _network().packed_host.nbytes / 1e6
  for members, t in legs:
    emit(what='VecPopulationAgent.act (ble_qnet_forward_grouped_f32)', shape=SHAPE, members=members, rows_per_member=n // members, **t,
         vs_plain_before=t['median_us'] / before['median_us'], vs_plain_after=t['median_us'] / after['median_us'],
         images_mb=members * image_mb, images_gb_per_s=members * image_mb / 1e3 / (t['median_us'] * 1e-6))


def es_rates(members):
  es = evolution.ESTrainer(_network(), members)
  fitness = torch.from_numpy(np.random.default_rng(2).standard_normal(members).astype(np.float32)).cuda()
  perturb = timed(es.perturb)
  emit(what='ESTrainer.perturb (ble_es_perturb_f32)', shape=SHAPE, members=members, parameters=int(sum(k.size + b.size for k, b in
       zip(es.network().kernels, es.network().biases))), **perturb)
  emit(what='ESTrainer.update (ranks in torch, ble_es_gradient_f32, ble_qnet_apply_grad_f32)', shape=SHAPE, members=members,
       **timed(lambda: es.update(fitness)))
  w = es.shape_fitness(fitness).contiguous()
  emit(what='ESTrainer.estimate (ble_es_gradient_f32 + the generation advance)', shape=SHAPE, members=members, **timed(lambda: es.estimate(w)))
  emit(what='ESTrainer.apply_grad (ble_qnet_apply_grad_f32)', shape=SHAPE, members=members, **timed(es.apply_grad))
  emit(what='ESTrainer.perturb (ble_es_perturb_f32), timed again', shape=SHAPE, members=members, **timed(es.perturb))


def generation_rate(members, per, steps, generations):
  """One generation by difference: a call of 1 + generations generations less a call of one (both build their evaluator and capture
  their graph once), by the host clock."""
  es = evolution.ESTrainer(_network(), members, sigma=0.02, lr=1e-2, seed=0)

  def run(count, first_seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = train_lib.run_es_loop_vec(es, num_generations=count, seeds_per_member=per, max_episode_length=steps, first_seed=first_seed)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, stats

  run(1, 0)                                    # warm-up
  one, _ = run(1, 1000)
  many, stats = run(1 + generations, 2000)
  whole = (many - one) / generations
  fitness = stats[-1]['fitness']
  update = timed(lambda: (es.perturb(), es.update(fitness)), iters=11, warmup=2)
  emit(what='run_es_loop_vec, one generation (a call of 1 + generations less a call of 1)', shape=SHAPE, members=members,
       seeds_per_member=per, steps=steps, generations=generations, seconds_per_generation=whole, seconds_first_generation=one,
       perturb_and_update_us=update['median_us'], update_share=update['median_us'] * 1e-6 / whole,
       transitions_per_s=(stats[-1]['transitions'] / (1 + generations)) / whole)


def learning_report(members, per, generations):
  """The small_eval score (the mean cumulative reward over seeds 0 .. 99, 960 steps) of the greedy centre before and after the budget."""
  es = evolution.ESTrainer(_network(0), members, sigma=0.02, lr=1e-2, seed=0)
  suite = suites.get_eval_suite('small_eval')
  score = lambda: float(np.mean([r.cumulative_reward for r in eval_lib.eval_agent_vec(qnet.VecQNetworkAgent(es.network()), suite)]))
  before = score()
  t0 = time.perf_counter()
  stats = train_lib.run_es_loop_vec(es, num_generations=generations, seeds_per_member=per, max_episode_length=960, first_seed=10_000)
  seconds = time.perf_counter() - t0
  emit(what='ES budget report (single run, not a gate)', shape=SHAPE, members=members, seeds_per_member=per, generations=generations,
       sigma=0.02, lr=1e-2, seconds=seconds, transitions=stats[-1]['transitions'], small_eval_before=before, small_eval_after=score(),
       mean_fitness_first=stats[0]['mean_fitness'], mean_fitness_last=stats[-1]['mean_fitness'],
       reference_points={'untrained': 203, "StationSeeker's clone": 457, 'StationSeeker': 732})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='small shapes: a check that the script runs')
  args = ap.parse_args()
  if args.quick:
    forward_rates(4096)
    es_rates(8)
    generation_rate(4, 2, 20, 2)
    learning_report(4, 2, 1)
    return
  forward_rates(65536)
  es_rates(256)
  generation_rate(256, 16, 960, 3)
  learning_report(256, 16, 20)


if __name__ == '__main__':
  main()
