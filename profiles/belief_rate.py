"""The belief's rates: the fit (ble_gp_fit_f32) next to the query it was split from, and the look-ahead in the belief
(ble_rollout_belief_f32) next to the look-ahead in the forecast and in the ground-truth noise.

Every environment holds a full window: 120 observations 180 s apart ending at its clock, within 40 km of the balloon, written straight
into the ring (the WindGP's cost does not depend on the values).

    (a) fit       fit_wind_belief against query_wind at q = 16 points (no forecast added), at 4 096 and 65 536 environments
    (b) rollout   rollout_plans(belief=) against rollout_plans() and rollout_plans(noise_seed=), 20 agent steps of 18 substeps per plan,
                  at (N, K) = (4 096, 64) and (65 536, 4) on a shared grid

Each launch is timed with HIP events; the median of --reps launches after --warmup is reported.  One JSON line per leg:

    python profiles/belief_rate.py [--reps 21] [--warmup 5] [--out profiles/belief_rate.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balloon_learning_environment_amd import vec_state  # noqa: E402

STEPS, SUBSTEPS, NOISE_SEED, Q = 20, 18, 7, 16
FIT_SIZES = (4096, 65536)
SHAPES = ((4096, 64), (65536, 4))


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e-3


def median_of(fn, reps, warmup):
  times = [timed(fn) for _ in range(warmup + reps)][warmup:]
  return {'median_s': float(np.median(times)), 'min_s': float(np.min(times)), 'max_s': float(np.max(times))}


def source(n):
  """A simulator four random agent steps into its episodes whose rings hold full windows around the balloons."""
  gen = torch.Generator(device='cuda').manual_seed(n)
  sim = vec_state.VecSimulator(n)
  sim.set_grid(torch.rand(vec_state.GRID_SHAPE, device='cuda', generator=gen) * 24.0 - 12.0)
  sim.reset_device(3)
  warm = torch.randint(0, 3, (4, n), dtype=torch.uint8, device='cuda', generator=gen)
  sim.step_n(warm, torch.zeros(4, n, device='cuda'), torch.zeros(4, n, dtype=torch.uint8, device='cuda'))
  sim.check_errors()
  sim._allocate_history(False)
  gp, s = sim._gp, sim.state
  centre = torch.stack([s['x'], s['y'], torch.zeros_like(s['x'])], -1)[:, None, :]
  spread = torch.rand(n, 120, 3, device='cuda', generator=gen) * torch.tensor([8.0e4, 8.0e4, 9000.0], device='cuda') + \
      torch.tensor([-4.0e4, -4.0e4, 5000.0], device='cuda')
  gp['xyp'][:, :120] = centre + spread
  gp['elapsed_s'][:, :120] = s['time_elapsed_s'][:, None] - 180 * torch.arange(119, -1, -1, device='cuda', dtype=torch.int32)[None, :]
  gp['err_uv'][:, :120] = torch.randn(n, 120, 2, device='cuda', generator=gen) * 2.0
  gp['count'].fill_(120)
  return sim, gen


def run_fit(n, reps, warmup):
  sim, gen = source(n)
  belief = sim.fit_wind_belief()
  spread = torch.rand(n, Q, 3, device='cuda', generator=gen) * torch.tensor([1.0e5, 1.0e5, 9000.0], device='cuda') + \
      torch.tensor([-5.0e4, -5.0e4, 5000.0], device='cuda')
  xyp = (torch.stack([sim.state['x'], sim.state['y'], torch.zeros_like(sim.state['x'])], -1)[:, None, :] + spread).contiguous()
  out = (torch.empty(n, Q, 2, device='cuda'), torch.empty(n, Q, device='cuda'))
  fit = median_of(lambda: sim.fit_wind_belief(out=belief), reps, warmup)
  query = median_of(lambda: sim.query_wind(xyp, add_forecast=False, out=out), reps, warmup)
  wind = median_of(lambda: sim.belief_wind(belief), reps, warmup)
  sim.check_errors()
  assert bool((belief.n_obs == 120).all()) and bool(torch.isfinite(out[0]).all())
  return [{'n': n, 'leg': 'fit', 'reps': reps, **fit, 'fit_vs_query_q16': fit['median_s'] / query['median_s']},
          {'n': n, 'leg': f'query_q{Q}', 'reps': reps, **query},
          {'n': n, 'leg': 'belief_wind', 'reps': reps, **wind}]


def run_rollout(n, k, reps, warmup):
  sim, gen = source(n)
  belief = sim.fit_wind_belief()
  plans = torch.randint(0, 3, (STEPS, n, k), dtype=torch.uint8, device='cuda', generator=gen)
  out = vec_state.Rollout(torch.empty(n, k, device='cuda'), torch.empty(n, k, dtype=torch.int32, device='cuda'), None, None)
  legs = {'forecast': {}, 'noise': {'noise_seed': NOISE_SEED}, 'belief': {'belief': belief}}
  t = {name: median_of(lambda kw=kw: sim.rollout_plans(plans, gamma=0.993, substeps=SUBSTEPS, out=out, **kw), reps, warmup)
       for name, kw in legs.items()}
  sim.check_errors()
  assert int(sim.rollout_flags.item()) == 0 and bool(torch.isfinite(out.returns).all())
  env_steps = n * k * STEPS
  return [{'n': n, 'k': k, 'leg': f'rollout_{name}', 'agent_steps': STEPS, 'substeps': SUBSTEPS, 'reps': reps, **t[name],
           'env_steps_per_s': env_steps / t[name]['median_s'], 'vs_forecast': t[name]['median_s'] / t['forecast']['median_s'],
           'vs_noise': t[name]['median_s'] / t['noise']['median_s']} for name in legs]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=21)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lines = []
  for rows in [run_fit(n, args.reps, args.warmup) for n in FIT_SIZES] + [run_rollout(n, k, args.reps, args.warmup) for n, k in SHAPES]:
    for r in rows:
      lines.append(json.dumps(r))
      print(lines[-1], flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
