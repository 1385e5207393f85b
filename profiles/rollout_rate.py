"""Look-ahead rate: VecSimulator.rollout_plans (ble_rollout_f32) next to the two ways of flying the same plans without it.

For every shape (N environments, K plans each; 20 agent steps of 18 substeps per plan) and with / without the in-kernel wind noise:

    rollout     one ble_rollout_f32 launch over the N sources, read in place
    step_n      (a) ble_step_n_f32 on N K environments of a shared grid for the same 20 steps: the same lane code on the same number of
                lanes, the state of the N K environments restored (untimed) before every launch
    workaround  (b) what a caller does today: gather the N sources into the N K simulator with torch indexing (every state tensor and
                the episode counters), then step_n -- timed end to end

Shapes: (4 096, 64), (256, 1 024) and (65 536, 4) on a shared grid, (4 096, 64) on per-environment grids.  Both baselines fly a shared
grid at every shape: N K per-environment grids (83 GB at 4 096 x 64) cannot be replicated, which is part of the point.  Each leg is timed
with HIP events; the median of --reps launches after --warmup is reported.  One JSON line per (shape, noise):

    python profiles/rollout_rate.py [--reps 21] [--warmup 5] [--out profiles/rollout_rate.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balloon_learning_environment_amd import vec_state  # noqa: E402

STEPS, SUBSTEPS, NOISE_SEED = 20, 18, 7
SHAPES = ((4096, 64, False), (256, 1024, False), (65536, 4, False), (4096, 64, True))


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e-3


def median_of(fn, reps, warmup, before=None):
  times = []
  for i in range(warmup + reps):
    if before is not None:
      before()
    t = timed(fn)
    if i >= warmup:
      times.append(t)
  return float(np.median(times)), float(np.min(times)), float(np.max(times))


def run(n, k, per_env, reps, warmup):
  gen = torch.Generator(device='cuda').manual_seed(n + k)
  shared = (torch.rand(vec_state.GRID_SHAPE, device='cuda', generator=gen) * 24.0 - 12.0)
  src = vec_state.VecSimulator(n)
  if per_env:
    src.set_grid(torch.rand((n,) + vec_state.GRID_SHAPE, device='cuda', generator=gen) * 24.0 - 12.0, per_env=True)
  else:
    src.set_grid(shared)
  src.reset_device(3)
  warm = torch.randint(0, 3, (4, n), dtype=torch.uint8, device='cuda', generator=gen)
  src.step_n(warm, torch.zeros(4, n, device='cuda'), torch.zeros(4, n, dtype=torch.uint8, device='cuda'))
  src.check_errors()
  plans = torch.randint(0, 3, (STEPS, n, k), dtype=torch.uint8, device='cuda', generator=gen)
  out = vec_state.Rollout(torch.empty(n, k, device='cuda'), torch.empty(n, k, dtype=torch.int32, device='cuda'), None, None)
  # the N K simulator of the baselines: environment e K + j is a copy of source e
  big = vec_state.VecSimulator(n * k)
  big.set_grid(shared)
  index = torch.arange(n, device='cuda').repeat_interleave(k)
  actions = plans.reshape(STEPS, n * k)
  rewards, terminals = torch.empty(STEPS, n * k, device='cuda'), torch.empty(STEPS, n * k, dtype=torch.uint8, device='cuda')

  def gather():
    for name, t in big.state.items():
      t.copy_(src.state[name][index])
    big.episode.copy_(src.episode[index])
  rows = []
  for noise in (False, True):
    seed = NOISE_SEED if noise else None
    t_roll = median_of(lambda: src.rollout_plans(plans, gamma=0.993, noise_seed=seed, substeps=SUBSTEPS, out=out), reps, warmup)
    t_step = median_of(lambda: big.step_n(actions, rewards, terminals, substeps=SUBSTEPS, noise_seed=seed), reps, warmup, before=gather)
    t_work = median_of(lambda: (gather(), big.step_n(actions, rewards, terminals, substeps=SUBSTEPS, noise_seed=seed)), reps, warmup)
    src.check_errors(); big.check_errors()
    assert int(src.rollout_flags.item()) == 0 and bool(torch.isfinite(out.returns).all())
    env_steps = n * k * STEPS
    rows.append({'n': n, 'k': k, 'grids': 'per_env' if per_env else 'shared', 'noise': noise, 'agent_steps': STEPS, 'substeps': SUBSTEPS,
                 'reps': reps, 'rollout_s': t_roll[0], 'rollout_min_s': t_roll[1], 'rollout_max_s': t_roll[2],
                 'step_n_s': t_step[0], 'step_n_min_s': t_step[1], 'step_n_max_s': t_step[2],
                 'workaround_s': t_work[0], 'workaround_min_s': t_work[1], 'workaround_max_s': t_work[2],
                 'rollout_env_steps_per_s': env_steps / t_roll[0], 'step_n_env_steps_per_s': env_steps / t_step[0],
                 'workaround_env_steps_per_s': env_steps / t_work[0],
                 'rollout_vs_step_n': t_step[0] / t_roll[0], 'rollout_vs_workaround': t_work[0] / t_roll[0],
                 'mean_steps_flown': float(out.steps_flown.float().mean().item())})
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=21)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lines = []
  for n, k, per_env in SHAPES:
    for r in run(n, k, per_env, args.reps, args.warmup):
      lines.append(json.dumps(r))
      print(lines[-1], flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
