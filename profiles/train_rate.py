"""Rates of the device QR-DQN trainer: updates/s of one captured update (sample + train step) at several batch sizes, and
env-steps/s of run_training_loop_vec at the reference's update ratio (one update of 32 rows per 4 transitions).

  python profiles/train_rate.py [--quick]                         # one JSON line per measurement
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/train_rate.py --quick    # the per-kernel shares

The backward TFLOP/s counts the dW and dX GEMMs of the unpadded shapes (2 B K M per layer each, no dX for layer 0) over the time of the
whole update: a lower bound of the backward kernels' own rate."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from balloon_learning_environment_amd import train_lib  # noqa: E402
from balloon_learning_environment_amd.agents import qnet, qnet_train  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402


def _replay(n_env=256, steps=64):
  rng = np.random.default_rng(0)
  rp = qnet_train.VecReplayBuffer(n_env, steps, 5, 0.993)
  for _ in range(steps):
    rp.add(torch.from_numpy(rng.random((n_env, 1099), dtype=np.float32)).cuda(), torch.from_numpy(rng.integers(0, 3, n_env).astype(np.uint8)).cuda(),
           torch.from_numpy(rng.random(n_env, dtype=np.float32)).cuda(), torch.from_numpy((rng.random(n_env) < 0.02).astype(np.uint8)).cuda())
  return rp


def _backward_flops(layers, hidden, atoms, b):
  dims = [1099] + [hidden] * (layers - 1) + [3 * atoms]
  return sum(2 * b * dims[l] * dims[l + 1] * (2 if l > 0 else 1) for l in range(layers))


def update_rate(layers, hidden, atoms, b, rp, iters):
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(qnet.init_params('quantile', 0, layers, hidden, atoms)))
  tr.capture(rp, b)
  for _ in range(5):
    tr.train_step(rp, b)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(iters):
    tr.train_step(rp, b)
  torch.cuda.synchronize()
  dt = (time.perf_counter() - t0) / iters
  tr.check_errors()
  return {'what': 'update', 'shape': [layers, hidden, atoms], 'batch': b, 'ms_per_update': dt * 1e3, 'updates_per_s': 1.0 / dt,
          'backward_tflops_lower_bound': _backward_flops(layers, hidden, atoms, b) / dt / 1e12}


def loop_rate(layers, hidden, atoms, n, steps):
  env = balloon_env.VecBalloonEnv(n, seed=0)
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(qnet.init_params('quantile', 0, layers, hidden, atoms)))
  rp = qnet_train.VecReplayBuffer(n, 64, 5, 0.993)
  kw = dict(max_episode_length=960, min_replay_history=0, update_period=4, target_update_period=100, batch_size=32)
  train_lib.run_training_loop_vec(env, tr, rp, num_iterations=1, steps_per_iteration=8, **kw)      # warm-up (allocations, capture)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = train_lib.run_training_loop_vec(env, tr, rp, num_iterations=1, steps_per_iteration=steps, **kw)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  return {'what': 'loop', 'shape': [layers, hidden, atoms], 'num_envs': n, 'steps': steps, 'env_steps_per_s': n * steps / dt,
          'updates': stats[0]['updates'], 'updates_per_s': stats[0]['updates'] / dt}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='fewer iterations (for a profiler run)')
  args = ap.parse_args()
  iters = 20 if args.quick else 200
  rp = _replay()
  for shape in ((8, 600, 51), (2, 64, 51)):
    for b in (32, 256, 1024, 4096):
      print(json.dumps(update_rate(*shape, b, rp, iters)), flush=True)
    for n in (256, 4096):
      print(json.dumps(loop_rate(*shape, n, 4 if args.quick else 16)), flush=True)


if __name__ == '__main__':
  main()
