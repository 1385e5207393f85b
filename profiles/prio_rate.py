"""Rates of prioritized replay and Marco Polo exploration: the tree add per vector step, a captured prioritized update
(sample + train step + set_priority) against the uniform one, and run_training_loop_vec env-steps/s with both features.

  python profiles/prio_rate.py [--quick]                          # one JSON line per measurement
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
from balloon_learning_environment_amd.agents import marco_polo, qnet, qnet_train  # noqa: E402
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402


def _fill(cls, n_env=256, steps=64):
  rng = np.random.default_rng(0)
  rp = cls(n_env, steps, 5, 0.993)
  for _ in range(steps):
    rp.add(torch.from_numpy(rng.random((n_env, 1099), dtype=np.float32)).cuda(), torch.from_numpy(rng.integers(0, 3, n_env).astype(np.uint8)).cuda(),
           torch.from_numpy(rng.random(n_env, dtype=np.float32)).cuda(), torch.from_numpy((rng.random(n_env) < 0.02).astype(np.uint8)).cuda())
  return rp


def tree_add_rate(n_env, capacity, iters):
  """The tree add alone (the ring's own copies excluded): the add kernel relaunched on a full ring."""
  import ctypes
  from balloon_learning_environment_amd import _lib, device as dev
  rp = _fill(qnet_train.VecPrioritizedReplayBuffer, n_env, capacity)
  st = rp.struct(rp.counter)
  lib, stream = _lib.lib(), dev.stream_ptr(rp.device)
  for _ in range(5):
    lib.ble_replay_tree_add_f64(ctypes.byref(st), ctypes.byref(rp._tree), stream)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(iters):
    lib.ble_replay_tree_add_f64(ctypes.byref(st), ctypes.byref(rp._tree), stream)
  torch.cuda.synchronize()
  dt = (time.perf_counter() - t0) / iters
  return {'what': 'tree_add', 'num_envs': n_env, 'capacity_steps': capacity, 'leaves': n_env * capacity, 'us_per_add': dt * 1e6}


def update_rate(shape, b, rp, iters):
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(qnet.init_params('quantile', 0, *shape)))
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
  rp.check_errors()
  return dt


def loop_rate(shape, n, steps, both):
  env = balloon_env.VecBalloonEnv(n, seed=0)
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(qnet.init_params('quantile', 0, *shape)))
  cls = qnet_train.VecPrioritizedReplayBuffer if both else qnet_train.VecReplayBuffer
  rp = cls(n, 64, 5, 0.993)
  kw = dict(max_episode_length=960, min_replay_history=0, update_period=4, target_update_period=100, batch_size=32)
  if both:
    kw.update(epsilon=0.0, exploration=marco_polo.VecMarcoPoloExploration(n, 0.8, seed=0))
  train_lib.run_training_loop_vec(env, tr, rp, num_iterations=1, steps_per_iteration=8, **kw)      # warm-up (allocations, capture)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = train_lib.run_training_loop_vec(env, tr, rp, num_iterations=1, steps_per_iteration=steps, **kw)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  return {'what': 'loop', 'prioritized_marco_polo': both, 'shape': list(shape), 'num_envs': n, 'steps': steps,
          'env_steps_per_s': n * steps / dt, 'updates': stats[0]['updates']}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='fewer iterations')
  args = ap.parse_args()
  iters = 20 if args.quick else 200
  for n in (256, 4096):
    print(json.dumps(tree_add_rate(n, 512, iters)), flush=True)
  uni, pri = _fill(qnet_train.VecReplayBuffer), _fill(qnet_train.VecPrioritizedReplayBuffer)
  shape = (8, 600, 51)
  for b in (32, 4096):
    tu, tp = update_rate(shape, b, uni, iters), update_rate(shape, b, pri, iters)
    print(json.dumps({'what': 'update', 'shape': list(shape), 'batch': b, 'uniform_ms': tu * 1e3, 'prioritized_ms': tp * 1e3,
                      'overhead_pct': 100.0 * (tp - tu) / tu}), flush=True)
  for both in (False, True):
    print(json.dumps(loop_rate(shape, 256, 4 if args.quick else 16, both)), flush=True)


if __name__ == '__main__':
  main()
