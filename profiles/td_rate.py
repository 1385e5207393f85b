"""Rates of the DQN and SARSA learners (DESIGN §3g "DQN and SARSA") beside the parent's parts they are built from, in one process:

 * the DQN update (DQNTrainer, sample + train step as one captured graph) at (8, 600, 1), B = 32 and 4096, beside QNetworkTrainer at
   the same shape and B -- the two differ by the loss kernel alone;
 * VecMLPAgent.step (one captured graph) at (1, -) and (2, 64), N = 256 and 4096, beside two VecQNetworkAgent forwards at N plus one
   QNetworkTrainer update on a given batch of B = N rows of the same shape (SARSA keeps one more forward's activations and
   back-propagates 2 N rows, so more than that sum is expected).

Device events around every single call, 200 calls after a warm-up: median, min and max in microseconds, one JSON line per measurement.

  python profiles/td_rate.py [--quick] > profiles/td_rate.jsonl
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/td_rate.py --quick      # the per-kernel shares
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from balloon_learning_environment_amd.agents import dqn_agent, mlp_agent, qnet, qnet_train  # noqa: E402


def _replay(n_env=256, steps=64):
  rng = np.random.default_rng(0)
  rp = qnet_train.VecReplayBuffer(n_env, steps, 5, 0.993)
  for _ in range(steps):
    rp.add(torch.from_numpy(rng.random((n_env, 1099), dtype=np.float32)).cuda(), torch.from_numpy(rng.integers(0, 3, n_env).astype(np.uint8)).cuda(),
           torch.from_numpy(rng.random(n_env, dtype=np.float32)).cuda(), torch.from_numpy((rng.random(n_env) < 0.02).astype(np.uint8)).cuda())
  return rp


def timed(call, iters, warmup=10):
  """Microseconds of each of `iters` calls, by a pair of device events around every call: (median, min, max)."""
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


def _mlp_params(layers, hidden):
  return qnet.init_params('mlp', 0, layers, hidden)


def update_rates(shape, b, rp, iters):
  layers, hidden = shape
  out = []
  for name, make in (('QNetworkTrainer', lambda net: qnet_train.QNetworkTrainer(net)),
                     ('DQNTrainer mse', lambda net: dqn_agent.DQNTrainer(net, loss_type='mse')),
                     ('DQNTrainer huber', lambda net: dqn_agent.DQNTrainer(net, loss_type='huber')),
                     ('QNetworkTrainer again', lambda net: qnet_train.QNetworkTrainer(net))):
    tr = make(qnet.QNetwork.from_params(_mlp_params(layers, hidden)))
    tr.capture(rp, b)
    r = timed(lambda: tr.train_step(rp, b), iters)
    tr.check_errors()
    out.append({'what': 'update', 'learner': name, 'shape': [layers, hidden, 1], 'batch': b, **r})
  return out


def step_rates(shape, n, iters):
  layers, hidden = shape
  rng = np.random.default_rng(1)
  obs = torch.from_numpy(rng.random((n, 1099), dtype=np.float32)).cuda()
  obs2 = torch.from_numpy(rng.random((n, 1099), dtype=np.float32)).cuda()
  reward = torch.from_numpy(rng.random(n, dtype=np.float32)).cuda()
  end = torch.from_numpy((rng.random(n) < 0.01).astype(np.uint8)).cuda()
  net = qnet.QNetwork.from_params(_mlp_params(layers, hidden))
  ag = mlp_agent.VecMLPAgent(n, net, learning_rate=1e-6)
  ag.begin_episode(obs)
  flip = [0]

  def step():
    flip[0] ^= 1
    ag.step(reward, obs2 if flip[0] else obs, end)
  eager = timed(step, iters)
  ag.capture()
  graph = timed(step, iters)
  ag.check_errors()
  # the parent's parts: a forward at N (timed alone; the sum below counts it twice) and one QR update at B = N on a given batch
  vec = qnet.VecQNetworkAgent(qnet.QNetwork.from_params(_mlp_params(layers, hidden)))
  actions = torch.zeros(n, dtype=torch.uint8, device='cuda')
  forward = timed(lambda: vec.act(obs, out=actions), iters)
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(_mlp_params(layers, hidden)))
  bt = qnet_train.TrainBatch.from_tensors(obs.cpu().numpy(), obs2.cpu().numpy(), reward.cpu().numpy(), np.full(n, 0.9, np.float32),
                                          rng.integers(0, 3, n), 'cuda')
  update = timed(lambda: tr.train_on_batch(bt), iters)
  # act's forward + head, the two kept forwards, the loss, per layer 2 dW + their reduction (+ dX below the last), SGD, two copies
  launches = (layers + 1) + 2 * layers + 1 + (3 * layers + (layers - 1)) + 1 + 2
  base = {'shape': [layers, hidden, 1], 'num_envs': n}
  return [{'what': 'VecMLPAgent.step eager (with its three input copies and two state copies)', **base, **eager},
          {'what': 'VecMLPAgent.step graph (with its three input copies)', **base, 'kernel_launches_in_graph': launches, **graph},
          {'what': 'VecQNetworkAgent.act eager', **base, **forward},
          {'what': 'QNetworkTrainer.train_on_batch eager, B = N', **base, **update},
          {'what': 'parts: 2 x act + 1 x update (medians)', **base, 'median_us': 2 * forward['median_us'] + update['median_us']}]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--quick', action='store_true', help='fewer calls (for a profiler run)')
  args = ap.parse_args()
  iters = 20 if args.quick else 200
  rp = _replay()
  for b in (32, 4096):
    for row in update_rates((8, 600), b, rp, iters):
      print(json.dumps(row), flush=True)
  for shape in ((1, 0), (2, 64)):
    for n in (256, 4096):
      for row in step_rates(shape, n, iters):
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
  main()
