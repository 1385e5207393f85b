"""The bits the three device learners compute for one fixed seed, as SHA-256 digests of the packed online image: after 20 updates of
QNetworkTrainer at (2, 64, 51) and of DQNTrainer 'mse' / 'huber' at (2, 64, 1) on one replay ring, and after 20 VecMLPAgent steps at
(1, -) and (2, 64) with N = 64.  Run on two commits (each from its own checkout, into one JSON file), the digests say whether a change of
the host code or the Python around the kernels moved a bit.

  python profiles/learner_bits.py LABEL [profiles/learner_refactor_bits.json]

adds {LABEL: digests} to the JSON file and exits 1 when two labels in it disagree."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from balloon_learning_environment_amd.agents import dqn_agent, mlp_agent, qnet, qnet_train  # noqa: E402

SEED, UPDATES, N, BATCH = 7, 20, 64, 32


def digest(learner) -> str:
  torch.cuda.synchronize()
  return hashlib.sha256(learner.weights.cpu().numpy().tobytes()).hexdigest()


def trainer_digest(make, network, replay) -> str:
  tr = make(network)
  for _ in range(UPDATES):
    tr.train_step(replay, BATCH)
  tr.check_errors()
  return digest(tr)


def mlp_digest(layers, hidden, rng) -> str:
  ag = mlp_agent.VecMLPAgent(N, qnet.QNetwork.from_params(qnet.init_params('mlp', SEED, layers, hidden)), learning_rate=1e-3, seed=SEED)
  obs = [torch.from_numpy(rng.random((N, 1099), dtype=np.float32)).cuda() for _ in range(UPDATES + 1)]
  ag.begin_episode(obs[0])
  for t in range(UPDATES):
    reward = torch.from_numpy(rng.random(N, dtype=np.float32)).cuda()
    end = torch.from_numpy((rng.random(N) < 0.05).astype(np.uint8)).cuda()
    ag.step(reward, obs[t + 1], end)
  ag.check_errors()
  return digest(ag)


def main():
  label = sys.argv[1]
  path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'learner_refactor_bits.json')
  rng = np.random.default_rng(SEED)
  replay = qnet_train.VecReplayBuffer(N, 32, 5, 0.993)
  for _ in range(32):
    replay.add(torch.from_numpy(rng.random((N, 1099), dtype=np.float32)).cuda(), torch.from_numpy(rng.integers(0, 3, N).astype(np.uint8)).cuda(),
               torch.from_numpy(rng.random(N, dtype=np.float32)).cuda(), torch.from_numpy((rng.random(N) < 0.02).astype(np.uint8)).cuda())
  quantile = qnet.QNetwork.from_params(qnet.init_params('quantile', SEED, 2, 64, 51), num_atoms=51)
  mlp = qnet.QNetwork.from_params(qnet.init_params('mlp', SEED, 2, 64))
  out = {'QNetworkTrainer (2, 64, 51)': trainer_digest(lambda n: qnet_train.QNetworkTrainer(n, lr=1e-3, seed=SEED), quantile, replay),
         **{f'DQNTrainer {k} (2, 64, 1)': trainer_digest(lambda n: dqn_agent.DQNTrainer(n, loss_type=k, lr=1e-3, seed=SEED), mlp, replay)
            for k in ('mse', 'huber')},
         'VecMLPAgent (1, -), N = 64': mlp_digest(1, 0, rng), 'VecMLPAgent (2, 64), N = 64': mlp_digest(2, 64, rng)}
  runs = json.load(open(path)) if os.path.exists(path) else {}
  runs[label] = out
  with open(path, 'w') as f:
    json.dump(runs, f, indent=1)
    f.write('\n')
  print(json.dumps({label: out}, indent=1))
  sys.exit(0 if all(r == out for r in runs.values()) else 1)


if __name__ == '__main__':
  main()
