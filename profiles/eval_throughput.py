"""Throughput of a batched evaluation: eval_agent_vec(VecStationSeekerAgent(), get_eval_suite(SUITE)) on one GPU.

  python profiles/eval_throughput.py --suite small_eval [--batch-size B] [--kernel-share OUT_DIR] [--agent seeker|quantile]

--agent quantile evaluates a VecQNetworkAgent with a Perciatelli44-shaped QR-DQN network (8 Dense layers, 600 units, 51 atoms) of
the reference's initialisation (qnet.init_params) in place of the StationSeeker.

Prints one JSON line: seeds, steps per seed, wall seconds of the timed evaluation (after an untimed one-seed warm-up that loads the
library and the decoder), env-steps/s and the mean cumulative reward / time within radius.  --kernel-share OUT_DIR runs the same
evaluation once more in a child process under `rocprofv3 --kernel-trace --stats` (output in OUT_DIR) and adds each kernel's share of
GPU time, the StationSeeker's among them (the profiled run is not the timed one).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_agent(kind):
  if kind == 'quantile':
    from balloon_learning_environment_amd.agents import qnet
    return qnet.VecQNetworkAgent(qnet.QNetwork.from_params(qnet.init_params('quantile', 0, 8, 600, 51)))
  from balloon_learning_environment_amd.agents import station_seeker_agent
  return station_seeker_agent.VecStationSeekerAgent()


def run(suite_name, batch_size, kind='seeker'):
  import torch
  from balloon_learning_environment_amd.eval import eval_lib, suites
  agent = make_agent(kind)
  suite = suites.get_eval_suite(suite_name)
  eval_lib.eval_agent_vec(agent, suites.EvaluationSuite([0], 8))          # warm-up: library, decoder weights, BLAS handles
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  res = eval_lib.eval_agent_vec(agent, suite, batch_size=batch_size)
  torch.cuda.synchronize()
  wall = time.perf_counter() - t0
  steps = sum(r.final_timestep for r in res)
  return {'suite': suite_name, 'agent': kind, 'seeds': len(res), 'steps': suite.max_episode_length, 'batch_size': batch_size or min(len(res), 16384),
          'wall_s': round(wall, 3), 'env_steps': steps, 'env_steps_per_s': round(steps / wall, 1),
          'mean_reward': round(sum(r.cumulative_reward for r in res) / len(res), 3),
          'mean_twr': round(sum(r.time_within_radius for r in res) / len(res), 4)}


def kernel_shares(out_dir, suite_name, batch_size, kind='seeker'):
  cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'eval', '--',
         sys.executable, os.path.abspath(__file__), '--suite', suite_name, '--agent', kind]
  if batch_size:
    cmd += ['--batch-size', str(batch_size)]
  subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
  path = sorted(glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True))[-1]
  with open(path) as f:
    rows = list(csv.DictReader(f))
  total = sum(float(r['TotalDurationNs']) for r in rows)
  share = {}
  for r in rows:
    name = r['Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:60]
    share[name] = share.get(name, 0.0) + float(r['TotalDurationNs']) / total
  top = dict(sorted(share.items(), key=lambda kv: -kv[1])[:8])
  seeker = sum(v for k, v in share.items() if 'station_seeker' in k)
  policy = sum(v for k, v in share.items() if 'qnet' in k)
  return {'gpu_time_s': round(total / 1e9, 3), 'seeker_share': round(seeker, 4), 'qnet_share': round(policy, 4),
          'top_kernels': {k: round(v, 4) for k, v in top.items()}}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--suite', default='small_eval')
  ap.add_argument('--batch-size', type=int, default=None)
  ap.add_argument('--kernel-share', default=None, metavar='OUT_DIR')
  ap.add_argument('--agent', default='seeker', choices=('seeker', 'quantile'))
  a = ap.parse_args()
  out = run(a.suite, a.batch_size, a.agent)
  if a.kernel_share:
    out.update(kernel_shares(a.kernel_share, a.suite, a.batch_size, a.agent))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
