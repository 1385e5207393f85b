"""WindGP query rate: VecSimulator.query_wind (ble_gp_query_f32) after a rollout that has filled the 6 h windows, next to the
observation launch of the same state.

For n in (4 096, 65 536): a VecBalloonEnv (wind noise on, auto-reset) flies --rollout agent steps (default 124: every environment that
has not been reset holds a full window of 120 observations), then

    observe     one observation launch (ble_observe_forecast_f32, carried factor) per repetition, inside the continuing rollout: the
                transition, the masked reset and the wind noise of the step are enqueued before the timed region
    query       query_wind at q in (16, 181, 512) points per environment, time_s = now, the forecast added, on the state the
                observation legs left; the points lie within 50 km of each balloon, anywhere in 5 000 .. 14 000 Pa

Each launch is timed with HIP events; the median of --reps repetitions after --warmup is reported.  One JSON line per (n, leg):

    python profiles/gp_query_rate.py [--reps 21] [--warmup 5] [--sizes 4096,65536] [--out profiles/gp_query_rate.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balloon_learning_environment_amd.env import balloon_env  # noqa: E402

QS = (16, 181, 512)


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e-3


def row(n, leg, times, reps, **extra):
  med = float(np.median(times))
  return {'n': n, 'leg': leg, 'reps': reps, 'median_s': med, 'min_s': float(np.min(times)), 'max_s': float(np.max(times)), **extra}


def run(n, rollout, reps, warmup):
  rng = np.random.default_rng(5)
  env = balloon_env.VecBalloonEnv(n, seed=1)
  env.reset()
  actions = torch.from_numpy(rng.integers(0, 3, (rollout + warmup + reps, n)).astype(np.uint8)).cuda()
  for k in range(rollout):
    env.step(actions[k])
  sim = env.arena.sim
  obs = torch.empty(n, 1099, dtype=torch.float32, device=sim.device)
  rows, times = [], []
  for i in range(warmup + reps):
    # one agent step of VecBalloonEnv with the observation launch timed on its own
    _, terminal = env.arena.step(actions[rollout + i], env._noise)
    env._terminal_buf.copy_(terminal)
    env.arena.reset_lanes(env._terminal_buf)
    noise = env._noise_now()
    t = timed(lambda: env.arena.observe(noise, out=obs))
    if i >= warmup:
      times.append(t)
  env.check_errors()
  window = torch.clamp(sim._gp['count'], max=120).float()
  fill = {'mean_window': float(window.mean().item()), 'full_windows': float((window == 120).float().mean().item())}
  rows.append(row(n, 'observe', times, reps, **fill))
  for q in QS:
    centre = torch.stack([sim.state['x'], sim.state['y'], torch.zeros_like(sim.state['x'])], -1)[:, None, :]
    spread = torch.from_numpy(np.concatenate([rng.uniform(-5.0e4, 5.0e4, (n, q, 2)), rng.uniform(5000.0, 14000.0, (n, q, 1))], -1)
                              .astype(np.float32)).to(sim.device)
    xyp = (centre + spread).contiguous()
    out = (torch.empty(n, q, 2, dtype=torch.float32, device=sim.device), torch.empty(n, q, dtype=torch.float32, device=sim.device))
    times = []
    for i in range(warmup + reps):
      t = timed(lambda: sim.query_wind(xyp, out=out))
      if i >= warmup:
        times.append(t)
    env.check_errors()
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
    r = row(n, f'query_q{q}', times, reps, q=q, **fill)
    r['queries_per_s'] = n * q / r['median_s']
    r['vs_observe'] = r['median_s'] / rows[0]['median_s']
    rows.append(r)
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=21)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--rollout', type=int, default=124)
  ap.add_argument('--sizes', default='4096,65536')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  lines = []
  for n in [int(s) for s in args.sizes.split(',')]:
    for r in run(n, args.rollout, args.reps, args.warmup):
      lines.append(json.dumps(r))
      print(lines[-1], flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
