"""Fleet cost: 32-step ble_step_n launches (prepare_step_n) at 65 536 and 8 192 environments, for

    default       the reference's vehicle (ble_state_f32.vehicle == NULL: compile-time constants; the four-wave form below 32 768)
    rt_vehicle    one run-time vehicle (ble_step_kernel<VehicleRt>, one lane per environment)
    fleet_1       a fleet of one (ble_step_kernel<VehicleFleet>)
    fleet_16      a fleet of 16 random vehicles, random indices
    fleet_16_noise  the same with the in-kernel wind-noise generator

Each repetition starts from the same device reset (outside the timed region), so every repetition does the same work; the time of one
launch is taken with HIP events and the median of --reps repetitions after --warmup is reported.  One JSON line per (n, leg):

    python profiles/fleet_rate.py [--reps 21] [--warmup 5] [--out profiles/fleet_rate.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balloon_learning_environment_amd import _abi, vec_state  # noqa: E402

K = 32


def vehicles(rng, count):
  out = []
  for j in range(count):
    v = {k: float(x * rng.uniform(0.9, 1.1)) for k, x in _abi.VEHICLE_DEFAULTS.items() if k != 'power_safety_layer_enabled'}
    v['power_safety_layer_enabled'] = int(j % 2)
    out.append(v)
  return out


def leg(n, name, reps, warmup, field, palette, index):
  sim = vec_state.VecSimulator(n, 'cuda:0')
  sim.set_grid(field)
  if name == 'rt_vehicle':
    sim.set_vehicle(**palette[0])
  elif name == 'fleet_1':
    sim.set_fleet(palette[:1])
  elif name.startswith('fleet_16'):
    sim.set_fleet(palette, torch.from_numpy(index))
  acts = torch.from_numpy(np.random.default_rng(7).integers(0, 3, (K, n)).astype(np.uint8)).cuda()
  r = torch.zeros(K, n, device='cuda'); t = torch.zeros(K, n, dtype=torch.uint8, device='cuda')
  launch = sim.prepare_step_n(acts, r, t, noise_seed=3 if name.endswith('noise') else None)
  times = []
  for i in range(warmup + reps):
    sim.reset_device(seed=123)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    launch()
    b.record()
    b.synchronize()
    if i >= warmup:
      times.append(a.elapsed_time(b) * 1e-3)
  sim.check_errors()
  med = float(np.median(times))
  return {'n': n, 'leg': name, 'steps_per_launch': K, 'reps': reps, 'median_s': med, 'min_s': float(np.min(times)),
          'max_s': float(np.max(times)), 'env_steps_per_s': n * K / med}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=21)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  rng = np.random.default_rng(2026)
  field = (rng.standard_normal((21, 21, 10, 9, 2)) * 6.0).astype(np.float32)
  palette = vehicles(rng, 16)
  lines = []
  for n in (65536, 8192):
    index = rng.integers(0, 16, n).astype(np.uint8)
    rows = {}
    for name in ('default', 'rt_vehicle', 'fleet_1', 'fleet_16', 'fleet_16_noise'):
      rows[name] = leg(n, name, args.reps, args.warmup, field, palette, index)
    for name, row in rows.items():
      row['vs_rt_vehicle'] = row['env_steps_per_s'] / rows['rt_vehicle']['env_steps_per_s']
      row['vs_default'] = row['env_steps_per_s'] / rows['default']['env_steps_per_s']
      lines.append(json.dumps(row))
      print(lines[-1], flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
